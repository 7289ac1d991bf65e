"""Register budgets of the MATS_NESTED kernels (mask / blendbsdf / null / thindielectric scenes), cross-compiled for gfx950 by the
route of test_kernel_budget.py: tools/probe_nested.hip instantiates what mi_render and mi_sample launch for such a scene, each beside
its MATS_ALL sibling.

Every MATS_NESTED instantiation is compiled for the wavefronts per SIMD of its sibling (the launch bounds do not depend on the
material class); what the wrapper state costs shows as scratch. The tree-walk path instantiations carry none, like their siblings.
The PACKET path instantiations (k_sample_rays<1, NESTED> and k_path_resident<true, 1, NESTED>) do: the sibling fills the 128 registers
of four wavefronts per SIMD exactly, and the chain's records, flip flags and the blend's running sum live across the inlined plugin
code. The numbers are hipcc's for this source, pinned as upper bounds."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-c",
         "-Rpass-analysis=kernel-resource-usage"]
ALL, NESTED = 0, 4

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


def _resources(tmp_path, mode, pattern):
    out = subprocess.run([HIPCC] + FLAGS + ["-DMIW_PROBE_NESTED=%d" % mode, os.path.join(ROOT, "tools", "probe_nested.hip"), "-o", str(tmp_path / "probe.o")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        m = re.match(pattern, blk.split()[0])
        if m:
            val = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
            res[tuple(int(g) for g in m.groups())] = dict(vgprs=val("VGPRs"), scratch=val("ScratchSize [bytes/lane]"), waves=val("Occupancy [waves/SIMD]"))
    return res


def _check(r, pinned, cap):
    """pinned: {(Tiny, Analytic, Integ): scratch bytes per lane of the MATS_NESTED instantiation}; keys of r: (Tiny, Mats, Analytic, Integ)"""
    assert sorted(r) == sorted([(t, m, a, i) for (t, a, i) in pinned for m in (ALL, NESTED)]), sorted(r)
    for (t, a, i), scratch in pinned.items():
        n, s = r[(t, NESTED, a, i)], r[(t, ALL, a, i)]
        assert n["waves"] == s["waves"], ((t, a, i), n, s)                 # compiled for its sibling's wavefronts per SIMD
        assert n["vgprs"] <= cap[n["waves"]] and n["scratch"] <= scratch, ((t, a, i), n)


# template arguments: Tiny (0 tree walk, 1 packets), Mats (0 ALL, 4 NESTED), Analytic, Integ (0 path, 1 direct)
def test_sample_kernels(tmp_path):
    r = _resources(tmp_path, 1, r"_Z13k_sample_raysILi(\d)ELi(\d)ELb([01])ELj([01])E")
    _check(r, {(1, 0, 0): 112, (0, 1, 0): 0, (1, 0, 1): 108, (0, 1, 1): 240}, {4: 128, 3: 168})
    assert r[(0, ALL, 1, 0)]["scratch"] == 0 and r[(1, ALL, 0, 0)]["scratch"] == 0     # the siblings: as test_sample_kernel_budget.py pins them


def test_resident_kernels(tmp_path):
    r = _resources(tmp_path, 2, r"_Z15k_path_residentILb1ELi(\d)ELi(\d)ELb([01])ELj([01])ELb0ELi0E")
    _check(r, {(1, 0, 0): 96, (0, 1, 0): 0, (1, 0, 1): 156, (0, 1, 1): 400}, {4: 128, 3: 168})


def test_phase_machine(tmp_path):
    r = _resources(tmp_path, 3, r"_Z13k_path_phasedILi(\d)ELb1ELb[01]ELi4ELi(\d)ELb0E")         # keys: (Mats, Wide)
    assert sorted(r) == [(ALL, 1), (ALL, 2), (NESTED, 1), (NESTED, 2)], sorted(r)
    for wide, scratch in ((2, 268), (1, 268)):
        n, s = r[(NESTED, wide)], r[(ALL, wide)]
        assert n["waves"] == s["waves"] == 4 and n["vgprs"] <= 128 and n["scratch"] <= scratch, (wide, n, s)
