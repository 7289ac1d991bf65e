"""Register budgets of the MATS_LIGHTS kernels (scenes with a point / spot / directional / constant emitter), cross-compiled for gfx950
by the route of test_nested_kernel_budget.py: tools/probe_lights.hip instantiates what mi_render and mi_sample launch for such a
scene, each beside its MATS_NESTED sibling.

MATS_LIGHTS is the MATS_NESTED table plus the light table (csrc/miw/light.h): every instantiation is compiled for its sibling's
wavefronts per SIMD (the launch bounds do not depend on the material class). The numbers are hipcc's for this source (DESIGN.md
section 4.9), pinned as upper bounds: VGPRs, scratch bytes per lane, and the occupancy exactly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-c",
         "-Rpass-analysis=kernel-resource-usage"]
NESTED, LIGHTS = 4, 5
# (the resident packet kernels and the phase machine stage the light table in LDS: their figures are those of that form)
RESIDENT = {(1, 0, 0): (128, 108, 4), (0, 1, 0): (168, 0, 3), (1, 0, 1): (168, 152, 3), (0, 1, 1): (168, 352, 3)}
PHASED = {2: (128, 264), 1: (128, 272)}

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


def _resources(tmp_path, mode, pattern):
    out = subprocess.run([HIPCC] + FLAGS + ["-DMIW_PROBE_LIGHTS=%d" % mode, os.path.join(ROOT, "tools", "probe_lights.hip"), "-o", str(tmp_path / "probe.o")],
                         capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        m = re.match(pattern, blk.split()[0])
        if m:
            val = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
            res[tuple(int(g) for g in m.groups())] = dict(vgprs=val("VGPRs"), scratch=val("ScratchSize [bytes/lane]"), waves=val("Occupancy [waves/SIMD]"))
    return res


def _check(r, pinned):
    """pinned: {(Tiny, Analytic, Integ): (VGPRs, scratch bytes per lane, wavefronts per SIMD) of the MATS_LIGHTS instantiation}; keys of r: (Tiny, Mats, Analytic, Integ)"""
    assert sorted(r) == sorted([(t, m, a, i) for (t, a, i) in pinned for m in (NESTED, LIGHTS)]), sorted(r)
    for (t, a, i), (vgprs, scratch, waves) in pinned.items():
        n, s = r[(t, LIGHTS, a, i)], r[(t, NESTED, a, i)]
        print((t, a, i), "lights", n, "nested", s)
        assert n["waves"] == waves == s["waves"], ((t, a, i), n, s)
        assert n["vgprs"] <= vgprs and n["scratch"] <= scratch, ((t, a, i), n)


# template arguments: Tiny (0 tree walk, 1 packets), Mats (4 NESTED, 5 LIGHTS), Analytic, Integ (0 path, 1 direct)
def test_sample_kernels(tmp_path):
    r = _resources(tmp_path, 1, r"_Z13k_sample_raysILi(\d)ELi(\d)ELb([01])ELj([01])E")
    _check(r, {(1, 0, 0): (128, 124, 4), (0, 1, 0): (168, 0, 3), (1, 0, 1): (168, 108, 3), (0, 1, 1): (168, 228, 3)})


def test_resident_kernels(tmp_path):
    r = _resources(tmp_path, 2, r"_Z15k_path_residentILb1ELi(\d)ELi(\d)ELb([01])ELj([01])ELb0ELi0E")
    _check(r, RESIDENT)


def test_phase_machine(tmp_path):
    r = _resources(tmp_path, 3, r"_Z13k_path_phasedILi(\d)ELb1ELb[01]ELi4ELi(\d)ELb0E")         # keys: (Mats, Wide)
    assert sorted(r) == [(NESTED, 1), (NESTED, 2), (LIGHTS, 1), (LIGHTS, 2)], sorted(r)
    for wide, (vgprs, scratch) in PHASED.items():
        n, s = r[(LIGHTS, wide)], r[(NESTED, wide)]
        print(wide, "lights", n, "nested", s)
        assert n["waves"] == s["waves"] == 4 and n["vgprs"] <= vgprs and n["scratch"] <= scratch, (wide, n, s)
