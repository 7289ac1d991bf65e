"""Register budgets of k_sample_rays (device/sample_kernel.h), cross-compiled for gfx950 by the route of test_kernel_budget.py:
tools/probe_sample.hip instantiates exactly what mi_sample launches.

The path instantiations carry no scratch at all: the packet kernels fit 128 registers (four wavefronts per SIMD), the tree kernels
168 (three — MIW_TREE_WAVES, what the lock-step tree kernels of mi_render are compiled for). The direct instantiations are compiled
for three wavefronts like the direct render kernels, and like them the ones with the BSDF table or the tree walk keep some values in
scratch there (resident_kernel.h: MIW_DIRECT_WAVES says why three is still the faster choice); the numbers below are the compiler's
for this source and are pinned as upper bounds. DESIGN.md quotes the occupancies."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-c",
         "-Rpass-analysis=kernel-resource-usage"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


def _resources(tmp_path, *defs):
    out = subprocess.run([HIPCC] + FLAGS + list(defs) + [os.path.join(ROOT, "tools", "probe_sample.hip"), "-o", str(tmp_path / "probe.o")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        m = re.match(r"_Z13k_sample_raysILi(\d)ELi(\d)ELb([01])ELj([01])E", blk.split()[0])
        if m:
            val = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
            res[tuple(int(g) for g in m.groups())] = dict(vgprs=val("VGPRs"), scratch=val("ScratchSize [bytes/lane]"), spilled=val("VGPRs Spill"),
                                                          waves=val("Occupancy [waves/SIMD]"))
    return res


# template arguments: Tiny (0 tree walk, 1 packets + 64-bit masks, 2 packets + 32-bit masks), Mats (0 ALL, 1 DIFFUSE, 2 PLAIN, 3 TRIO), Analytic, Integ
def test_path_instantiations_carry_no_scratch(tmp_path):
    r = _resources(tmp_path)
    packets = [(2, 1, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0), (1, 2, 0, 0), (1, 0, 0, 0)]
    trees = [(0, 0, 1, 0), (0, 3, 0, 0), (0, 2, 0, 0), (0, 2, 1, 0)]
    assert sorted(r) == sorted(packets + trees), sorted(r)
    for k in packets:
        assert r[k]["scratch"] == 0 and r[k]["spilled"] == 0 and r[k]["waves"] == 4 and r[k]["vgprs"] <= 128, (k, r[k])
    for k in trees:
        assert r[k]["scratch"] == 0 and r[k]["spilled"] == 0 and r[k]["waves"] == 3 and r[k]["vgprs"] <= 168, (k, r[k])
    assert r[(2, 1, 0, 0)]["vgprs"] <= 112                     # the all-diffuse Cornell kernel (no BSDF dispatch)


def test_direct_instantiations_keep_their_pinned_scratch(tmp_path):
    r = _resources(tmp_path, "-DMIW_PROBE_DIRECT=1")
    pinned = {(1, 0, 0, 1): 24, (1, 2, 0, 1): 0, (0, 0, 1, 1): 148, (0, 2, 1, 1): 132}     # bytes of scratch per lane
    assert sorted(r) == sorted(pinned), sorted(r)
    for k, scratch in pinned.items():
        assert r[k]["waves"] == 3 and r[k]["vgprs"] <= 168 and r[k]["scratch"] <= scratch, (k, r[k])
