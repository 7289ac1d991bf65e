"""Register budgets of k_sample_volpath (device/volpath_kernel.h), cross-compiled for gfx950 by the route of
test_sample_kernel_budget.py: tools/probe_volpath.hip instantiates exactly what mi_sample launches for MI_INTEGRATOR_VOLPATH.

The kernels are compiled for two wavefronts per SIMD (MIW_VOLPATH_WAVES: 256 registers); the compiled occupancy must equal that
launch bound. A lane of the state machine carries far more than k_sample_rays' — and the flattened loops keep all of it live
across the one scene query —, so the compiler keeps part of it in scratch; the bytes below are the compiler's for this source and
are pinned as upper bounds. DESIGN.md section 4.12 quotes the table."""
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

# (Tiny, Mats, Analytic) -> bytes of scratch per lane. Mats: 4 NESTED
PINNED = {(1, 4, 0): 3168, (0, 4, 0): 3220}
WAVES = 2


def test_volpath_instantiations_keep_their_launch_bound_and_pinned_scratch(tmp_path):
    out = subprocess.run([HIPCC] + FLAGS + [os.path.join(ROOT, "tools", "probe_volpath.hip"), "-o", str(tmp_path / "probe.o")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        m = re.match(r"_Z16k_sample_volpathILi(\d)ELi(\d)ELb([01])EE", blk.split()[0])
        if m:
            val = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
            res[tuple(int(g) for g in m.groups())] = dict(vgprs=val("VGPRs"), scratch=val("ScratchSize [bytes/lane]"), waves=val("Occupancy [waves/SIMD]"))
    assert sorted(res) == sorted(PINNED), sorted(res)
    for k, scratch in PINNED.items():
        print(k, res[k])
        assert res[k]["waves"] == WAVES and res[k]["vgprs"] <= 256 and res[k]["scratch"] <= scratch, (k, res[k])
