"""The frame twin of the headline packet kernel with the job pool and the per-wavefront counters compiled in, held to the resources it had without them
(no GPU needed: hipcc cross-compiles gfx950).

ONE compile of tools/probe_resident_frame.hip (k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 0, FEAT_FRAME>), reading the kernel's resource
counts only. The bounds are the twin's row before the pool (profiles/r10_frame_twin.txt: 96 registers, 8 vector and 33 scalar spills, 36 bytes of scratch per
lane, 1 024 bytes of static LDS beside the lean kernel's 1 040): the pool's cursor, its ring and the three counters live in DYNAMIC LDS, which the launch
reserves (miwave.hip: path_route), and the twin still runs five wavefronts per SIMD.

The twin as committed holds the parent's row to the digit: 96 registers, 8 vector and 33 scalar spills, 36 bytes of scratch, 1 024 bytes of static LDS. What
holds it: a wavefront's block stands at a constant address (the end of a launch of one fixed size, render_plan.h: MIW_TWIN_LDS) and its ring has a fixed
number of slots, so neither the block's offset nor the pool's size is kept in a register through the pixel loop. Forms that kept either spilled 34 to 36
scalar registers or 10 to 12 vector ones (profiles/r12_job_pool.txt).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-S", "--cuda-device-only"]
TWIN = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj16EE"     # <true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 0, FEAT_FRAME>
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("job_pool_budget") / "frame.s")
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join(ROOT, "tools", "probe_resident_frame.hip"), "-o", out], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(out).read()
    recs = [r for r in re.split(r"\n  - \.", text[text.index("amdhsa.kernels"):]) if re.search(r"\.name:\s+%s\w*\n" % re.escape(TWIN), r)]
    assert len(recs) == 1, len(recs)
    row = {k: int(re.search(r"\.%s:\s+(\d+)" % k, recs[0]).group(1)) for k in FIELDS}
    print(row)
    return row, text


def test_registers_allow_five_wavefronts_per_simd(twin):
    assert twin[0]["vgpr_count"] <= 96, twin[0]


def test_spills_and_scratch_no_more_than_before_the_pool(twin):
    row = twin[0]
    assert row["vgpr_spill_count"] <= 8, row
    assert row["sgpr_spill_count"] <= 33, row
    assert row["private_segment_fixed_size"] <= 36, row


def test_static_lds_stays_the_lean_kernels(twin):
    assert twin[0]["group_segment_fixed_size"] <= 1040, twin[0]


def test_the_pool_is_compiled_in(twin):
    # the counters are LDS adds, and the ring is written and read: the probe is the kernel with the pool, not a build without it
    text = twin[1]
    body = text[re.search(r"^%s\w*:" % re.escape(TWIN), text, re.M).start():]
    body = body[:body.index("s_endpgm")]
    assert len(re.findall(r"\bds_add_u64\b", body)) == 3, "segments, samples, shadow rays"
    # the state word's load past the L2: at the draw and the direct one (the compiler may copy a loop's)
    assert len(re.findall(r"global_load_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off sc1", body)) >= 2
