"""The frame twin of the headline packet kernel against its lean and its full kernel, all three compiled here (no GPU needed: hipcc cross-compiles gfx950).

tools/probe_resident.hip holds k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH> (every template parameter after that at its default), tools/probe_resident_lean.hip
its lean twin (Feat = FEAT_NONE), tools/probe_resident_frame.hip the lean twin's frame twin (Feat = FEAT_FRAME: chunk jobs from one queue, the 16-byte log, no tail priorities
and the leaf filter compiled in, device/resident_kernel.h). The twin exists to carry less through the pixel loop at the same five wavefronts per SIMD; from ONE compile
of the three probes, reading the kernels' resource counts only:

  * the twin's vector spills, scalar spills and scratch bytes are no larger than the lean kernel's;
  * its registers still allow five wavefronts per SIMD (at most 96 vector registers), and its static LDS is no larger than the lean
    kernel's, which the launch accounts for (miwave.hip: MIW_LDS_STATIC);
  * the two other probes have the resource rows they had before the twin existed, under the names they had (profiles/r09_lean_packet.txt, step 0b).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-S", "--cuda-device-only"]
FULL = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj15EE"     # <true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 0, FEAT_ALL>
LEAN = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj0EE"      # <..., FEAT_NONE>
TWIN = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj16EE"     # <..., FEAT_FRAME>
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


def _row(text, kernel):
    """the kernel's record in the code object's metadata (amdhsa.kernels), its resource fields only"""
    recs = [r for r in re.split(r"\n  - \.", text[text.index("amdhsa.kernels"):]) if re.search(r"\.name:\s+%s\w*\n" % re.escape(kernel), r)]
    assert len(recs) == 1, (kernel, len(recs))
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, recs[0]).group(1)) for k in FIELDS}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_twin_budget")
    jobs = [(probe, str(d / (probe + ".s"))) for probe in ("probe_resident.hip", "probe_resident_lean.hip", "probe_resident_frame.hip")]
    procs = [subprocess.Popen([HIPCC] + FLAGS + [os.path.join(ROOT, "tools", probe), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for probe, out in jobs]                                 # (side by side: about a minute each)
    for p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
    res = {}
    for (probe, out), kernel in zip(jobs, (FULL, LEAN, TWIN)):
        text = open(out).read()
        assert sum(k in text for k in (FULL, LEAN, TWIN)) == 1, probe        # one path kernel per probe
        res[kernel] = _row(text, kernel)
        print(probe, res[kernel])
    return res


def test_twin_spills_no_more_than_the_lean_kernel(rows):
    lean, twin = rows[LEAN], rows[TWIN]
    for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert twin[k] <= lean[k], (k, twin[k], lean[k])


def test_twin_keeps_five_wavefronts_per_simd(rows):
    twin = rows[TWIN]
    # 512 vector registers per SIMD lane, allocated in blocks of 8: five wavefronts hold 96 each (vgpr_count is the unified file: accumulation registers included)
    assert twin["vgpr_count"] <= 96, twin
    assert twin["group_segment_fixed_size"] <= rows[LEAN]["group_segment_fixed_size"] <= 1024 + 16, (twin, rows[LEAN])     # MIW_LDS_STATIC + s_prog


def test_default_parameter_probes_have_the_rows_they_had(rows):
    had = dict(vgpr_count=96, sgpr_count=106, private_segment_fixed_size=52, group_segment_fixed_size=1040)
    assert rows[FULL] == dict(had, vgpr_spill_count=18, sgpr_spill_count=69), rows[FULL]
    assert rows[LEAN] == dict(had, vgpr_spill_count=17, sgpr_spill_count=47), rows[LEAN]
