"""The lean twin of the headline packet kernel against the full kernel, both compiled here (no GPU needed: hipcc cross-compiles gfx950).

tools/probe_resident.hip holds k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH> with every scene feature compiled in (Feat = FEAT_ALL, the
default), tools/probe_resident_lean.hip the same kernel with none (FEAT_NONE: no environment map, no vertex normals on shapes or emitter faces, no
moment pass — miw/scene.h). The lean kernel exists to run fewer instructions per segment at the same five wavefronts per SIMD, so what it must not
do is pay for that in registers: the bounds are the full kernel's own numbers from the same compile, not a table.

  * the lean kernel keeps the five-wavefront budget: vgpr_count <= 96;
  * its vector spills and the scratch instructions of its pixel loop are no more than the full kernel's;
  * its pixel loop holds strictly fewer vector-ALU instructions;
  * the full kernel's symbol is still there, with the counts tests/test_kernel_budget.py pins for it (96 registers, at most 19 spilled, at most
    32 scratch instructions) and the static counts DESIGN.md section 9 and profiles/r08_packet_diet.txt record: 3 485 vector-ALU and 22 scratch
    instructions in the pixel loop, 18 vector spills.

The counting is tools/valu_count.py's (the pixel loop = from the header of the first loop that contains other loops onwards).
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-S", "--cuda-device-only"]
FULL = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj15EE"      # <true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 0, FEAT_ALL>
LEAN = "_Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj0EE"       # <..., FEAT_NONE>

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import valu_count
    d = tmp_path_factory.mktemp("lean_budget")
    jobs = [(probe, str(d / (probe + ".s"))) for probe in ("probe_resident.hip", "probe_resident_lean.hip")]
    procs = [subprocess.Popen([HIPCC] + FLAGS + [os.path.join(ROOT, "tools", probe), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for probe, out in jobs]                                 # (the two compiles side by side: ~1 minute each)
    for p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
    res = {}
    for (probe, out), kernel in zip(jobs, (FULL, LEAN)):
        text = open(out).read()
        assert text.count("\n" + kernel) >= 1, "no %s in %s" % (kernel, probe)
        tot, loop, _, moves = valu_count.count(out, kernel)
        res[kernel] = dict(tot=tot, loop=loop, moves=moves, **valu_count.resources(out, kernel))
        print(probe, res[kernel])
    assert LEAN not in open(jobs[0][1]).read() and FULL not in open(jobs[1][1]).read()   # one kernel per probe
    return res


def test_lean_kernel_keeps_the_five_wavefront_register_budget(counts):
    assert counts[LEAN]["vgpr_count"] <= 96, counts[LEAN]


def test_lean_kernel_spills_no_more_than_the_full_kernel(counts):
    full, lean = counts[FULL], counts[LEAN]
    assert lean["vgpr_spill_count"] <= full["vgpr_spill_count"], (lean["vgpr_spill_count"], full["vgpr_spill_count"])
    assert lean["loop"]["scratch"] <= full["loop"]["scratch"], (lean["loop"]["scratch"], full["loop"]["scratch"])


def test_lean_kernel_has_fewer_vector_instructions_in_its_pixel_loop(counts):
    assert counts[LEAN]["loop"]["valu"] < counts[FULL]["loop"]["valu"], (counts[LEAN]["loop"]["valu"], counts[FULL]["loop"]["valu"])


def test_full_kernel_is_the_one_it_was(counts):
    full = counts[FULL]
    assert full["vgpr_count"] <= 96 and full["vgpr_spill_count"] <= 19 and full["tot"]["scratch"] <= 32, full     # tests/test_kernel_budget.py
    assert (full["loop"]["valu"], full["loop"]["scratch"], full["vgpr_spill_count"], full["sgpr_spill_count"]) == (3485, 22, 18, 69), full
    assert (full["tot"]["valu"], full["tot"]["salu"], full["moves"]["v_readlane_b32"], full["moves"]["v_writelane_b32"]) == (4022, 2499, 100, 6), full
