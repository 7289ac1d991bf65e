"""Register budgets of the film replay in equal chains (device/film_kernels.h: k_film_chains; no GPU needed: hipcc cross-compiles gfx950).

k_film_chains runs k_film_lanes' body once per position of a wavefront's chain, so its 30 specialised sample loops sit one loop level deeper (chain position ->
pixel step -> sample trip). tools/probe_film_chains.hip holds the instantiations mi_render can launch:

    k_film_chains<4, 1, 3>   four records in flight per lane, compiled for three wavefronts per SIMD: at most 168 registers
    k_film_chains<8, 1, 2>   eight records in flight, two wavefronts per SIMD: at most 256 registers

For both the rule tests/test_kernel_budget.py applies to k_film_lanes holds: what the compiler keeps in scratch is moved around the sample loops, never inside
one, and every one of them is a sample loop (a trip's U samples x at least one row x one column pair x five channels of v_pk_add_f32)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")

KERNELS = [("_Z13k_film_chainsILi4ELi1ELi3E", 168, 3, 4), ("_Z13k_film_chainsILi8ELi1ELi2E", 256, 2, 8)]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("film_chains_budget")
    out = subprocess.run([HIPCC] + FLAGS + [os.path.join(ROOT, "tools", "probe_film_chains.hip"), "-o", str(d / "probe.s")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return open(d / "probe.s").read().split("\n")


@pytest.mark.parametrize("name,cap,waves,records", KERNELS)
def test_chain_kernel_fits_its_registers_and_keeps_its_sample_loops_free_of_scratch(isa, name, cap, waves, records):
    start = next(i for i, l in enumerate(isa) if l.startswith(name))
    end = next(i for i in range(start, len(isa)) if "s_endpgm" in isa[i])
    body = isa[start:end]
    meta = "\n".join(isa)
    blk = meta[meta.index(".name:           " + name):]
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
    assert vgprs <= cap and 512 // max(vgprs, 1) >= waves, vgprs          # (512 vector registers per SIMD lane, allocated in eights: 168 -> 3, 256 -> 2)
    loops = 0
    for i, l in enumerate(body):
        if "Inner Loop Header: Depth=3" not in l:
            continue
        j = i
        while not re.match(r"^\.LBB\d+_\d+:", body[j]):
            j -= 1
        label = body[j].split(":")[0]
        k = j + 1
        while not ("s_cbranch" in body[k] and label in body[k]):
            k += 1
        assert not any("scratch_" in b for b in body[j:k]), "scratch traffic inside the sample loop at %s" % label
        assert sum("v_pk_add_f32" in b for b in body[j:k]) >= 5 * records
        loops += 1
    assert loops == 30                                                     # 10 row ranges x 3 column-pair ranges
