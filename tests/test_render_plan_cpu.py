"""csrc/render_plan.h: the launch arithmetic of mi_render that reads plain numbers only.

A host program built from the header prints

    the chunk-job schedule        spp 1 .. 600  x  MIW_JOB_CHUNK in {0, 1, 4, 8, 32, 48, 64, 128}
    the dealing of placed pieces  pieces in {1, 2, 255, 256, 1024, 4096}  x  queues in {2, 3, 256, 1024}, 4 slots per queue
    lds_workgroups                at its granule boundaries
    persistent_grid               without room, and with room = 32 on both sides of full > 2 * room

and the test compares the rows with restatements written here: the chunk schedule from the DEVICE's rule (device/resident_kernel.h,
QueueWork::job_end / fetch_job: a chunk ends where the samples still to do are a power of two >= job_min; chunk j > 0 starts at
spp - (job_pow >> (j - 1))), the rest from the hardware's numbers (160 KB of LDS per CU in granules of 512 bytes, 1024 + 16 bytes static).
"""
import subprocess

import pytest

from conftest import ROOT

SPP = range(1, 601)
JMIN = (0, 1, 4, 8, 32, 48, 64, 128)
PIECES = (1, 2, 255, 256, 1024, 4096)
QUEUES = (2, 3, 256, 1024)
SLOTS = 4
EMPTY = 0xffffffff
LDS_DYN = (0, 39920, 39921, 31728, 31729, 65536)          # 39920 + 1040 = 80 granules, 31728 + 1040 = 32 KB
# (grid_x, cu_count, wg_per_cu, room, resident_waves)
GRIDS = ((8100, 256, 5, 0, 5), (100, 256, 5, 0, 5), (8100, 256, 4, 0, 3), (8100, 16, 4, 32, 4), (8100, 13, 5, 32, 5), (8100, 256, 5, 32, 5),
         (8100, 256, 4, 32, 3), (40, 13, 5, 32, 5))

MAIN = r"""
#include <stdio.h>
#include "mitsuba2_amd/csrc/render_plan.h"
int main() {
    const unsigned jmins[] = { @JMIN@ }, pieces[] = { @PIECES@ }, queues[] = { @QUEUES@ };
    const size_t dyn[] = { @LDS_DYN@ };
    const unsigned grids[][5] = { @GRIDS@ };
    for (unsigned spp = 1; spp <= 600; ++spp) for (unsigned j : jmins) {
        const miw_plan::ChunkSchedule s = miw_plan::chunk_schedule(spp, j);
        printf("C %u %u %u %u %llu\n", spp, j, s.job_min, s.job_pow, (unsigned long long) s.chunks);
    }
    for (unsigned n : pieces) for (unsigned q : queues) {
        std::vector<uint32_t> list(3, 7u);                       // (a refusal leaves the list alone)
        const uint32_t nq = miw_plan::deal_pieces(n, q, @SLOTS@, list);
        printf("D %u %u %u", n, q, nq); for (uint32_t v : list) printf(" %u", v); printf("\n");
    }
    for (size_t d : dyn) printf("L %zu %u\n", d, miw_plan::lds_workgroups(d));
    for (const unsigned *g : grids) printf("G %u %u %u %u %u %u\n", g[0], g[1], g[2], g[3], g[4], miw_plan::persistent_grid(g[0], g[1], g[2], g[3], g[4]));
    printf("W %u %u %u\n", miw_plan::persistent_wg_per_cu(false, 5), miw_plan::persistent_wg_per_cu(false, 3), miw_plan::persistent_wg_per_cu(true, 5));
    printf("E %d %d\n", (int) miw_plan::chunks_enough(19660, 4, 64), (int) miw_plan::chunks_enough(19661, 4, 64));
    printf("P %d %d %d %d\n", (int) miw_plan::place_window(2047, 4, 64), (int) miw_plan::place_window(2048, 4, 64), (int) miw_plan::place_window(16384, 4, 64), (int) miw_plan::place_window(16385, 4, 64));
    // phased: its waves; trees: tree_waves; plain-diffuse packets: five up to 32 triangles unless the shard form, else four; other packets: packet_waves_all
    printf("R %u %u %u %u %u %u\n", miw_plan::res_waves_compiled(true, 4, false, false, false, false, 3, 5, 4), miw_plan::res_waves_compiled(false, 4, false, false, false, false, 3, 5, 4),
           miw_plan::res_waves_compiled(false, 4, true, true, true, false, 3, 5, 4), miw_plan::res_waves_compiled(false, 4, true, true, true, true, 3, 5, 4),
           miw_plan::res_waves_compiled(false, 4, true, true, false, false, 3, 5, 4), miw_plan::res_waves_compiled(false, 4, true, false, true, false, 3, 5, 3));
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("render_plan")
    main = MAIN
    for key, val in (("JMIN", JMIN), ("PIECES", PIECES), ("QUEUES", QUEUES), ("LDS_DYN", LDS_DYN)):
        main = main.replace("@%s@" % key, ", ".join(str(v) for v in val))
    main = main.replace("@GRIDS@", ", ".join("{ %s }" % ", ".join(str(v) for v in g) for g in GRIDS)).replace("@SLOTS@", str(SLOTS))
    (d / "main.cpp").write_text(main)
    subprocess.check_call([build.CXX, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")])
    out = {}
    for line in subprocess.run([str(d / "plan")], capture_output=True, text=True, check=True).stdout.splitlines():
        out.setdefault(line[0], []).append([int(x) for x in line.split()[1:]])
    return out


# ---- chunk schedule ----------------------------------------------------------------------------------------------------------------

def device_chunks(spp, job_min):
    """the chunks a lane's walk through one pixel produces (resident_kernel.h: QueueWork::job_end, called after every finished sample): a chunk
    ends at sample index i where the samples still to do, spp - i, are a power of two >= job_min; the pixel's end ends the last"""
    sizes, start = [], 0
    for i in range(1, spp):
        r = spp - i
        if r & (r - 1) == 0 and r >= job_min:
            sizes.append(i - start)
            start = i
    return sizes + [spp - start]


def host_job_min(jmin):
    """MIW_JOB_CHUNK as the host passes it on: a value that is no power of two (and 0) means no chunk jobs"""
    return jmin if jmin and jmin & (jmin - 1) == 0 else 0


def test_chunk_schedule_is_the_devices_walk(rows):
    table = {(spp, j): (job_min, job_pow, chunks) for spp, j, job_min, job_pow, chunks in rows["C"]}
    assert sorted(table) == [(spp, j) for spp in SPP for j in JMIN]
    for (spp, j), (job_min, job_pow, chunks) in table.items():
        assert job_min == host_job_min(j), (spp, j)
        assert job_pow < max(spp, 2) and 2 * job_pow >= spp and job_pow & (job_pow - 1) == 0, (spp, j, job_pow)     # the largest power of two below spp
        if not job_min:
            assert chunks == 1, (spp, j)                                  # no chunk jobs
            continue
        sizes = device_chunks(spp, job_min)
        assert sum(sizes) == spp and chunks == len(sizes), (spp, j, sizes, chunks)
        # where fetch_job expects chunk j > 0 to start: spp - (job_pow >> (j - 1))
        starts = [sum(sizes[:k]) for k in range(len(sizes))]
        assert starts == [0] + [spp - (job_pow >> (k - 1)) for k in range(1, len(sizes))], (spp, j, starts)


def test_chunk_schedule_hand_checked(rows):
    table = {(spp, j): (job_min, job_pow, chunks) for spp, j, job_min, job_pow, chunks in rows["C"]}
    assert table[(512, 64)] == (64, 256, 4) and device_chunks(512, 64) == [256, 128, 64, 64]
    assert table[(16, 4)][2] == 3
    assert table[(128, 64)][2] == 2
    assert table[(100, 8)][2] == 5
    assert table[(64, 64)][2] == 1
    assert all(table[(spp, 48)][0] == 0 and table[(spp, 48)][2] == 1 for spp in SPP)      # 48 is no power of two: off


# ---- dealing -------------------------------------------------------------------------------------------------------------------------

def test_dealing(rows):
    seen = set()
    for n, q, nq, *lst in rows["D"]:
        seen.add((n, q))
        if q < 2 or q * SLOTS < n:                                        # the guard refuses: one queue, the list untouched
            assert nq == 0 and lst == [7, 7, 7], (n, q)
            continue
        assert nq == q and len(lst) == q * SLOTS, (n, q)
        dealt = [v for v in lst if v != EMPTY]
        assert sorted(dealt) == list(range(n)), (n, q)                    # every piece exactly once
        for queue in range(q):
            for r in range(SLOTS):
                v = lst[queue * SLOTS + r]
                if v != EMPTY:
                    assert v // q == r, (n, q, queue, r, v)               # slot r holds a piece of round r
        for i in range(min(n, q)):
            assert lst[i * SLOTS] == i, (n, q, i)                         # round 0: piece i to queue i
        for i in range(q, min(n, 2 * q)):
            assert lst[(q - 1 - (i - q)) * SLOTS + 1] == i, (n, q, i)     # round 1 runs in reverse
    assert seen == {(n, q) for n in PIECES for q in QUEUES}
    assert sum(1 for n, q, nq, *_ in rows["D"] if nq == 0) == 9           # 255, 256 and 1024 pieces on 2 and 3 queues, 4096 on 2, 3 and 256


# ---- LDS workgroups, persistent grid ---------------------------------------------------------------------------------------------------

def test_lds_workgroups_at_the_granule_boundaries(rows):
    got = {d: w for d, w in rows["L"]}
    for d, w in got.items():
        granules = -(-(d + 1024 + 16) // 512)                            # dynamic + static (s_job_pend 1024, s_prog 16), in granules of 512 bytes
        assert w == (160 * 1024) // (granules * 512), d
    assert got[0] == 106
    assert (got[39920], got[39921]) == (4, 3)                             # exactly 40 KB per workgroup, and one byte past it
    assert (got[31728], got[31729]) == (5, 4)                             # 32 KB: five workgroups against four
    assert got[65536] == 2


def test_persistent_grid(rows):
    got = {tuple(r[:5]): r[5] for r in rows["G"]}
    # no room: min(grid.x, cu * wg_per_cu)
    assert got[(8100, 256, 5, 0, 5)] == 1280 and got[(100, 256, 5, 0, 5)] == 100 and got[(8100, 256, 4, 0, 3)] == 1024
    # room = 32: taken from what is resident, and only where more than twice the room is there
    assert got[(8100, 16, 4, 32, 4)] == 64                                # full = 64 = 2 * room: kept whole
    assert got[(8100, 13, 5, 32, 5)] == 33                                # full = 65 > 2 * room: 65 - 32
    assert got[(8100, 256, 5, 32, 5)] == 1280 - 32
    assert got[(8100, 256, 4, 32, 3)] == 768 - 32                         # three resident per CU though four are launched per CU without room
    assert got[(40, 13, 5, 32, 5)] == 33                                  # the lanes' grid bounds it after the room is taken
    assert rows["W"] == [[5, 4, 4]]                                       # never fewer than four workgroups per CU; the direct integrator four


def test_windows_and_compiled_waves(rows):
    assert rows["E"] == [[0, 1]]                                          # 1.2 pixels per resident lane, 4 wavefronts x 64 SIMDs x 64 lanes = 16384 lanes: from 19661 pixels on
    assert rows["P"] == [[0, 1, 1, 0]]                                    # from half a pixel per SIMD lane (2048) to every pixel resident (16384)
    assert rows["R"] == [[4, 3, 5, 4, 4, 3]]
