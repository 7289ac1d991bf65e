"""The job pool of a frame twin's wavefront on the CPU (csrc/render_plan.h: miw_plan::pool_*, the functions device/resident_kernel.h calls).

tools/job_pool_check.cpp, a host program built from the header, runs three models and prints a row per configuration:

    C  coverage    job_total in {1, 63, 64, 65, 1000, 8 294 400}  x  pool in {0, 8, 16, 32}  x  1 .. 40 wavefronts asking in a fixed pseudo-random
                   order, 1 .. 64 lanes at a time: every id in [0, job_total) served exactly once, none at or above it; a served id's ring slot
                   holds what its batch wrote there (a violation inside the program)
    P  progress    n_lanes in {64, 320} pixel slots  x  2 .. 5 chunks per pixel  x  the pools  x  fewer, as many and more wavefronts than slots:
                   lanes park a job whose predecessor has not finished; the scheduler always steps the wavefront holding the largest ids. The run
                   ends, every job ran once, every lane is exhausted
    T, S, B        a batch at and around job_total, MIW_JOB_POOL as given -> the pool, the bytes of a wavefront's block

The test restates the cursor arithmetic here, in Python, and compares; the same program runs once more under the address and undefined-behaviour
sanitizers, as a stand-alone program.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "job_pool_check.cpp")
TOTALS = (1, 63, 64, 65, 1000, 8294400)
POOLS = (0, 8, 16, 32)
DRY = 0xffffffff

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="needs the host compiler")


def _run(tmp_path_factory, name, extra, env=None):
    from mitsuba2_amd import build
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([build.CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", ROOT] + extra + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout[-1500:], out.stderr[-2000:])
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _run(tmp_path_factory, "job_pool_check", [])


@pytest.fixture(scope="module")
def rows(plain):
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    out = {}
    for line in plain.stdout.splitlines():
        if line[:2] in ("C ", "P ", "T ", "S ", "B "):
            out.setdefault(line[0], []).append([int(x) for x in line.split()[1:]])
    return out


def test_no_violation(plain):
    assert plain.returncode == 0 and plain.stdout.splitlines()[-1] == "violations 0", plain.stderr[-2000:]


def test_every_id_is_served_exactly_once(rows):
    seen = set()
    for total, pool, waves, once, asks, from_pool, beyond in rows["C"]:
        seen.add((total, pool, waves))
        assert once == total, (total, pool, waves, once)
        assert asks >= -(-total // 64)                                     # at most 64 lanes per ask
        if pool == 0:
            assert from_pool == 0 and beyond >= 1, (total, waves)           # every wavefront retires on an id past the end
        else:
            assert from_pool <= total
            if total == 8294400:
                # the pool carries its share of a long queue: an ask of 1 .. 64 lanes (32.5 on average) finds at most `pool` ids there, so at least an eighth even at 8
                # (a short queue may be gone after each wavefront's first ask, which finds the cursor empty)
                assert from_pool > total // 8, (total, pool, waves, from_pool)
    assert seen == {(t, p, w) for t in TOTALS for p in POOLS for w in range(1, 41)}


def test_progress_under_the_adversarial_scheduler(rows):
    seen = set()
    parked = 0
    for n_lanes, chunks, pool, waves, once, parks, stuck, all_out in rows["P"]:
        seen.add((n_lanes, chunks, pool, waves))
        assert (once, stuck, all_out) == (n_lanes * chunks, 0, 1), (n_lanes, chunks, pool, waves)
        if waves * 64 > n_lanes:
            assert parks > 0, (n_lanes, chunks, pool, waves)               # more lanes than slots: chunks are drawn before their predecessors end
            parked += 1
    assert seen == {(n, c, p, w) for n in (64, 320) for c in range(2, 6) for p in POOLS for w in (1, 2, n // 64, n // 64 + 3)}
    assert parked >= 2 * 4 * 4


def py_batch(base, pool, total):
    """the cursor after a draw that returned `base`: ids at or above job_total are dropped; a batch that begins there says the queue is dry"""
    return (DRY, DRY) if base >= total else (base, min(base + pool, total))


def test_batches_at_the_queues_end(rows):
    assert len(rows["T"]) == 10
    for base, pool, total, asking, nxt, end, dry, take, after, slot in rows["T"]:
        want = py_batch(base, pool, total)
        assert (nxt, end) == want and dry == (want[0] == DRY), (base, pool, total)
        want_take = 0 if dry else min(asking, want[1] - want[0])
        assert take == want_take and after == (nxt + want_take) % 2 ** 32, (base, pool, total, asking)
        assert slot == nxt % pool
    by = {tuple(r[:3]): r for r in rows["T"]}
    assert by[(176, 32, 192)][4:6] == [176, 192] and by[(192, 32, 192)][6] == 1 and by[(0, 8, 1)][4:8] == [0, 1, 0, 1]     # hand-checked: cut at job_total, dry, a queue of one


def test_pool_option_and_block_bytes(rows):
    assert {g: p for g, p in rows["S"]} == {-1: 0, 0: 0, 1: 0, 2: 2, 3: 0, 8: 8, 16: 16, 24: 0, 32: 32, 64: 0, 65: 0, 128: 0}
    # cursor 8 B + the pool's size in 8 B + three 8-byte counters + 8 B spare, then 16 B + 4 B per pooled id; four wavefronts per workgroup
    assert rows["B"] == [[p, 48 + 20 * p, 4 * (48 + 20 * p)] for p in POOLS]
    assert rows["B"][-1][2] == 2752


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory, plain):
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded and asks nothing of what its environment preloads)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = _run(tmp_path_factory, "job_pool_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                                                       "-static-libasan", "-static-libubsan"], env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout == plain.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
