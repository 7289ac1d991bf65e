"""csrc/film_chains.h: the chain table of the film replay in equal chains (device/film_kernels.h: k_film_chains).

A tile of the replay by texel blocks has patches x patches block positions (blocks of 4 x 4 texels over the tile's bordered side); a position's window is
the tile pixels within the filter's reach of its block, and the header packs the positions into chains no heavier than the largest window (first-fit
decreasing), one wavefront per chain. A host program built from the header prints the table over

    tile sizes 1 .. 64  x  border 0 .. 2  x  reach 0 .. 2

and the test checks that every position appears in exactly one chain, that no chain outweighs the largest window, and that the window sizes are those a
brute-force count with the kernel's `in` predicate (film_lanes_block, restated here) gives. The headline's shape (32-pixel tiles, border 2, reach 2: 9 x 9
positions) must come out as 64 chains of weight 64: 49 interior positions alone, 14 pairs of edge positions, the four corners together.
"""
import subprocess

import pytest

from conftest import ROOT
from film_chains_ref import BS, first_fit_decreasing, in_axis, window_sizes

MAIN = r"""
#include <stdio.h>
#include "mitsuba2_amd/csrc/film_chains.h"
int main() {
    for (int tile = 1; tile <= 64; ++tile) for (int border = 0; border <= 2; ++border) for (int reach = 0; reach <= 2; ++reach) {
        const unsigned patches = (unsigned) (tile + 2 * border + @BS@ - 1) / @BS@;
        const miw_chains::Table t = miw_chains::build(patches, patches, @BS@, tile, border, reach);
        const std::vector<unsigned> packed = t.packed();
        printf("T %d %d %d %u %u %u\n", tile, border, reach, patches, t.cap, t.chains());
        printf("W"); for (unsigned w : t.weight) printf(" %u", w); printf("\n");
        printf("P"); for (unsigned v : packed) printf(" %u", v); printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("film_chains")
    (d / "main.cpp").write_text(MAIN.replace("@BS@", str(BS)))
    subprocess.check_call([build.CXX, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "chains")])
    lines = subprocess.run([str(d / "chains")], capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for i in range(0, len(lines), 3):
        tile, border, reach, patches, cap, n_chains = (int(x) for x in lines[i].split()[1:])
        weight = [int(x) for x in lines[i + 1].split()[1:]]
        packed = [int(x) for x in lines[i + 2].split()[1:]]
        start, order = packed[:n_chains + 1], packed[n_chains + 1:]          # what the kernel reads: start[0 .. chains], then the positions chain by chain
        out[(tile, border, reach)] = (patches, cap, weight, [order[start[c]:start[c + 1]] for c in range(n_chains)], order)
    return out


def _window(tile, border, reach, tx0, ty0):
    """the tile pixels the predicate accepts for the block at texel (tx0, ty0), pixel by pixel"""
    return sum(1 for y in range(tile) for x in range(tile) if in_axis(tile, border, reach, tx0, x) and in_axis(tile, border, reach, ty0, y))


def test_every_shape_is_there(tables):
    assert sorted(tables) == [(t, b, r) for t in range(1, 65) for b in range(3) for r in range(3)]


def test_every_position_is_in_exactly_one_chain(tables):
    for key, (patches, cap, weight, chains, order) in tables.items():
        assert len(weight) == patches * patches, key
        assert sorted(order) == list(range(patches * patches)), key
        assert sum(len(c) for c in chains) == patches * patches and all(len(c) >= 1 for c in chains), key


def test_no_chain_outweighs_the_largest_window(tables):
    for key, (patches, cap, weight, chains, order) in tables.items():
        assert cap == max(weight) and cap >= 1, key
        assert cap <= 64, key                                            # (the kernel's window list holds 64 pixels)
        for c in chains:
            assert sum(weight[p] for p in c) <= cap, (key, c)


def test_window_sizes_are_the_kernels(tables):
    for (tile, border, reach), (patches, cap, weight, chains, order) in tables.items():
        assert weight == window_sizes(tile, border, reach), (tile, border, reach)      # counted per axis ...
        if tile <= 12 or tile in (32, 64):                               # ... and, where that is quick, the whole window
            want = [_window(tile, border, reach, (p % patches) * BS, (p // patches) * BS) for p in range(patches * patches)]
            assert weight == want, (tile, border, reach)


def test_first_fit_decreasing_with_ties_by_position(tables):
    for key, (patches, cap, weight, chains, order) in tables.items():
        assert chains == first_fit_decreasing(weight), key


def test_headline_shape_is_64_chains_of_64(tables):
    patches, cap, weight, chains, order = tables[(32, 2, 2)]
    assert patches == 9 and cap == 64 and len(chains) == 64
    assert all(sum(weight[p] for p in c) == 64 for c in chains)
    edge = lambda p: (p % 9 in (0, 8)) + (p // 9 in (0, 8))            # 0: interior, 1: edge, 2: corner
    singles = [c for c in chains if len(c) == 1]
    pairs = [c for c in chains if len(c) == 2]
    fours = [c for c in chains if len(c) == 4]
    assert (len(singles), len(pairs), len(fours)) == (49, 14, 1)
    assert all(edge(c[0]) == 0 and weight[c[0]] == 64 for c in singles)
    assert all(edge(p) == 1 and weight[p] == 32 for c in pairs for p in c)
    assert sorted(fours[0]) == [0, 8, 72, 80] and all(weight[p] == 16 for p in fours[0])
