"""The chain table of the film replay (csrc/film_chains.h), restated once for the tests that need it: tests/test_film_chains_cpu.py checks the header against
this, tests/test_film_chains_gpu.py takes from it how many chains a launch must report."""

BS = 4                                                        # device/film_kernels.h: MIW_FL_BS


def patches_of(tile, border):
    """block positions per axis of a tile of `tile` pixels with its border"""
    return (tile + 2 * border + BS - 1) // BS


def in_axis(tile, border, reach, t0, x):
    """one axis of the kernel's `in` predicate (film_lanes_block): pixel x of the tile lies within reach of the block at texel t0"""
    return 0 <= x < tile and t0 - border - reach <= x <= t0 + BS - 1 - border + reach


def window_sizes(tile, border, reach):
    """[position] the tile pixels the predicate accepts, counted per axis pixel by pixel (the predicate is a conjunction of one test per axis)"""
    patches = patches_of(tile, border)
    axis = [sum(in_axis(tile, border, reach, k * BS, x) for x in range(tile)) for k in range(patches)]
    return [axis[p % patches] * axis[p // patches] for p in range(patches * patches)]


def first_fit_decreasing(weight):
    """the positions by falling weight (equal weights by rising position), each into the first chain whose sum stays within the largest weight"""
    cap, bins, sums = max(weight), [], []
    for p in sorted(range(len(weight)), key=lambda p: (-weight[p], p)):
        c = next((c for c in range(len(bins)) if sums[c] + weight[p] <= cap), None)
        if c is None:
            bins.append([]); sums.append(0); c = len(bins) - 1
        bins[c].append(p); sums[c] += weight[p]
    return bins
