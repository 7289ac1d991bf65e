// The chain table of the film replay by texel blocks (device/film_kernels.h: k_film_chains), stated once on the host.
// Plain C++17 without HIP types, so that a host program can enumerate it (tests/test_film_chains_cpu.py).
//
// k_film_lanes replays one block position of a tile (a block of BS x BS texels) per wavefront: the runs of the tile pixels within the filter's reach
// of the block. A position in the tile's interior has a full window, one at an edge or a corner a clipped one, so the wavefronts of one launch differ
// in length by up to the ratio of the largest window to the smallest (64 : 16 pixel runs for 32-pixel tiles). A CHAIN is a list of positions one
// wavefront replays one after the other; the positions are packed into chains no heavier than the heaviest single position, so that every wavefront
// of the launch has (nearly) the same number of pixel runs to read and the launch's demand on memory does not fall off while its longest chains run on.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace miw_chains {

// the tile pixels of one axis within reach of the block at texel t0 = pos * bs: exactly the pixels x of 0 .. tile_px - 1 the kernel's `in` predicate
// accepts, t0 - border - reach <= x <= t0 + bs - 1 - border + reach (tiles are squares of a power of two of pixels; the weights balance the chains, they decide
// nothing about what a position adds)
inline uint32_t axis_window(int pos, int bs, int tile_px, int border, int reach) {
    const int lo = std::max(pos * bs - border - reach, 0), hi = std::min(pos * bs + bs - 1 - border + reach, tile_px - 1);
    return hi >= lo ? (uint32_t) (hi - lo + 1) : 0u;
}

struct Table {
    uint32_t patches_x = 0, patches_y = 0;
    uint32_t cap = 0;                       // the largest window = the most a chain may weigh
    std::vector<uint32_t> weight;           // [position] pixels in its window; position = py * patches_x + px
    std::vector<uint32_t> start;            // [chain], and one more: its positions are order[start[c] .. start[c + 1])
    std::vector<uint32_t> order;            // [patches_x * patches_y] every position once, chain by chain
    uint32_t chains() const { return start.empty() ? 0u : (uint32_t) start.size() - 1u; }
    uint32_t chain_weight(uint32_t c) const { uint32_t w = 0; for (uint32_t i = start[c]; i < start[c + 1]; ++i) w += weight[order[i]]; return w; }
    // what the kernel reads: start[0 .. chains], then order[0 .. positions)
    std::vector<uint32_t> packed() const { std::vector<uint32_t> p(start); p.insert(p.end(), order.begin(), order.end()); return p; }
};

// First-fit decreasing: the positions by falling weight (equal weights by rising position), each into the first chain it fits. A chain holds as many
// positions as fit (tiny tiles: all of them may have empty windows but one).
inline Table build(uint32_t patches_x, uint32_t patches_y, int bs, int tile_px, int border, int reach) {
    Table t;
    t.patches_x = patches_x; t.patches_y = patches_y;
    const uint32_t n = patches_x * patches_y;
    t.weight.resize(n);
    for (uint32_t p = 0; p < n; ++p)
        t.weight[p] = axis_window((int) (p % patches_x), bs, tile_px, border, reach) * axis_window((int) (p / patches_x), bs, tile_px, border, reach);
    std::vector<uint32_t> by_weight(n);
    for (uint32_t p = 0; p < n; ++p) by_weight[p] = p;
    std::stable_sort(by_weight.begin(), by_weight.end(), [&](uint32_t a, uint32_t b) { return t.weight[a] > t.weight[b]; });
    t.cap = n ? t.weight[by_weight[0]] : 0u;
    std::vector<std::vector<uint32_t>> chain;
    std::vector<uint32_t> sum;
    for (uint32_t p : by_weight) {
        size_t c = 0;
        while (c < chain.size() && sum[c] + t.weight[p] > t.cap) ++c;
        if (c == chain.size()) { chain.emplace_back(); sum.push_back(0u); }
        chain[c].push_back(p); sum[c] += t.weight[p];
    }
    t.start.push_back(0u);
    for (const std::vector<uint32_t> &c : chain) { t.order.insert(t.order.end(), c.begin(), c.end()); t.start.push_back((uint32_t) t.order.size()); }
    return t;
}

}  // namespace miw_chains
