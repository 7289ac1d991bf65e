// Ordered film assembly for N channels — the order contract of film_gather.h (a bordered block accumulates in float32, its
// pixels in Morton order, each pixel's samples front to back; a film texel sums the block partials that cover it in ascending
// spiral id) for the films of integrators with AOV channels (integrator.cpp:67-73: X Y Z A W + aov_names()).
//
// The log it reads is the aov integrator's: [pixel lane][sample], `stride` floats per record,
//   rec[0..1]  position_sample (x = NaN: the sample was rejected by ImageBlock::put, imageblock.cpp:85-109 — with AOVs only the
//              finiteness test remains, and it covers all channels of the sample together)
//   rec[2..5]  X Y Z A
//   rec[6.. ]  the nch - 5 AOV channels
// and the value ImageBlock::put receives is X Y Z A 1 aov... (W is the constant 1). MIW_FILM_CHANNELS and the five-channel
// functions of film.h / film_gather.h stay as they are; with nch = 5 the functions below compute what those compute, bit for bit
// (tests/test_aov.py). The device's k_aov_film (device/aov_kernel.h) is the lane-parallel re-expression of film_block_replay_n.
#pragma once
#include "base.h"
#include "rng.h"
#include "film.h"
#include "film_gather.h"

namespace miw {

#define MIW_AOV_LOG_HEAD 6u              /* floats of a record in front of the AOV channels: position, X Y Z A */

// channel k of the value a log record stands for
MIW_HD float aov_log_value(const float *rec, uint32_t k) { return k < 4u ? rec[2u + k] : k == 4u ? 1.f : rec[1u + k]; }

struct BlockReplayArgsN {
    const float *log; uint32_t stride, nch, spp;    // [lane][sample], every pixel inside the film has `spp` records
    const uint32_t *block_ids;                      // row-major block -> spiral id
    const int32_t *block_tile;                      // row-major block -> tile index, or -1
    const uint32_t *tile_list;                      // tile -> row-major block (nullptr: identity)
    uint32_t blocks_x, blocks_y;
    uint32_t bs2_log2;                              // log2(block_size^2): lanes per tile
    uint32_t tile_stride;                           // floats per block tile: (bs + 2 * border)^2 * nch
    uint32_t tile0;                                 // the log holds the lanes of the tiles from this one on (a frame assembled in groups of tiles)
};

// ImageBlock::put (imageblock.cpp:111-170) for one axis: lo, hi and the n discretised weights, from the block-local position
struct SplatAxis { int lo, hi; float w[8]; };
MIW_HD SplatAxis splat_axis(const FilmRec &f, float pos, int size, int n) {
    SplatAxis a;
    a.lo = ceil2int(pos - f.radius); if (a.lo < 0) a.lo = 0;
    a.hi = floor2int(pos + f.radius); if (a.hi > size - 1) a.hi = size - 1;
    const float base = (float) a.lo - pos;
    for (int i = 0; i < 8; ++i) a.w[i] = i < n ? filter_eval_discretized(f, base + (float) i) : 0.f;
    return a;
}
MIW_HD int splat_count(const FilmRec &f) { int n = ceil2int((f.radius - 2.f * MIW_RAY_EPSILON) * 2.f); return n > 8 ? 8 : n; }
MIW_HD bool splat_one_texel(const FilmRec &f) { return !(f.radius > 0.5f + MIW_RAY_EPSILON); }

// block_splat() of film.h for `nch` channels: add(block_texel, channel, term), in the reference's loop order (:148-161)
template <typename Value, typename Add>
MIW_HD void block_splat_n(const FilmRec &f, int off_x, int off_y, int bw, int bh, V2 pos_, Value value, uint32_t nch, Add add) {
    const int size_x = bw + 2 * f.border, size_y = bh + 2 * f.border;
    const float posx = pos_.x - ((float) (off_x - f.border) + .5f), posy = pos_.y - ((float) (off_y - f.border) + .5f);   // :114
    if (!splat_one_texel(f)) {
        const int n = splat_count(f);
        const SplatAxis ax = splat_axis(f, posx, size_x, n), ay = splat_axis(f, posy, size_y, n);
        for (int yr = 0; yr < n; ++yr) {
            const int y = ay.lo + yr;
            bool enabled = y <= ay.hi;
            for (int xr = 0; xr < n; ++xr) {
                const int x = ax.lo + xr;
                const float weight = ay.w[yr] * ax.w[xr];
                enabled = enabled && x <= ax.hi;
                if (enabled) {
                    const int texel = y * size_x + x;
                    for (uint32_t k = 0; k < nch; ++k) add(texel, k, value(k) * weight);
                }
            }
        }
    } else {                                             // :163-170
        const int lo_x = ceil2int(posx - .5f), lo_y = ceil2int(posy - .5f);
        if (lo_x >= 0 && lo_y >= 0 && lo_x < size_x && lo_y < size_y) {
            const int texel = lo_y * size_x + lo_x;
            for (uint32_t k = 0; k < nch; ++k) add(texel, k, value(k));
        }
    }
}

// Step 1, portable: replay one block into acc[size_y * size_x * nch] (zeroed by the caller)
MIW_HD void film_block_replay_n(const FilmRec &f, const BlockReplayArgsN &a, uint32_t tile, float *acc) {
    const uint32_t b = a.tile_list ? a.tile_list[tile] : tile;
    const BlockGeom g = block_geom(f, a.blocks_x, b);
    const uint32_t bs2 = 1u << a.bs2_log2, nch = a.nch;
    for (uint32_t q = 0; q < bs2; ++q) {                  // render_block's pixel order, integrator.cpp:196-203
        uint32_t x, y;
        morton_decode2(q, x, y);
        if ((int) x >= g.bw || (int) y >= g.bh) continue;
        const uint32_t lane = ((tile - a.tile0) << a.bs2_log2) + q;
        const float *run = a.log + (size_t) lane * a.spp * a.stride;
        for (uint32_t j = 0; j < a.spp; ++j) {            // this pixel's samples, back to back
            const float *rec = run + (size_t) j * a.stride;
            if (!(rec[0] == rec[0])) continue;            // rejected sample
            block_splat_n(f, g.px0 + f.crop_x, g.py0 + f.crop_y, g.bw, g.bh, v2(rec[0], rec[1]),
                          [rec](uint32_t k) { return aov_log_value(rec, k); }, nch,
                          [acc, nch](int texel, uint32_t k, float term) { acc[(size_t) texel * nch + k] += term; });
        }
    }
}

// Step 2: channel k of film texel (fx, fy), crop-relative: the block tiles that cover it, summed in ascending spiral id
// (film_merge_texel of film_gather.h for one channel of nch). `out`: 0, or what earlier passes left in the texel (their block ids are smaller)
MIW_HD float film_merge_channel_n(const FilmRec &f, const BlockReplayArgsN &a, const float *tiles, int fx, int fy, uint32_t k, float out = 0.f) {
    const int bs = f.block_size;
    int bx_lo = (fx - f.border) / bs, bx_hi = (fx + f.border) / bs, by_lo = (fy - f.border) / bs, by_hi = (fy + f.border) / bs;
    if (fx - f.border < 0) bx_lo = 0;
    if (fy - f.border < 0) by_lo = 0;
    if (bx_hi > (int) a.blocks_x - 1) bx_hi = (int) a.blocks_x - 1;
    if (by_hi > (int) a.blocks_y - 1) by_hi = (int) a.blocks_y - 1;
    uint64_t floor_id = 0;
    for (;;) {
        uint64_t best_id = ~0ull; uint32_t best_b = 0;
        for (int by = by_lo; by <= by_hi; ++by)
            for (int bx = bx_lo; bx <= bx_hi; ++bx) {
                const uint32_t b = (uint32_t) by * a.blocks_x + (uint32_t) bx;
                if (a.block_tile[b] < 0) continue;
                const uint64_t id = a.block_ids[b];
                if (id >= floor_id && id < best_id) { best_id = id; best_b = b; }
            }
        if (best_id == ~0ull) break;
        floor_id = best_id + 1;
        const BlockGeom g = block_geom(f, a.blocks_x, best_b);
        const int tx = fx - g.px0 + f.border, ty = fy - g.py0 + f.border;
        if (tx < 0 || ty < 0 || tx >= g.size_x || ty >= g.size_y) continue;
        out += tiles[(size_t) a.block_tile[best_b] * a.tile_stride + ((size_t) ty * g.size_x + tx) * a.nch + k];   // imageblock.cpp:49-77
    }
    return out;
}

} // namespace miw
