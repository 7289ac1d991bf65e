// The aov integrator's kernels (src/integrators/aov.cpp around SamplingIntegrator::render): k_aov_samples, k_aov_finish, k_aov_film,
// k_aov_film_merge and their launch functions (device/aov_launch.h).
// Compiled in csrc/miwave_aov.hip (a split build) or in csrc/miwave.hip; not a stand-alone header.
//
// k_aov_samples: a lane is a pixel of the shard's tile list, seeded as the render kernels seed it (k_init_pixels). For the samples
// [j0, j1) of its pixel it runs the camera draws (lane_begin_sample), ONE closest-hit query — the routes k_sample_rays takes: the
// staged triangle packets behind the octant leaf boxes (Tiny = 1), or the lock-step LDS-stack tree walk (Tiny = 0) —, the full surface
// interaction and the partials beside it (miw/aov.h), and writes one log record per sample (miw/film_gather_n.h) with plain vector
// stores. It evaluates no BSDF and draws nothing of its own (aov.cpp:156-254), so one instantiation serves every material class.
// The pixel's sampler state lives in AovArgs::st between launches: a frame is one launch or many.
template <int Tiny, bool Analytic>
__global__ __launch_bounds__(MIW_BLOCK, Tiny ? 4 : MIW_TREE_WAVES)
void k_aov_samples(RenderParams P, SceneView sc, AovArgs A, uint32_t j0, uint32_t j1, TraceLds cfg) {
    extern __shared__ uint4 smem[];
    stage_to_lds(sc, cfg, smem);
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= A.n_lanes) return;
    U4 st = A.st[lane];
    const bool live = !(st.z & LF_DONE);
    const uint32_t pixel = A.pixel[lane];
    LaneRegs L;
    L.rng.state = (uint64_t) st.x | ((uint64_t) st.y << 32); L.rng.inc = MIW_PCG32_SCALAR_INC;
    for (uint32_t j = j0; j < j1; ++j) {
        if (live) { L.sample_idx = j; lane_begin_sample(P, pixel, L, j1); }         // integrator.cpp:233-261: three draws, sensor_sample_ray
        else {                                                                      // a lane outside the film: the ray through the film's centre, traced for nothing
            L.ray = sensor_sample_ray(P.sensor, v2(.5f, .5f), v3(P.cam_o[0], P.cam_o[1], P.cam_o[2]));
            L.pos = v2(0.f, 0.f);
        }
        const V3 o = L.ray.o, d = L.ray.d;
        if (A.rng_state) {                                                          // what the child's sample() receives: the same ray, the same sampler
            A.ray[0][lane] = o.x; A.ray[1][lane] = o.y; A.ray[2][lane] = o.z; A.ray[3][lane] = d.x; A.ray[4][lane] = d.y; A.ray[5][lane] = d.z;
            A.ray[6][lane] = L.ray.mint; A.ray[7][lane] = L.ray.maxt;
            A.rng_state[lane] = L.rng.state;
        }
        F4 h; bool occ;
        trace2<Tiny, Analytic>(sc, cfg, smem, o, L.ray.mint, d, L.ray.maxt, live, d, L.ray.maxt, false, h, occ);   // scene->ray_intersect(ray), aov.cpp:166
        if (!live) continue;
        const uint32_t tri = f2u(h.w);
        const bool valid = tri != MIW_MISS;
        SurfaceInteraction si; AovPartials pt;
        si.t = 0.f; si.p = si.n = si.sh.n = v3(0.f); si.uv = v2(0.f, 0.f); pt.dp_du = pt.dp_dv = v3(0.f);
        if (valid) {
            uint32_t bsdf_index; int32_t emitter;
            hit_surface_interaction<Analytic, true>(sc, tri, h.x, h.y, h.z, [o]() { return o; }, d, si, bsdf_index, emitter);
            pt = aov_hit_partials<Analytic>(sc, tri, si);
        }
        float *rec = A.log + ((size_t) lane * A.spp + j) * A.stride;
        rec[1] = L.pos.y; rec[2] = rec[3] = rec[4] = rec[5] = 0.f;                  // no child: (Spectrum, Mask) = (0, false), aov.cpp:164
        aov_fill(si, pt, valid, A.types, A.n_types, rec + MIW_AOV_LOG_HEAD);
        bool ok = true;                                                             // imageblock.cpp:85-109, warn_negative = false: all channels together
        for (uint32_t k = 0; k < A.n_geo; ++k) ok = ok && isfinite_(rec[MIW_AOV_LOG_HEAD + k]);
        rec[0] = ok ? L.pos.x : __builtin_nanf("");
    }
    if (live) { st.x = (uint32_t) L.rng.state; st.y = (uint32_t) (L.rng.state >> 32); st.w = j1; A.st[lane] = st; }
}

#if !MIW_SPECTRAL
// k_aov_finish: sample j of every pixel after the child's k_sample_rays — X Y Z as lane_finish_sample forms them (integrator.cpp:272-273),
// A from the mask, the child's .R .G .B (the raw spectrum in scalar_rgb) .A behind the geometric channels (aov.cpp:221-249), the
// finiteness test over all channels of the sample, and the sampler state handed on to sample j + 1.
__global__ __launch_bounds__(MIW_BLOCK) void k_aov_finish(AovArgs A, const float *spec, const uint8_t *valid, uint32_t j) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= A.n_lanes) return;
    U4 st = A.st[lane];
    if (st.z & LF_DONE) return;
    const V3 res = v3(spec[3 * (size_t) lane], spec[3 * (size_t) lane + 1], spec[3 * (size_t) lane + 2]);
    const V3 xyz = srgb_to_xyz(res);
    const float a = valid[lane] ? 1.f : 0.f;
    float *rec = A.log + ((size_t) lane * A.spp + j) * A.stride;
    float *child = rec + MIW_AOV_LOG_HEAD + A.n_geo;
    rec[2] = xyz.x; rec[3] = xyz.y; rec[4] = xyz.z; rec[5] = a;
    child[0] = res.x; child[1] = res.y; child[2] = res.z; child[3] = a;
    const bool ok = rec[0] == rec[0] && isfinite_(xyz.x) && isfinite_(xyz.y) && isfinite_(xyz.z) && isfinite_(res.x) && isfinite_(res.y) && isfinite_(res.z);
    if (!ok) rec[0] = __builtin_nanf("");
    const uint64_t state = A.rng_state[lane];
    st.x = (uint32_t) state; st.y = (uint32_t) (state >> 32); A.st[lane] = st;
}
#endif

// k_aov_film: film_block_replay_n (miw/film_gather_n.h) lane-parallel. A thread owns one texel of one bordered block and eight of its
// channels; it GATHERS: the pixels of the block whose samples can reach the texel, in Morton order, each pixel's samples front to back,
// the weight by ImageBlock::put's expressions for exactly this texel — the float32 sums the portable scatter form builds, term for
// term in the same order. No atomics, no LDS; a block tile is written once.
#define MIW_AOV_FILM_CHANNELS 8u         /* channels a thread of k_aov_film accumulates (registers; the position and the weights are formed once for them) */
MIW_HD uint32_t morton_spread1(uint32_t x) {
    x &= 0x0000ffffu;
    x = (x | (x << 8)) & 0x00ff00ffu; x = (x | (x << 4)) & 0x0f0f0f0fu; x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__global__ __launch_bounds__(MIW_BLOCK) void k_aov_film(const FilmRec *fp, BlockReplayArgsN a, float *tiles) {
    const FilmRec &f = *fp;
    const uint32_t tile = a.tile0 + blockIdx.y, b = a.tile_list ? a.tile_list[tile] : tile;
    const BlockGeom g = block_geom(f, a.blocks_x, b);
    const int t = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= g.size_x * g.size_y) return;
    const int tx = t % g.size_x, ty = t / g.size_x;
    const uint32_t k0 = blockIdx.z * MIW_AOV_FILM_CHANNELS, nch = a.nch;
    float acc[MIW_AOV_FILM_CHANNELS];
    for (uint32_t c = 0; c < MIW_AOV_FILM_CHANNELS; ++c) acc[c] = 0.f;
    const bool one = splat_one_texel(f);
    // a sample of the pixel at texel tp has its block-local position in [tp - .5, tp + .5] (float32 rounding included), so its footprint
    // [ceil(pos - r), floor(pos + r)] lies inside [tp - floor(r + .5), tp + floor(r + .5)]: 5 x 5 pixels for r = 2, 3 x 3 for the box filter
    const int n = splat_count(f), reach = floor2int(f.radius + .5f);
    const float radius = f.radius;
    // the pixels (block-local) whose footprint can hold this texel, visited in ascending Morton code
    int x_lo = tx - f.border - reach, x_hi = tx - f.border + reach, y_lo = ty - f.border - reach, y_hi = ty - f.border + reach;
    if (x_lo < 0) x_lo = 0;
    if (y_lo < 0) y_lo = 0;
    if (x_hi > g.bw - 1) x_hi = g.bw - 1;
    if (y_hi > g.bh - 1) y_hi = g.bh - 1;
    if (x_lo <= x_hi && y_lo <= y_hi) {
        const float org_x = (float) (g.px0 + f.crop_x - f.border) + .5f, org_y = (float) (g.py0 + f.crop_y - f.border) + .5f;   // imageblock.cpp:114
        const uint32_t q_lo = morton_spread1((uint32_t) x_lo) | (morton_spread1((uint32_t) y_lo) << 1),
                       q_hi = morton_spread1((uint32_t) x_hi) | (morton_spread1((uint32_t) y_hi) << 1);
        for (uint32_t q = q_lo; q <= q_hi; ++q) {
            uint32_t x, y;
            morton_decode2(q, x, y);
            if ((int) x < x_lo || (int) x > x_hi || (int) y < y_lo || (int) y > y_hi) continue;
            const uint32_t lane = (blockIdx.y << a.bs2_log2) + q;
            const float *run = a.log + (size_t) lane * a.spp * a.stride;
            for (uint32_t j = 0; j < a.spp; ++j) {
                const float *rec = run + (size_t) j * a.stride;
                const float px = rec[0];
                if (!(px == px)) continue;                    // rejected sample
                const float posx = px - org_x, posy = rec[1] - org_y;
                float weight = 1.f;
                if (!one) {
                    int lo_x = ceil2int(posx - radius), lo_y = ceil2int(posy - radius);
                    if (lo_x < 0) lo_x = 0;
                    if (lo_y < 0) lo_y = 0;
                    int hi_x = floor2int(posx + radius), hi_y = floor2int(posy + radius);
                    if (hi_x > g.size_x - 1) hi_x = g.size_x - 1;
                    if (hi_y > g.size_y - 1) hi_y = g.size_y - 1;
                    const int xr = tx - lo_x, yr = ty - lo_y;
                    if (xr < 0 || yr < 0 || xr >= n || yr >= n || tx > hi_x || ty > hi_y) continue;
                    const float wx = filter_eval_discretized(f, ((float) lo_x - posx) + (float) xr),
                                wy = filter_eval_discretized(f, ((float) lo_y - posy) + (float) yr);
                    weight = wy * wx;
                } else if (ceil2int(posx - .5f) != tx || ceil2int(posy - .5f) != ty) continue;
                // (the one-texel branch adds the value itself, imageblock.cpp:163-170: no product)
#pragma unroll
                for (uint32_t c = 0; c < MIW_AOV_FILM_CHANNELS; ++c)
                    if (k0 + c < nch) { const float v = aov_log_value(rec, k0 + c); acc[c] += one ? v : v * weight; }
            }
        }
    }
    float *dst = tiles + (size_t) tile * a.tile_stride + (size_t) t * nch;
#pragma unroll
    for (uint32_t c = 0; c < MIW_AOV_FILM_CHANNELS; ++c)
        if (k0 + c < nch) dst[k0 + c] = acc[c];
}

// the block -> film step: one thread per film texel and channel (film_merge_channel_n)
__global__ __launch_bounds__(MIW_BLOCK) void k_aov_film_merge(const FilmRec *fp, BlockReplayArgsN a, const float *tiles, float *film, uint32_t accumulate) {
    const FilmRec &f = *fp;
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x, total = (size_t) f.crop_w * f.crop_h * a.nch;
    if (i >= total) return;
    const uint32_t k = (uint32_t) (i % a.nch); const size_t texel = i / a.nch;
    const float v = film_merge_channel_n(f, a, tiles, (int) (texel % (size_t) f.crop_w), (int) (texel / (size_t) f.crop_w), k, accumulate ? film[i] : 0.f);
    film[i] = v;
}

// ---- launch functions (device/aov_launch.h) ----
hipError_t aov_launch_samples(bool tiny, bool analytic, size_t lds_bytes, hipStream_t s, const RenderParams &P, const SceneView &sc, const AovArgs &A,
                              uint32_t j0, uint32_t j1, const TraceLds &cfg) {
    const dim3 grid((A.n_lanes + MIW_BLOCK - 1) / MIW_BLOCK), block(MIW_BLOCK);
    if (tiny) hipLaunchKernelGGL((k_aov_samples<1, false>), grid, block, lds_bytes, s, P, sc, A, j0, j1, cfg);
    else if (analytic) hipLaunchKernelGGL((k_aov_samples<0, true>), grid, block, lds_bytes, s, P, sc, A, j0, j1, cfg);
    else hipLaunchKernelGGL((k_aov_samples<0, false>), grid, block, lds_bytes, s, P, sc, A, j0, j1, cfg);
    return hipGetLastError();
}
hipError_t aov_launch_finish(hipStream_t s, const AovArgs &A, const float *spec, const uint8_t *valid, uint32_t j) {
#if !MIW_SPECTRAL
    hipLaunchKernelGGL(k_aov_finish, dim3((A.n_lanes + MIW_BLOCK - 1) / MIW_BLOCK), dim3(MIW_BLOCK), 0, s, A, spec, valid, j);
    return hipGetLastError();
#else
    (void) s; (void) A; (void) spec; (void) valid; (void) j;
    return hipErrorNotSupported;
#endif
}
hipError_t aov_launch_film(hipStream_t s, const FilmRec *film_dev, const FilmRec &fh, const BlockReplayArgsN &a, uint32_t n_tiles, float *tiles) {
    const uint32_t side = (uint32_t) (fh.block_size + 2 * fh.border), texels = side * side;
    const dim3 grid((texels + MIW_BLOCK - 1) / MIW_BLOCK, n_tiles, (a.nch + MIW_AOV_FILM_CHANNELS - 1u) / MIW_AOV_FILM_CHANNELS);
    hipLaunchKernelGGL(k_aov_film, grid, dim3(MIW_BLOCK), 0, s, film_dev, a, tiles);
    return hipGetLastError();
}
hipError_t aov_launch_merge(hipStream_t s, const FilmRec *film_dev, const FilmRec &fh, const BlockReplayArgsN &a, const float *tiles, float *film, bool accumulate) {
    const size_t total = (size_t) fh.crop_w * fh.crop_h * a.nch;
    hipLaunchKernelGGL(k_aov_film_merge, dim3((unsigned) ((total + MIW_BLOCK - 1) / MIW_BLOCK)), dim3(MIW_BLOCK), 0, s, film_dev, a, tiles, film, accumulate ? 1u : 0u);
    return hipGetLastError();
}
