// mi_render_aov: the aov integrator's frame (include/miwave.h). Host side; part of the translation unit csrc/miwave.hip (included
// there inside its extern "C" block, after mi_render and mi_sample, whose internals it calls; not a stand-alone header).
//
// A frame is assembled in groups of tiles whose sample log fits MIW_AOV_LOG_BYTES: per group k_init_pixels (the render kernels' pixel
// map and seeds), then the samples — without a child k_aov_samples over [j, j + samples_per_launch), with one the round
// k_aov_samples [j, j + 1) -> k_sample_rays (mi_sample's launch for device-resident rays, its usual Mats choice) -> k_aov_finish per
// sample —, then k_aov_film replays the group's blocks into their tiles; k_aov_film_merge sums the tiles into the film at the end.
// Every buffer is a temporary of the call: nothing of the context's render state is touched (cfg->profile writes times into mi_counters).
#ifndef MIW_AOV_LOG_BYTES
#define MIW_AOV_LOG_BYTES ((size_t) 1 << 31)
#endif

static std::string aov_cfg_problem(const mi_aov_cfg *a) {
    char buf[200];
    if (a->struct_size != sizeof(mi_aov_cfg)) {
        snprintf(buf, sizeof buf, "mi_render_aov: unknown mi_aov_cfg::struct_size %u (this library: %zu)", a->struct_size, sizeof(mi_aov_cfg));
        return buf;
    }
    if (a->n_types > MI_AOV_MAX_TYPES) {
        snprintf(buf, sizeof buf, "mi_render_aov: %u AOV types (at most %d)", a->n_types, MI_AOV_MAX_TYPES);
        return buf;
    }
    for (uint32_t i = 0; i < a->n_types; ++i)
        if (aov_type_channels(a->types[i]) == 0u) {
            snprintf(buf, sizeof buf, "mi_render_aov: Invalid AOV type %u (entry %u)", (unsigned) a->types[i], i);
            return buf;
        }
    if (a->nested < MI_AOV_NESTED_NONE || a->nested > MI_AOV_NESTED_DIRECT) {
        snprintf(buf, sizeof buf, "mi_render_aov: unknown nested integrator %d (served: MI_AOV_NESTED_NONE, _PATH, _DIRECT)", a->nested);
        return buf;
    }
    return std::string();
}

struct AovEvents {                                               // cfg->profile: three HIP events of the call's own
    hipEvent_t e[3] = { nullptr, nullptr, nullptr };
    ~AovEvents() { for (hipEvent_t x : e) if (x) (void) hipEventDestroy(x); }
};

int32_t mi_aov_channel_count(const mi_aov_cfg *a) {
    if (!a || !aov_cfg_problem(a).empty()) return 0;
    return (int32_t) (MIW_FILM_CHANNELS + aov_channels(a->types, a->n_types) + (a->nested != MI_AOV_NESTED_NONE ? 4u : 0u));
}

mi_status mi_render_aov(mi_ctx *c, const mi_render_cfg *cfg, const mi_aov_cfg *aov, void *film) {
    if (!aov) return MI_ERR_INVALID;
    {
        const std::string why = aov_cfg_problem(aov);
        if (!why.empty()) { if (c) c->error = why; else g_global_error = why; return MI_ERR_INVALID; }
    }
    if (!c || !cfg || !film) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_render_aov: call mi_scene_upload and mi_bvh_build first");
    if (cfg->tile_list) return fail(c, MI_ERR_INVALID, "mi_render_aov: a frame with AOV channels is rendered by one context; tile shards (world > 1) are not served");
    const bool child = aov->nested != MI_AOV_NESTED_NONE;
    RenderParams PC;                                             // the child's sample(): what mi_sample builds from a mi_sample_cfg
    memset(&PC, 0, sizeof PC);
    if (child) {
#if MIW_SPECTRAL
        return fail(c, MI_ERR_INVALID, "mi_render_aov: a nested integrator is served by the scalar_rgb library only (its .R .G .B need pdf_rgb_spectrum and xyz_to_srgb)");
#endif
        mi_sample_cfg sc = aov->child;
        sc.integrator = aov->nested == MI_AOV_NESTED_PATH ? MI_INTEGRATOR_PATH : MI_INTEGRATOR_DIRECT;
        const std::string why = sample_cfg_problem(&sc);
        if (!why.empty()) return fail(c, MI_ERR_INVALID, "mi_render_aov: child: %s", why.c_str());
        PC.spp = 1u; PC.max_depth = sc.max_depth; PC.rr_depth = sc.rr_depth;
        if (sc.integrator == MI_INTEGRATOR_DIRECT) { PC.integrator = INTEG_DIRECT; direct_constants(PC.direct, sc.emitter_samples, sc.bsdf_samples, sc.hide_emitters != 0); }
    }
    mi_render_cfg base = *cfg;                                   // camera, film and filter; the integrator fields are not this entry point's
    base.integrator = MI_INTEGRATOR_PATH; base.max_depth = -1; base.rr_depth = 5; base.moment_pass = MI_MOMENT_OFF;
    RenderParams P;
    { const mi_status st = fill_params(c, &base, P); if (st != MI_OK) return st; }
    P.film.warn_negative = 0u;                                   // integrator.cpp:113: has_aovs
    const uint32_t bs = (uint32_t) cfg->block_size, bs2 = bs * bs;
    uint32_t bs2_log2 = 0; while ((1u << bs2_log2) < bs2) ++bs2_log2;
    const uint32_t blocks_x = (cfg->crop_w + bs - 1) / bs, blocks_y = (cfg->crop_h + bs - 1) / bs, n_tiles = blocks_x * blocks_y;
    if (!cfg->block_ids || cfg->block_count != n_tiles) return fail(c, MI_ERR_INVALID, "mi_render_aov: block_ids must hold %u entries", n_tiles);
    if ((uint64_t) n_tiles * bs2 >= (1ull << 31)) return fail(c, MI_ERR_INVALID, "mi_render_aov: too many lanes");
    const uint32_t n_geo = aov_channels(aov->types, aov->n_types), nch = (uint32_t) mi_aov_channel_count(aov), stride = MIW_AOV_LOG_HEAD + nch - MIW_FILM_CHANNELS;
    const uint32_t spp = cfg->spp;
    const size_t film_n = (size_t) cfg->crop_w * cfg->crop_h * nch;

    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const auto wall0 = std::chrono::steady_clock::now();
    c->cancel.store(0);
    auto stop_requested = [&]() {
        return c->cancel.load() != 0 || (cfg->timeout_s > 0.f && std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() > cfg->timeout_s);
    };

    // tiles per group: the group's log within MIW_AOV_LOG_BYTES (one tile at least)
    const size_t tile_log = (size_t) bs2 * std::max<uint32_t>(spp, 1u) * stride * sizeof(float);
    const uint32_t group = (uint32_t) std::max<size_t>(1, std::min<size_t>(n_tiles, MIW_AOV_LOG_BYTES / tile_log));
    const uint32_t group_lanes = group * bs2, side = bs + 2u * (uint32_t) cfg->filter_border;

    TmpBuf<U4> d_st; TmpBuf<uint32_t> d_pixel, d_block_ids, d_iota; TmpBuf<int32_t> d_block_tile; TmpBuf<float> d_log, d_tiles, d_film, d_rays, d_spec;
    TmpBuf<uint8_t> d_types, d_valid; TmpBuf<uint64_t> d_rng; TmpBuf<FilmRec> d_filmrec;
    HIP_TRY(c, d_st.resize(group_lanes)); HIP_TRY(c, d_pixel.resize(group_lanes));
    HIP_TRY(c, d_log.resize((size_t) group_lanes * std::max<uint32_t>(spp, 1u) * stride));
    HIP_TRY(c, d_block_ids.resize(n_tiles)); HIP_TRY(c, d_block_tile.resize(n_tiles));
    HIP_TRY(c, d_tiles.resize((size_t) n_tiles * side * side * nch));
    HIP_TRY(c, d_types.resize(MI_AOV_MAX_TYPES)); HIP_TRY(c, d_filmrec.resize(1));
    HIP_TRY(c, hipMemcpyAsync(d_block_ids.p, cfg->block_ids, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    std::vector<int32_t> block_tile(n_tiles);                    // (host vectors outlive the copies: the stream is synchronised before they go)
    for (uint32_t t = 0; t < n_tiles; ++t) block_tile[t] = (int32_t) t;
    HIP_TRY(c, hipMemcpyAsync(d_block_tile.p, block_tile.data(), n_tiles * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, d_iota.resize(n_tiles));
    HIP_TRY(c, hipMemcpyAsync(d_iota.p, block_tile.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipMemcpyAsync(d_types.p, aov->types, MI_AOV_MAX_TYPES, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_filmrec.p, &P.film, sizeof(FilmRec), hipMemcpyHostToDevice, s));
    if (child) {
        HIP_TRY(c, d_rays.resize((size_t) 8 * group_lanes)); HIP_TRY(c, d_spec.resize((size_t) MIW_SPEC_N * group_lanes));
        HIP_TRY(c, d_valid.resize(group_lanes)); HIP_TRY(c, d_rng.resize(group_lanes));
        HIP_TRY(c, c->d_next_ray.resize(1));
    }
    float *film_dev = (float *) film;
    if (!cfg->film_on_device) {
        HIP_TRY(c, d_film.resize(film_n));
        film_dev = d_film.p;
        if (cfg->accumulate) HIP_TRY(c, hipMemcpyAsync(film_dev, film, film_n * sizeof(float), hipMemcpyHostToDevice, s));
    }

    BlockReplayArgsN R;
    R.log = d_log.p; R.stride = stride; R.nch = nch; R.spp = spp;
    R.block_ids = d_block_ids.p; R.block_tile = d_block_tile.p; R.tile_list = nullptr;
    R.blocks_x = blocks_x; R.blocks_y = blocks_y; R.bs2_log2 = bs2_log2; R.tile_stride = side * side * nch; R.tile0 = 0;
    const bool tiny = c->lds_cfg.brute != 0, analytic = !c->rects.empty();
    const uint32_t per_launch = child ? 1u : (cfg->samples_per_launch > 0 ? (uint32_t) cfg->samples_per_launch : std::max<uint32_t>(spp, 1u));

    // cfg->profile: time per launch class into mi_counters — ms_path: k_init_pixels + the sample rounds (k_aov_samples, with a child
    // k_sample_rays and k_aov_finish too), ms_film_blocks: k_aov_film, ms_film_merge: k_aov_film_merge; ms_render: the call's wall time
    const bool prof = cfg->profile != 0;
    AovEvents ev; double ms_samples = 0.0, ms_film = 0.0, ms_merge = 0.0;
    if (prof) for (hipEvent_t &x : ev.e) HIP_TRY(c, hipEventCreate(&x));
    auto add_ms = [&](double &sum, hipEvent_t a, hipEvent_t b) { float ms = 0.f; if (hipEventElapsedTime(&ms, a, b) == hipSuccess) sum += ms; };

    bool stopped = false;
    for (uint32_t tile0 = 0; tile0 < n_tiles && !stopped; tile0 += group) {
        const uint32_t tiles_here = std::min(group, n_tiles - tile0), lanes = tiles_here * bs2;
        RenderParams PG = P; PG.n_lanes = lanes;
        InitArgs I; I.block_ids = d_block_ids.p; I.tile_list = nullptr; I.blocks_x = blocks_x; I.blocks_y = blocks_y; I.bs = bs; I.bs2_log2 = bs2_log2; I.base_seed = cfg->base_seed;
        I.tile_list = d_iota.p + tile0;                           // the group's tiles are the blocks tile0 ...
        AovArgs A;
        A.st = d_st.p; A.pixel = d_pixel.p; A.log = d_log.p; A.types = d_types.p;
        A.n_lanes = lanes; A.spp = spp; A.stride = stride; A.n_types = aov->n_types; A.n_geo = n_geo;
        for (int k = 0; k < 8; ++k) A.ray[k] = child ? d_rays.p + (size_t) k * group_lanes : nullptr;
        A.rng_state = child ? d_rng.p : nullptr;
        if (prof) HIP_TRY(c, hipEventRecord(ev.e[0], s));
        hipLaunchKernelGGL(k_init_pixels, dim3((lanes + MIW_BLOCK - 1) / MIW_BLOCK), dim3(MIW_BLOCK), 0, s, PG, d_st.p, d_pixel.p, I);
        HIP_TRY(c, hipGetLastError());
        for (uint32_t j = 0; j < spp; j += per_launch) {
            if (stop_requested()) { stopped = true; break; }
            const uint32_t j1 = std::min(spp, j + per_launch);
            HIP_TRY(c, aov_launch_samples(tiny, analytic, c->lds_bytes, s, PG, c->view, A, j, j1, c->lds_cfg));
            if (child) {
                SampleIO io;
                io.R = { A.ray[0], A.ray[1], A.ray[2], A.ray[3], A.ray[4], A.ray[5], A.ray[6], A.ray[7] };
                io.wavelengths = nullptr; io.rng_state = d_rng.p; io.rng_inc = nullptr; io.spec = d_spec.p; io.valid = d_valid.p; io.n = lanes;
                const mi_status ls = sample_launch(c, PC, io, s);
                if (ls != MI_OK) return ls;
                HIP_TRY(c, aov_launch_finish(s, A, d_spec.p, d_valid.p, j));
            }
            if (cfg->timeout_s > 0.f || child) HIP_TRY(c, hipStreamSynchronize(s));   // (the stop test looks at finished work; the ray queue's counter is reused per round)
        }
        if (stopped) break;
        R.tile0 = tile0;
        if (prof) HIP_TRY(c, hipEventRecord(ev.e[1], s));
        HIP_TRY(c, aov_launch_film(s, d_filmrec.p, P.film, R, tiles_here, d_tiles.p));
        if (prof) HIP_TRY(c, hipEventRecord(ev.e[2], s));
        HIP_TRY(c, hipStreamSynchronize(s));                      // the next group overwrites the log
        if (prof) { add_ms(ms_samples, ev.e[0], ev.e[1]); add_ms(ms_film, ev.e[1], ev.e[2]); }
    }
    if (stopped) return fail(c, MI_ERR_CANCELLED, "mi_render_aov: stopped by mi_cancel or timeout_s");
    if (prof) HIP_TRY(c, hipEventRecord(ev.e[0], s));
    HIP_TRY(c, aov_launch_merge(s, d_filmrec.p, P.film, R, d_tiles.p, film_dev, cfg->accumulate != 0));
    if (prof) HIP_TRY(c, hipEventRecord(ev.e[1], s));
    if (!cfg->film_on_device) HIP_TRY(c, hipMemcpyAsync(film, film_dev, film_n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (prof) {
        add_ms(ms_merge, ev.e[0], ev.e[1]);
        mi_counters &K = c->counters;
        K.ms_path = ms_samples; K.ms_film_blocks = ms_film; K.ms_film_merge = ms_merge; K.ms_resolve = ms_film + ms_merge;
        K.ms_render = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return MI_OK;
}
