// mi_render_sensor, mi_sensor_sample_ray: the general sensor route (include/miwave.h). Host side; part of the translation unit
// csrc/miwave.hip (included there inside its extern "C" block, after mi_render_aov, whose film launches and log budget it shares;
// not a stand-alone header).
//
// A frame is assembled in groups of tiles whose sample log fits MIW_AOV_LOG_BYTES: per group k_init_pixels (the render kernels' pixel
// map and seeds), then spp rounds of k_sensor_step -> k_sample_rays (mi_sample's launch for device-resident rays, its usual Mats
// choice) and one closing k_sensor_step, then k_aov_film replays the group's blocks into their tiles with five channels;
// k_aov_film_merge sums the tiles into the film at the end. Every buffer is a temporary of the call.
static std::string sensor_desc_problem(const mi_sensor_desc *d) {
    char buf[200];
    if (d->struct_size != sizeof(mi_sensor_desc)) {
        snprintf(buf, sizeof buf, "mi_sensor_desc: unknown struct_size %u (this library: %zu)", d->struct_size, sizeof(mi_sensor_desc));
        return buf;
    }
    if (d->type != MI_SENSOR_PERSPECTIVE && d->type != MI_SENSOR_THINLENS) {
        snprintf(buf, sizeof buf, "mi_sensor_desc: unknown type %d (served: MI_SENSOR_PERSPECTIVE, MI_SENSOR_THINLENS)", d->type);
        return buf;
    }
    if (d->type == MI_SENSOR_THINLENS) {
        if (!(d->aperture_radius > 0.f) || !std::isfinite(d->aperture_radius)) {
            snprintf(buf, sizeof buf, "mi_sensor_desc: aperture_radius must be finite and > 0 (is %g)", (double) d->aperture_radius);
            return buf;
        }
        if (!(d->focus_distance > 0.f) || !std::isfinite(d->focus_distance)) {
            snprintf(buf, sizeof buf, "mi_sensor_desc: focus_distance must be finite and > 0 (is %g)", (double) d->focus_distance);
            return buf;
        }
    }
    if (!std::isfinite(d->shutter_open) || !std::isfinite(d->shutter_open_time) || d->shutter_open_time < 0.f) {
        snprintf(buf, sizeof buf, "mi_sensor_desc: shutter_open / shutter_open_time must be finite, the time not negative");
        return buf;
    }
    return std::string();
}

static void sensor_records(const mi_render_cfg *cfg, const mi_sensor_desc *d, SensorRec &S, LensRec &L) {
    memset(&S, 0, sizeof S);
    memcpy(S.sample_to_camera, cfg->sample_to_camera, 64);
    memcpy(S.to_world, cfg->to_world, 64);
    S.near_clip = cfg->near_clip; S.far_clip = cfg->far_clip;
    S.pp_offset[0] = cfg->principal_point_offset[0]; S.pp_offset[1] = cfg->principal_point_offset[1];
    L.kind = d->type == MI_SENSOR_THINLENS ? (uint32_t) LENS_THINLENS : (uint32_t) LENS_PERSPECTIVE;
    L.aperture_radius = d->aperture_radius; L.focus_distance = d->focus_distance;
    L.draw_time = d->shutter_open_time > 0.f ? 1u : 0u;
}

struct SensorEvents {                                            // cfg->profile: HIP events of the call's own
    std::vector<hipEvent_t> e;
    ~SensorEvents() { for (hipEvent_t x : e) if (x) (void) hipEventDestroy(x); }
};

mi_status mi_render_sensor(mi_ctx *c, const mi_render_cfg *cfg, const mi_sensor_desc *desc, void *film) {
    if (!desc) return MI_ERR_INVALID;
    {
        const std::string why = sensor_desc_problem(desc);
        if (!why.empty()) { if (c) c->error = why; else g_global_error = why; return MI_ERR_INVALID; }
    }
    if (!c || !cfg || !film) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_render_sensor: call mi_scene_upload and mi_bvh_build first");
    if (cfg->tile_list) return fail(c, MI_ERR_INVALID, "mi_render_sensor: tile_list: a frame of this route is rendered by one context; tile shards (world > 1) are not served");
    if (cfg->film_f64) return fail(c, MI_ERR_INVALID, "mi_render_sensor: film_f64: the film of this route is float32, assembled in the reference's order");
    if (cfg->film_mode == 2) return fail(c, MI_ERR_INVALID, "mi_render_sensor: film_mode 2 is not served (the film is always replayed from the sample log)");
    if (cfg->plan == 1) return fail(c, MI_ERR_INVALID, "mi_render_sensor: plan 1 is not served");
    if (cfg->moment_pass != MI_MOMENT_OFF) return fail(c, MI_ERR_INVALID, "mi_render_sensor: moment_pass: the moment integrator is not served by this route");
    RenderParams PC;                                             // the child's sample(): what mi_sample builds from a mi_sample_cfg
    memset(&PC, 0, sizeof PC);
    {
        mi_sample_cfg sc;
        memset(&sc, 0, sizeof sc);
        sc.struct_size = (uint32_t) sizeof sc; sc.integrator = cfg->integrator; sc.max_depth = cfg->max_depth; sc.rr_depth = cfg->rr_depth;
        sc.emitter_samples = cfg->emitter_samples; sc.bsdf_samples = cfg->bsdf_samples; sc.hide_emitters = cfg->hide_emitters;
        const std::string why = sample_cfg_problem(&sc);
        if (!why.empty()) return fail(c, MI_ERR_INVALID, "mi_render_sensor: %s", why.c_str());
        PC.spp = 1u; PC.max_depth = sc.max_depth; PC.rr_depth = sc.rr_depth;
        if (sc.integrator == MI_INTEGRATOR_DIRECT) { PC.integrator = INTEG_DIRECT; direct_constants(PC.direct, sc.emitter_samples, sc.bsdf_samples, sc.hide_emitters != 0); }
#if !MIW_SPECTRAL
        if (sc.integrator == MI_INTEGRATOR_VOLPATH) { PC.integrator = INTEG_VOLPATH; PC.direct.hide_emitters = sc.hide_emitters != 0 ? 1u : 0u; }
#endif
    }
    const bool volpath = cfg->integrator == MI_INTEGRATOR_VOLPATH;
    RenderParams P;                                              // camera, film and filter (k_init_pixels, the film launches)
    {   // (the camera and film fields are the integrator's all the same: volpath's child is described above)
        mi_render_cfg camera = *cfg;
        if (volpath) camera.integrator = MI_INTEGRATOR_PATH;
        MI_TRY(fill_params(c, &camera, P));
    }
    const uint32_t bs = (uint32_t) cfg->block_size, bs2 = bs * bs;
    uint32_t bs2_log2 = 0; while ((1u << bs2_log2) < bs2) ++bs2_log2;
    const uint32_t blocks_x = (cfg->crop_w + bs - 1) / bs, blocks_y = (cfg->crop_h + bs - 1) / bs, n_tiles = blocks_x * blocks_y;
    if (!cfg->block_ids || cfg->block_count != n_tiles) return fail(c, MI_ERR_INVALID, "mi_render_sensor: block_ids must hold %u entries", n_tiles);
    if ((uint64_t) n_tiles * bs2 >= (1ull << 31)) return fail(c, MI_ERR_INVALID, "mi_render_sensor: too many lanes");
    const uint32_t nch = MIW_FILM_CHANNELS, stride = MIW_AOV_LOG_HEAD, spp = cfg->spp;
    const size_t film_n = (size_t) cfg->crop_w * cfg->crop_h * nch;

    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const auto wall0 = std::chrono::steady_clock::now();
    c->cancel.store(0);
    auto stop_requested = [&]() {
        return c->cancel.load() != 0 || (cfg->timeout_s > 0.f && std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() > cfg->timeout_s);
    };

    // tiles per group: the group's log within MIW_AOV_LOG_BYTES (one tile at least), or what the caller asks for
    const size_t tile_log = (size_t) bs2 * std::max<uint32_t>(spp, 1u) * stride * sizeof(float);
    uint32_t group = (uint32_t) std::max<size_t>(1, std::min<size_t>(n_tiles, MIW_AOV_LOG_BYTES / tile_log));
    if (desc->debug_group_tiles) group = std::min(n_tiles, desc->debug_group_tiles);
    const uint32_t group_lanes = group * bs2, side = bs + 2u * (uint32_t) cfg->filter_border;

    TmpBuf<U4> d_st; TmpBuf<uint32_t> d_pixel, d_block_ids, d_iota; TmpBuf<int32_t> d_block_tile; TmpBuf<float> d_log, d_tiles, d_film, d_rays, d_spec;
    TmpBuf<F2> d_pos; TmpBuf<F4> d_wl, d_weight; TmpBuf<uint8_t> d_valid; TmpBuf<uint64_t> d_rng; TmpBuf<FilmRec> d_filmrec;
    HIP_TRY(c, d_st.resize(group_lanes)); HIP_TRY(c, d_pixel.resize(group_lanes)); HIP_TRY(c, d_pos.resize(group_lanes));
    HIP_TRY(c, d_log.resize((size_t) group_lanes * std::max<uint32_t>(spp, 1u) * stride));
    HIP_TRY(c, d_block_ids.resize(n_tiles)); HIP_TRY(c, d_block_tile.resize(n_tiles)); HIP_TRY(c, d_iota.resize(n_tiles));
    HIP_TRY(c, d_tiles.resize((size_t) n_tiles * side * side * nch));
    HIP_TRY(c, d_filmrec.resize(1));
    HIP_TRY(c, d_rays.resize((size_t) 8 * group_lanes)); HIP_TRY(c, d_spec.resize((size_t) MIW_SPEC_N * group_lanes));
    HIP_TRY(c, d_valid.resize(group_lanes)); HIP_TRY(c, d_rng.resize(group_lanes));
    if (MIW_SPECTRAL) { HIP_TRY(c, d_wl.resize(group_lanes)); HIP_TRY(c, d_weight.resize(group_lanes)); }
    HIP_TRY(c, c->d_next_ray.resize(1));
#if !MIW_SPECTRAL
    if (volpath) MI_TRY(volpath_capped_reset(c, s));
#endif
    std::vector<int32_t> block_tile(n_tiles);
    for (uint32_t t = 0; t < n_tiles; ++t) block_tile[t] = (int32_t) t;
    HIP_TRY(c, hipMemcpyAsync(d_block_ids.p, cfg->block_ids, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_block_tile.p, block_tile.data(), n_tiles * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_iota.p, block_tile.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_filmrec.p, &P.film, sizeof(FilmRec), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));                         // (block_tile goes out of use here)
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

    SensorStepArgs A;
    memset(&A, 0, sizeof A);
    sensor_records(cfg, desc, A.sensor, A.lens);
    for (int k = 0; k < 4; ++k) A.crop_f[k] = P.crop_f[k];
    A.warn_negative = P.film.warn_negative; A.spp = spp;
    A.st = d_st.p; A.pixel = d_pixel.p; A.pos = d_pos.p; A.wl = d_wl.p; A.weight = d_weight.p; A.log = d_log.p;
    for (int k = 0; k < 8; ++k) A.ray[k] = d_rays.p + (size_t) k * group_lanes;
    A.rng_state = d_rng.p; A.spec = d_spec.p; A.valid = d_valid.p;

    // cfg->profile: time per launch class into mi_counters — ms_path: k_init_pixels + the rounds, of which ms_init: k_init_pixels +
    // k_sensor_step (events around every launch of it, read once per group); ms_film_blocks: k_aov_film; ms_film_merge: k_aov_film_merge
    const bool prof = cfg->profile != 0;
    SensorEvents ev; size_t ev_used = 0;
    double ms_rounds = 0.0, ms_step = 0.0, ms_film = 0.0, ms_merge = 0.0;
    auto stamp = [&](size_t &idx) -> hipError_t {
        if (ev_used == ev.e.size()) { hipEvent_t x = nullptr; const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; ev.e.push_back(x); }
        idx = ev_used++;
        return hipEventRecord(ev.e[idx], s);
    };
    auto add_ms = [&](double &sum, size_t a, size_t b) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev.e[a], ev.e[b]) == hipSuccess) sum += ms; };

    bool stopped = false;
    for (uint32_t tile0 = 0; tile0 < n_tiles && !stopped; tile0 += group) {
        const uint32_t tiles_here = std::min(group, n_tiles - tile0), lanes = tiles_here * bs2;
        RenderParams PG = P; PG.n_lanes = lanes;
        InitArgs I; I.block_ids = d_block_ids.p; I.blocks_x = blocks_x; I.blocks_y = blocks_y; I.bs = bs; I.bs2_log2 = bs2_log2; I.base_seed = cfg->base_seed;
        I.tile_list = d_iota.p + tile0;                           // the group's tiles are the blocks tile0 ...
        A.n_lanes = lanes;
        SampleIO io;
        io.R = { A.ray[0], A.ray[1], A.ray[2], A.ray[3], A.ray[4], A.ray[5], A.ray[6], A.ray[7] };
        io.wavelengths = MIW_SPECTRAL ? reinterpret_cast<const float *>(d_wl.p) : nullptr;
        io.rng_state = d_rng.p; io.rng_inc = nullptr; io.spec = d_spec.p; io.valid = d_valid.p; io.n = lanes;
        ev_used = 0;
        std::vector<std::pair<size_t, size_t>> steps;             // (event before, event after) of every k_sensor_step of this group
        size_t e_begin = 0, e_film = 0, e_end = 0;
        if (prof) HIP_TRY(c, stamp(e_begin));
        hipLaunchKernelGGL(k_init_pixels, dim3((lanes + MIW_BLOCK - 1) / MIW_BLOCK), dim3(MIW_BLOCK), 0, s, PG, d_st.p, d_pixel.p, I);
        HIP_TRY(c, hipGetLastError());
        for (uint32_t j = 0; j <= spp && spp != 0u; ++j) {        // launch j finishes sample j - 1 and begins sample j
            if (stop_requested()) { stopped = true; break; }
            size_t e0 = 0, e1 = 0;
            if (prof && j != 0u) HIP_TRY(c, stamp(e0));
            HIP_TRY(c, sensor_launch_step(s, A, j, j != 0u, j != spp));
            if (prof) { HIP_TRY(c, stamp(e1)); steps.emplace_back(j != 0u ? e0 : e_begin, e1); }
            if (j == spp) break;
            const mi_status ls = sample_launch(c, PC, io, s);     // (its ray counter is reset by a stream-ordered memset: no host wait per round)
            if (ls != MI_OK) return ls;
            if (cfg->timeout_s > 0.f || (j & 15u) == 15u) HIP_TRY(c, hipStreamSynchronize(s));   // the stop test looks at finished work; else the host runs at most 16 rounds ahead
        }
        if (stopped) break;
        R.tile0 = tile0;
        if (prof) HIP_TRY(c, stamp(e_film));
        HIP_TRY(c, aov_launch_film(s, d_filmrec.p, P.film, R, tiles_here, d_tiles.p));
        if (prof) HIP_TRY(c, stamp(e_end));
        HIP_TRY(c, hipStreamSynchronize(s));                      // the next group overwrites the log
        if (prof) {
            add_ms(ms_rounds, e_begin, e_film); add_ms(ms_film, e_film, e_end);
            for (const auto &p : steps) add_ms(ms_step, p.first, p.second);
        }
    }
    if (stopped) { (void) hipStreamSynchronize(s); return fail(c, MI_ERR_CANCELLED, "mi_render_sensor: stopped by mi_cancel or timeout_s"); }
    size_t m0 = 0, m1 = 0;
    ev_used = 0;
    if (prof) HIP_TRY(c, stamp(m0));
    HIP_TRY(c, aov_launch_merge(s, d_filmrec.p, P.film, R, d_tiles.p, film_dev, cfg->accumulate != 0));
    if (prof) HIP_TRY(c, stamp(m1));
    if (!cfg->film_on_device) HIP_TRY(c, hipMemcpyAsync(film, film_dev, film_n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    mi_counters &K = c->counters;
    K.samples = (uint64_t) cfg->crop_w * (uint64_t) cfg->crop_h * spp;
#if !MIW_SPECTRAL
    if (volpath) MI_TRY(volpath_capped_read(c, s));
#endif
    if (prof) {
        add_ms(ms_merge, m0, m1);
        K.ms_path = ms_rounds; K.ms_init = ms_step; K.ms_film_blocks = ms_film; K.ms_film_merge = ms_merge; K.ms_resolve = ms_film + ms_merge;
        K.ms_render = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return MI_OK;
}

mi_status mi_sensor_sample_ray(mi_ctx *c, const mi_render_cfg *cfg, const mi_sensor_desc *desc,
                               const float *position_sample, const float *aperture_sample, const float *wavelength_sample,
                               const mi_rays_soa *rays, float *wavelengths, float *weights, uint64_t n, int32_t on_device) {
    if (!desc) return MI_ERR_INVALID;
    {
        const std::string why = sensor_desc_problem(desc);
        if (!why.empty()) { if (c) c->error = why; else g_global_error = why; return MI_ERR_INVALID; }
    }
    if (!c || !cfg) return MI_ERR_INVALID;
    if (!position_sample || !rays) return fail(c, MI_ERR_INVALID, "mi_sensor_sample_ray: null position_sample / rays");
    const float *dst[8] = { rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->mint, rays->maxt };
    for (int k = 0; k < 8; ++k) if (!dst[k]) return fail(c, MI_ERR_INVALID, "mi_sensor_sample_ray: null ray array");
    if (MIW_SPECTRAL && (wavelengths || weights) && !wavelength_sample) return fail(c, MI_ERR_INVALID, "mi_sensor_sample_ray: wavelengths and weights need wavelength_sample");
    if (n >= (1ull << 31)) return fail(c, MI_ERR_INVALID, "mi_sensor_sample_ray: at most 2^31 - 1 samples per call");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SensorRaysArgs A;
    memset(&A, 0, sizeof A);
    sensor_records(cfg, desc, A.sensor, A.lens);
    A.n = (uint32_t) n;
    if (on_device) {
        A.position = position_sample; A.aperture = aperture_sample; A.wavelength_sample = MIW_SPECTRAL ? wavelength_sample : nullptr;
        for (int k = 0; k < 8; ++k) A.ray[k] = const_cast<float *>(dst[k]);
        A.wavelengths = wavelengths; A.weights = weights;
        HIP_TRY(c, sensor_launch_rays(s, A));
        HIP_TRY(c, hipStreamSynchronize(s));
        return MI_OK;
    }
    // host arrays: one staging buffer of the call's own, [position 2n][aperture 2n][wavelength sample n][rays 8n][wavelengths 4n][weights 4n]
    TmpBuf<float> d;
    HIP_TRY(c, d.resize((size_t) 21 * n));
    float *p = d.p;
    float *d_pos = p, *d_ap = p + 2 * n, *d_ws = p + 4 * n, *d_ray = p + 5 * n, *d_wl = p + 13 * n, *d_wt = p + 17 * n;
    HIP_TRY(c, hipMemcpyAsync(d_pos, position_sample, 2 * n * sizeof(float), hipMemcpyHostToDevice, s));
    if (aperture_sample) HIP_TRY(c, hipMemcpyAsync(d_ap, aperture_sample, 2 * n * sizeof(float), hipMemcpyHostToDevice, s));
    const bool have_ws = MIW_SPECTRAL && wavelength_sample;
    if (have_ws) HIP_TRY(c, hipMemcpyAsync(d_ws, wavelength_sample, n * sizeof(float), hipMemcpyHostToDevice, s));
    A.position = d_pos; A.aperture = aperture_sample ? d_ap : nullptr; A.wavelength_sample = have_ws ? d_ws : nullptr;
    for (int k = 0; k < 8; ++k) A.ray[k] = d_ray + (size_t) k * n;
    A.wavelengths = wavelengths ? d_wl : nullptr; A.weights = weights ? d_wt : nullptr;
    HIP_TRY(c, sensor_launch_rays(s, A));
    for (int k = 0; k < 8; ++k) HIP_TRY(c, hipMemcpyAsync(const_cast<float *>(dst[k]), A.ray[k], n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (MIW_SPECTRAL && wavelengths) HIP_TRY(c, hipMemcpyAsync(wavelengths, d_wl, 4 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (weights) HIP_TRY(c, hipMemcpyAsync(weights, d_wt, (size_t) MIW_SPEC_N * n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return MI_OK;
}
