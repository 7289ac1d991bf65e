// VolumetricPathIntegrator (src/integrators/volpath.cpp, scalar_rgb) over homogeneous media, as ONE per-lane state machine.
//
// The reference nests three loops: the bounce loop of sample() (:72-255) calls sample_emitter (:261-367) and evaluate_direct_light
// (:370-465), each a walk through media and index-matched surfaces with closest-hit queries of its own. The device's scene query
// (device/trace.h: trace2) is a wave-cooperative call with ONE call site per loop trip, so the three loops are flattened: a lane is
// in one of three modes — main, emitter walk, direct-light walk — and in a state that names where it resumes once the query it
// posted has been answered. A trip answers at most one closest-hit query per lane (no shadow query: hasS = false); lanes in
// different modes share the trip. The lane is serial, so the sampler draws and the float additions into `result` keep the
// reference's order. The two walks share their code (the medium segment, the surface step): they differ in a handful of lines.
//
// Draw ledger of one sample() (scalar semantics: a call that is reached draws, whatever its mask):
//   1        the RGB channel (:66)
//   per bounce, in this order:
//     1      Russian roulette, EVERY bounce, also before rr_depth and for a dead path (:82)
//     in a medium: 1 free flight (:105), 1 null-scatter decision (:123: never selects, sigma_n = 0);
//       on a scatter with sample_emitters: the emitter walk; then 2 for the phase function (:171)
//     on a surface: with a smooth BSDF and depth + 1 < max_depth the emitter walk; 1 + 2 for the BSDF (:215-216); with
//       add_emitter the direct-light walk
//   emitter walk: 2 for the emitter (:267), then 1 per medium segment (:294)
//   direct-light walk: 1 per medium segment (:391)
//
// What a homogeneous medium makes dead, and is therefore not carried: sigma_n = 0, so a medium event inside either walk zeroes the
// transmittance (:330-332, :417-419) and ends it — the ray origin moved to mi.p and `si.t -= mi.t` (:325-327, :412-414) are never
// read again; in sample() the null-scatter branch (:128-131, :140-144) is never taken (the draw of :123 is made). A carried hit
// is kept as its record (t, u, v, triangle) with the origin of the ray that found it; its SurfaceInteraction is rebuilt from them
// where it is read, which gives the bits the reference computed once.
//
// Every loop ends: a ray whose lane loop runs past MIW_VOLPATH_MAX_TRIPS trips (far above any real path: a condition, not a
// measurement) is ended with L = 0 and valid = 0 and counted (mi_volpath_capped).
#pragma once
#include "path.h"
#include "medium.h"

namespace miw {

#define MIW_VOLPATH_MAX_TRIPS 65536u
enum : uint32_t { INTEG_VOLPATH = 2 };

#if !MIW_SPECTRAL     // served by the scalar_rgb library (include/miwave.h)

enum : uint32_t {                    // where a lane resumes
    VS_IDLE = 0,                     // no ray: fetch one
    VS_BOUNCE,                       // top of the bounce loop, :72
    VS_MAIN_MEDIUM,                  // after the medium segment's query, :109
    VS_MAIN_SURFACE,                 // after the surface query, :182
    VS_MAIN_NEXT,                    // after the query of the sampled direction, :241
    VS_EM_ITER, VS_EM_MEDIUM, VS_EM_SURFACE,      // sample_emitter: top of its loop :282, after :298, after :339
    VS_DL_ITER, VS_DL_MEDIUM, VS_DL_SURFACE       // evaluate_direct_light: :385, after :395, after :425
};
enum : uint32_t {
    VF_ACTIVE = 1u << 0, VF_SPECULAR_CHAIN = 1u << 1, VF_VALID = 1u << 2, VF_NEEDS = 1u << 3,          // sample()'s masks
    VF_W_NEEDS = 1u << 6, VF_W_ESCAPED = 1u << 7, VF_W_ACTIVE_MEDIUM = 1u << 8, VF_W_HAD_MEDIUM = 1u << 9,   // the walk's
    VF_EM_FROM_MEDIUM = 1u << 10,    // the emitter walk under way was started by a medium scatter (else by a surface)
    VF_DS_DELTA = 1u << 11, VF_QUERIED = 1u << 12
};
#define MIW_VOL_NO_TRANSITION 0xffffffffu

struct VolLane {
    PCG32 rng; Wavelengths wl;
    uint32_t st, flags, medium, channel, depth, trips;
    Spec tp, res; float eta;
    Ray ray;                         // sample()'s ray
    F4 si_h; V3 si_o;                // its carried hit record (w = MIW_MISS: none) and the origin of the ray that found it
    float seg_t, seg_ts;             // mi.t and sampled_t of the medium segment under way (main or walk)
    // a walk
    uint32_t w_medium, next_medium;
    Ray wray; F4 w_h; V3 w_o;
    Spec T, emitter_val;
    float ds_dist, ds_pdf, total_dist, remaining, bs_pdf;
};

MIW_HD float vol_hit_t(F4 h) { return f2u(h.w) != MIW_MISS ? h.x : MIW_INFINITY; }
MIW_HD F4 vol_no_hit() { F4 h; h.x = MIW_INFINITY; h.y = h.z = 0.f; h.w = u2f(MIW_MISS); return h; }

// the SurfaceInteraction of a hit record, si.bsdf() and si.emitter() (the environment for a miss)
template <int Mats, bool Analytic>
MIW_HD bool vol_si(const SceneView &sc, F4 h, V3 o, V3 d, SurfaceInteraction &si, uint32_t &bsdf_index, int32_t &emitter) {
    const uint32_t tri_idx = f2u(h.w);
    bsdf_index = 0;
    if (tri_idx == MIW_MISS) { emitter = miss_emitter<mats_lights(Mats)>(sc); return false; }
    hit_surface_interaction<Analytic, mats_full(Mats)>(sc, tri_idx, h.x, h.y, h.z, [o]() { return o; }, d, si, bsdf_index, emitter);
    return true;
}

MIW_HD void vol_begin(VolLane &L, const RenderParams &P, const MediaView &mv) {
    L.tp = spec(1.f); L.res = spec(0.f); L.eta = 1.f;                         // :54-61
    L.medium = mv.start_medium; L.depth = 0u; L.trips = 0u;
    L.flags = VF_ACTIVE | VF_NEEDS | (P.direct.hide_emitters ? 0u : VF_SPECULAR_CHAIN);
    const uint32_t ci = (uint32_t) (next_1d(L.rng) * 3.f);                    // :66
    L.channel = ci < 2u ? ci : 2u;
    L.si_h = vol_no_hit(); L.si_o = v3(0.f);                                  // :69-70
    L.st = VS_BOUNCE;
}

// One trip of a lane. `h` answers the query the lane posted in the trip before (VF_QUERIED). Returns true when the lane posts a
// query: q. L.st == VS_IDLE afterwards: sample() has returned (L.res, VF_VALID).
template <int Mats, bool Analytic>
MIW_HD bool vol_step(const RenderParams &P, const SceneView &sc, const MediaView &mv, VolLane &L, F4 h, Ray &q) {
    constexpr bool Lights = mats_lights(Mats);
    const uint32_t max_depth = (uint32_t) P.max_depth, rr_depth = (uint32_t) P.rr_depth;
    const bool queried = (L.flags & VF_QUERIED) != 0u;
    L.flags &= ~VF_QUERIED;
    bool is_dl = L.st >= VS_DL_ITER;                 // which walk the shared walk code serves
    bool after_em = false;                           // main_surface: resumed after the emitter walk it started

    switch (L.st) {
        case VS_BOUNCE: goto bounce;
        case VS_MAIN_MEDIUM: goto main_medium;
        case VS_MAIN_SURFACE: goto main_surface;
        case VS_MAIN_NEXT: goto main_next;
        case VS_EM_ITER: case VS_DL_ITER: goto walk_iter;
        case VS_EM_MEDIUM: case VS_DL_MEDIUM: goto walk_medium;
        case VS_EM_SURFACE: case VS_DL_SURFACE: goto walk_surface;
        default: return false;
    }

    // ------------------------------------------------------------------------------------------------ sample(), :72-255
bounce: {
        bool active = (L.flags & VF_ACTIVE) != 0u;
        active = active && !all_zero(L.tp);                                   // :79
        const float qrr = min_(hmax(L.tp) * sqr(L.eta), .95f);               // :80
        const bool perform_rr = L.depth > rr_depth;
        active = (next_1d(L.rng) < qrr || !perform_rr) && active;            // :82
        if (perform_rr) L.tp = L.tp * rcp(qrr);                               // :83
        if (!active || L.depth >= max_depth) { L.st = VS_IDLE; return false; }   // :85-87
        if (L.medium) {                                                       // :104-110
            const MediumInteraction mi = medium_sample_interaction(mv.media[L.medium - 1u], L.ray, next_1d(L.rng), L.channel);
            L.seg_t = mi.t; L.seg_ts = mi.ts;
            if (mi.t != MIW_INFINITY) L.ray.maxt = mi.t;                      // :106
            if (L.flags & VF_NEEDS) { L.st = VS_MAIN_MEDIUM; q = L.ray; L.flags |= VF_QUERIED; return true; }
            goto main_medium;
        }
        goto main_surface_pre;
    }
main_medium: {
        if (queried) { L.si_h = h; L.si_o = L.ray.o; }
        L.flags &= ~VF_NEEDS;                                                 // :110
        const MediumRec &m = mv.media[L.medium - 1u];
        MediumInteraction mi;
        mi.t = L.seg_t; mi.mint = max_(L.ray.mint, 0.f); mi.sigma_t = medium_sigma_t(m);
        const float si_t = vol_hit_t(L.si_h);
        if (si_t < mi.t) mi.t = MIW_INFINITY;                                 // :112
        if (m.has_spectral_extinction) {                                      // :113-117
            Spec tr, pdf;
            medium_eval_tr_and_pdf(mi, si_t, tr, pdf);
            L.tp = L.tp * medium_tr_weight(tr, pdf, L.channel);
        }
        const bool active_medium = mi.t != MIW_INFINITY;                      // :119-120
        const float st_c = spec_at(mi.sigma_t, L.channel);
        const bool null_scatter = next_1d(L.rng) >= st_c / st_c;              // :123 (combined_extinction = sigma_t: never)
        bool act_medium_scatter = !null_scatter && active_medium;             // :125-126
        if (act_medium_scatter) L.depth++;                                    // :133
        const bool active = L.depth < max_depth;                              // :137
        if (!active) L.flags &= ~VF_ACTIVE;
        act_medium_scatter = act_medium_scatter && active;
        if (!act_medium_scatter) {
            if (active_medium) { L.st = VS_BOUNCE; return false; }            // cut by max_depth, or the null event: :254 keeps `active`
            goto main_surface_pre;
        }
        const Spec sigma_s = mi.sigma_t * medium_albedo(m);
        if (m.has_spectral_extinction) L.tp = L.tp * ((sigma_s * st_c) / st_c);   // :147-149
        else L.tp = L.tp * spec_div(sigma_s, mi.sigma_t);                     // :150-151
        L.flags |= VF_VALID;                                                  // :158
        L.flags &= ~VF_SPECULAR_CHAIN;                                        // :159-160
        if (!m.sample_emitters) L.flags |= VF_SPECULAR_CHAIN;
        L.ray.o = v3(fmadd(L.ray.d.x, L.seg_ts, L.ray.o.x), fmadd(L.ray.d.y, L.seg_ts, L.ray.o.y), fmadd(L.ray.d.z, L.seg_ts, L.ray.o.z));   // mi.p
        L.ray.mint = 0.f;
        if (m.sample_emitters) {                                              // :162-167
            L.flags |= VF_EM_FROM_MEDIUM;
            L.wray.o = L.ray.o; L.wray.mint = 0.f;                            // :275-276
            goto em_start;
        }
        goto main_phase;
    }
main_phase: {                                                                 // :169-175
        const MediumRec &m = mv.media[L.medium - 1u];
        float pdf;
        const V3 wo = phase_sample(m, L.ray.d, next_2d(L.rng), pdf);
        L.ray.d = wo; L.ray.mint = 0.f; L.ray.maxt = MIW_INFINITY;            // mi.spawn_ray(wo), mint = 0
        L.flags |= VF_NEEDS;
        L.st = VS_BOUNCE;                                                     // (:254: active_medium holds)
        return false;
    }
main_surface_pre: {                                                           // :179-182
        if (L.flags & VF_NEEDS) { L.st = VS_MAIN_SURFACE; q = L.ray; L.flags |= VF_QUERIED; return true; }
        goto main_surface;
    }
main_surface: {
        if (queried && !after_em) { L.si_h = h; L.si_o = L.ray.o; }
        SurfaceInteraction si; uint32_t bsdf_index; int32_t emitter;
        const bool valid = vol_si<Mats, Analytic>(sc, L.si_h, L.si_o, L.ray.d, si, bsdf_index, emitter);
        if (!after_em) {
            if ((L.flags & VF_SPECULAR_CHAIN) && emitter >= 0)                // :186-191
                L.res = L.res + L.tp * (valid ? emitter_eval(sc.emitters[emitter], si.wi, L.wl) : miss_eval<Lights>(sc, L.ray.d, L.wl));
            if (!valid) { L.flags &= ~VF_ACTIVE; L.st = VS_BOUNCE; return false; }   // :193, :254
        }
        const BsdfSide bsdf = bsdf_side<true>(sc.bsdfs, bsdf_index, si.wi);   // :197
        const TexCtx tc(L.wl, si.uv, sc.bitmaps, sc.bsdf_tables);
        if (!after_em && (bsdf.flags & BSDF_Smooth) && L.depth + 1u < max_depth) {   // :198-201
            L.flags &= ~VF_EM_FROM_MEDIUM;
            L.wray.o = si.p; L.wray.mint = spawn_mint(si.p);                  // :275
            goto em_start;
        }
        if (after_em && L.ds_pdf != 0.f) {                                    // :204-211 (L.T = emitted)
            const V3 wo = to_local(si.sh, L.wray.d);
            const Spec bsdf_val = bsdf_side_eval<true, false, true>(bsdf, si.wi, wo, tc);
            const float bsdf_pdf = bsdf_side_pdf<true, false, true>(bsdf, si.wi, wo, tc);
            L.res = L.res + L.tp * bsdf_val * mis_weight(L.ds_pdf, (L.flags & VF_DS_DELTA) ? 0.f : bsdf_pdf) * L.T;
        }
        const float s1 = next_1d(L.rng);                                      // :215-216
        const V2 s2 = next_2d(L.rng);
        BSDFSample bs;
        const Spec bsdf_val = bsdf_side_sample<true, false, true>(bsdf, si.wi, s1, s2, bs, tc);
        L.tp = L.tp * bsdf_val;                                               // :219-220
        L.eta *= bs.eta;
        L.ray.o = si.p; L.ray.d = to_world(si.sh, bs.wo); L.ray.mint = spawn_mint(si.p); L.ray.maxt = MIW_INFINITY;   // :222-223
        L.flags |= VF_NEEDS;
        const bool non_null = !(bs.sampled_type & BSDF_Null);                 // :226-231
        if (non_null) { L.depth++; L.flags |= VF_VALID; }
        if (non_null && (bs.sampled_type & BSDF_Delta)) L.flags |= VF_SPECULAR_CHAIN;
        if (bs.sampled_type & BSDF_Smooth) L.flags &= ~VF_SPECULAR_CHAIN;
        const bool add_emitter = !(bs.sampled_type & BSDF_Delta) && !all_zero(L.tp) && L.depth < max_depth;   // :233-234
        L.bs_pdf = bs.pdf;
        L.next_medium = is_medium_transition(mv, si.shape) ? target_medium(mv, si.shape, L.ray.d, si.n) : MIW_VOL_NO_TRANSITION;   // :249-250
        if (add_emitter) { L.st = VS_MAIN_NEXT; q = L.ray; L.flags |= VF_QUERIED; return true; }   // :238-241
        goto main_finish;
    }
main_next: {                                                                  // :242-245: si_new = h; evaluate_direct_light starts
        L.si_h = h; L.si_o = L.ray.o;                                         // (:252)
        L.flags &= ~(VF_NEEDS | VF_W_NEEDS);                                  // :242, :380
        L.w_medium = L.medium; L.wray = L.ray; L.w_h = h; L.w_o = L.ray.o;
        L.T = spec(1.f);
        is_dl = true; L.st = VS_DL_ITER;
        goto walk_iter;
    }
main_finish: {
        if (L.next_medium != MIW_VOL_NO_TRANSITION) L.medium = L.next_medium; // :249-250
        L.st = VS_BOUNCE;                                                     // (:254: active_surface holds)
        return false;
    }

    // ------------------------------------------------------------------------------------------------ sample_emitter(), :261-281
em_start: {
        DirectionSample ds;
        const Spec ev = sample_emitter_direction<Analytic, Lights>(sc, L.wray.o, next_2d(L.rng), ds, L.wl);   // :267
        L.ds_pdf = ds.pdf; L.ds_dist = ds.dist;
        L.flags &= ~VF_DS_DELTA;
        if (Lights && ds.delta) L.flags |= VF_DS_DELTA;
        L.T = spec(0.f);
        if (ds.pdf == 0.f) goto em_end;                                       // :268-273
        L.emitter_val = ev;
        L.wray.d = ds.d; L.wray.maxt = MIW_INFINITY;                          // :275
        L.total_dist = 0.f; L.w_h = vol_no_hit(); L.w_o = v3(0.f);            // :278-281
        L.flags |= VF_W_NEEDS;
        L.w_medium = L.medium; L.T = spec(1.f);
        is_dl = false; L.st = VS_EM_ITER;
        goto walk_iter;
    }
em_end: {                                                                     // :366: L.T = transmittance * emitter_val
        if (L.ds_pdf != 0.f) L.T = L.T * L.emitter_val;
        if (L.flags & VF_EM_FROM_MEDIUM) {                                    // :164-166
            if (L.ds_pdf != 0.f) L.res = L.res + L.tp * phase_eval(mv.media[L.medium - 1u], L.ray.d, L.wray.d) * L.T;
            goto main_phase;
        }
        after_em = true;
        goto main_surface;
    }

    // ------------------------------------------------------------------------------------------------ the two walks
walk_iter: {                                                                  // :283-299 / :386-396
        if (!is_dl) {
            L.remaining = L.ds_dist * (1.f - MIW_SHADOW_EPSILON) - L.total_dist;
            L.wray.maxt = L.remaining;
            if (!(L.remaining > 0.f)) goto em_end;                            // :285-287
        }
        L.flags &= ~(VF_W_ESCAPED | VF_W_ACTIVE_MEDIUM | VF_W_HAD_MEDIUM);
        if (L.w_medium) {
            L.flags |= VF_W_HAD_MEDIUM;
            const MediumInteraction mi = medium_sample_interaction(mv.media[L.w_medium - 1u], L.wray, next_1d(L.rng), L.channel);
            L.seg_t = mi.t;
            if (mi.t != MIW_INFINITY) L.wray.maxt = is_dl ? mi.t : min_(mi.t, L.remaining);   // :392 / :295
            if (L.flags & VF_W_NEEDS) { L.st = is_dl ? VS_DL_MEDIUM : VS_EM_MEDIUM; q = L.wray; L.flags |= VF_QUERIED; return true; }
            goto walk_medium;
        }
        if (L.flags & VF_W_NEEDS) { L.st = is_dl ? VS_DL_SURFACE : VS_EM_SURFACE; q = L.wray; L.flags |= VF_QUERIED; return true; }   // :337-339 / :424-425
        goto walk_surface;
    }
walk_medium: {                                                                // :300-333 / :397-420
        if (queried) { L.w_h = h; L.w_o = L.wray.o; }
        const MediumRec &m = mv.media[L.w_medium - 1u];
        MediumInteraction mi;
        mi.t = L.seg_t; mi.mint = max_(L.wray.mint, 0.f); mi.sigma_t = medium_sigma_t(m);
        const float si_t = vol_hit_t(L.w_h);
        if (si_t < mi.t) mi.t = MIW_INFINITY;                                 // :300 / :397
        L.flags &= ~VF_W_NEEDS;                                               // :301 / :407
        if (m.has_spectral_extinction) {
            Spec tr, pdf;
            if (is_dl) medium_eval_tr_and_pdf(mi, si_t, tr, pdf);             // :402
            else {                                                            // :306-308
                const float t = min_(L.remaining, min_(mi.t, si_t)) - mi.mint;
                tr = spec_exp(-t * mi.sigma_t);
                pdf = (si_t < mi.t || mi.t > L.remaining) ? tr : tr * mi.sigma_t;
            }
            L.T = L.T * medium_tr_weight(tr, pdf, L.channel);                 // :310 / :404
        }
        if (!is_dl) {                                                         // :314-315
            if (mi.t > L.remaining && mi.t != MIW_INFINITY) L.total_dist = L.ds_dist;
            if (mi.t > L.remaining) mi.t = MIW_INFINITY;
        }
        if (mi.t != MIW_INFINITY) {                                           // a medium event: :322-332 / :411-419, sigma_n = 0
            L.flags |= VF_W_ACTIVE_MEDIUM;
            if (!is_dl) L.total_dist += mi.t;
            L.T = L.T * spec(0.f);
        } else L.flags |= VF_W_ESCAPED;
        goto walk_surface;
    }
walk_surface: {                                                               // :337-364 / :424-462
        if (queried && (L.st == VS_EM_SURFACE || L.st == VS_DL_SURFACE)) { L.w_h = h; L.w_o = L.wray.o; L.flags &= ~VF_W_NEEDS; }
        const bool active_medium = (L.flags & VF_W_ACTIVE_MEDIUM) != 0u;
        bool active_surface = !(L.flags & VF_W_HAD_MEDIUM) || (L.flags & VF_W_ESCAPED);   // :341 / :427
        if (!is_dl && active_surface) L.total_dist += vol_hit_t(L.w_h);       // :342
        if (active_surface) {
            SurfaceInteraction si; uint32_t bsdf_index; int32_t emitter;
            const bool valid = vol_si<Mats, Analytic>(sc, L.w_h, L.w_o, L.wray.d, si, bsdf_index, emitter);
            if (is_dl && emitter >= 0) {                                      // :430-440: the walk found an emitter
                V3 d = L.wray.d; float dist = 0.f; V3 n = v3(0.f), ref_p = v3(0.f);   // DirectionSample3f(si, ref), records.h:168-174
                if (valid) {
                    ref_p = L.ray.o;
                    d = si.p - ref_p;
                    dist = norm(d);
                    d = d / dist;
                    n = si.sh.n;
                }
                const Spec emitter_val = valid ? emitter_eval(sc.emitters[emitter], si.wi, L.wl) : miss_eval<Lights>(sc, L.wray.d, L.wl);
                const float emitter_pdf = pdf_emitter_direction<Analytic, Lights>(sc, (uint32_t) emitter, d, dist, n, ref_p);
                if (emitter_pdf != 0.f)                                       // :246-247
                    L.res = L.res + mis_weight(L.bs_pdf, emitter_pdf) * L.tp * (L.T * emitter_val);
                goto main_finish;
            }
            active_surface = valid && !active_medium;                         // :344 / :442
            if (active_surface) {
                const TexCtx tc(L.wl, si.uv, sc.bitmaps, sc.bsdf_tables);
                L.T = L.T * bsdf_null_transmission(sc.bsdfs, bsdf_index, si.wi, tc);   // :346-349 / :444-448
                L.wray.o = si.p; L.wray.mint = spawn_mint(si.p); L.wray.maxt = MIW_INFINITY;   // :353 / :452
                L.flags |= VF_W_NEEDS;                                        // :355 / :453
                if (is_medium_transition(mv, si.shape)) L.w_medium = target_medium(mv, si.shape, L.wray.d, si.n);   // :361-364 / :459-462
            }
        }
        if (!is_dl) L.wray.maxt = L.remaining;                                // :354
        if ((active_medium || active_surface) && !all_zero(L.T)) {            // :358 / :456
            L.st = is_dl ? VS_DL_ITER : VS_EM_ITER;
            return false;
        }
        if (is_dl) goto main_finish;                                          // (emitter_pdf = 0: nothing is added)
        goto em_end;
    }
}

// The ray-fed loop, as ray_stream_sample (path.h): feed.fetch / feed.store, one trace2 call site per trip, a lane that finishes a
// ray fetches the next inside the loop. `capped`: the counter of rays ended by MIW_VOLPATH_MAX_TRIPS.
template <int Mats, bool Analytic, typename Feed, typename Trace2>
MIW_HD void ray_stream_sample_volpath(const RenderParams &P, const SceneView &sc, const MediaView &mv, Feed &feed, Trace2 trace2, uint32_t *capped) {
    VolLane L;
    L.st = VS_IDLE; L.flags = 0u; L.trips = 0u;
    LaneRegs F;
    F.flags = LF_DONE; F.rng.state = 0; F.rng.inc = MIW_PCG32_SCALAR_INC;
    Ray q; q.o = q.d = v3(0.f); q.mint = 0.f; q.maxt = -1.f;
    bool has = false;
    for (;;) {
        if (L.st == VS_IDLE) {
            if (!feed.fetch(F)) break;
            L.rng = F.rng; L.wl = F.wl; L.ray = F.ray;
            vol_begin(L, P, mv);
            has = false;
            continue;
        }
        F4 h; bool occluded = false;
        trace2(q.o, q.mint, q.d, q.maxt, has, v3(0.f), -1.f, false, h, occluded);
        has = vol_step<Mats, Analytic>(P, sc, mv, L, h, q);
        if (L.st != VS_IDLE && ++L.trips > MIW_VOLPATH_MAX_TRIPS) {           // no real path gets here
            L.res = spec(0.f); L.flags &= ~VF_VALID; L.st = VS_IDLE; has = false;
#if defined(__HIP_DEVICE_COMPILE__)
            atomicAdd(capped, 1u);
#else
            ++*capped;
#endif
        }
        if (L.st == VS_IDLE) {
            F.res = L.res; F.flags = (L.flags & VF_VALID) ? (uint32_t) LF_VALID_RAY : 0u; F.rng = L.rng;
            feed.store(F);
        }
    }
}

#endif   // !MIW_SPECTRAL

} // namespace miw
