// The aov integrator's leaf arithmetic (src/integrators/aov.cpp): the channel table, the surface partials dp_du / dp_dv that
// no other kernel keeps, and the per-sample fill. float32, shared by host and device.
//
// Follows: src/integrators/aov.cpp:83-154 (channel grammar), :156-254 (per-sample work),
// src/librender/mesh.cpp:491-511, src/shapes/rectangle.cpp:86-90,200-201, src/shapes/sphere.cpp:362-388 (dp_du, dp_dv),
// include/mitsuba/render/interaction.h:593 (duv_dx = duv_dy = 0: only si.bsdf(ray) -> compute_uv_partials fills them, and
// aov.cpp never calls it — the two channel types are always zero, and stay so here).
//
// The compute_surface_interaction* bodies of shape.h are not touched (their compiled form is pinned by the register-budget
// tests): the partials are computed BESIDE them, by the statements those bodies run and then drop.
#pragma once
#include "base.h"
#include "shape.h"
#include "scene.h"

namespace miw {

// aov.cpp:66-81 (Type), in the order of the grammar's branches (:92-131)
enum : uint32_t {
    AOV_DEPTH = 0, AOV_POSITION = 1, AOV_UV = 2, AOV_GEO_NORMAL = 3, AOV_SH_NORMAL = 4,
    AOV_DP_DU = 5, AOV_DP_DV = 6, AOV_DUV_DX = 7, AOV_DUV_DY = 8, AOV_TYPE_COUNT = 9
};
#define MIW_AOV_MAX_TYPES 32
#define MIW_AOV_MAX_CHANNELS (3 * MIW_AOV_MAX_TYPES)

MIW_HD uint32_t aov_type_channels(uint32_t type) {
    switch (type) {
        case AOV_DEPTH: return 1u;
        case AOV_UV: case AOV_DUV_DX: case AOV_DUV_DY: return 2u;
        case AOV_POSITION: case AOV_GEO_NORMAL: case AOV_SH_NORMAL: case AOV_DP_DU: case AOV_DP_DV: return 3u;
        default: return 0u;                              // unknown type
    }
}
template <typename Types>
MIW_HD uint32_t aov_channels(Types types, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c += aov_type_channels(types[i]);
    return c;
}

struct AovPartials { V3 dp_du, dp_dv; };

// mesh.cpp:486-511. `tc` = the face's texture coordinates (u0 v0 u1 v1 u2 v2) or nullptr
MIW_HD AovPartials aov_partials_triangle(V3 p0, V3 p1, V3 p2, const float *tc) {
    V3 dp0 = p1 - p0, dp1 = p2 - p0;
    const V3 n = normalize(cross(dp0, dp1));           // :487
    AovPartials r;
    coordinate_system(n, r.dp_du, r.dp_dv);            // :491
    if (tc) {                                          // :492-511
        const V2 uv0 = v2(tc[0], tc[1]), uv1 = v2(tc[2], tc[3]), uv2 = v2(tc[4], tc[5]);
        const V2 duv0 = v2(uv1.x - uv0.x, uv1.y - uv0.y), duv1 = v2(uv2.x - uv0.x, uv2.y - uv0.y);
        const float det = fmsub(duv0.x, duv1.y, duv0.y * duv1.x), inv_det = rcp(det);             // :503-504
        if (det != 0.f) {                                                                          // :506-509
            r.dp_du = fmsub3(dp0, duv1.y, dp1 * duv0.y) * inv_det;
            r.dp_dv = fnmadd3(dp0, duv1.x, dp1 * duv0.x) * inv_det;
        }
    }
    return r;
}
// rectangle.cpp:86-90 (m_frame.s, m_frame.t) -> :200-201
MIW_HD AovPartials aov_partials_rect(const AnalyticRec &r) {
    AovPartials o;
    o.dp_du = xf_vector(r.to_world, v3(2.f, 0.f, 0.f));
    o.dp_dv = xf_vector(r.to_world, v3(0.f, 2.f, 0.f));
    return o;
}
// sphere.cpp:362-388. `p` = si.p (the point re-projected onto the sphere, :359)
MIW_HD AovPartials aov_partials_sphere(const AnalyticRec &r, V3 p) {
    const V3 local = xf_point_affine(r.to_object, p);  // :362
    const float rd_2 = sqr(local.x) + sqr(local.y);    // :364
    AovPartials o;
    o.dp_du = v3(-local.y, local.x, 0.f);              // :372
    const float rd = __builtin_sqrtf(rd_2), inv_rd = rcp(rd), cos_phi = local.x * inv_rd, sin_phi = local.y * inv_rd;   // :374-377
    o.dp_dv = v3(local.z * cos_phi, local.z * sin_phi, -rd);                                                            // :379-381
    if (rd == 0.f) o.dp_dv = v3(1.f, 0.f, 0.f);        // :383-385
    o.dp_du = xf_vector(r.to_world, o.dp_du) * (2.f * MIW_PI);   // :387
    o.dp_dv = xf_vector(r.to_world, o.dp_dv) * MIW_PI;           // :388
    return o;
}

// The partials of the hit hit_surface_interaction() (scene.h) built `si` for: triangle `tri_idx` in leaf order
template <bool Analytic>
MIW_HD AovPartials aov_hit_partials(const SceneView &sc, uint32_t tri_idx, const SurfaceInteraction &si) {
    const Tri &tr = sc.tris[tri_idx];
    if (Analytic && tr.pad) {
        const AnalyticRec &a = sc.rects[tr.pad - 1u];
        return a.kind == ANALYTIC_SPHERE ? aov_partials_sphere(a, si.p) : aov_partials_rect(a);
    }
    const float *tc = (sc.shapes[tr.shape].flags & SHAPE_HAS_TEXCOORDS) ? sc.tri_uv + 6 * (size_t) tr.prim : nullptr;
    return aov_partials_triangle(ld3(tr.p0), ld3(tr.p1), ld3(tr.p2), tc);
}

// aov.cpp:166-219: the channels of one sample, in the order of `types`; everything zero for an invalid interaction (:167 —
// `depth` of a miss is 0, not +inf). Returns the number of floats written.
template <typename Types>
MIW_HD uint32_t aov_fill(const SurfaceInteraction &si, const AovPartials &pt, bool valid, Types types, uint32_t n, float *out) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        V3 v = v3(0.f); uint32_t c = 0;
        switch (types[i]) {
            case AOV_DEPTH: v.x = si.t; c = 1u; break;
            case AOV_POSITION: v = si.p; c = 3u; break;
            case AOV_UV: v.x = si.uv.x; v.y = si.uv.y; c = 2u; break;
            case AOV_GEO_NORMAL: v = si.n; c = 3u; break;
            case AOV_SH_NORMAL: v = si.sh.n; c = 3u; break;
            case AOV_DP_DU: v = pt.dp_du; c = 3u; break;
            case AOV_DP_DV: v = pt.dp_dv; c = 3u; break;
            case AOV_DUV_DX: case AOV_DUV_DY: c = 2u; break;       // interaction.h:593
            default: break;
        }
        if (!valid) v = v3(0.f);
        if (c > 0u) out[k] = v.x;
        if (c > 1u) out[k + 1] = v.y;
        if (c > 2u) out[k + 2] = v.z;
        k += c;
    }
    return k;
}

} // namespace miw
