// Participating media: HomogeneousMedium (src/media/homogeneous.cpp over src/librender/medium.cpp), the isotropic and
// Henyey-Greenstein phase functions (src/phase/isotropic.cpp, hg.cpp), BSDF::eval_null_transmission of the plugin table and the
// medium a surface hands a ray over to (interaction.h:178-200, shape.h:341-348). Leaf arithmetic shared by the gfx950 kernel
// (device/volpath_kernel.h) and the host compile (mih_medium_* / mih_phase_*): float32, the reference's operation order, the
// frozen Enoki semantics of base.h (array / scalar = array * rcp(scalar); array / array = IEEE division per component).
#pragma once
#include "base.h"
#include "warp.h"
#include "special.h"
#include "bsdf.h"
#include "light.h"

namespace miw {

enum : uint32_t { PHASE_ISOTROPIC = 0, PHASE_HG = 1 };            // = MI_PHASE_* of include/miwave.h
// HomogeneousMedium after its constructor ran (the layout of mi_medium): sigma_t = `sigma_t` * `scale` (homogeneous.cpp:30-32),
// both volumes constant.
struct MediumRec {
    float sigma_t[3], albedo[3];
    uint32_t has_spectral_extinction, sample_emitters;             // homogeneous.cpp:27, medium.cpp:29
    uint32_t phase; float g;
};
// The media of a scene as the volpath kernel sees them. A medium REFERENCE is index + 1, 0 = none (include/miwave.h).
struct MediaView {
    const MediumRec *media; uint32_t media_count;
    const uint32_t *shape_media;                                    // nullptr, or per shape: interior, exterior
    uint32_t start_medium;
};

MIW_HD float spec_at(const Spec &s, uint32_t ch) {
#if MIW_SPECTRAL
    return s.c[ch];
#else
    return ch == 0u ? s.x : ch == 1u ? s.y : s.z;
#endif
}
MIW_HD Spec medium_sigma_t(const MediumRec &m) {
#if MIW_SPECTRAL
    return spec(m.sigma_t[0]);                                      // (not served: see miw/volpath.h)
#else
    return v3(m.sigma_t[0], m.sigma_t[1], m.sigma_t[2]);
#endif
}
MIW_HD Spec medium_albedo(const MediumRec &m) {
#if MIW_SPECTRAL
    return spec(m.albedo[0]);
#else
    return v3(m.albedo[0], m.albedo[1], m.albedo[2]);
#endif
}
MIW_HD Spec spec_exp(Spec a) {
#if MIW_SPECTRAL
    Spec r; for (int i = 0; i < 4; ++i) r.c[i] = exp_(a.c[i]); return r;
#else
    return v3(exp_(a.x), exp_(a.y), exp_(a.z));
#endif
}
MIW_HD Spec spec_div(Spec a, Spec b) {                              // array / array
#if MIW_SPECTRAL
    Spec r; for (int i = 0; i < 4; ++i) r.c[i] = a.c[i] / b.c[i]; return r;
#else
    return div3(a, b);
#endif
}

// MediumInteraction3f, the fields volpath reads. sigma_n = 0 and combined_extinction = sigma_t for a homogeneous medium
// (homogeneous.cpp:34-49), so neither is stored.
struct MediumInteraction {
    float t, mint;                   // t = inf: no interaction (is_valid() false)
    float ts;                        // sampled_t, whether it became t or not
    V3 p;                            // ray(sampled_t), also when the interaction is not valid
    Spec sigma_s, sigma_t;
};

// Medium::sample_interaction, medium.cpp:36-75, with HomogeneousMedium::intersect_aabb = (true, 0, inf) (homogeneous.cpp:51-54)
MIW_HD MediumInteraction medium_sample_interaction(const MediumRec &m, const Ray &ray, float sample, uint32_t channel) {
    MediumInteraction mi;
    const float mint = max_(ray.mint, 0.f), maxt = min_(ray.maxt, MIW_INFINITY);      // :53-54
    const Spec combined_extinction = medium_sigma_t(m);
    const float me = spec_at(combined_extinction, channel);                           // :57-63
    const float sampled_t = mint + (-log_(1.f - sample) / me);                        // :65
    const bool valid_mi = sampled_t <= maxt;                                          // :66
    mi.t = valid_mi ? sampled_t : MIW_INFINITY;
    mi.p = v3(fmadd(ray.d.x, sampled_t, ray.o.x), fmadd(ray.d.y, sampled_t, ray.o.y), fmadd(ray.d.z, sampled_t, ray.o.z));   // ray(t), ray.h:65
    mi.mint = mint; mi.ts = sampled_t;
    mi.sigma_t = combined_extinction;                                                 // homogeneous.cpp:45-48
    mi.sigma_s = combined_extinction * medium_albedo(m);
    return mi;
}

// Medium::eval_tr_and_pdf, medium.cpp:80-89 (si_t = si.t)
MIW_HD void medium_eval_tr_and_pdf(const MediumInteraction &mi, float si_t, Spec &tr, Spec &pdf) {
    const float t = min_(mi.t, si_t) - mi.mint;
    tr = spec_exp(-t * mi.sigma_t);
    pdf = si_t < mi.t ? tr : tr * mi.sigma_t;
}
// throughput *= select(tr_pdf > 0, tr / tr_pdf, 0), volpath.cpp:116 / :310 / :404
MIW_HD Spec medium_tr_weight(Spec tr, Spec pdf, uint32_t channel) {
    const float tr_pdf = spec_at(pdf, channel);
    return tr_pdf > 0.f ? tr / tr_pdf : spec(0.f);
}

// ---- phase functions: isotropic.cpp:30-45, hg.cpp:51-81 (wi = -ray.d, the frame is Frame3f(ray.d), medium.cpp:42-43) ----
MIW_HD float hg_eval(float g, float cos_theta) {
    const float temp = 1.f + g * g + 2.f * g * cos_theta;
    return 0.07957747154594766788f * (1.f - g * g) / (temp * __builtin_sqrtf(temp));
}
MIW_HD float phase_eval(const MediumRec &m, V3 ray_d, V3 wo) {
    if (m.phase == PHASE_HG) return hg_eval(m.g, dot(wo, -ray_d));
    return square_to_uniform_sphere_pdf();
}
MIW_HD V3 phase_sample(const MediumRec &m, V3 ray_d, V2 sample, float &pdf) {
    if (m.phase == PHASE_HG) {
        const float g = m.g;
        float cos_theta;
        if (abs_(g) < MIW_EPSILON) {
            cos_theta = 1.f - 2.f * sample.x;
        } else {
            const float sqr_term = (1.f - g * g) / (1.f - g + 2.f * g * sample.x);
            cos_theta = (1.f + g * g - sqr_term * sqr_term) / (2.f * g);
        }
        const float sin_theta = safe_sqrt(1.f - cos_theta * cos_theta);
        float sin_phi, cos_phi;
        sincos_(2.f * MIW_PI * sample.y, sin_phi, cos_phi);
        Frame f; f.n = ray_d;
        coordinate_system(f.n, f.s, f.t);
        pdf = hg_eval(g, -cos_theta);
        return to_world(f, v3(sin_theta * cos_phi, sin_theta * sin_phi, cos_theta));
    }
    pdf = square_to_uniform_sphere_pdf();
    return square_to_uniform_sphere(sample);
}

// ---- BSDF::eval_null_transmission for record `index` of the table: 0 by default (src/librender/bsdf.cpp:11; twosided and
// blendbsdf do not override it), null.cpp:69, thindielectric.cpp:162-176, mask.cpp:158-161 over its nested record ----
MIW_HD Spec bsdf_null_transmission(const BsdfRec *table, uint32_t index, V3 wi, const TexCtx &tc) {
    const BsdfRec *b = table + index, *mask = nullptr;
    if (b->type == BSDF_TYPE_MASK) { mask = b; b = table + b->back; }
    Spec v = spec(0.f);
    if (!(b->flags & BSDF_REC_TWOSIDED)) {
        if (b->type == BSDF_TYPE_NULL) v = spec(1.f);
        else if (b->type == BSDF_TYPE_THINDIELECTRIC) v = spec(1.f - thindielectric_reflectance(*b, wi)) * tex_eval(b->tex[1], tc);
    }
    if (mask) {
        const float opacity = tex_eval_1_clamped(mask->tex[0], tc);
        v = spec(1.f) + (-1.f) * (opacity * (spec(1.f) + (-1.f) * v));             // 1 - opacity * (1 - nested)
    }
    return v;
}

// si.is_medium_transition() / si.target_medium(d): the exterior where dot(d, n) > 0 with the geometric normal, else the interior
MIW_HD bool is_medium_transition(const MediaView &mv, uint32_t shape) {
    return mv.shape_media && (mv.shape_media[2u * shape] | mv.shape_media[2u * shape + 1u]) != 0u;
}
MIW_HD uint32_t target_medium(const MediaView &mv, uint32_t shape, V3 d, V3 n) {
    return dot(d, n) > 0.f ? mv.shape_media[2u * shape + 1u] : mv.shape_media[2u * shape];
}

} // namespace miw
