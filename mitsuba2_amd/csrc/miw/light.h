// The shapeless emitters: point (src/emitters/point.cpp), spot (spot.cpp), directional (directional.cpp) and the constant
// environment (constant.cpp). sample_direction / pdf_direction / eval in float32, in the reference's operation order.
// A light is an EmitterRec whose `type` is one of EMITTER_POINT .. EMITTER_CONSTANT and whose `tri_first` indexes the light
// table (SceneView::lights); it has no shape and no face tables. Point, spot and directional are delta emitters: never hit,
// pdf_direction = 0, DirectionSample::delta set. Only code compiled with Lights = true (scene.h) reads any of this.
#pragma once
#include "base.h"
#include "special.h"
#include "spectrum.h"
#include "warp.h"
#include "shape.h"

namespace miw {

// EmitterRec::type (scene.h). 0: area light on a shape; 1: the environment map; 2 .. 5: a light, also LightRec::type
enum : uint32_t { EMITTER_AREA = 0, EMITTER_ENVMAP = 1, EMITTER_POINT = 2, EMITTER_SPOT = 3, EMITTER_DIRECTIONAL = 4, EMITTER_CONSTANT = 5 };

struct LightRec {
    TexRec value;               // intensity (point, spot), irradiance (directional), radiance (constant): a constant texture
    uint32_t type;              // EMITTER_POINT .. EMITTER_CONSTANT (scene.h)
    uint32_t emitter_index;     // its slot in SceneView::emitters
    float position[3];          // point, spot: trafo.translation()
    float direction[3];         // directional: trafo.transform_affine(Vector3f(0, 0, 1))
    float to_object[16];        // spot: trafo.inverse(), column-major
    float cutoff_angle, cos_cutoff_angle, cos_beam_width, inv_transition_width;   // spot.cpp:88-96
    float dist;                 // directional, constant: 2 x the enlarged bounding-sphere radius (set_scene)
    float pad[2];
};
static_assert(sizeof(LightRec) == 144, "LightRec: nine 16-byte words");

// set_scene of directional.cpp / constant.cpp: max(RayEpsilon, radius * (1 + RayEpsilon))
MIW_HD float light_bsphere_radius(float radius) { return max_(MIW_RAY_EPSILON, radius * (1.f + MIW_RAY_EPSILON)); }

// warp.h:255-260 (circ(z) = sqrt(1 - z^2), frozen as safe_sqrt(fnmadd(z, z, 1)))
MIW_HD V3 square_to_uniform_sphere(V2 sample) {
    float z = fnmadd(2.f, sample.y, 1.f), r = safe_sqrt(fnmadd(z, z, 1.f)), s, c;
    sincos_((2.f * MIW_PI) * sample.x, s, c);
    return v3(r * c, r * s, z);
}
// warp.h:269-276: math::InvFourPi
MIW_HD float square_to_uniform_sphere_pdf() { return 0.07957747154594766788f; }

// What sample_direction fills of a DirectionSample3f
struct LightSample { V3 p, n, d; float dist, pdf; bool delta; };

// SpotLight::falloff_curve (spot.cpp:99-118) without the projection texture (refused at upload)
MIW_HD Spec spot_falloff_curve(const LightRec &l, V3 d, const Wavelengths &wl) {
    Spec result = tex_eval(l.value, wl);
    const V3 local_dir = normalize(d);
    const float cos_theta = local_dir.z;
    const Spec beam_res = cos_theta >= l.cos_beam_width ? result
                                                         : result * ((l.cutoff_angle - acos_(cos_theta)) * l.inv_transition_width);
    return cos_theta <= l.cos_cutoff_angle ? spec(0.f) : beam_res;
}

// PointLight / SpotLight / DirectionalEmitter / ConstantBackgroundEmitter::sample_direction. Returns the emitter value / pdf.
MIW_HD Spec light_sample_direction(const LightRec &l, V3 ref_p, V2 sample, LightSample &ds, const Wavelengths &wl) {
    if (l.type == EMITTER_POINT || l.type == EMITTER_SPOT) {                            // point.cpp:75-99, spot.cpp:141-164
        ds.p = ld3(l.position);
        ds.n = v3(0.f);
        ds.pdf = 1.f;
        ds.delta = true;
        ds.d = ds.p - ref_p;
        ds.dist = norm(ds.d);
        const float inv_dist = rcp(ds.dist);
        ds.d = ds.d * inv_dist;
        if (l.type == EMITTER_POINT) return tex_eval(l.value, wl) * sqr(inv_dist);
        const V3 local_d = xf_vector(l.to_object, -ds.d);
        return spot_falloff_curve(l, local_d, wl) * (inv_dist * inv_dist);
    }
    if (l.type == EMITTER_DIRECTIONAL) {                                            // directional.cpp:106-131
        const V3 d = ld3(l.direction);
        ds.p = ref_p - d * l.dist;
        ds.n = d;
        ds.pdf = 1.f;
        ds.delta = true;
        ds.d = -d;
        ds.dist = l.dist;
        return tex_eval(l.value, wl);
    }
    const V3 d = square_to_uniform_sphere(sample);                 // constant.cpp:91-115
    ds.p = ref_p + d * l.dist;
    ds.n = -d;
    ds.pdf = square_to_uniform_sphere_pdf();
    ds.delta = false;
    ds.d = d;
    ds.dist = l.dist;
    return tex_eval(l.value, wl) / ds.pdf;
}

// pdf_direction: 0 for the delta lights (point.cpp:101-104, spot.cpp:166-168, directional.cpp:133-137); constant.cpp:117-121
MIW_HD float light_pdf_direction(const LightRec &l) { return l.type == EMITTER_CONSTANT ? square_to_uniform_sphere_pdf() : 0.f; }

// eval: 0 for the delta lights; the radiance for the constant environment (constant.cpp:61-65)
MIW_HD Spec light_eval(const LightRec &l, const Wavelengths &wl) { return l.type == EMITTER_CONSTANT ? tex_eval(l.value, wl) : spec(0.f); }

} // namespace miw
