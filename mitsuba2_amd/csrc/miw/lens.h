// The sensors of the general sensor route (mi_render_sensor, mi_sensor_sample_ray): the leaf arithmetic, shared by the gfx950
// build (device/sensor_kernel.h) and the host library (host/: ThinLensCamera::sample_ray).
//
// SensorRec (scene.h) holds the projective state both cameras share; LensRec holds what the thin lens adds and which of the two a
// record stands for. The render kernels know SensorRec alone: nothing here is read by them.
#pragma once
#include "base.h"
#include "warp.h"
#include "special.h"
#include "shape.h"
#include "scene.h"

namespace miw {

enum { LENS_PERSPECTIVE = 0, LENS_THINLENS = 1 };

struct LensRec {
    uint32_t kind;                       // LENS_*
    float aperture_radius, focus_distance;
    uint32_t draw_time;                  // shutter_open_time > 0: render_sample draws one next_1d for the time (integrator.cpp:248-250)
};

MIW_HD bool lens_needs_aperture_sample(const LensRec &l) { return l.kind == LENS_THINLENS; }

// thinlens.cpp:166-185, operation for operation. No principal-point offset: the thin lens has none. No ray differentials.
MIW_HD Ray thinlens_sample_ray(const SensorRec &s, const LensRec &l, V2 position_sample, V2 aperture_sample) {
    const V3 near_p = xf_point_persp(s.sample_to_camera, v3(position_sample.x, position_sample.y, 0.f));   // :167-168
    const V2 disk = square_to_uniform_disk_concentric(aperture_sample);                                     // :171
    const V3 aperture_p = v3(l.aperture_radius * disk.x, l.aperture_radius * disk.y, 0.f);
    const V3 focus_p = near_p * (l.focus_distance / near_p.z);                                              // :175
    const V3 d = normalize(focus_p - aperture_p);                                                           // :178
    const float inv_z = rcp(d.z);
    Ray r;
    r.mint = s.near_clip * inv_z;
    r.maxt = s.far_clip * inv_z;
    r.o = xf_point_affine(s.to_world, aperture_p);                                                          // :184
    r.d = xf_vector(s.to_world, d);
    return r;
}

// Sensor::sample_ray of the record's kind; LENS_PERSPECTIVE is sensor_sample_ray (scene.h), bit for bit
MIW_HD Ray sensor_sample(const SensorRec &s, const LensRec &l, V2 position_sample, V2 aperture_sample) {
    if (l.kind == LENS_THINLENS) return thinlens_sample_ray(s, l, position_sample, aperture_sample);
    return sensor_sample_ray(s, position_sample);
}

} // namespace miw
