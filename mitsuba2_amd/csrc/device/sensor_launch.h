// The general sensor route's kernels as mi_render_sensor and mi_sensor_sample_ray see them: their argument records and one launch
// function per kernel. Part of the translation unit csrc/miwave.hip (included there after the kernel headers; not a stand-alone
// header). In a split build (-DMIW_SPLIT_SENSOR=1, mitsuba2_amd/build.py) the kernels and these functions are compiled in
// csrc/miwave_sensor.hip and linked into the one library; without the macro miwave.hip includes device/sensor_kernel.h itself.
struct SensorStepArgs {
    SensorRec sensor; LensRec lens;
    float crop_f[4];                 // (float) crop_x, crop_y, crop_w, crop_h (integrator.cpp:254-256)
    uint32_t warn_negative;          // FilmRec::warn_negative
    uint32_t n_lanes, spp;
    // per pixel lane, in HBM between the launches
    U4 *st;                          // PCG32 state (x, y), LF_DONE for a lane outside the film (z), samples begun (w) — k_init_pixels' record
    const uint32_t *pixel;           // x | y << 16
    F2 *pos;                         // the film position of the sample under way
    F4 *wl, *weight;                 // scalar_spectral: its four wavelengths and its ray weight; else nullptr
    float *log;                      // [lane][sample][MIW_AOV_LOG_HEAD] (miw/film_gather_n.h, nch = 5)
    // k_sample_rays' device SoA (index = lane): in — ray, wavelengths (= wl), sampler state; out — spectrum, mask, sampler state
    float *ray[8]; uint64_t *rng_state; const float *spec; const uint8_t *valid;
};
struct SensorRaysArgs {              // mi_sensor_sample_ray: Sensor::sample_ray for n samples
    SensorRec sensor; LensRec lens;
    const float *position, *aperture, *wavelength_sample;   // 2n, 2n or nullptr = (.5, .5), n or nullptr
    float *ray[8], *wavelengths, *weights;                  // n each; 4n and MIW_SPEC_N n, or nullptr
    uint32_t n;
};
// `finish`: sample j - 1 of every lane is logged; `begin`: sample j is drawn. The first launch of a frame only begins, the last only finishes.
hipError_t sensor_launch_step(hipStream_t s, const SensorStepArgs &A, uint32_t j, bool finish, bool begin);
hipError_t sensor_launch_rays(hipStream_t s, const SensorRaysArgs &A);
