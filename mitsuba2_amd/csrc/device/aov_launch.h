// The aov integrator's kernels as mi_render_aov sees them: their argument records and one launch function per kernel.
// Part of the translation unit csrc/miwave.hip (included there after the kernel headers; not a stand-alone header). In a split build
// (-DMIW_SPLIT_AOV=1, mitsuba2_amd/build.py) the kernels and these functions are compiled in csrc/miwave_aov.hip and linked into the
// one library; without the macro miwave.hip includes device/aov_kernel.h itself and stays a complete library of its own.
struct AovArgs {
    U4 *st;                          // per pixel lane: PCG32 state (x, y), LF_DONE for a lane outside the film (z), samples done (w) — k_init_pixels' record
    const uint32_t *pixel;           // per lane: x | y << 16
    float *log;                      // [lane][sample][stride] (miw/film_gather_n.h)
    const uint8_t *types;            // n_types AOV_* values (device memory)
    uint32_t n_lanes, spp, stride, n_types, n_geo;   // n_geo: channels the types add up to
    // with a child integrator: the ray and the sampler state after the camera draws, in mi_sample's device SoA layout (index = lane); else nullptr
    float *ray[8]; uint64_t *rng_state;
};
// the four launches (block of MIW_BLOCK threads each); `tiny` / `analytic`: the instantiation of k_aov_samples
hipError_t aov_launch_samples(bool tiny, bool analytic, size_t lds_bytes, hipStream_t s, const RenderParams &P, const SceneView &sc, const AovArgs &A,
                              uint32_t j0, uint32_t j1, const TraceLds &cfg);
hipError_t aov_launch_finish(hipStream_t s, const AovArgs &A, const float *spec, const uint8_t *valid, uint32_t j);
hipError_t aov_launch_film(hipStream_t s, const FilmRec *film_dev, const FilmRec &film_host, const BlockReplayArgsN &a, uint32_t n_tiles, float *tiles);
hipError_t aov_launch_merge(hipStream_t s, const FilmRec *film_dev, const FilmRec &film_host, const BlockReplayArgsN &a, const float *tiles, float *film, bool accumulate);
