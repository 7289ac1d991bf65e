// The volpath integrator's kernel as mi_sample's launch sees it: one launch function. Part of the translation unit csrc/miwave.hip
// (included there after the kernel headers; not a stand-alone header). In a split build (-DMIW_SPLIT_VOLPATH=1,
// mitsuba2_amd/build.py) the kernels and this function are compiled in csrc/miwave_volpath.hip and linked into the one library;
// without the macro miwave.hip includes device/volpath_kernel.h itself.
//
// The instantiations that exist: k_sample_volpath<Tiny, MATS_NESTED, false> for Tiny = 1 — packet scenes — and 0 — tree scenes:
// MATS_NESTED holds every BSDF plugin (MATS_ALL plus the wrappers and the null / thindielectric leaves, which a medium boundary
// usually carries). Scenes with shapeless emitters or analytic shapes are refused by name before the launch.
// volpath_launch_eval: MI_EVAL_MEDIUM / MI_EVAL_PHASE over device arrays.
// volpath_waves: wavefronts per SIMD the kernel of that shape is compiled for (the persistent grid's size).
// Returns hipErrorInvalidValue for a tuple outside the list.
#if !MIW_SPECTRAL
unsigned volpath_waves(int tiny);
hipError_t volpath_launch(hipStream_t s, bool say, int tiny, int mats, bool analytic, dim3 grid, size_t lds_bytes, const RenderParams &P,
                          const SceneView &sc, const MediaView &mv, const SampleIO &io, const TraceLds &cfg, uint32_t *next_ray, uint32_t *capped);
hipError_t volpath_launch_eval(hipStream_t s, int op, const MediaView &mv, const float *in, int is, float *out, int os, uint64_t n);
#endif
