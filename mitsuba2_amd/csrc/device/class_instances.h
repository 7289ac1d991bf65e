// The MATS_NESTED (mask / blendbsdf / null / thindielectric scenes) and MATS_LIGHTS (scenes with a point / spot / directional / constant
// emitter) instantiations mi_render and mi_sample launch, listed once for both classes: MATS_LIGHTS is the MATS_NESTED table plus the light
// table (miw/light.h), route for route. Part of the translation unit csrc/miwave.hip (included there after the kernels; not a stand-alone header).
//
// Each of them inlines the whole plugin table plus the wrapper resolution, and hipcc generates a translation unit's kernels one
// after the other: compiled inside miwave.hip they double the library's build time. With -DMIW_SPLIT_CLASSES=1 (mitsuba2_amd/build.py)
// miwave.hip only DECLARES them (extern template) and csrc/miwave_class.hip, compiled beside it once per class and part (-DMIW_CLASS=MATS_NESTED | MATS_LIGHTS,
// -DMIW_CLASS_PART = 1 .. MIW_CLASS_PARTS), defines them (the parts are sized by what the scalar_spectral compile of each takes); the objects are linked into
// the one library. Without the macro miwave.hip instantiates them itself where it launches them and
// stays a complete library of its own (tools/build_ab.sh, tools/kernel_resources.py, the debug builds with __device__ counters).
// The kernels are the same either way: an explicit instantiation is the code the implicit one would have been.
// M = the class; R(M, UseLog, Tiny, Analytic, Integ) = k_path_resident, PH(M, Waves, Wide, Placed) = k_path_phased, S(M, Tiny, Analytic, Integ) = k_sample_rays
// part 1: the logging film (packets, lock-step tree walk; path and direct) and the phase machine (8-wide and 4-wide tree, placed or not)
#define MIW_CLASS_PART_1(M, R, PH, S)                                                                          \
    R(M, true, 1, false, INTEG_PATH) R(M, true, 0, true, INTEG_PATH) R(M, true, 1, false, INTEG_DIRECT) R(M, true, 0, true, INTEG_DIRECT) \
    PH(M, 4, 2, true) PH(M, 4, 2, false) PH(M, 4, 1, true) PH(M, 4, 1, false) PH(M, 3, 1, false)
// parts 2, 3: the float64-atomics film, path and direct
#define MIW_CLASS_PART_2(M, R, PH, S) R(M, false, 1, false, INTEG_PATH) R(M, false, 0, true, INTEG_PATH)
#define MIW_CLASS_PART_3(M, R, PH, S) R(M, false, 1, false, INTEG_DIRECT) R(M, false, 0, true, INTEG_DIRECT)
// parts 4, 5: mi_sample, path and direct
#define MIW_CLASS_PART_4(M, R, PH, S) S(M, 1, false, INTEG_PATH) S(M, 0, true, INTEG_PATH)
#define MIW_CLASS_PART_5(M, R, PH, S) S(M, 1, false, INTEG_DIRECT) S(M, 0, true, INTEG_DIRECT)
#define MIW_CLASS_PARTS 5

#define MIW_CLASS_R(M, UL, T, A, I) MIW_CLASS_KW template __global__ void k_path_resident<UL, T, M, A, I>(RenderParams, SceneView, LaneQueues, double *, Counters *, TraceLds, uint32_t, TileArgs, uint32_t *);
#define MIW_CLASS_PH(M, WV, W, PL) MIW_CLASS_KW template __global__ void k_path_phased<M, true, MIW_PHASE_SPEC != 0, WV, W, PL>(RenderParams, SceneView, LaneQueues, Counters *, TraceLds, uint32_t, uint32_t *);
#define MIW_CLASS_S(M, T, A, I) MIW_CLASS_KW template __global__ void k_sample_rays<T, M, A, I>(RenderParams, SceneView, SampleIO, TraceLds, uint32_t *);
#define MIW_CLASS_PART_(K, M) MIW_CLASS_PART_##K(M, MIW_CLASS_R, MIW_CLASS_PH, MIW_CLASS_S)
#define MIW_CLASS_PART_OF(K, M) MIW_CLASS_PART_(K, M)
#if defined(MIW_CLASS_PART)                        /* csrc/miwave_class.hip: the definitions of this part of class MIW_CLASS */
#if MIW_CLASS_PART < 1 || MIW_CLASS_PART > MIW_CLASS_PARTS
#error "MIW_CLASS_PART must be 1 .. MIW_CLASS_PARTS"
#endif
#define MIW_CLASS_KW
MIW_CLASS_PART_OF(MIW_CLASS_PART, MIW_CLASS)
#undef MIW_CLASS_KW
#elif defined(MIW_SPLIT_CLASSES)                   /* csrc/miwave.hip of a split build: declarations only */
#define MIW_CLASS_KW extern
#define MIW_CLASS_ALL_PARTS(M) MIW_CLASS_PART_OF(1, M) MIW_CLASS_PART_OF(2, M) MIW_CLASS_PART_OF(3, M) MIW_CLASS_PART_OF(4, M) MIW_CLASS_PART_OF(5, M)
MIW_CLASS_ALL_PARTS(MATS_NESTED)
MIW_CLASS_ALL_PARTS(MATS_LIGHTS)
#undef MIW_CLASS_ALL_PARTS
#undef MIW_CLASS_KW
#endif
#undef MIW_CLASS_PART_OF
#undef MIW_CLASS_PART_
#undef MIW_CLASS_R
#undef MIW_CLASS_PH
#undef MIW_CLASS_S
