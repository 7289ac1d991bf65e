// The MATS_NESTED instantiations mi_render and mi_sample launch (mask / blendbsdf / null / thindielectric scenes), listed once.
// Part of the translation unit csrc/miwave.hip (included there after the kernels; not a stand-alone header).
//
// Each of them inlines the whole plugin table plus the wrapper resolution, and hipcc generates a translation unit's kernels one
// after the other: compiled inside miwave.hip they double the library's build time. With -DMIW_SPLIT_NESTED=1 (mitsuba2_amd/build.py)
// miwave.hip only DECLARES them (extern template) and csrc/miwave_nested.hip, compiled beside it once per MIW_NESTED_PART = 1 .. MIW_NESTED_PARTS, defines
// them (the parts are sized by what the scalar_spectral compile of each takes); the objects are linked into the one library. Without the macro miwave.hip instantiates them itself where it launches them and
// stays a complete library of its own (tools/build_ab.sh, tools/kernel_resources.py, the debug builds with __device__ counters).
// The kernels are the same either way: an explicit instantiation is the code the implicit one would have been.
// R(UseLog, Tiny, Analytic, Integ) = k_path_resident, PH(Waves, Wide, Placed) = k_path_phased, S(Tiny, Analytic, Integ) = k_sample_rays
// part 1: the logging film (packets, lock-step tree walk; path and direct) and the phase machine (8-wide and 4-wide tree, placed or not)
#define MIW_NESTED_PART_1(R, PH, S)                                                                            \
    R(true, 1, false, INTEG_PATH) R(true, 0, true, INTEG_PATH) R(true, 1, false, INTEG_DIRECT) R(true, 0, true, INTEG_DIRECT) \
    PH(4, 2, true) PH(4, 2, false) PH(4, 1, true) PH(4, 1, false) PH(3, 1, false)
// parts 2, 3: the float64-atomics film, path and direct
#define MIW_NESTED_PART_2(R, PH, S) R(false, 1, false, INTEG_PATH) R(false, 0, true, INTEG_PATH)
#define MIW_NESTED_PART_3(R, PH, S) R(false, 1, false, INTEG_DIRECT) R(false, 0, true, INTEG_DIRECT)
// parts 4, 5: mi_sample, path and direct
#define MIW_NESTED_PART_4(R, PH, S) S(1, false, INTEG_PATH) S(0, true, INTEG_PATH)
#define MIW_NESTED_PART_5(R, PH, S) S(1, false, INTEG_DIRECT) S(0, true, INTEG_DIRECT)
#define MIW_NESTED_PARTS 5

#define MIW_NESTED_R(UL, T, A, I) MIW_NESTED_KW template __global__ void k_path_resident<UL, T, MATS_NESTED, A, I>(RenderParams, SceneView, LaneQueues, double *, Counters *, TraceLds, uint32_t, TileArgs, uint32_t *);
#define MIW_NESTED_PH(WV, W, PL) MIW_NESTED_KW template __global__ void k_path_phased<MATS_NESTED, true, MIW_PHASE_SPEC != 0, WV, W, PL>(RenderParams, SceneView, LaneQueues, Counters *, TraceLds, uint32_t, uint32_t *);
#define MIW_NESTED_S(T, A, I) MIW_NESTED_KW template __global__ void k_sample_rays<T, MATS_NESTED, A, I>(RenderParams, SceneView, SampleIO, TraceLds, uint32_t *);
#if defined(MIW_NESTED_PART)                       /* csrc/miwave_nested.hip: this part's definitions */
#define MIW_NESTED_KW
#if MIW_NESTED_PART == 1
MIW_NESTED_PART_1(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#elif MIW_NESTED_PART == 2
MIW_NESTED_PART_2(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#elif MIW_NESTED_PART == 3
MIW_NESTED_PART_3(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#elif MIW_NESTED_PART == 4
MIW_NESTED_PART_4(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#elif MIW_NESTED_PART == 5
MIW_NESTED_PART_5(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#else
#error "MIW_NESTED_PART must be 1 .. MIW_NESTED_PARTS"
#endif
#undef MIW_NESTED_KW
#elif defined(MIW_SPLIT_NESTED)                    /* csrc/miwave.hip of a split build: declarations only */
#define MIW_NESTED_KW extern
MIW_NESTED_PART_1(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
MIW_NESTED_PART_2(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
MIW_NESTED_PART_3(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
MIW_NESTED_PART_4(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
MIW_NESTED_PART_5(MIW_NESTED_R, MIW_NESTED_PH, MIW_NESTED_S)
#undef MIW_NESTED_KW
#endif
#undef MIW_NESTED_R
#undef MIW_NESTED_PH
#undef MIW_NESTED_S
