// The MATS_LIGHTS instantiations mi_render and mi_sample launch (scenes with a point / spot / directional / constant emitter), listed
// once. Part of the translation unit csrc/miwave.hip (included there after the kernels; not a stand-alone header).
//
// The scheme of device/nested_instances.h, route for route: MATS_LIGHTS is the MATS_NESTED table plus the light table (miw/light.h), so each
// of these kernels costs what its MATS_NESTED sibling costs to compile. With -DMIW_SPLIT_LIGHTS=1 (mitsuba2_amd/build.py) miwave.hip only DECLARES
// them (extern template) and csrc/miwave_lights.hip, compiled beside it once per MIW_LIGHTS_PART = 1 .. MIW_LIGHTS_PARTS, defines them; the
// objects are linked into the one library. Without the macro miwave.hip instantiates them itself where it launches them.
// R(UseLog, Tiny, Analytic, Integ) = k_path_resident, PH(Waves, Wide, Placed) = k_path_phased, S(Tiny, Analytic, Integ) = k_sample_rays
// part 1: the logging film (packets, lock-step tree walk; path and direct) and the phase machine (8-wide and 4-wide tree, placed or not)
#define MIW_LIGHTS_PART_1(R, PH, S)                                                                            \
    R(true, 1, false, INTEG_PATH) R(true, 0, true, INTEG_PATH) R(true, 1, false, INTEG_DIRECT) R(true, 0, true, INTEG_DIRECT) \
    PH(4, 2, true) PH(4, 2, false) PH(4, 1, true) PH(4, 1, false) PH(3, 1, false)
// parts 2, 3: the float64-atomics film, path and direct
#define MIW_LIGHTS_PART_2(R, PH, S) R(false, 1, false, INTEG_PATH) R(false, 0, true, INTEG_PATH)
#define MIW_LIGHTS_PART_3(R, PH, S) R(false, 1, false, INTEG_DIRECT) R(false, 0, true, INTEG_DIRECT)
// parts 4, 5: mi_sample, path and direct
#define MIW_LIGHTS_PART_4(R, PH, S) S(1, false, INTEG_PATH) S(0, true, INTEG_PATH)
#define MIW_LIGHTS_PART_5(R, PH, S) S(1, false, INTEG_DIRECT) S(0, true, INTEG_DIRECT)
#define MIW_LIGHTS_PARTS 5

#define MIW_LIGHTS_R(UL, T, A, I) MIW_LIGHTS_KW template __global__ void k_path_resident<UL, T, MATS_LIGHTS, A, I>(RenderParams, SceneView, LaneQueues, double *, Counters *, TraceLds, uint32_t, TileArgs, uint32_t *);
#define MIW_LIGHTS_PH(WV, W, PL) MIW_LIGHTS_KW template __global__ void k_path_phased<MATS_LIGHTS, true, MIW_PHASE_SPEC != 0, WV, W, PL>(RenderParams, SceneView, LaneQueues, Counters *, TraceLds, uint32_t, uint32_t *);
#define MIW_LIGHTS_S(T, A, I) MIW_LIGHTS_KW template __global__ void k_sample_rays<T, MATS_LIGHTS, A, I>(RenderParams, SceneView, SampleIO, TraceLds, uint32_t *);
#if defined(MIW_LIGHTS_PART)                       /* csrc/miwave_lights.hip: this part's definitions */
#define MIW_LIGHTS_KW
#if MIW_LIGHTS_PART == 1
MIW_LIGHTS_PART_1(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#elif MIW_LIGHTS_PART == 2
MIW_LIGHTS_PART_2(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#elif MIW_LIGHTS_PART == 3
MIW_LIGHTS_PART_3(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#elif MIW_LIGHTS_PART == 4
MIW_LIGHTS_PART_4(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#elif MIW_LIGHTS_PART == 5
MIW_LIGHTS_PART_5(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#else
#error "MIW_LIGHTS_PART must be 1 .. MIW_LIGHTS_PARTS"
#endif
#undef MIW_LIGHTS_KW
#elif defined(MIW_SPLIT_LIGHTS)                    /* csrc/miwave.hip of a split build: declarations only */
#define MIW_LIGHTS_KW extern
MIW_LIGHTS_PART_1(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
MIW_LIGHTS_PART_2(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
MIW_LIGHTS_PART_3(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
MIW_LIGHTS_PART_4(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
MIW_LIGHTS_PART_5(MIW_LIGHTS_R, MIW_LIGHTS_PH, MIW_LIGHTS_S)
#undef MIW_LIGHTS_KW
#endif
#undef MIW_LIGHTS_R
#undef MIW_LIGHTS_PH
#undef MIW_LIGHTS_S
