// ISA probe: the MATS_LIGHTS instantiations mi_render and mi_sample launch for a scene with a point / spot / directional / constant emitter,
// each beside its MATS_NESTED sibling (see tools/probe_nested.hip; tests/test_lights_kernel_budget.py):
//   cd /tmp/x && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero -c -save-temps <repo>/tools/probe_lights.hip
//   -DMIW_PROBE_LIGHTS=1: k_sample_rays, =2: k_path_resident (packet, lock-step tree, direct), =3: k_path_phased
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../include/miwave.h"
#include "../mitsuba2_amd/csrc/miw/base.h"
#include "../mitsuba2_amd/csrc/miw/rng.h"
#include "../mitsuba2_amd/csrc/miw/warp.h"
#include "../mitsuba2_amd/csrc/miw/special.h"
#include "../mitsuba2_amd/csrc/miw/shape.h"
#include "../mitsuba2_amd/csrc/miw/bsdf.h"
#include "../mitsuba2_amd/csrc/miw/scene.h"
#include "../mitsuba2_amd/csrc/miw/film.h"
#include "../mitsuba2_amd/csrc/miw/bvh.h"
#include "../mitsuba2_amd/csrc/miw/bvh4.h"
#include "../mitsuba2_amd/csrc/miw/bvh8.h"
#include "../mitsuba2_amd/csrc/miw/path.h"
#include "../mitsuba2_amd/csrc/miw/direct.h"
using namespace miw;
#define MIW_BLOCK 256
#define MIW_CNT_SHARDS 1024
#include "../mitsuba2_amd/csrc/device/trace.h"
#include "../mitsuba2_amd/csrc/device/wavefront_kernels.h"
#include "../mitsuba2_amd/csrc/device/resident_kernel.h"
#include "../mitsuba2_amd/csrc/device/eval_kernels.h"
#include "../mitsuba2_amd/csrc/device/sample_kernel.h"
#if MIW_PROBE_LIGHTS == 1
#define PROBE(T, M, A, I) template __global__ void k_sample_rays<T, M, A, I>(RenderParams, SceneView, SampleIO, TraceLds, unsigned int *)
PROBE(1, MATS_LIGHTS, false, INTEG_PATH); PROBE(0, MATS_LIGHTS, true, INTEG_PATH); PROBE(1, MATS_NESTED, false, INTEG_PATH); PROBE(0, MATS_NESTED, true, INTEG_PATH);
PROBE(1, MATS_LIGHTS, false, INTEG_DIRECT); PROBE(0, MATS_LIGHTS, true, INTEG_DIRECT); PROBE(1, MATS_NESTED, false, INTEG_DIRECT); PROBE(0, MATS_NESTED, true, INTEG_DIRECT);
#elif MIW_PROBE_LIGHTS == 2
#define PROBE(T, M, A, I) template __global__ void k_path_resident<true, T, M, A, I>(RenderParams, SceneView, LaneQueues, double *, Counters *, TraceLds, uint32_t, TileArgs, uint32_t *)
PROBE(1, MATS_LIGHTS, false, INTEG_PATH); PROBE(0, MATS_LIGHTS, true, INTEG_PATH); PROBE(1, MATS_NESTED, false, INTEG_PATH); PROBE(0, MATS_NESTED, true, INTEG_PATH);
PROBE(1, MATS_LIGHTS, false, INTEG_DIRECT); PROBE(0, MATS_LIGHTS, true, INTEG_DIRECT); PROBE(1, MATS_NESTED, false, INTEG_DIRECT); PROBE(0, MATS_NESTED, true, INTEG_DIRECT);
#elif MIW_PROBE_LIGHTS == 3
#include "../mitsuba2_amd/csrc/device/phased_kernel.h"
#define PROBE(M, W) template __global__ void k_path_phased<M, true, MIW_PHASE_SPEC != 0, 4, W, false>(RenderParams, SceneView, LaneQueues, Counters *, TraceLds, uint32_t, uint32_t *)
PROBE(MATS_LIGHTS, 2); PROBE(MATS_NESTED, 2); PROBE(MATS_LIGHTS, 1); PROBE(MATS_NESTED, 1);
#endif
