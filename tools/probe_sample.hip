// ISA probe: every instantiation of k_sample_rays that mi_sample launches (see tools/probe_phased.hip; tests/test_sample_kernel_budget.py):
//   cd /tmp/x && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero -c -save-temps <repo>/tools/probe_sample.hip
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
#define PROBE(T, M, A, I) template __global__ void k_sample_rays<T, M, A, I>(RenderParams, SceneView, SampleIO, TraceLds, unsigned int *)
#ifndef MIW_PROBE_DIRECT
PROBE(2, MATS_DIFFUSE, false, INTEG_PATH); PROBE(1, MATS_DIFFUSE, false, INTEG_PATH); PROBE(2, MATS_PLAIN, false, INTEG_PATH); PROBE(1, MATS_PLAIN, false, INTEG_PATH);
PROBE(1, MATS_ALL, false, INTEG_PATH); PROBE(0, MATS_ALL, true, INTEG_PATH); PROBE(0, MATS_TRIO, false, INTEG_PATH); PROBE(0, MATS_PLAIN, false, INTEG_PATH); PROBE(0, MATS_PLAIN, true, INTEG_PATH);
#else
PROBE(1, MATS_ALL, false, INTEG_DIRECT); PROBE(1, MATS_PLAIN, false, INTEG_DIRECT); PROBE(0, MATS_ALL, true, INTEG_DIRECT); PROBE(0, MATS_PLAIN, true, INTEG_DIRECT);
#endif
