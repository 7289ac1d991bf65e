// ISA probe: every instantiation of k_sample_volpath that mi_sample launches for MI_INTEGRATOR_VOLPATH (see tools/probe_sample.hip;
// tests/test_volpath_kernel_budget.py):
//   cd /tmp/x && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero -c -save-temps <repo>/tools/probe_volpath.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
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
#include "../mitsuba2_amd/csrc/miw/volpath.h"
using namespace miw;
#define MIW_BLOCK 256
#define MIW_CNT_SHARDS 1024
#include "../mitsuba2_amd/csrc/device/trace.h"
#include "../mitsuba2_amd/csrc/device/wavefront_kernels.h"
#include "../mitsuba2_amd/csrc/device/resident_kernel.h"
#include "../mitsuba2_amd/csrc/device/eval_kernels.h"
#include "../mitsuba2_amd/csrc/device/sample_kernel.h"
#include "../mitsuba2_amd/csrc/device/volpath_launch.h"
#include "../mitsuba2_amd/csrc/device/volpath_kernel.h"     /* (its launch function instantiates the kernels of MIW_VOLPATH_LIST) */
