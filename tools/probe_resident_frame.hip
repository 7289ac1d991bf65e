// ISA probe: only the FRAME twin of the C2 kernel, k_path_resident<true, 2, MATS_DIFFUSE, ..., Feat = FEAT_FRAME> — the lean kernel of tools/probe_resident_lean.hip
// with what a full frame's launch fixes compiled in: chunk jobs from one queue, 16-byte log records, no tail priorities, the leaf filter on (device/resident_kernel.h). Compile it
// the same way as the other two:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero -S --cuda-device-only tools/probe_resident_frame.hip -o frame.s
//   python tools/valu_count.py frame.s _Z15k_path_residentILb1ELi2ELi1ELb0ELj0ELb0ELi0ELj16E
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
template __global__ void k_path_resident<true, 2, 1, false, 0u, false, 0, 16u>(RenderParams, SceneView, LaneQueues, double *, Counters *, TraceLds, unsigned int, TileArgs, unsigned int *);
