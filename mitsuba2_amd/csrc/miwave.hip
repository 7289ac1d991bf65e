// libmiwave.so — gfx950 kernels and the C ABI declared in include/miwave.h. One translation unit (the build compiles the kernels of
// two material classes beside it, device/class_instances.h):
//   miw/*.h                      leaf arithmetic shared with the CPU checker (float32, fixed operation order)
//   device/trace.h               LDS staging, packet sweep + leaf filter, LDS-stack BVH walk, trace2
//   device/wavefront_kernels.h   plan 1: k_init_lanes, k_trace<closest|any>, k_shade over SoA queues in HBM
//   device/resident_kernel.h     plan 2: k_init_pixels, the pixel queue, k_path_resident (path / direct)
//   device/phased_kernel.h       plan 2 over a tree: k_path_phased (wave-level phase machine: node steps / triangle tests / shade)
//   device/stream_trace.h        plan 1 over a tree: k_trace_stream (persistent walk kernel, dynamic ray fetch), k_sort_hits
//   device/film_kernels.h        k_film_resolve, k_film_groups (16-byte class records), k_film_blocks (24-byte position log), k_film_merge
//   device/eval_kernels.h        k_trace_soa (mi_trace), k_eval (mi_eval)
//   lbvh_device.h, bvh4_device.h device LBVH builder, level-synchronous collapse into the 4-wide tree
// followed here by the host side: context, scene upload, BVH build, mi_trace, mi_render, mi_eval, mi_selftest.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <string>
#include <vector>
#include <chrono>
#include <atomic>
#include <cmath>
#include <map>
#include <string>
#include <algorithm>

#include "../../include/miwave.h"
#include "kernel_pick.h"
#if defined(MIW_CLASS_PART) || defined(MIW_AOV_UNIT) || defined(MIW_SENSOR_UNIT) || defined(MIW_VOLPATH_UNIT)   /* miwave_class.hip, miwave_aov.hip, miwave_sensor.hip, miwave_volpath.hip: the kernel headers alone */
#define MIW_KERNELS_ONLY 1
#endif
// Section clock (debug builds, -DMIW_SECTION_PROFILE=1): wall cycles per wavefront between markers, summed
// into g_sections and printed by mi_render when MIW_DEBUG is set. Not compiled into the product library.
#if defined(MIW_SECTION_PROFILE)
__device__ unsigned long long g_sections[16];
#endif
#if defined(MIW_PHASE_STATS)
__device__ unsigned long long g_phase_stats[15];   // k_path_phased: per bucket (node trip, triangle trip, walk end, shade, vote) runs, lanes, wall cycles
#endif
#if defined(MIW_WALK_STATS)
__device__ unsigned long long g_walk_stats[8];     // per ray kind (closest 0.., any 4..): node lane-steps, triangle lane-steps, rays
__device__ float g_walk_statsf[8];                 //                                      node wave-steps, triangle wave-steps
#endif
#if defined(MIW_VERIFY_FILTER)
__device__ unsigned int g_verify_n;
__device__ float g_verify[16 * 16];
#endif
#if defined(MIW_SECTION_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ unsigned long long *miw_sec_buf() { __shared__ unsigned long long b[4][16]; return &b[threadIdx.x >> 6][0]; }
#define MIW_SECTION(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); unsigned long long *b_ = miw_sec_buf(); \
        if ((threadIdx.x & 63u) == (unsigned) __ffsll((long long) __ballot(1)) - 1u) { b_[i] += now_ - b_[15]; b_[15] = now_; } } while (0)
#endif
#include "miw/base.h"
#include "miw/rng.h"
#include "miw/warp.h"
#include "miw/special.h"
#include "miw/shape.h"
#include "miw/bsdf.h"
#include "miw/scene.h"
#include "miw/film.h"
#include "miw/bvh.h"
#include "miw/path.h"
#include "miw/direct.h"
#if defined(MIW_KERNELS_ONLY)            /* miwave_class.hip: the path kernels alone (device/class_instances.h); the library's other kernels have one definition, here */
#include "miw/bvh4.h"
#include "miw/bvh8.h"
#define MIW_KERNEL static __global__    /* ... and those of their headers that are no templates stay out of its objects */
#else
#include "rect_build.h"
#include "miw/film_gather.h"
#include "texture_build.h"
#include "bvh_build.h"
#include "bvh4_build.h"
#include "envmap_build.h"
#include "film_classes.h"
#include "film_chains.h"
#include "render_plan.h"
#include "lbvh_device.h"
#include "sah_device.h"
#include "bvh4_device.h"
#include "bvh8_device.h"
#include "film_reduce.h"
#endif

using namespace miw;

static_assert(sizeof(BvhNode) == 64, "BvhNode must be one 64-byte line");
static_assert(sizeof(Tri) == 48, "Tri must be 48 bytes");
static_assert(sizeof(BsdfRec) == 128 && sizeof(mi_bsdf) == 128, "bsdf record layout");
static_assert(sizeof(TexRec) == sizeof(mi_texture), "texture record layout");

#define MIW_BLOCK 256
#ifndef MIW_POOL_NW
#define MIW_POOL_NW 12              /* wavefronts per workgroup of k_path_pooled (device/pooled_kernel.h): one workgroup per CU, three wavefronts per SIMD */
#endif
#define MIW_CNT_SHARDS 1024        /* power of two */
#define MIW_BRUTE_MAX_LEAF 2        /* triangles per leaf box of the resident plan's candidate filter */
#define MIW_BRUTE_MAX_TRIS 64       /* <= this many triangles: LDS brute-force sweep instead of the BVH */
#define MIW_PLACE_PIECES 4          /* placed pixel queues: 64-lane pieces per SIMD queue (= wavefronts per SIMD of the packet kernel) */

#include "device/trace.h"
#include "device/wavefront_kernels.h"
#include "device/resident_kernel.h"
#include "device/phased_kernel.h"
#if !defined(MIW_KERNELS_ONLY)
#if !MIW_SPECTRAL
#include "device/pooled_kernel.h"      /* (experimental, opt-in: the scalar_rgb library only) */
#endif
#include "device/stream_trace.h"
#include "device/film_kernels.h"
#endif
#include "device/eval_kernels.h"
#include "device/sample_kernel.h"
#include "device/class_instances.h"    /* a split build (-DMIW_SPLIT_CLASSES=1) compiles the MATS_NESTED and MATS_LIGHTS kernels in miwave_class.hip */
#if defined(MIW_AOV_UNIT) || !defined(MIW_KERNELS_ONLY)
#include "miw/aov.h"
#include "miw/film_gather_n.h"
#include "device/aov_launch.h"         /* the aov integrator's kernels (mi_render_aov): compiled in miwave_aov.hip (-DMIW_SPLIT_AOV=1), else here */
#if defined(MIW_AOV_UNIT) || !defined(MIW_SPLIT_AOV)
#include "device/aov_kernel.h"
#endif
#endif
#if defined(MIW_SENSOR_UNIT) || !defined(MIW_KERNELS_ONLY)
#include "miw/lens.h"
#include "miw/film_gather_n.h"
#include "device/sensor_launch.h"      /* the general sensor route's kernels (mi_render_sensor): compiled in miwave_sensor.hip (-DMIW_SPLIT_SENSOR=1), else here */
#if defined(MIW_SENSOR_UNIT) || !defined(MIW_SPLIT_SENSOR)
#include "device/sensor_kernel.h"
#endif
#endif
#if defined(MIW_VOLPATH_UNIT) || !defined(MIW_KERNELS_ONLY)
#include "miw/volpath.h"
#include "device/volpath_launch.h"     /* the volpath integrator's kernels (mi_sample, mi_render_sensor): compiled in miwave_volpath.hip (-DMIW_SPLIT_VOLPATH=1), else here */
#if defined(MIW_VOLPATH_UNIT) || !defined(MIW_SPLIT_VOLPATH)
#include "device/volpath_kernel.h"
#endif
#endif

#if !defined(MIW_KERNELS_ONLY)           /* (miwave_class.hip includes this file for the kernels above alone) */
__global__ void k_iota(uint32_t *out, uint32_t n) { const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = i; }

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------

template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0;
    hipError_t resize(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) (void) hipFree(p);
        p = nullptr; n = 0;
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **) &p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const std::vector<T> &v, hipStream_t s) {
        hipError_t e = resize(std::max<size_t>(v.size(), 1));
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
    void release() { if (p) (void) hipFree(p); p = nullptr; n = 0; }
};

// a DevBuf local to one call: freed on every return path (HIP_TRY returns early)
template <typename T> struct TmpBuf : DevBuf<T> { TmpBuf() = default; TmpBuf(const TmpBuf &) = delete; ~TmpBuf() { this->release(); } };

// ---- options --------------------------------------------------------------------------------
// Every switch of the library (A/B runs, tests, fallbacks). The ENVIRONMENT is read ONCE, by mi_create, into the context's own copy;
// after that the caller's environment does not matter to this context: a switch is changed with mi_set_option(ctx, name, value)
// (value NULL: back to unset). INTEGRATION.md section 5 lists them; mi_render_cfg::debug_* carry the ones a caller may want per render.
struct KnobInfo { const char *name, *what; };
static const KnobInfo g_knobs[] = {
    { "MIW_DEBUG", "1: diagnostics on stderr (LDS layout, builder statistics, phase statistics of -DMIW_PHASE_STATS builds)" },
    { "MIW_DEBUG_ALLOC", "1: mi_bvh_build times its uploads and allocations" },
    { "MIW_DEVICE_BUILDER", "mi_bvh_build quality 0: sah (default) | lbvh: which device builder runs" },
    { "MIW_SAH_HUGE", "0: the device SAH sweep bins every candidate in one workgroup (round 4's form)" },
    { "MIW_LBVH_LEAF", "radix tree: triangles per leaf" },
    { "MIW_MAX_LEAF", "host SAH builder: triangles per leaf" },
    { "MIW_NO_STACK", "1: no LDS-stack walk (stackless BVH2 walk, wavefront plan)" },
    { "MIW_BVH4", "0: no 4-wide tree (the phase machine steps through the BVH2)" },
    { "MIW_BVH4_FAN", "2 | 3 | 4: widest node the 4-wide collapse may build" },
    { "MIW_BVH4_HOST", "1: the 4-wide tree is collapsed on the host from the read-back BVH2" },
    { "MIW_BVH8", "0: mi_bvh_build skips the 8-wide tree / mi_render keeps the 4-wide walk" },
    { "MIW_STACK8_FULL", "1: the 8-wide walk keeps the 16-entry LDS column instead of one entry per tree level" },
    { "MIW_ENV_TOP", "0: the environment warp's top levels are not staged in LDS" },
    { "MIW_PHASED", "0: tree scenes take the lock-step kernel instead of the phase machine" },
    { "MIW_PHASED_WAVES", "3 | 4: wavefronts per SIMD the phase machine is launched for" },
    { "MIW_TRIO", "0: MATS_PLAIN kernels where the MATS_TRIO class would do" },
    { "MIW_SHADE_VOTE", "num:den of the phase machine's shade vote" },
    { "MIW_LOOP_EXIT", "node:triangle hand-over ratios of the phase machine's walk loops" },
    { "MIW_POOLED", "1: tree scenes take k_path_pooled (walk jobs pooled across the workgroup; experimental, slower: DESIGN.md)" },
    { "MIW_POOL_SHAPE", "12x1 | 8x2: wavefronts per workgroup x pixels per lane of k_path_pooled" },
    { "MIW_POOL_VOTE", "shade_min:walk_min:node_min:tri_min:claim_min of k_path_pooled" },
    { "MIW_TAIL_PRIO", "0: no least-progress-first wave priorities; 1: also in a packet kernel's launch of chunk jobs, which runs without them by default (and then keeps its lean kernel instead of the frame twin)" },
    { "MIW_WG_PER_CU", "workgroups per CU of the packet kernels' persistent grid" },
    { "MIW_PLACE", "0: shards of about one pixel per lane skip the measuring launch + placed queues" },
    { "MIW_JOB_CHUNK", "smallest chunk of a full frame's pixel jobs, in samples (a power of two; default 64, the phase machine 32): the pixels' sample streams are cut into halving chunks drawn chunk-major from one queue; 0: a job = all the samples of a pixel" },
    { "MIW_JOB_CHUNK_FORCE", "1: chunk jobs whatever the frame's size (tests of the hand-over between lanes)" },
    { "MIW_LEAN", "0: a packet scene without environment map and vertex normals, rendered without the moment integrator, keeps the full path kernel instead of its lean twin (kernel_pick.h: packet_features)" },
    { "MIW_FRAME_TWIN", "0: a full frame of chunk jobs keeps the lean twin of its packet path kernel instead of the frame twin, which has the facts of such a launch compiled in (kernel_pick.h: frame_twin)" },
    { "MIW_JOB_POOL", "chunk-job ids a wavefront of a frame twin draws from the queue at a time, their state words read into its LDS block with the draw (a power of two from 2 to 32; default 32); 0: every job drawn on its own (resident_kernel.h: QueueWork::refill)" },
    { "MIW_PACKET_SHARD4", "0: a plain-diffuse packet job of at most four wavefronts of pixels per SIMD keeps the five-wavefront (96-register) kernel" },
    { "MIW_PLACE_MEASURE", "divisor: the measuring launch runs spp / divisor samples" },
    { "MIW_PLACE_SPREAD", "0 | 1: placed pieces = consecutive sorted lanes | one lane of every cost stratum" },
    { "MIW_STREAM", "0: plan 1 walks with one kernel per list slice instead of the persistent stream kernel" },
    { "MIW_FILM_LEGACY", "1: the 24-byte position log + k_film_blocks for every filter" },
    { "MIW_FILM_LANES", "0 | 1 | 2: k_film_lanes off / over the tile-interleaved log / over [lane][sample]" },
    { "MIW_FILM_CHAINS", "0: the replay over the tile-interleaved log runs k_film_lanes (a wavefront per block position) instead of k_film_chains (a wavefront per chain of positions of equal weight)" },
    { "MIW_FILM_CHAINS_U", "4 | 8: records in flight per lane of k_film_chains: 8 (the default) compiled for two wavefronts per SIMD, 4 for three" },
    { "MIW_FILM_QUADS", "0 | 24 | 28 | 42 | 44: k_film_quads group shape (0: off)" },
    { "MIW_FILM_COLUMNS", "0 | 42 | 44 | 82: k_film_columns group shape" },
    { "MIW_FILM_GROUP", "2 | 3 | 4: k_film_groups group shape" },
    { "MIW_FL_NT", "0: k_film_lanes reads the log with plain instead of streaming loads" },
    { "MIW_FILM_OVERLAP", "1: part of the film replay of a full Cornell-class frame is queued on three more streams beside the path kernel, sets of 64-tile groups each behind the flags their last pixels raise (default 0: measured +0 - 1 %); 2: without the waits (timing probe: the film is the previous frame's)" },
    { "MIW_FILM_OVERLAP_SET", "groups of 64 tiles per launch of that replay (default 4)" },
    { "MIW_FILM_OVERLAP_ROOM", "workgroups the path kernel's grid is short of filling the device while the replay runs beside it (default 32: one per CU on 32 CUs)" },
    { "MIW_FILM_OVERLAP_LEAN", "0: the launches of that replay are the 168-register kernel (default 1: the 128-register form)" },
    { "MIW_FILM_OVERLAP_BESIDE", "groups of 64 tiles replayed beside the path kernel; the rest in one launch after it (default: three quarters)" },
    { "MIW_FILM_OVERLAP_PRIO", "s_setprio of the replay wavefronts that run beside the path kernel, 0 .. 3 (default 0)" },
    { "MIW_FQ_U", "2 | 4 | 8: records per trip of k_film_quads" },
    { "MIW_RCCL", "0: mi_film_reduce never uses RCCL (device add)" },
    { "MIW_RCCL_FORCE", "1: mi_film_reduce takes the RCCL branch for one context too (tests)" }
};
struct Options {
    std::map<std::string, std::string> v;
    void from_env() { for (const KnobInfo &k : g_knobs) if (const char *e = getenv(k.name)) v[k.name] = e; }
    static bool known(const char *name) { for (const KnobInfo &k : g_knobs) if (!strcmp(k.name, name)) return true; return false; }
    const char *get(const char *name) const { auto it = v.find(name); return it == v.end() ? nullptr : it->second.c_str(); }
    // a switch is off / on when it is SET and atoi of its value is 0 / not 0 (a value that is no number counts as 0); unset is neither: the default holds
    bool off(const char *name) const { const char *e = get(name); return e && atoi(e) == 0; }
    bool on(const char *name) const { const char *e = get(name); return e && atoi(e) != 0; }
    int num(const char *name, int unset) const { const char *e = get(name); return e ? atoi(e) : unset; }
};

struct mi_ctx {
    int device = 0;
    Options opt;
    hipStream_t stream = nullptr;
    std::string error;
    std::atomic<int> cancel{0};

    // host copy of the scene (input order)
    std::vector<Tri> tris_in;
    std::vector<float> tri_vn_in;       // 9 per tri or empty
    std::vector<float> tri_uv_in;       // 6 per face (texture coordinates, texture_build.h) or empty
    std::vector<ShapeRec> shapes;
    std::vector<AnalyticRec> rects;                 // analytic rectangles
    std::vector<BsdfRec> bsdfs; bool diffuse_only = false;   // every record one-sided smooth diffuse
    bool trio = false;                                       // every record diffuse / dielectric / roughconductor: MATS_TRIO kernels
    bool nested = false;                                     // a mask / blendbsdf / null / thindielectric record: MATS_NESTED kernels (textured is set too)
    bool textured = false;                                   // texture coordinates, bitmaps or an "extended" plugin: MATS_ALL kernels
    std::vector<float> bsdf_tables; DevBuf<float> d_bsdf_tables;
    std::vector<EmitterRec> emitters;
    std::vector<LightRec> lights; DevBuf<LightRec> d_lights; int32_t constant_light = -1;   // point / spot / directional / constant emitters (miw/light.h); index of the constant one
    bool lights_on = false;                                  // the emitter table holds a light: MATS_LIGHTS kernels (nested and textured are set too)
    std::vector<float> emit_tri, emit_vnorm, emit_pmf, emit_cdf;
    bool have_scene = false, have_bvh = false;

    // device scene
    DevBuf<BvhNode> d_nodes; DevBuf<Tri> d_tris; DevBuf<float> d_tri_vn, d_tri_uv, d_bitmap_data; DevBuf<BitmapRec> d_bitmaps; uint32_t bitmap_count = 0;
    DevBuf<ShapeRec> d_shapes; DevBuf<BsdfRec> d_bsdfs; DevBuf<EmitterRec> d_emitters; DevBuf<AnalyticRec> d_rects;
    DevBuf<float> d_emit_tri, d_emit_vnorm, d_emit_pmf, d_emit_cdf;
    DevBuf<LeafBox> d_leaf_boxes; DevBuf<TriBounds> d_tri_bounds; DevBuf<Bvh4Node> d_nodes4; uint32_t nodes4_count = 0, nodes4_stack = 0;
    DevBuf<Bvh8Node> d_nodes8; DevBuf<Tri> d_tris8; DevBuf<float> d_tri_vn8; uint32_t nodes8_count = 0, nodes8_depth = 0;   // the 8-wide tree (miw/bvh8.h) and the triangles / vertex normals in its order
    DevBuf<float> d_env_data, d_env_levels; DevBuf<EnvmapRec> d_env; EnvmapRec env_host{}; size_t env_levels_total = 0;   // (host copy of the record: level offsets for the LDS staging)
    bool have_env = false;
    bool shape_normals = false, emitter_normals = false;     // a shape / an area emitter's mesh has vertex normals; with have_env, the facts kernel_pick.h's packet_features reads
    SceneView view{};
    TraceLds lds_cfg{}; size_t lds_bytes = 0;

    // render state
    DevBuf<F4> q_tp, q_res, q_ray_o, q_ray_d, q_hit, q_sh_d, q_sh_c;
    DevBuf<U4> q_st; DevBuf<F2> q_pos; DevBuf<uint32_t> q_pixel, q_sh_vis;
    DevBuf<double> d_accum; DevBuf<unsigned char> d_out;
    DevBuf<F2> q_log_pos; DevBuf<F4> q_log_val;         // 24-byte sample log (filters without phase classes)
    DevBuf<U4> q_log_rec;                               // 16-byte sample log (miw/film.h: phase classes)
    FilmClasses classes; FilmRec classes_of{}; bool classes_valid = false;   // the class tables of the last filter rendered with (ok or refused), and that filter
    DevBuf<float> d_fc_thr, d_fc_w;
    DevBuf<uint32_t> d_next_pixel; int cu_count = 256;
    DevBuf<uint32_t> d_lane_cost, d_cost_sorted, d_lane_iota, d_lane_sorted, d_piece_list, d_simd_ids;   // placed pixel queues of small shards (resident_kernel.h: QueueWork)
    DevBuf<unsigned char> d_place_tmp;
    DevBuf<uint32_t> d_lists, d_list_counts;    // wavefront plan: 2 parities x WL_LISTS lists / counters
    DevBuf<uint32_t> d_block_ids, d_tile_list; DevBuf<int32_t> d_block_tile; DevBuf<float> d_tiles;
    DevBuf<Counters> d_cnt;
    Counters *h_cnt = nullptr;          // pinned
    std::vector<uint32_t> h_piece_list, h_simd_ids;   // the placed launch's dealing (host side): uploaded without waiting, so they live here
    // film replay beside the render (round 6): a second stream, fork / join events, per group of 64 tiles the pixels done / expected (device) and
    // the flag its last pixel raises (host-coherent: what hipStreamWaitValue32 polls)
    hipStream_t stream2[3] = { nullptr, nullptr, nullptr }; hipEvent_t ev_fork = nullptr, ev_join[3] = { nullptr, nullptr, nullptr };   // (kernels of ONE stream run one after the other: three replay streams)
    DevBuf<uint32_t> d_group_done, d_group_expected; uint32_t *h_group_flag = nullptr; uint32_t group_flag_cap = 0;
    std::vector<uint32_t> h_group_expected; std::vector<int32_t> h_block_tile;
    // the chain table of k_film_chains (csrc/film_chains.h) and what it was built from: rebuilt and uploaded when one of them changes
    DevBuf<uint32_t> d_film_chains; std::vector<uint32_t> h_film_chains; uint32_t film_chains_n = 0; int64_t film_chains_key = -1;
    int overlap_state = -1;             // -1: not tried; 0: the runtime refused (hipStreamWaitValue32 / the allocations); 1: available
    bool replay_enqueued = false;       // this frame's k_film_lanes launches already sit in the replay streams (assemble_film only joins)
    uint32_t replay_launches = 0;

    DevBuf<unsigned char> d_sample_stage; DevBuf<uint32_t> d_next_ray;   // mi_sample: the staged chunk of a host-pointer call, the ray queue's counter
    // participating media (MI_INTEGRATOR_VOLPATH; miw/medium.h): the records, per shape its interior / exterior reference, the medium rays start in
    std::vector<MediumRec> media; std::vector<uint32_t> shape_media; uint32_t start_medium = 0;
    DevBuf<MediumRec> d_media; DevBuf<uint32_t> d_shape_media, d_volpath_capped; uint64_t volpath_capped = 0;   // (the last call's count: mi_volpath_capped)

    std::vector<hipEvent_t> ev_pool;
    mi_counters counters{};
};

static mi_status fail(mi_ctx *c, mi_status code, const char *fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->error = buf;
    return code;
}
#define HIP_TRY(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail(c, MI_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define MI_TRY(expr) do { const mi_status st_ = (expr); if (st_ != MI_OK) return st_; } while (0)   /* a phase that failed has said why (fail) */

static thread_local std::string g_global_error;

extern "C" {

int32_t mi_spectrum_channels(void) { return MIW_SPEC_N; }

mi_status mi_device_count(int32_t *count) {
    if (!count) return MI_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; g_global_error = hipGetErrorString(e); return MI_ERR_DEVICE; }
    *count = n;
    return MI_OK;
}

mi_status mi_create(int32_t device, mi_ctx **out) {
    if (!out) return MI_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_global_error = "no HIP device visible"; return MI_ERR_DEVICE; }
    if (device < 0 || device >= n) { g_global_error = "device index out of range"; return MI_ERR_INVALID; }
    if (hipSetDevice(device) != hipSuccess) { g_global_error = "hipSetDevice failed"; return MI_ERR_DEVICE; }
    mi_ctx *c = new mi_ctx();
    c->device = device;
    c->opt.from_env();                                           // the only place the library reads the environment
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->cu_count = prop.multiProcessorCount; }
    if (hipHostMalloc((void **) &c->h_cnt, sizeof(Counters) * MIW_CNT_SHARDS) != hipSuccess) { delete c; g_global_error = "hipHostMalloc failed"; return MI_ERR_DEVICE; }
    *out = c;
    g_live_contexts.fetch_add(1);
    return MI_OK;
}

void mi_destroy(mi_ctx *c) {
    if (!c) return;
    (void) hipSetDevice(c->device);
    (void) hipDeviceSynchronize();
    c->d_nodes.release(); c->d_tris.release(); c->d_tri_vn.release(); c->d_tri_uv.release(); c->d_bitmap_data.release(); c->d_bitmaps.release(); c->d_bsdf_tables.release(); c->d_shapes.release(); c->d_rects.release(); c->d_bsdfs.release();
    c->d_media.release(); c->d_shape_media.release(); c->d_volpath_capped.release();
    c->d_emitters.release(); c->d_lights.release(); c->d_leaf_boxes.release(); c->d_tri_bounds.release(); c->d_nodes4.release(); c->d_nodes8.release(); c->d_tris8.release(); c->d_tri_vn8.release(); c->d_env_data.release(); c->d_env_levels.release(); c->d_env.release(); c->d_emit_tri.release(); c->d_emit_vnorm.release(); c->d_emit_pmf.release(); c->d_emit_cdf.release();
    c->q_tp.release(); c->q_res.release(); c->q_ray_o.release(); c->q_ray_d.release(); c->q_hit.release();
    c->q_sh_d.release(); c->q_sh_c.release(); c->q_st.release(); c->q_pos.release(); c->q_pixel.release(); c->q_sh_vis.release();
    c->d_accum.release(); c->d_out.release(); c->d_next_pixel.release(); c->d_lane_cost.release(); c->d_cost_sorted.release(); c->d_lane_iota.release(); c->d_lane_sorted.release(); c->d_place_tmp.release(); c->d_piece_list.release(); c->d_simd_ids.release(); c->d_lists.release(); c->d_list_counts.release(); c->d_block_ids.release(); c->d_tile_list.release(); c->d_cnt.release();
    c->q_log_pos.release(); c->q_log_val.release(); c->q_log_rec.release(); c->d_fc_thr.release(); c->d_fc_w.release(); c->d_block_tile.release(); c->d_tiles.release(); c->d_film_chains.release();
    for (hipEvent_t e : c->ev_pool) (void) hipEventDestroy(e);
    c->d_group_done.release(); c->d_group_expected.release(); c->d_sample_stage.release(); c->d_next_ray.release();
    if (c->h_group_flag) (void) hipHostFree(c->h_group_flag);
    if (c->ev_fork) (void) hipEventDestroy(c->ev_fork);
    for (int i = 0; i < 3; ++i) { if (c->ev_join[i]) (void) hipEventDestroy(c->ev_join[i]); if (c->stream2[i]) (void) hipStreamDestroy(c->stream2[i]); }
    if (c->h_cnt) (void) hipHostFree(c->h_cnt);
    delete c;
    if (g_live_contexts.fetch_sub(1) == 1) rccl_release_comms();
}

mi_status mi_set_stream(mi_ctx *c, void *s) { if (!c) return MI_ERR_INVALID; c->stream = (hipStream_t) s; return MI_OK; }

const char *mi_last_error(mi_ctx *c) { return c ? c->error.c_str() : g_global_error.c_str(); }

mi_status mi_set_option(mi_ctx *c, const char *name, const char *value) {
    if (!c || !name) return MI_ERR_INVALID;
    if (!Options::known(name)) return fail(c, MI_ERR_INVALID, "mi_set_option: unknown option %s", name);
    if (value) c->opt.v[name] = value; else c->opt.v.erase(name);
    return MI_OK;
}
const char *mi_get_option(mi_ctx *c, const char *name) { return c && name ? c->opt.get(name) : nullptr; }
int32_t mi_option_count(void) { return (int32_t) (sizeof(g_knobs) / sizeof(g_knobs[0])); }
const char *mi_option_name(int32_t i) { return i >= 0 && i < mi_option_count() ? g_knobs[i].name : nullptr; }
const char *mi_option_help(int32_t i) { return i >= 0 && i < mi_option_count() ? g_knobs[i].what : nullptr; }

mi_status mi_cancel(mi_ctx *c) { if (!c) return MI_ERR_INVALID; c->cancel.store(1); return MI_OK; }

mi_status mi_volpath_capped(mi_ctx *c, uint64_t *out) {
    if (!c || !out) return MI_ERR_INVALID;
    *out = c->volpath_capped;
    return MI_OK;
}

mi_status mi_get_counters(mi_ctx *c, mi_counters *out) {
    if (!c || !out) return MI_ERR_INVALID;
    *out = c->counters;
    return MI_OK;
}

// ---- N-GPU frames inside one process: device films and their reduce (film_reduce.h) ------------------------------
mi_status mi_film_alloc(mi_ctx *c, uint64_t count, void **film) {
    if (!c || !film) return MI_ERR_INVALID;
    *film = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    float *p = nullptr;
    HIP_TRY(c, hipMalloc((void **) &p, std::max<uint64_t>(count, 1) * sizeof(float)));
    hipError_t e = hipMemsetAsync(p, 0, count * sizeof(float), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void) hipFree(p); return fail(c, MI_ERR_DEVICE, "mi_film_alloc: %s", hipGetErrorString(e)); }
    *film = p;
    return MI_OK;
}
void mi_film_free(mi_ctx *c, void *film) {
    if (!c || !film) return;
    (void) hipSetDevice(c->device);
    (void) hipFree(film);
}
mi_status mi_film_download(mi_ctx *c, const void *film, float *host, uint64_t count) {
    if (!c || !film || !host) return MI_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host, film, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}
mi_status mi_film_reduce(mi_ctx *const *ctxs, void *const *films, int32_t n, uint64_t count, int32_t root, int32_t *how) {
    if (how) *how = MI_REDUCE_NONE;
    if (!ctxs || !films || n < 1 || root < 0 || root >= n) return MI_ERR_INVALID;
    for (int32_t i = 0; i < n; ++i) if (!ctxs[i] || !films[i]) return MI_ERR_INVALID;
    mi_ctx *r = ctxs[root];
    // everything the contexts still have in flight on their streams lands first
    for (int32_t i = 0; i < n; ++i) { HIP_TRY(r, hipSetDevice(ctxs[i]->device)); HIP_TRY(r, hipStreamSynchronize(ctxs[i]->stream)); }
    // (one context: nothing to add — unless MIW_RCCL_FORCE=1 asks for the RCCL branch anyway: a communicator of one rank, an in-place
    // reduce that leaves the film as it is. That is how the branch — dlopen, ncclCommInitAll, the grouped ncclReduce, the stream
    // waits — runs on a one-GPU box: tests/test_multi_gpu.py)
    const bool force_rccl = r->opt.on("MIW_RCCL_FORCE");
    if (count == 0 || (n == 1 && !force_rccl)) return MI_OK;
    std::vector<int> devs(n);
    bool distinct = true;
    for (int32_t i = 0; i < n; ++i) { devs[i] = ctxs[i]->device; for (int32_t j = 0; j < i; ++j) distinct = distinct && devs[j] != devs[i]; }
    if (distinct) {
        std::lock_guard<std::mutex> lock(g_rccl_mutex);
        if (g_rccl.load(!r->opt.off("MIW_RCCL"))) {
            auto it = g_rccl_comms.find(devs);
            if (it == g_rccl_comms.end()) {
                std::vector<ncclComm_t> comms(n);
                const ncclResult_t rc = g_rccl.CommInitAll(comms.data(), n, devs.data());
                if (rc != ncclSuccess) return fail(r, MI_ERR_DEVICE, "mi_film_reduce: ncclCommInitAll: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
                it = g_rccl_comms.emplace(devs, comms).first;
            }
            // (no return between GroupStart and GroupEnd: a failure is remembered, the group is always closed, then reported — ADVICE r05)
            ncclResult_t rc = g_rccl.GroupStart();
            hipError_t he = hipSuccess;
            for (int32_t i = 0; i < n && rc == ncclSuccess && he == hipSuccess; ++i) {
                he = hipSetDevice(devs[i]);
                if (he == hipSuccess) rc = g_rccl.Reduce(films[i], films[i], (size_t) count, ncclFloat, ncclSum, root, it->second[i], ctxs[i]->stream);
            }
            const ncclResult_t re = g_rccl.GroupEnd();
            if (rc == ncclSuccess) rc = re;
            if (he != hipSuccess) return fail(r, MI_ERR_DEVICE, "mi_film_reduce: hipSetDevice: %s", hipGetErrorString(he));
            if (rc != ncclSuccess) return fail(r, MI_ERR_DEVICE, "mi_film_reduce: ncclReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
            for (int32_t i = 0; i < n; ++i) { HIP_TRY(r, hipSetDevice(devs[i])); HIP_TRY(r, hipStreamSynchronize(ctxs[i]->stream)); }
            HIP_TRY(r, hipSetDevice(r->device));
            if (how) *how = MI_REDUCE_RCCL;
            return MI_OK;
        }
    }
    if (n == 1) return MI_OK;                                   // (MIW_RCCL_FORCE without RCCL)
    // rank-ordered device add onto the root's film (contexts sharing a device, or no RCCL)
    HIP_TRY(r, hipSetDevice(r->device));
    TmpBuf<float> stage;
    const dim3 blk(256), grd((unsigned) ((count + 255) / 256));
    for (int32_t i = 0; i < n; ++i) {
        if (i == root) continue;
        const float *src = (const float *) films[i];
        if (ctxs[i]->device != r->device) {
            HIP_TRY(r, stage.resize(count));
            HIP_TRY(r, hipMemcpyPeerAsync(stage.p, r->device, films[i], ctxs[i]->device, count * sizeof(float), r->stream));
            src = stage.p;
        }
        hipLaunchKernelGGL(k_film_add, grd, blk, 0, r->stream, (float *) films[root], src, count);
    }
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (how) *how = MI_REDUCE_DEVICE_ADD;
    return MI_OK;
}

// ---- scene upload ---------------------------------------------------------------------
mi_status mi_scene_upload(mi_ctx *c, const mi_scene_desc *s) {
    if (!c || !s) return MI_ERR_INVALID;
    c->have_scene = c->have_bvh = false;
    if (s->face_count && (!s->vertex_positions || !s->faces)) return fail(c, MI_ERR_INVALID, "scene: null geometry pointers");
    if (!s->shapes || s->shape_count == 0) return fail(c, MI_ERR_INVALID, "scene: no shapes");
    if (!s->bsdfs || s->bsdf_count == 0) return fail(c, MI_ERR_INVALID, "scene: no bsdfs");
    if (s->face_count >= (1u << 27) - 16u) return fail(c, MI_ERR_INVALID, "scene: too many faces");   // leaf codes (first << 4 | count - 1) must stay clear of MIW_BVH4_ABSENT / MIW_WALK_DONE

    // participating media (read by MI_INTEGRATOR_VOLPATH alone): HomogeneousMedium records, references = index + 1, 0 = none
    if (s->media_count && !s->media) return fail(c, MI_ERR_INVALID, "scene: media_count without media");
    if (s->start_medium > s->media_count) return fail(c, MI_ERR_INVALID, "scene: start_medium %u out of range (%u media; a reference is index + 1)", s->start_medium, s->media_count);
    for (uint32_t k = 0; k < s->media_count; ++k) {
        const mi_medium &m = s->media[k];
        for (int a = 0; a < 3; ++a) {
            if (!(std::isfinite(m.sigma_t[a]) && m.sigma_t[a] > 0.f)) return fail(c, MI_ERR_INVALID, "medium %u: sigma_t[%d] = %g must be finite and > 0", k, a, (double) m.sigma_t[a]);
            if (!(m.albedo[a] >= 0.f && m.albedo[a] <= 1.f)) return fail(c, MI_ERR_INVALID, "medium %u: albedo[%d] = %g must lie in [0, 1]", k, a, (double) m.albedo[a]);
        }
        if (m.phase != MI_PHASE_ISOTROPIC && m.phase != MI_PHASE_HG) return fail(c, MI_ERR_INVALID, "medium %u: unknown phase function %u", k, m.phase);
        if (m.phase == MI_PHASE_HG && !(m.g > -1.f && m.g < 1.f)) return fail(c, MI_ERR_INVALID, "medium %u: The asymmetry parameter must lie in the interval (-1, 1)! (g = %g)", k, (double) m.g);
    }
    if (s->shape_media)
        for (uint32_t i = 0; i < 2u * s->shape_count; ++i)
            if (s->shape_media[i] > s->media_count)
                return fail(c, MI_ERR_INVALID, "shape %u: %s medium %u out of range (%u media; a reference is index + 1)", i / 2u, (i & 1u) ? "exterior" : "interior", s->shape_media[i], s->media_count);
#if MIW_SPECTRAL
    if (s->media_count) return fail(c, MI_ERR_INVALID, "scene: media are served by the scalar_rgb library");
#endif
    c->media.clear(); c->shape_media.clear(); c->start_medium = s->start_medium;
    for (uint32_t k = 0; k < s->media_count; ++k) {
        const mi_medium &m = s->media[k];
        MediumRec r; memset(&r, 0, sizeof r);
        for (int a = 0; a < 3; ++a) { r.sigma_t[a] = m.sigma_t[a]; r.albedo[a] = m.albedo[a]; }
        r.has_spectral_extinction = m.has_spectral_extinction ? 1u : 0u; r.sample_emitters = m.sample_emitters ? 1u : 0u;
        r.phase = m.phase; r.g = m.g;
        c->media.push_back(r);
    }
    if (s->shape_media) c->shape_media.assign(s->shape_media, s->shape_media + 2u * (size_t) s->shape_count);

    // Scene::m_emitters order: the environment map and the lights sit at their emitter_index, the area emitters fill the other slots in order
    if (s->light_count && !s->lights) return fail(c, MI_ERR_INVALID, "scene: light_count without lights");
    const uint32_t emitter_total = s->emitter_count + (s->envmap ? 1u : 0u) + s->light_count;
    std::vector<int32_t> slot_light(emitter_total, -1);        // slot -> light record, -2: the environment map, -1: an area emitter
    std::vector<int32_t> area_slot(s->emitter_count, -1);
    if (s->envmap && s->envmap->emitter_index >= emitter_total) return fail(c, MI_ERR_INVALID, "envmap: emitter_index out of range");
    if (s->light_count) {
        if (s->envmap) slot_light[s->envmap->emitter_index] = -2;
        int32_t constant = -1;
        for (uint32_t k = 0; k < s->light_count; ++k) {
            const mi_light &l = s->lights[k];
            if (l.type > MI_LIGHT_CONSTANT) return fail(c, MI_ERR_INVALID, "light %u: unknown type %u", k, l.type);
            if (l.emitter_index >= emitter_total) return fail(c, MI_ERR_INVALID, "light %u: emitter_index %u leaves a gap in the emitter list (%u emitters)", k, l.emitter_index, emitter_total);
            if (slot_light[l.emitter_index] != -1) return fail(c, MI_ERR_INVALID, "light %u: emitter_index %u collides with %s", k, l.emitter_index, slot_light[l.emitter_index] == -2 ? "the envmap" : "another light");
            slot_light[l.emitter_index] = (int32_t) k;
            if (l.type == MI_LIGHT_CONSTANT) {
                if (s->envmap) return fail(c, MI_ERR_INVALID, "light %u: a constant emitter together with an envmap (one environment emitter per scene)", k);
                if (constant >= 0) return fail(c, MI_ERR_INVALID, "light %u: a second constant emitter (light %d is one; one environment emitter per scene)", k, constant);
                constant = (int32_t) k;
            }
            if (l.type == MI_LIGHT_SPOT && l.value_tex.type == MI_TEX_BITMAP) return fail(c, MI_ERR_INVALID, "light %u: a spot emitter with a texture child is not supported", k);
            if (l.type == MI_LIGHT_SPOT && !(l.cutoff_angle >= l.beam_width)) return fail(c, MI_ERR_INVALID, "light %u: spot: cutoff_angle must not be below beam_width", k);
            if (l.type == MI_LIGHT_DIRECTIONAL) {
                const float n2 = l.direction[0] * l.direction[0] + l.direction[1] * l.direction[1] + l.direction[2] * l.direction[2];
                if (!(std::fabs(n2 - 1.f) <= 1e-4f)) return fail(c, MI_ERR_INVALID, "light %u: directional: direction is not of unit length", k);
            }
            if ((l.type == MI_LIGHT_DIRECTIONAL || l.type == MI_LIGHT_CONSTANT) && !(l.bsphere_radius >= 0.f && isfinite_(l.bsphere_radius)))
                return fail(c, MI_ERR_INVALID, "light %u: bsphere_radius must be finite and not negative", k);
#if MIW_SPECTRAL
            if (l.value_tex.type != MI_TEX_D65 && l.value_tex.type != MI_TEX_SRGB_D65 && l.value_tex.type != MI_TEX_UNIFORM)
                return fail(c, MI_ERR_INVALID, "light %u: the scalar_spectral library needs a spectral value record", k);
#endif
        }
        uint32_t slot = 0;
        for (uint32_t i = 0; i < s->emitter_count; ++i) { while (slot_light[slot] != -1) ++slot; area_slot[i] = (int32_t) slot++; }
    }

    c->tris_in.assign(s->face_count, Tri{});
    std::vector<uint32_t> face_shape(s->face_count, 0xffffffffu);
    bool any_normals = false;
    c->shapes.resize(s->shape_count);
    for (uint32_t i = 0; i < s->shape_count; ++i) {
        const mi_shape &sh = s->shapes[i];
        if (sh.bsdf >= s->bsdf_count) return fail(c, MI_ERR_INVALID, "shape %u: bsdf index out of range", i);
        if (sh.emitter >= (int32_t) s->emitter_count) return fail(c, MI_ERR_INVALID, "shape %u: emitter index out of range", i);
        if ((uint64_t) sh.first_face + sh.face_count > s->face_count) return fail(c, MI_ERR_INVALID, "shape %u: face range out of bounds", i);
        if ((sh.flags & MI_SHAPE_HAS_NORMALS) && !s->vertex_normals) return fail(c, MI_ERR_INVALID, "shape %u: HAS_NORMALS without vertex_normals", i);
        for (uint32_t f = sh.first_face; f < sh.first_face + sh.face_count; ++f) {
            if (face_shape[f] != 0xffffffffu) return fail(c, MI_ERR_INVALID, "face %u belongs to two shapes", f);
            face_shape[f] = i;
        }
        // emitter ids index the combined list: the environment map sits at envmap->emitter_index
        int32_t emitter_id = sh.emitter;
        if (emitter_id >= 0 && s->light_count) emitter_id = area_slot[emitter_id];
        else if (emitter_id >= 0 && s->envmap && (uint32_t) emitter_id >= s->envmap->emitter_index) emitter_id += 1;
        ShapeRec r; r.bsdf = sh.bsdf; r.emitter = emitter_id; r.flags = sh.flags & (MI_SHAPE_HAS_NORMALS | MI_SHAPE_HAS_TEXCOORDS); r.pad = 0;
        if (sh.flags & (MI_SHAPE_RECTANGLE | MI_SHAPE_SPHERE)) {
            if (sh.face_count != 1) return fail(c, MI_ERR_INVALID, "shape %u: an analytic shape is one primitive (face_count == 1)", i);
            if (sh.flags & (MI_SHAPE_HAS_NORMALS | MI_SHAPE_HAS_TEXCOORDS)) return fail(c, MI_ERR_INVALID, "shape %u: an analytic shape has no vertex normals / texture coordinates", i);
            if ((sh.flags & MI_SHAPE_RECTANGLE) && (sh.flags & MI_SHAPE_SPHERE)) return fail(c, MI_ERR_INVALID, "shape %u: rectangle and sphere", i);
        }
        c->shapes[i] = r;
        any_normals = any_normals || (r.flags & 1u);
    }
    // analytic rectangles: record + two bounding triangles (the second one appended behind the faces)
    c->rects.clear();
    if (s->rectangle_count && !s->rectangles) return fail(c, MI_ERR_INVALID, "scene: rectangle_count without rectangles");
    std::vector<int32_t> shape_rect(s->shape_count, -1);
    for (uint32_t k = 0; k < s->rectangle_count; ++k) {
        const mi_rectangle &q = s->rectangles[k];
        if (q.shape >= s->shape_count || !(s->shapes[q.shape].flags & MI_SHAPE_RECTANGLE) || shape_rect[q.shape] >= 0)
            return fail(c, MI_ERR_INVALID, "rectangle %u: shape %u is not a (single) MI_SHAPE_RECTANGLE shape", k, q.shape);
        shape_rect[q.shape] = (int32_t) k;
        c->rects.push_back(rect_record(q.to_world, q.to_object, q.shape, s->shapes[q.shape].first_face));
        if (!(c->rects.back().inv_area > 0.f) || !isfinite_(c->rects.back().inv_area))
            return fail(c, MI_ERR_INVALID, "rectangle %u: degenerate to_world", k);
    }
    if (s->sphere_count && !s->spheres) return fail(c, MI_ERR_INVALID, "scene: sphere_count without spheres");
    for (uint32_t k = 0; k < s->sphere_count; ++k) {          // spheres follow the rectangles in the analytic table
        const mi_sphere &q = s->spheres[k];
        if (q.shape >= s->shape_count || !(s->shapes[q.shape].flags & MI_SHAPE_SPHERE) || shape_rect[q.shape] >= 0)
            return fail(c, MI_ERR_INVALID, "sphere %u: shape %u is not a (single) MI_SHAPE_SPHERE shape", k, q.shape);
        if (!(q.radius > 0.f) || !isfinite_(q.radius)) return fail(c, MI_ERR_INVALID, "sphere %u: radius must be positive", k);
        shape_rect[q.shape] = (int32_t) c->rects.size();
        c->rects.push_back(sphere_record(q.center, q.radius, q.flip_normals != 0, q.to_world, q.to_object, q.shape, s->shapes[q.shape].first_face));
    }
    for (uint32_t i = 0; i < s->shape_count; ++i)
        if ((s->shapes[i].flags & (MI_SHAPE_RECTANGLE | MI_SHAPE_SPHERE)) && shape_rect[i] < 0)
            return fail(c, MI_ERR_INVALID, "shape %u: no mi_rectangle record", i);
    if (!build_face_texcoords(s, c->tri_uv_in)) return fail(c, MI_ERR_INVALID, "scene: MI_SHAPE_HAS_TEXCOORDS without vertex_texcoords (or a vertex index out of range)");
    c->tris_in.resize((size_t) s->face_count + c->rects.size());
    c->tri_vn_in.clear();
    if (any_normals) c->tri_vn_in.assign(c->tris_in.size() * 9, 0.f);
    for (uint32_t f = 0; f < s->face_count; ++f) {
        if (face_shape[f] == 0xffffffffu) return fail(c, MI_ERR_INVALID, "face %u belongs to no shape", f);
        Tri &t = c->tris_in[f];
        if (shape_rect[face_shape[f]] >= 0) {                  // the rectangle's primitive slot: its two bounding triangles
            Tri two[2];
            analytic_bounding_tris(c->rects[shape_rect[face_shape[f]]], (uint32_t) shape_rect[face_shape[f]], two);
            t = two[0]; c->tris_in[(size_t) s->face_count + shape_rect[face_shape[f]]] = two[1];
            continue;
        }
        for (int k = 0; k < 3; ++k) {
            uint32_t vi = s->faces[3 * f + k];
            if (vi >= s->vertex_count) return fail(c, MI_ERR_INVALID, "face %u: vertex index out of range", f);
            float *dst = k == 0 ? t.p0 : (k == 1 ? t.p1 : t.p2);
            memcpy(dst, s->vertex_positions + 3 * (size_t) vi, 12);
            if (any_normals && (c->shapes[face_shape[f]].flags & 1u))
                memcpy(&c->tri_vn_in[(size_t) f * 9 + 3 * k], s->vertex_normals + 3 * (size_t) vi, 12);
        }
        t.shape = face_shape[f]; t.prim = f; t.pad = 0;
    }
    c->bsdfs.resize(s->bsdf_count);
    for (uint32_t i = 0; i < s->bsdf_count; ++i) {
        const mi_bsdf &b = s->bsdfs[i];
        BsdfRec r; int slot = 0;
        if (s->bsdf_table_floats && !s->bsdf_tables) return fail(c, MI_ERR_INVALID, "scene: bsdf_table_floats without bsdf_tables");
        if (const char *why = bsdf_record_from_abi(b, s->bitmap_count, s->bsdf_table_floats, r, &slot))
            return slot < 0 ? fail(c, MI_ERR_INVALID, "bsdf %u: %s", i, why) : fail(c, MI_ERR_INVALID, "bsdf %u: texture %d: %s", i, slot, why);
        if (!(b.flags & MI_BSDF_FLAG_TWOSIDED) && b.type != BSDF_TYPE_MASK && b.type != BSDF_TYPE_BLEND) r.back = 0;
        c->bsdfs[i] = r;
    }
    for (uint32_t i = 0; i < s->bsdf_count; ++i)               // twosided.cpp:62-92 and the chain rule of the wrappers
        if (const char *why = bsdf_chain_check(c->bsdfs, i, s->bitmaps)) return fail(c, MI_ERR_INVALID, "bsdf %u: %s", i, why);
    c->diffuse_only = true;
    for (const BsdfRec &r : c->bsdfs) if (r.type != BSDF_TYPE_DIFFUSE || (r.flags & BSDF_REC_TWOSIDED)) c->diffuse_only = false;
    if (!c->tri_uv_in.empty()) c->diffuse_only = false;          // texture coordinates steer the shading frame (mesh.cpp:492-511)
    for (const BsdfRec &r : c->bsdfs) if (bsdf_uses_bitmap(r)) c->diffuse_only = false;   // the plain-diffuse kernel reads constants only
    {   // bitmap textures: one device buffer of texels, records pointing into it
        std::vector<BitmapRec> recs; uint32_t bad = 0;
        if (const char *why = build_bitmap_table(s, recs, &bad)) return fail(c, MI_ERR_INVALID, "bitmap %u: %s", bad, why);
        std::vector<size_t> first(recs.size() + 1, 0);
        for (size_t i = 0; i < recs.size(); ++i) first[i + 1] = first[i] + (size_t) recs[i].width * recs[i].height * recs[i].channels;
        HIP_TRY(c, c->d_bitmap_data.resize(std::max<size_t>(first.back(), 1)));
        for (size_t i = 0; i < recs.size(); ++i) {
            HIP_TRY(c, hipMemcpyAsync(c->d_bitmap_data.p + first[i], recs[i].data, (first[i + 1] - first[i]) * sizeof(float), hipMemcpyHostToDevice, c->stream));
            recs[i].data = c->d_bitmap_data.p + first[i];
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));            // the caller's arrays may go away after this call
        HIP_TRY(c, c->d_bitmaps.upload(recs, c->stream));
        c->bitmap_count = (uint32_t) recs.size();
    }
    c->trio = true;
    for (const BsdfRec &r : c->bsdfs) if (r.type != BSDF_TYPE_DIFFUSE && r.type != BSDF_TYPE_DIELECTRIC && r.type != BSDF_TYPE_ROUGHCONDUCTOR) c->trio = false;
    c->textured = !c->tri_uv_in.empty();
    for (const BsdfRec &r : c->bsdfs) if (bsdf_uses_bitmap(r) || bsdf_is_extended(r)) c->textured = true;   // -> the MATS_ALL kernels
    c->nested = false;
    for (const BsdfRec &r : c->bsdfs) if (bsdf_is_nested(r)) c->nested = c->textured = true;                // -> the MATS_NESTED kernels
    c->bsdf_tables.assign(s->bsdf_tables, s->bsdf_tables + s->bsdf_table_floats);
    HIP_TRY(c, c->d_bsdf_tables.upload(c->bsdf_tables, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // emitters: Mesh::build_pmf (mesh.cpp:285-312) + DiscreteDistribution (distr_1d.h:55-87)
    c->emitters.clear(); c->emit_tri.clear(); c->emit_vnorm.clear(); c->emit_pmf.clear(); c->emit_cdf.clear();
    bool any_emit_normals = false;
    auto push_env = [&]() { EmitterRec r; memset(&r, 0, sizeof r); r.type = EMITTER_ENVMAP; r.shape = 0xffffffffu; c->emitters.push_back(r); };
    c->lights.clear(); c->constant_light = -1; c->lights_on = s->light_count != 0;
    auto push_light = [&](uint32_t k) {                        // an emitter record without shape and face tables: `tri_first` = its light record
        const mi_light &l = s->lights[k];
        LightRec q; memset(&q, 0, sizeof q);
#if MIW_SPECTRAL
        memcpy(&q.value, &l.value_tex, sizeof(TexRec));
#else
        q.value.type = TEX_RGB; memcpy(q.value.v, l.value, 12);
#endif
        q.type = EMITTER_POINT + l.type; q.emitter_index = (uint32_t) c->emitters.size();
        memcpy(q.position, l.position, 12); memcpy(q.direction, l.direction, 12); memcpy(q.to_object, l.to_object, 64);
        q.cutoff_angle = l.cutoff_angle; q.cos_cutoff_angle = l.cos_cutoff_angle; q.cos_beam_width = l.cos_beam_width; q.inv_transition_width = l.inv_transition_width;
        q.dist = 2.f * light_bsphere_radius(l.bsphere_radius);
        EmitterRec r; memset(&r, 0, sizeof r); r.type = q.type; r.shape = 0xffffffffu; r.tri_first = (uint32_t) c->lights.size();
        if (l.type == MI_LIGHT_CONSTANT) c->constant_light = (int32_t) c->lights.size();
        c->lights.push_back(q); c->emitters.push_back(r);
    };
    // (with lights: every slot before an area emitter's own that the environment map or a light takes)
    auto push_specials = [&]() { while (c->emitters.size() < emitter_total && slot_light[c->emitters.size()] != -1) { const int32_t k = slot_light[c->emitters.size()]; if (k == -2) push_env(); else push_light((uint32_t) k); } };
    for (uint32_t i = 0; i < s->emitter_count; ++i) {
        if (s->light_count) push_specials();
        else if (s->envmap && s->envmap->emitter_index == i) push_env();
        const mi_emitter &e = s->emitters[i];
        if (e.shape >= s->shape_count) return fail(c, MI_ERR_INVALID, "emitter %u: shape index out of range", i);
        const mi_shape &sh = s->shapes[e.shape];
        if (sh.emitter != (int32_t) i) return fail(c, MI_ERR_INVALID, "emitter %u: shape %u does not point back to it", i, e.shape);
        if (sh.face_count == 0) return fail(c, MI_ERR_INVALID, "emitter %u: cannot create sampling table for an empty mesh", i);
        EmitterRec r; memset(&r, 0, sizeof r);
#if MIW_SPECTRAL
        if (e.radiance_tex.type != MI_TEX_D65 && e.radiance_tex.type != MI_TEX_SRGB_D65 && e.radiance_tex.type != MI_TEX_UNIFORM)
            return fail(c, MI_ERR_INVALID, "emitter %u: the scalar_spectral library needs a spectral radiance record", i);
        memcpy(&r.radiance, &e.radiance_tex, sizeof(TexRec));
#else
        r.radiance.type = TEX_RGB; memcpy(r.radiance.v, e.radiance, 12);
#endif
        if (shape_rect[e.shape] >= 0) {                        // area light on an analytic rectangle: no face tables
            const AnalyticRec &q = c->rects[shape_rect[e.shape]];
            r.shape = e.shape; r.tri_first = (uint32_t) shape_rect[e.shape]; r.tri_count = 0; r.flags = 2u;
            r.valid_lo = r.valid_hi = 0; r.normalization = q.inv_area; r.sum = rcp(q.inv_area);
            c->emitters.push_back(r);
            continue;
        }
        r.shape = e.shape; r.tri_first = (uint32_t) c->emit_pmf.size(); r.tri_count = sh.face_count;
        r.flags = (sh.flags & MI_SHAPE_HAS_NORMALS) ? 1u : 0u;
        any_emit_normals = any_emit_normals || r.flags;
        double sum = 0.0; uint32_t vlo = 0xffffffffu, vhi = 0;
        for (uint32_t k = 0; k < sh.face_count; ++k) {
            const Tri &t = c->tris_in[sh.first_face + k];
            float area = face_area(ld3(t.p0), ld3(t.p1), ld3(t.p2));
            if (area < 0.f) return fail(c, MI_ERR_INVALID, "emitter %u: negative face area", i);
            c->emit_pmf.push_back(area);
            sum += (double) area;
            c->emit_cdf.push_back((float) sum);
            if (area > 0.f) { if (vlo == 0xffffffffu) vlo = k; vhi = k; }
            for (int q = 0; q < 3; ++q) c->emit_tri.push_back(t.p0[q]);
            for (int q = 0; q < 3; ++q) c->emit_tri.push_back(t.p1[q]);
            for (int q = 0; q < 3; ++q) c->emit_tri.push_back(t.p2[q]);
            for (int q = 0; q < 9; ++q)
                c->emit_vnorm.push_back(r.flags ? c->tri_vn_in[(size_t) (sh.first_face + k) * 9 + q] : 0.f);
        }
        if (vlo == 0xffffffffu) return fail(c, MI_ERR_INVALID, "emitter %u: no probability mass found", i);
        r.valid_lo = vlo; r.valid_hi = vhi;
        r.sum = (float) sum; r.normalization = (float) (1.0 / sum);
        c->emitters.push_back(r);
    }
    if (!any_emit_normals) c->emit_vnorm.clear();
    c->shape_normals = any_normals; c->emitter_normals = any_emit_normals;
    if (s->light_count) push_specials();
    else if (s->envmap && s->envmap->emitter_index >= s->emitter_count) push_env();
    if (c->lights_on) { c->nested = c->textured = true; c->diffuse_only = c->trio = false; }    // -> the MATS_LIGHTS kernels (the MATS_NESTED table + miw/light.h)

    HIP_TRY(c, hipSetDevice(c->device));
    c->have_env = false;
#if MIW_SPECTRAL
    if (s->envmap && !s->envmap->density)
        return fail(c, MI_ERR_INVALID, "envmap: the scalar_spectral library needs mi_envmap::density (its texels are model coefficients, include/miwave.h)");
#endif
    if (s->envmap) {
        EnvmapTables t = envmap_build(*s->envmap);
        if (!t.ok) return fail(c, MI_ERR_INVALID, "envmap: needs >= 2x2 texels, a non-zero luminance sum and an invertible to_world");
        HIP_TRY(c, c->d_env_data.upload(t.data, c->stream));
        HIP_TRY(c, c->d_env_levels.upload(t.levels, c->stream));
        t.rec.data = c->d_env_data.p; t.rec.levels = c->d_env_levels.p;
        c->env_host = t.rec; c->env_levels_total = t.levels.size();
        std::vector<EnvmapRec> one(1, t.rec);
        HIP_TRY(c, c->d_env.upload(one, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->have_env = true;
    }
    HIP_TRY(c, c->d_shapes.upload(c->shapes, c->stream));
    HIP_TRY(c, c->d_tri_uv.upload(c->tri_uv_in, c->stream));
    HIP_TRY(c, c->d_rects.upload(c->rects, c->stream));
    HIP_TRY(c, c->d_bsdfs.upload(c->bsdfs, c->stream));
    HIP_TRY(c, c->d_emitters.upload(c->emitters, c->stream));
    HIP_TRY(c, c->d_lights.upload(c->lights, c->stream));
    HIP_TRY(c, c->d_media.upload(c->media, c->stream));
    HIP_TRY(c, c->d_shape_media.upload(c->shape_media, c->stream));
    HIP_TRY(c, c->d_emit_tri.upload(c->emit_tri, c->stream));
    HIP_TRY(c, c->d_emit_vnorm.upload(c->emit_vnorm, c->stream));
    HIP_TRY(c, c->d_emit_pmf.upload(c->emit_pmf, c->stream));
    HIP_TRY(c, c->d_emit_cdf.upload(c->emit_cdf, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->have_scene = true;
    return MI_OK;
}

// ---- BVH build ------------------------------------------------------------------------
// dwords of the tables stage_tables() copies into LDS (shapes, bsdfs, emitters, emit_tri, emit_vnorm, emit_pmf, emit_cdf), each
// padded to 16 bytes; returns the bytes of the block
static size_t lds_table_bytes(const mi_ctx *c, uint32_t words[12], bool with_tris) {
    words[0] = (uint32_t) (c->shapes.size() * sizeof(ShapeRec) / 4); words[1] = (uint32_t) (c->bsdfs.size() * sizeof(BsdfRec) / 4);
    words[2] = (uint32_t) (c->emitters.size() * sizeof(EmitterRec) / 4);
    words[3] = (uint32_t) c->emit_tri.size(); words[4] = (uint32_t) c->emit_vnorm.size(); words[5] = (uint32_t) c->emit_pmf.size(); words[6] = (uint32_t) c->emit_cdf.size();
    // packet scenes: the triangle records (leaf order), their vertex normals and per-face texture coordinates as well
    words[7] = with_tris ? (uint32_t) (c->tris_in.size() * sizeof(Tri) / 4) : 0u;
    words[8] = with_tris ? (uint32_t) c->tri_vn_in.size() : 0u; words[9] = with_tris ? (uint32_t) c->tri_uv_in.size() : 0u;
    // ... and the two tables the packet kernels build behind them (trace.h: stage_tables): a TriFrame per triangle, a normal (16 B) per emitter face
    words[10] = with_tris ? (uint32_t) (c->tris_in.size() * sizeof(TriFrame) / 4) : 0u;
    words[11] = with_tris ? (uint32_t) (c->emit_tri.size() / 9 * 4) : 0u;
    size_t total = 0;
    for (int k = 0; k < 12; ++k) total += ((size_t) words[k] + 3u) / 4u * 16u;
    total += c->lights.size() * sizeof(LightRec);             // the light table behind them (TraceLds::light_words; sizeof(LightRec) is a multiple of 16)
    return total;
}

mi_status mi_bvh_build(mi_ctx *c, int32_t quality) {
    if (!c) return MI_ERR_INVALID;
    if (!c->have_scene) return fail(c, MI_ERR_STATE, "mi_bvh_build: no scene uploaded");
    const bool force_tree = (quality & MI_BVH_FORCE_TREE) != 0;
    const int32_t quality_flags = quality;
    quality &= ~(MI_BVH_FORCE_TREE | MI_BVH_NO_LEAF_FILTER | MI_BVH_RADIX_TREE);
    if (quality != 1 && quality != 0) return fail(c, MI_ERR_INVALID, "mi_bvh_build: quality must be 0 or 1");
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    const float pad_unit = scene_pad_unit(c->tris_in);        // 1e-5 x the largest |coordinate| (bvh_build.h): boxes grow by two units, the accept rule by one
    BvhBuildResult r;                       // host SAH result (nodes kept for the tiny-scene leaf filter)
    uint32_t node_count = 0, tri_count = (uint32_t) c->tris_in.size(), depth = 0;
    bool built_on_device = false;
    // quality 0: the 4-wide tree is collapsed on the device as well (bvh4_device.h); these say whether that happened
    bool wide_on_device = false; uint32_t dev4_nodes = 0, dev4_stack = 0;
    const bool wide_on = !c->opt.off("MIW_BVH4");
    // the 8-wide tree (the phase machine's default since round 5): off with MIW_BVH8=0, and whenever the 4-wide walk is asked for by name
    const bool wide8_on = wide_on && !c->opt.off("MIW_BVH8") && !c->opt.get("MIW_BVH4_FAN");
    uint32_t dev8_nodes = 0, dev8_depth = 0; double ms_bvh8 = 0.0;
    std::vector<uint32_t> sah_level_start;                    // the device SAH builder's level table (first node of every level)
    int max_fan = 4;
    if (const char *e = c->opt.get("MIW_BVH4_FAN")) max_fan = std::min(4, std::max(2, atoi(e)));
    double ms_bvh4 = 0.0;
    uint32_t tab_words_[12];
    // (the packet kernels read the scene's small tables from LDS: a scene of <= 64 triangles whose tables would not fit beside the
    // packets — dozens of unused BSDF records — is walked as a tree instead)
    const bool tiny = c->tris_in.size() <= MIW_BRUTE_MAX_TRIS && !force_tree && c->rects.empty() &&   // packets are triangles only
                      (!MIW_LDS_TABLES || lds_table_bytes(c, tab_words_, true) <= 24u * 1024u);
    if (quality == 0 && !tiny && tri_count >= 2) {
        // ---- device LBVH (lbvh_device.h) ----
        hipStream_t s = c->stream;
        const int n = (int) tri_count;
        TmpBuf<Tri> d_in; TmpBuf<float> d_vn_in; TmpBuf<uint64_t> d_keys, d_keys_sorted; TmpBuf<uint32_t> d_bounds, d_arrivals, d_height, d_span, d_first;
        uint32_t lbvh_leaf = 2u;                               // triangles per fat leaf (measured on the interior: 1 -> 311, 2 -> 352, 4 -> 334, 8 -> 302 Msamples/s; SAH 369); MIW_LBVH_LEAF = 1 .. 16 overrides
        if (const char *e = c->opt.get("MIW_LBVH_LEAF")) lbvh_leaf = (uint32_t) std::min(16, std::max(1, atoi(e)));
        if ((uint32_t) n <= lbvh_leaf) lbvh_leaf = 1u;          // (the root must stay an inner node)
        TmpBuf<LbvhBox> d_boxes; TmpBuf<LbvhLinks> d_inner; TmpBuf<int32_t> d_leaf_parent; TmpBuf<unsigned char> d_tmp;
        auto free_tmp = [&]() { d_in.release(); d_vn_in.release(); d_keys.release(); d_keys_sorted.release(); d_bounds.release();
                                d_arrivals.release(); d_height.release(); d_boxes.release(); d_inner.release(); d_leaf_parent.release(); d_tmp.release();
                                d_span.release(); d_first.release(); };
        // MIW_DEBUG_ALLOC=1: where the set-up time of a build goes (stderr, ms since the previous mark)
        auto lap_t = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) {
            if (!c->opt.get("MIW_DEBUG_ALLOC")) return;
            (void) hipStreamSynchronize(s);
            const auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "[miwave]   build set-up: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - lap_t).count());
            lap_t = now;
        };
        HIP_TRY(c, d_in.upload(c->tris_in, s));
        lap("triangle upload");
        if (!c->tri_vn_in.empty()) HIP_TRY(c, d_vn_in.upload(c->tri_vn_in, s));
        lap("vertex-normal upload");
        HIP_TRY(c, c->d_nodes.resize(n)); HIP_TRY(c, c->d_tris.resize(n)); HIP_TRY(c, d_height.resize(n));
        if (!c->tri_vn_in.empty()) HIP_TRY(c, c->d_tri_vn.resize((size_t) n * 9));
        lap("node / triangle buffers");
        const dim3 blk(256), grd((unsigned) ((n + 255) / 256));
        // Which device builder. Default: the level-by-level binned-SAH sweep (sah_device.h) — the host builder's tree, node for node.
        // MI_BVH_RADIX_TREE / MIW_DEVICE_BUILDER=lbvh: the radix tree over Morton codes of rounds 2 - 3 (lbvh_device.h; measured 7 % / 16 % behind the SAH
        // tree on the interior / the material balls: A/B runs). A scene the sweep hands back (need_host: coincident centroids) takes
        // the host builder, like quality 1.
        enum { DEV_SAH = 0, DEV_LBVH = 1 } dev_builder = (quality_flags & MI_BVH_RADIX_TREE) ? DEV_LBVH : DEV_SAH;
        if (const char *e = c->opt.get("MIW_DEVICE_BUILDER")) {        // only the two names override the flag; anything else leaves the caller's choice alone
            if (!strcmp(e, "lbvh")) dev_builder = DEV_LBVH; else if (!strcmp(e, "sah")) dev_builder = DEV_SAH;
        }
        bool sah_need_host = false;
        if (dev_builder == DEV_SAH) {
            uint32_t max_leaf = 4u;                                        // (bvh_build_sah's default leaf size: the same tree; MIW_MAX_LEAF overrides on both sides)
            if (const char *e = c->opt.get("MIW_MAX_LEAF")) max_leaf = (uint32_t) std::min(16, std::max(1, atoi(e)));
            const uint32_t un = (uint32_t) n;
            const float pad = 2.f * pad_unit;
            TmpBuf<SahPrim> d_prim; TmpBuf<uint32_t> d_ia, d_ib, d_flags, d_rank; TmpBuf<SahCand> d_ca, d_cb; TmpBuf<SahDecision> d_dec; TmpBuf<SahState> d_state;
            TmpBuf<unsigned char> d_scan_tmp; TmpBuf<SahHuge> d_huge;
            HIP_TRY(c, d_huge.resize(MIW_SAH_HUGE_CANDS));
            HIP_TRY(c, d_prim.resize(un)); HIP_TRY(c, d_ia.resize(un)); HIP_TRY(c, d_ib.resize(un)); HIP_TRY(c, d_flags.resize(un)); HIP_TRY(c, d_rank.resize(un));
            HIP_TRY(c, d_ca.resize(un)); HIP_TRY(c, d_cb.resize(un)); HIP_TRY(c, d_dec.resize(un)); HIP_TRY(c, d_state.resize(1));
            size_t scan_bytes = 0;
            HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, d_flags.p, d_rank.p, 0u, (size_t) n, rocprim::plus<uint32_t>(), s));
            HIP_TRY(c, d_scan_tmp.resize(scan_bytes + 16));
            lap("builder temporaries");
            HIP_TRY(c, hipStreamSynchronize(s));
            const auto t_setup = std::chrono::steady_clock::now();     // (uploads and allocations behind us)
            hipLaunchKernelGGL(k_sah_prims, grd, blk, 0, s, d_in.p, un, pad, d_prim.p, d_ia.p);
            const SahCand root = { 0u, un, -1, 0u };
            HIP_TRY(c, hipMemcpyAsync(d_ca.p, &root, sizeof root, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemsetAsync(d_state.p, 0, sizeof(SahState), s));
            std::vector<uint32_t> level_start{ 0u };
            uint32_t n_cand = 1u, base = 0u, level = 0u;
            bool big_left = true;                                        // candidates of more than MIW_SAH_BIG triangles in the current level
            uint32_t level_max = un;                                     // the largest candidate of the current level (0: none above MIW_SAH_BIG)
            const bool huge_on = !c->opt.off("MIW_SAH_HUGE");     // MIW_SAH_HUGE=0: one workgroup per candidate, as round 4 (A/B runs)
            while (n_cand > 0u && !sah_need_host) {
                const SahCand *cur = (level & 1u) ? d_cb.p : d_ca.p; SahCand *nxt = (level & 1u) ? d_ca.p : d_cb.p;
                const uint32_t *ic = (level & 1u) ? d_ib.p : d_ia.p; uint32_t *in = (level & 1u) ? d_ia.p : d_ib.p;
                // few candidates: 1024 threads each. Many: one wavefront each — except those above MIW_SAH_BIG triangles (an unbalanced
                // split leaves a 100 k-triangle candidate next to thousands of small ones twelve levels down; one wavefront on it cost
                // 15 ms), which a second launch of the 1024-thread kernel takes; `big_left` (read back with the level's totals) says
                // whether the level holds any.
                const bool all_big = n_cand <= 512u;
                const uint32_t none = 0u, all = 0xffffffffu;
                // candidates above MIW_SAH_HUGE triangles: sliced over several workgroups (sah_device.h: k_sah_huge_*), the others as before
                const bool huge = huge_on && level_max > MIW_SAH_HUGE && n_cand <= MIW_SAH_HUGE_CANDS;
                if (huge) {
                    const dim3 hgrid(n_cand, (level_max + MIW_SAH_SLICE - 1u) / MIW_SAH_SLICE);
                    const uint32_t words = n_cand * (uint32_t) (sizeof(SahHuge) / 4u);
                    hipLaunchKernelGGL(k_sah_huge_init, dim3((words + 255u) / 256u), dim3(256), 0, s, d_huge.p, n_cand);
                    hipLaunchKernelGGL(k_sah_huge_box, hgrid, dim3(1024), 0, s, cur, n_cand, ic, d_prim.p, d_huge.p);
                    hipLaunchKernelGGL(k_sah_huge_bins, hgrid, dim3(1024), 0, s, cur, n_cand, ic, d_prim.p, level, d_huge.p);
                    hipLaunchKernelGGL(k_sah_huge_finish, dim3(n_cand), dim3(64), 0, s, cur, n_cand, level, max_leaf, d_huge.p, d_dec.p, d_flags.p, d_state.p);
                }
                if (all_big || big_left) hipLaunchKernelGGL(k_sah_decide<1024>, dim3(n_cand), dim3(1024), 0, s, cur, n_cand, ic, d_prim.p, level, max_leaf, d_dec.p, d_flags.p, d_state.p, all_big ? none : MIW_SAH_BIG, huge ? MIW_SAH_HUGE : all);
                if (!all_big) hipLaunchKernelGGL(k_sah_decide<64>, dim3(n_cand), dim3(64), 0, s, cur, n_cand, ic, d_prim.p, level, max_leaf, d_dec.p, d_flags.p, d_state.p, none, big_left ? MIW_SAH_BIG : all);
                HIP_TRY(c, rocprim::exclusive_scan(d_scan_tmp.p, scan_bytes, d_flags.p, d_rank.p, 0u, (size_t) n_cand, rocprim::plus<uint32_t>(), s));
                hipLaunchKernelGGL(k_sah_totals, dim3(1), dim3(1), 0, s, d_flags.p, d_rank.p, n_cand, d_state.p);
                if (all_big || big_left) hipLaunchKernelGGL(k_sah_apply<1024>, dim3(n_cand), dim3(1024), 0, s, cur, n_cand, ic, in, d_prim.p, d_dec.p, d_rank.p, base, c->d_nodes.p, nxt, d_state.p, all_big ? none : MIW_SAH_BIG, all, un);
                if (!all_big) hipLaunchKernelGGL(k_sah_apply<64>, dim3(n_cand), dim3(64), 0, s, cur, n_cand, ic, in, d_prim.p, d_dec.p, d_rank.p, base, c->d_nodes.p, nxt, d_state.p, none, big_left ? MIW_SAH_BIG : all, un);
                SahState h;
                HIP_TRY(c, hipMemcpyAsync(&h, d_state.p, sizeof h, hipMemcpyDeviceToHost, s));
                HIP_TRY(c, hipStreamSynchronize(s));
                HIP_TRY(c, hipGetLastError());
                sah_need_host = h.need_host != 0u || level >= 62u || (uint64_t) base + h.n_inner > (uint64_t) un - 1u;
                big_left = h.max_count > MIW_SAH_BIG; level_max = h.max_count;
                if (big_left) HIP_TRY(c, hipMemsetAsync(&d_state.p->max_count, 0, sizeof(uint32_t), s));     // (counts the next level afresh)
                depth = level;
                base += h.n_inner; level_start.push_back(base);
                n_cand = 2u * h.n_inner; ++level;
            }
            const auto t_levels = std::chrono::steady_clock::now();
            if (!sah_need_host) {
                for (size_t L = level_start.size() - 1; L-- > 0;) {
                    const uint32_t cnt = level_start[L + 1] - level_start[L];
                    if (cnt) hipLaunchKernelGGL(k_sah_heights, dim3((cnt + 255u) / 256u), blk, 0, s, c->d_nodes.p, level_start[L], level_start[L + 1], d_height.p);
                }
                const uint32_t *idx_final = (level & 1u) ? d_ib.p : d_ia.p;
                hipLaunchKernelGGL(k_sah_gather, grd, blk, 0, s, d_in.p, c->tri_vn_in.empty() ? (const float *) nullptr : d_vn_in.p, idx_final, un,
                                   c->d_tris.p, c->tri_vn_in.empty() ? (float *) nullptr : c->d_tri_vn.p);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipStreamSynchronize(s));
                node_count = base;
                built_on_device = true;
                sah_level_start = level_start;
                c->counters.bvh_builder = 3u;
                if (c->opt.get("MIW_DEBUG")) {
                    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                    fprintf(stderr, "[miwave] device builder: binned SAH by levels, %u triangles, %u inner nodes, depth %u; upload + allocations %.2f ms, %u levels %.2f ms, heights + gather %.2f ms\n",
                            un, node_count, depth, ms(t0, t_setup), level, ms(t_setup, t_levels), ms(t_levels, std::chrono::steady_clock::now()));
                }
            }
        } else {
            HIP_TRY(c, d_keys.resize(n)); HIP_TRY(c, d_keys_sorted.resize(n)); HIP_TRY(c, d_bounds.resize(6));
            HIP_TRY(c, d_arrivals.resize(n)); HIP_TRY(c, d_boxes.resize((size_t) 2 * n));
            HIP_TRY(c, d_inner.resize(n)); HIP_TRY(c, d_leaf_parent.resize(n)); HIP_TRY(c, d_span.resize(n)); HIP_TRY(c, d_first.resize(n));
            const uint32_t init_bounds[6] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u };
            HIP_TRY(c, hipMemcpyAsync(d_bounds.p, init_bounds, sizeof init_bounds, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemsetAsync(d_arrivals.p, 0, (size_t) n * sizeof(uint32_t), s));
            HIP_TRY(c, hipMemsetAsync(d_height.p, 0, (size_t) n * sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_lbvh_bounds, dim3(std::min<unsigned>(grd.x, 1024u)), blk, 0, s, d_in.p, (uint32_t) n, d_bounds.p);
            hipLaunchKernelGGL(k_lbvh_morton, grd, blk, 0, s, d_in.p, (uint32_t) n, d_bounds.p, d_keys.p);
            size_t tmp_bytes = 0;
            HIP_TRY(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys.p, d_keys_sorted.p, (size_t) n, 0u, 64u, s));
            HIP_TRY(c, d_tmp.resize(tmp_bytes + 16));
            HIP_TRY(c, rocprim::radix_sort_keys(d_tmp.p, tmp_bytes, d_keys.p, d_keys_sorted.p, (size_t) n, 0u, 64u, s));
            // box padding (bvh.h, bvh_build.h: scene_pad_unit): 2e-5 x the largest |coordinate|
            uint32_t hb[6];
            HIP_TRY(c, hipMemcpyAsync(hb, d_bounds.p, sizeof hb, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            float m = 0.f;
            for (int k = 0; k < 6; ++k) { uint32_t o = hb[k]; float f = u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); m = std::max(m, std::fabs(f)); }
            const float pad = 2.f * std::max(1e-5f * m, 1e-30f);
            // the radix tree over the Morton order (lbvh_device.h)
            HIP_TRY(c, hipMemsetAsync(d_height.p, 0, (size_t) n * sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_lbvh_leaves, grd, blk, 0, s, d_in.p, c->tri_vn_in.empty() ? (const float *) nullptr : d_vn_in.p, d_keys_sorted.p,
                               (uint32_t) n, pad, c->d_tris.p, c->tri_vn_in.empty() ? (float *) nullptr : c->d_tri_vn.p, d_boxes.p);
            hipLaunchKernelGGL(k_lbvh_tree, grd, blk, 0, s, d_keys_sorted.p, n, d_inner.p, d_leaf_parent.p, d_span.p, d_first.p);
            hipLaunchKernelGGL(k_lbvh_fit, grd, blk, 0, s, d_inner.p, d_leaf_parent.p, n, d_boxes.p, d_arrivals.p, d_height.p, d_span.p, lbvh_leaf);
            hipLaunchKernelGGL(k_lbvh_emit, grd, blk, 0, s, d_inner.p, d_boxes.p, n, c->d_nodes.p, d_span.p, d_first.p, lbvh_leaf);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(&depth, d_height.p, sizeof depth, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            c->counters.bvh_builder = 1u;
            if (c->opt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] device builder: LBVH, %u triangles, height %u\n", (uint32_t) n, depth);
        node_count = (uint32_t) (n - 1);
        built_on_device = depth <= MIW_BVH_MAX_DEPTH;     // deeper (many coincident centroids): take the SAH builder
        }
        // ---- the 4-wide tree of the phase machine, collapsed level by level on the device (bvh4_device.h); the heights the
        // collapse's fit test needs are the builder's (k_sah_heights / k_lbvh_fit). MIW_BVH4_HOST=1 keeps round 2's read-back + host collapse (A/B runs) ----
        const uint32_t budget4 = MIW_STACK_ENTRIES - 1;    // one entry of slack: the node body's unconditional stores
        if (built_on_device && wide_on && depth <= budget4 && !c->opt.get("MIW_NO_STACK") && !c->opt.get("MIW_BVH4_HOST")) {
            auto t4 = std::chrono::steady_clock::now();
            TmpBuf<Bvh4Item> fa, fb; TmpBuf<Bvh4Levels> lv;
            HIP_TRY(c, fa.resize(n)); HIP_TRY(c, fb.resize(n)); HIP_TRY(c, lv.resize(1)); HIP_TRY(c, c->d_nodes4.resize(n));
            Bvh4Levels h; memset(&h, 0, sizeof h); h.count[0] = 1;
            const Bvh4Item root = { 0, budget4 };
            HIP_TRY(c, hipMemcpyAsync(lv.p, &h, sizeof h, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(fa.p, &root, sizeof root, hipMemcpyHostToDevice, s));
            const uint32_t levels = std::min<uint32_t>(depth + 1u, 62u);
            for (uint32_t L = 0; L < levels; ++L)
                hipLaunchKernelGGL(k_bvh4_level, grd, blk, 0, s, c->d_nodes.p, d_height.p, (L & 1u) ? fb.p : fa.p, (L & 1u) ? fa.p : fb.p, lv.p,
                                   c->d_nodes4.p, L, budget4, max_fan);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(&h, lv.p, sizeof h, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            for (uint32_t L = 0; L < levels; ++L) dev4_nodes += h.count[L];
            dev4_stack = h.stack_bound;
            wide_on_device = !h.failed && h.count[levels] == 0 && dev4_stack <= budget4 && dev4_nodes <= (uint32_t) n;
            ms_bvh4 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t4).count();
        }
        // ---- the 8-wide tree (miw/bvh8.h) from the same BVH2, on the device as well (bvh8_device.h): the programme bottom-up over the
        // builder's levels, the collapse top-down, triangles + vertex normals gathered into the tree's order. SAH sweep only (the
        // radix tree has no level table: it keeps the 4-wide tree). MIW_BVH8=0 / MIW_BVH4=0 / MIW_BVH4_FAN switch it off (A/B runs). ----
        if (built_on_device && dev_builder == DEV_SAH && wide8_on && !c->opt.get("MIW_NO_STACK")) {
            auto t8 = std::chrono::steady_clock::now();
            TmpBuf<Bvh8Dp> d_dp; TmpBuf<int32_t> ga, gb; TmpBuf<Bvh8Levels> lv8; TmpBuf<uint32_t> d_perm;
            HIP_TRY(c, d_dp.resize(node_count)); HIP_TRY(c, ga.resize(n)); HIP_TRY(c, gb.resize(n)); HIP_TRY(c, lv8.resize(1)); HIP_TRY(c, d_perm.resize(n));
            HIP_TRY(c, c->d_nodes8.resize(n)); HIP_TRY(c, c->d_tris8.resize(n));
            if (!c->tri_vn_in.empty()) HIP_TRY(c, c->d_tri_vn8.resize((size_t) n * 9));
            for (size_t L = sah_level_start.size() - 1; L-- > 0;) {
                const uint32_t cnt = sah_level_start[L + 1] - sah_level_start[L];
                if (cnt) hipLaunchKernelGGL(k_bvh8_dp, dim3((cnt + 255u) / 256u), blk, 0, s, c->d_nodes.p, d_dp.p, sah_level_start[L], sah_level_start[L + 1]);
            }
            Bvh8Levels h8; memset(&h8, 0, sizeof h8); h8.count[0] = 1;
            const int32_t root8 = 0;
            HIP_TRY(c, hipMemcpyAsync(lv8.p, &h8, sizeof h8, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(ga.p, &root8, sizeof root8, hipMemcpyHostToDevice, s));
            const uint32_t levels8 = std::min<uint32_t>(depth + 1u, 62u);
            for (uint32_t L = 0; L < levels8; ++L)
                hipLaunchKernelGGL(k_bvh8_level, grd, blk, 0, s, c->d_nodes.p, d_dp.p, (L & 1u) ? gb.p : ga.p, (L & 1u) ? ga.p : gb.p, lv8.p,
                                   c->d_nodes8.p, d_perm.p, L, (uint32_t) n, (uint32_t) n);
            hipLaunchKernelGGL(k_bvh8_gather, grd, blk, 0, s, c->d_tris.p, c->tri_vn_in.empty() ? (const float *) nullptr : c->d_tri_vn.p, d_perm.p, (uint32_t) n,
                               c->d_tris8.p, c->tri_vn_in.empty() ? (float *) nullptr : c->d_tri_vn8.p);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(&h8, lv8.p, sizeof h8, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            uint32_t nn = 0, dd = 0;
            for (uint32_t L = 0; L < levels8; ++L) { nn += h8.count[L]; dd += h8.count[L] ? 1u : 0u; }
            if (!h8.failed && h8.count[levels8] == 0 && h8.tri_next == (uint32_t) n && dd <= MIW_BVH8_STACK && nn <= (uint32_t) n) { dev8_nodes = nn; dev8_depth = dd; }
            ms_bvh8 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t8).count();
        }
        free_tmp();
    }
    std::vector<float> vn;
    if (!built_on_device) {
        // ---- host binned SAH (bvh_build.h) ----
        // tiny scenes are swept through their SAH leaves' boxes (trace2): leaf size tuned for that filter
        uint32_t max_leaf = tiny ? MIW_BRUTE_MAX_LEAF : 4u;
        if (const char *e = c->opt.get("MIW_MAX_LEAF")) max_leaf = (uint32_t) atoi(e);
        r = bvh_build_sah(c->tris_in, -1.f, max_leaf);
        if (r.depth > MIW_BVH_MAX_DEPTH) return fail(c, MI_ERR_INVALID, "BVH depth %u exceeds the traversal trail", r.depth);
        if (!c->tri_vn_in.empty()) {
            vn.resize(c->tri_vn_in.size());
            for (size_t i = 0; i < r.order.size(); ++i)
                memcpy(&vn[i * 9], &c->tri_vn_in[(size_t) r.order[i] * 9], 36);
        }
        HIP_TRY(c, c->d_nodes.upload(r.nodes, c->stream));
        HIP_TRY(c, c->d_tris.upload(r.tris, c->stream));
        HIP_TRY(c, c->d_tri_vn.upload(vn, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        node_count = (uint32_t) r.nodes.size(); tri_count = (uint32_t) r.tris.size(); depth = r.depth;
    }
    c->counters.bvh_on_device = built_on_device ? 1u : 0u;
    if (!built_on_device) c->counters.bvh_builder = 0u;

    SceneView &v = c->view;
    v.accept_pad = pad_unit;                                  // shape.h: the bounds rule of every triangle hit
    v.tri_bounds = nullptr;
    v.nodes = c->d_nodes.p; v.node_count = node_count;
    v.tris = c->d_tris.p; v.tri_count = tri_count;
    v.tri_vn = c->tri_vn_in.empty() ? nullptr : c->d_tri_vn.p;
    v.tri_uv = c->tri_uv_in.empty() ? nullptr : c->d_tri_uv.p;
    v.bitmaps = c->bitmap_count ? c->d_bitmaps.p : nullptr;
    v.bsdf_tables = c->bsdf_tables.empty() ? nullptr : c->d_bsdf_tables.p;
    v.shapes = c->d_shapes.p; v.shape_count = (uint32_t) c->shapes.size();
    v.bsdfs = c->d_bsdfs.p; v.bsdf_count = (uint32_t) c->bsdfs.size();
    v.emitters = c->d_emitters.p; v.emitter_count = (uint32_t) c->emitters.size();
    scene_view_prepare(v);
    v.emit_tri = c->d_emit_tri.p; v.emit_vnorm = c->emit_vnorm.empty() ? nullptr : c->d_emit_vnorm.p;
    v.emit_pmf = c->d_emit_pmf.p; v.emit_cdf = c->d_emit_cdf.p;
    v.env = c->have_env ? c->d_env.p : nullptr;
    v.lights = c->lights.empty() ? nullptr : c->d_lights.p;
    v.constant = c->constant_light >= 0 ? c->d_lights.p + c->constant_light : nullptr;
    v.env_top = nullptr; v.env_top_count = v.env_top_base = 0;      // (set inside the kernels that stage them: trace.h stage_tables)
    v.tri_frames = nullptr; v.emit_face_n = nullptr;                // (built in LDS by the packet kernels that read them: trace.h stage_tables)
    v.rects = c->rects.empty() ? nullptr : c->d_rects.p; v.rect_count = (uint32_t) c->rects.size();

    // LDS plan: whole scene if it fits in 16 KiB (keeps 8 workgroups/CU resident),
    // otherwise the top of the tree only.
    size_t all = (size_t) node_count * sizeof(BvhNode) + (size_t) tri_count * sizeof(Tri);
    c->lds_cfg.brute = 0; c->lds_cfg.leaves = 0; c->lds_cfg.stack = 0; c->lds_cfg.stack16 = 0; v.leaf_boxes = nullptr; v.nodes4 = nullptr; c->nodes4_count = c->nodes4_stack = 0;
    v.nodes8 = nullptr; c->nodes8_count = c->nodes8_depth = 0; bool wide8_on_device = false;
    if (tiny && v.tri_count > 0) {
        // tiny scene (Cornell class): a branch-free sweep over LDS triangle packets beats any tree walk
        c->lds_cfg.brute = 1; c->lds_cfg.nodes_staged = 0; c->lds_cfg.tris_staged = v.tri_count;
        // the SAH leaves (padded boxes, <= 4 triangles each) become the resident plan's candidate filter
        std::vector<LeafBox> leaves;
        auto add_leaf = [&](const float *lo, const float *hi, int32_t child) {
            if (child >= 0 || !(lo[0] <= hi[0])) return;          // inner node, or absent child (inverted box)
            const uint32_t code = (uint32_t) ~child;
            const uint32_t first = code >> 4, count = (code & 15u) + 1u;
            const unsigned long long bits = (count >= 64u ? ~0ull : ((1ull << count) - 1ull)) << first;
            LeafBox b; for (int a = 0; a < 3; ++a) { b.p[2 * a] = lo[a]; b.p[2 * a + 1] = hi[a]; } b.mask_lo = (uint32_t) bits; b.mask_hi = (uint32_t) (bits >> 32);
            leaves.push_back(b);
        };
        for (const BvhNode &n : r.nodes) { add_leaf(n.lo0, n.hi0, n.child0); add_leaf(n.lo1, n.hi1, n.child1); }
        HIP_TRY(c, c->d_leaf_boxes.upload(leaves, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        v.leaf_boxes = c->d_leaf_boxes.p;
        c->lds_cfg.leaves = (quality_flags & MI_BVH_NO_LEAF_FILTER) ? 0u : (uint32_t) leaves.size();
        std::vector<TriBounds> bounds(v.tri_count);               // per packet (leaf order), staged behind the boxes
        for (uint32_t i = 0; i < v.tri_count; ++i)
            bounds[i] = tri_bounds(ld3(r.tris[i].p0), ld3(r.tris[i].p1), ld3(r.tris[i].p2), v.accept_pad);
        HIP_TRY(c, c->d_tri_bounds.upload(bounds, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        v.tri_bounds = c->d_tri_bounds.p;
        c->lds_bytes = v.tri_count * sizeof(TriPacket) + leaves.size() * MIW_LEAF_BOX_COPIES * sizeof(LeafBox) + v.tri_count * sizeof(TriBounds);   // (trace.h: stage_to_lds)
    } else {
        // A whole tree that fits 16 KiB could be walked out of LDS with the stackless trail walk; measured (r02 triangle-count
        // series: 172 triangles, 375 Msamples/s that way against 850 with the LDS-stack walk of the phase machine, whose
        // node fetches hit L1) that only pays for the forced-tree test path of <= 64 triangles, which keeps it covered.
        const bool stack_ok = depth <= MIW_STACK_ENTRIES && !c->opt.get("MIW_NO_STACK");
        const bool resident_tree = all <= 16 * 1024 && (!stack_ok || v.tri_count <= MIW_BRUTE_MAX_TRIS);
        if (resident_tree) { c->lds_cfg.nodes_staged = v.node_count; c->lds_cfg.tris_staged = v.tri_count; }
        else { c->lds_cfg.nodes_staged = MIW_LDS_TOP ? std::min<uint32_t>(v.node_count, 255) : 0u; c->lds_cfg.tris_staged = 0; }
        c->lds_bytes = c->lds_cfg.nodes_staged * sizeof(BvhNode) + c->lds_cfg.tris_staged * sizeof(Tri);
        c->lds_cfg.stack = 0; c->lds_cfg.stack16 = 0;
        if (!resident_tree && stack_ok) {
            c->lds_cfg.stack = 1; c->lds_cfg.stack16 = (uint32_t) (c->lds_bytes / 16);
            c->lds_bytes += (size_t) MIW_STACK_ENTRIES * MIW_BLOCK * sizeof(int32_t);
        }
        // The phase machine (plan 2 over a stack-walked tree) walks the 4-wide quantised collapse of this tree (miw/bvh4.h,
        // bvh4_build.h; +10 % on the material balls and the interior against the BVH2 walk). The BVH2 stays for
        // mi_trace, the scene queries and plan 1; a device-built LBVH is collapsed on the device (bvh4_device.h, above). MIW_BVH4=0 switches it
        // off (A/B runs), MIW_BVH4_FAN = 2..4 caps the fan-out. A tree the collapse refuses (height above the stack budget,
        // coordinates beyond the quantisation range) is rendered by the lock-step kernel.
        if (c->lds_cfg.stack && wide_on && wide_on_device) {
            v.nodes4 = c->d_nodes4.p; c->nodes4_count = dev4_nodes; c->nodes4_stack = dev4_stack;
            if (c->opt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] bvh4 (device): %u nodes (bvh2 %u), stack bound %u, %.2f ms\n", dev4_nodes, node_count, dev4_stack, ms_bvh4);
        } else if (c->lds_cfg.stack && wide_on) {
            auto t4 = std::chrono::steady_clock::now();
            if (built_on_device) {
                r.nodes.resize(node_count);
                HIP_TRY(c, hipMemcpy(r.nodes.data(), c->d_nodes.p, (size_t) node_count * sizeof(BvhNode), hipMemcpyDeviceToHost));
            }
            const Bvh4BuildResult b4 = bvh4_collapse(r.nodes, MIW_STACK_ENTRIES - 1, max_fan);   // one entry of slack: the node body's unconditional stores
            if (b4.ok) {
                HIP_TRY(c, c->d_nodes4.upload(b4.nodes, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                v.nodes4 = c->d_nodes4.p; c->nodes4_count = (uint32_t) b4.nodes.size(); c->nodes4_stack = b4.stack_bound;
            }
            ms_bvh4 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t4).count();
            if (c->opt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] bvh4: %zu nodes (bvh2 %u), depth %u, stack bound %u, ok %d\n", b4.nodes.size(), node_count, b4.depth, b4.stack_bound, (int) b4.ok);
        }
        // The 8-wide tree (miw/bvh8.h; walked instead of the 4-wide one whenever it exists — mi_render, MIW_BVH8=0 at render time keeps
        // the 4-wide walk): collapsed on the device above, or here on the host from the host-built BVH2 (quality 1). c->view keeps
        // the BVH2's triangle order; mi_render hands the phase machine a view whose tris / tri_vn are d_tris8 / d_tri_vn8.
        if (c->lds_cfg.stack && v.nodes4 && dev8_nodes) {
            c->nodes8_count = dev8_nodes; c->nodes8_depth = dev8_depth; wide8_on_device = true;
            if (c->opt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] bvh8 (device): %u nodes (bvh2 %u, bvh4 %u), depth %u, %.2f ms\n", dev8_nodes, node_count, c->nodes4_count, dev8_depth, ms_bvh8);
        } else if (c->lds_cfg.stack && v.nodes4 && wide8_on && !built_on_device) {
            auto t8 = std::chrono::steady_clock::now();
            const Bvh8BuildResult b8 = bvh8_collapse(r.nodes, tri_count);
            if (b8.ok) {
                std::vector<Tri> t8v(b8.perm.size()); std::vector<float> vn8;
                for (size_t i = 0; i < t8v.size(); ++i) t8v[i] = r.tris[b8.perm[i]];
                if (!vn.empty()) { vn8.resize(vn.size()); for (size_t i = 0; i < t8v.size(); ++i) memcpy(&vn8[i * 9], &vn[(size_t) b8.perm[i] * 9], 36); }
                HIP_TRY(c, c->d_nodes8.upload(b8.nodes, c->stream)); HIP_TRY(c, c->d_tris8.upload(t8v, c->stream)); HIP_TRY(c, c->d_tri_vn8.upload(vn8, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                c->nodes8_count = (uint32_t) b8.nodes.size(); c->nodes8_depth = b8.depth;
            }
            ms_bvh8 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t8).count();
            if (c->opt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] bvh8: %zu nodes (bvh2 %u), depth %u, ok %d, %.2f ms\n", b8.nodes.size(), node_count, b8.depth, (int) b8.ok, ms_bvh8);
        }
    }

    // the 8-wide arrays were sized for the worst case (one node per triangle) before the collapse ran: a tree that was refused or is
    // not adopted gives them back, an adopted one keeps the nodes it has (0.9 M triangles: 6.9 MB instead of 73 MB) — ADVICE r05
    if (c->nodes8_count == 0) { c->d_nodes8.release(); c->d_tris8.release(); c->d_tri_vn8.release(); }
    else if (c->d_nodes8.n > 2 * (size_t) c->nodes8_count) {
        DevBuf<Bvh8Node> fit;
        HIP_TRY(c, fit.resize(c->nodes8_count));
        HIP_TRY(c, hipMemcpyAsync(fit.p, c->d_nodes8.p, (size_t) c->nodes8_count * sizeof(Bvh8Node), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->d_nodes8.release(); c->d_nodes8 = fit;
    }

    c->counters.ms_bvh_build = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->counters.bvh_nodes = v.node_count; c->counters.bvh_tris = v.tri_count; c->counters.bvh_depth = depth;
    c->counters.bvh4_on_device = (v.nodes4 && wide_on_device) ? 1u : 0u; c->counters.ms_bvh4 = ms_bvh4;
    c->counters.bvh8_nodes = c->nodes8_count; c->counters.bvh8_depth = c->nodes8_depth; c->counters.bvh8_on_device = wide8_on_device ? 1u : 0u; c->counters.ms_bvh8 = ms_bvh8;
    c->have_bvh = true;
    return MI_OK;
}

// ---- mi_trace --------------------------------------------------------------------------
mi_status mi_trace(mi_ctx *c, const mi_rays_soa *rays, const mi_hits_soa *hits, uint64_t n, int32_t any_hit) {
    if (!c || !rays || !hits) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_trace: call mi_scene_upload and mi_bvh_build first");
    if (n == 0) return MI_OK;
    if (!hits->t) return fail(c, MI_ERR_INVALID, "mi_trace: hits->t is required");
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> in, out; TmpBuf<uint32_t> outu;
    HIP_TRY(c, in.resize(8 * n)); HIP_TRY(c, out.resize(3 * n)); HIP_TRY(c, outu.resize(2 * n));
    const float *src[8] = { rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->mint, rays->maxt };
    for (int k = 0; k < 8; ++k) {
        if (!src[k]) return fail(c, MI_ERR_INVALID, "mi_trace: null ray array");
        HIP_TRY(c, hipMemcpyAsync(in.p + k * n, src[k], n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    SoaRays R = { in.p, in.p + n, in.p + 2 * n, in.p + 3 * n, in.p + 4 * n, in.p + 5 * n, in.p + 6 * n, in.p + 7 * n };
    SoaHits H = { out.p, out.p + n, out.p + 2 * n, outu.p, outu.p + n };
    dim3 grid((unsigned) ((n + MIW_BLOCK - 1) / MIW_BLOCK)), block(MIW_BLOCK);
    if (any_hit) hipLaunchKernelGGL(k_trace_soa<true>, grid, block, c->lds_bytes, c->stream, c->view, R, H, n, c->lds_cfg);
    else         hipLaunchKernelGGL(k_trace_soa<false>, grid, block, c->lds_bytes, c->stream, c->view, R, H, n, c->lds_cfg);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(hits->t, out.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (hits->u) HIP_TRY(c, hipMemcpyAsync(hits->u, out.p + n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (hits->v) HIP_TRY(c, hipMemcpyAsync(hits->v, out.p + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (hits->prim) HIP_TRY(c, hipMemcpyAsync(hits->prim, outu.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (hits->shape) HIP_TRY(c, hipMemcpyAsync(hits->shape, outu.p + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

// ---- the Scene query surface: mi_ray_intersect, mi_sample_emitter_direction, mi_pdf_emitter_direction, mi_emitter_eval ----
// (host arrays in, host arrays out, like mi_trace; temporaries are RAII so that an early HIP_TRY return frees them)
mi_status mi_ray_intersect(mi_ctx *c, const mi_rays_soa *rays, mi_surface_interaction *si, uint64_t n) {
    if (!c || !rays || !si) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_ray_intersect: call mi_scene_upload and mi_bvh_build first");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> in; TmpBuf<mi_surface_interaction> out;
    HIP_TRY(c, in.resize(8 * n)); HIP_TRY(c, out.resize(n));
    const float *src[8] = { rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->mint, rays->maxt };
    for (int k = 0; k < 8; ++k) {
        if (!src[k]) return fail(c, MI_ERR_INVALID, "mi_ray_intersect: null ray array");
        HIP_TRY(c, hipMemcpyAsync(in.p + k * n, src[k], n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    SoaRays R = { in.p, in.p + n, in.p + 2 * n, in.p + 3 * n, in.p + 4 * n, in.p + 5 * n, in.p + 6 * n, in.p + 7 * n };
    hipLaunchKernelGGL(k_ray_intersect, dim3((unsigned) ((n + MIW_BLOCK - 1) / MIW_BLOCK)), dim3(MIW_BLOCK), c->lds_bytes, c->stream, c->view, R, out.p, n, c->lds_cfg);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(si, out.p, n * sizeof(mi_surface_interaction), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

mi_status mi_sample_emitter_direction(mi_ctx *c, int32_t emitter, const float *ref_p, const float *sample, const float *wavelengths,
                                      int32_t test_visibility, mi_direction_sample *ds, float *spec_out, uint64_t n) {
    if (!c || !ref_p || !sample || !ds || !spec_out) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_sample_emitter_direction: call mi_scene_upload and mi_bvh_build first");
    if (emitter >= (int32_t) c->emitters.size()) return fail(c, MI_ERR_INVALID, "mi_sample_emitter_direction: emitter index out of range");
    if (MIW_SPECTRAL && !wavelengths) return fail(c, MI_ERR_INVALID, "mi_sample_emitter_direction: the scalar_spectral library needs wavelengths");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> d_ref, d_smp, d_wl, d_spec; TmpBuf<mi_direction_sample> d_ds;
    HIP_TRY(c, d_ref.resize(3 * n)); HIP_TRY(c, d_smp.resize(2 * n)); HIP_TRY(c, d_spec.resize(MIW_SPEC_N * n)); HIP_TRY(c, d_ds.resize(n));
    HIP_TRY(c, hipMemcpyAsync(d_ref.p, ref_p, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_smp.p, sample, 2 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (MIW_SPECTRAL) {
        HIP_TRY(c, d_wl.resize(4 * n));
        HIP_TRY(c, hipMemcpyAsync(d_wl.p, wavelengths, 4 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_sample_emitter_direction, dim3((unsigned) ((n + MIW_BLOCK - 1) / MIW_BLOCK)), dim3(MIW_BLOCK), c->lds_bytes, c->stream,
                       c->view, emitter, d_ref.p, d_smp.p, d_wl.p, test_visibility, d_ds.p, d_spec.p, n, c->lds_cfg);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(ds, d_ds.p, n * sizeof(mi_direction_sample), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(spec_out, d_spec.p, MIW_SPEC_N * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

mi_status mi_pdf_emitter_direction(mi_ctx *c, int32_t emitter, const float *ref_p, const mi_direction_sample *ds, float *pdf, uint64_t n) {
    if (!c || !ref_p || !ds || !pdf) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_pdf_emitter_direction: call mi_scene_upload and mi_bvh_build first");
    if (emitter >= (int32_t) c->emitters.size()) return fail(c, MI_ERR_INVALID, "mi_pdf_emitter_direction: emitter index out of range");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> d_ref, d_pdf; TmpBuf<mi_direction_sample> d_ds;
    HIP_TRY(c, d_ref.resize(3 * n)); HIP_TRY(c, d_pdf.resize(n)); HIP_TRY(c, d_ds.resize(n));
    HIP_TRY(c, hipMemcpyAsync(d_ref.p, ref_p, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_ds.p, ds, n * sizeof(mi_direction_sample), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pdf_emitter_direction, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, c->stream, c->view, emitter, d_ref.p, d_ds.p, d_pdf.p, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pdf, d_pdf.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

mi_status mi_emitter_eval(mi_ctx *c, const mi_surface_interaction *si, const float *wavelengths, float *spec_out, uint64_t n) {
    if (!c || !si || !spec_out) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_emitter_eval: call mi_scene_upload and mi_bvh_build first");
    if (MIW_SPECTRAL && !wavelengths) return fail(c, MI_ERR_INVALID, "mi_emitter_eval: the scalar_spectral library needs wavelengths");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> d_wl, d_spec; TmpBuf<mi_surface_interaction> d_si;
    HIP_TRY(c, d_spec.resize(MIW_SPEC_N * n)); HIP_TRY(c, d_si.resize(n));
    HIP_TRY(c, hipMemcpyAsync(d_si.p, si, n * sizeof(mi_surface_interaction), hipMemcpyHostToDevice, c->stream));
    if (MIW_SPECTRAL) {
        HIP_TRY(c, d_wl.resize(4 * n));
        HIP_TRY(c, hipMemcpyAsync(d_wl.p, wavelengths, 4 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_emitter_eval, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, c->stream, c->view, d_si.p, d_wl.p, d_spec.p, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(spec_out, d_spec.p, MIW_SPEC_N * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

// ---- render ----------------------------------------------------------------------------
static void direct_constants(DirectRec &D, uint32_t ne, uint32_t nb, bool hide_emitters) {   // direct.cpp:82-103
    D.emitter_samples = ne; D.bsdf_samples = nb; D.hide_emitters = hide_emitters ? 1u : 0u;
    D.weight_bsdf = 1.f / (float) nb; D.weight_lum = 1.f / (float) ne;
    D.frac_bsdf = (float) nb / (float) (ne + nb); D.frac_lum = (float) ne / (float) (ne + nb);
}
static mi_status fill_params(mi_ctx *c, const mi_render_cfg *cfg, RenderParams &P) {
    if (cfg->crop_w <= 0 || cfg->crop_h <= 0 || cfg->crop_x < 0 || cfg->crop_y < 0)
        return fail(c, MI_ERR_INVALID, "render: bad crop window");
    if (cfg->crop_x + cfg->crop_w > 65535 || cfg->crop_y + cfg->crop_h > 65535)
        return fail(c, MI_ERR_INVALID, "render: film larger than 65535 pixels per side");
    if (cfg->block_size <= 0 || (cfg->block_size & (cfg->block_size - 1)))
        return fail(c, MI_ERR_INVALID, "render: block_size must be a power of two");
    if (cfg->integrator == MI_INTEGRATOR_PATH && cfg->rr_depth <= 0) return fail(c, MI_ERR_INVALID, "\"rr_depth\" must be set to a value greater than zero!");
    if (cfg->integrator == MI_INTEGRATOR_PATH && cfg->max_depth < 0 && cfg->max_depth != -1) return fail(c, MI_ERR_INVALID, "\"max_depth\" must be set to -1 (infinite) or a value >= 0");
    if (cfg->filter_radius <= 0.f || cfg->filter_radius > 4.f) return fail(c, MI_ERR_INVALID, "render: filter radius out of range (0, 4]");
    memset(&P, 0, sizeof P);
    memcpy(P.sensor.sample_to_camera, cfg->sample_to_camera, 64);
    memcpy(P.sensor.to_world, cfg->to_world, 64);
    P.sensor.near_clip = cfg->near_clip; P.sensor.far_clip = cfg->far_clip;
    P.sensor.pp_offset[0] = cfg->principal_point_offset[0]; P.sensor.pp_offset[1] = cfg->principal_point_offset[1];
    P.film.crop_w = cfg->crop_w; P.film.crop_h = cfg->crop_h; P.film.crop_x = cfg->crop_x; P.film.crop_y = cfg->crop_y;
    P.film.block_size = cfg->block_size; P.film.border = cfg->filter_border;
    P.film.radius = cfg->filter_radius;
    P.film.scale_factor = (float) MIW_FILTER_RESOLUTION / cfg->filter_radius;
    memcpy(P.film.lut, cfg->filter_lut, sizeof P.film.lut);
    P.film.warn_negative = cfg->moment_pass ? 0u : 1u;           // integrator.cpp:113: !has_aovs
    P.spp = cfg->spp; P.max_depth = cfg->max_depth; P.rr_depth = cfg->rr_depth;
    if (cfg->integrator == MI_INTEGRATOR_DIRECT) {               // direct.cpp:82-103
        const uint32_t ne = cfg->emitter_samples, nb = cfg->bsdf_samples;
        if (ne + nb == 0) return fail(c, MI_ERR_INVALID, "Must have at least 1 BSDF or emitter sample!");
        P.integrator = INTEG_DIRECT;
        direct_constants(P.direct, ne, nb, cfg->hide_emitters != 0);
    } else if (cfg->integrator == MI_INTEGRATOR_VOLPATH)
        return fail(c, MI_ERR_INVALID, "render: volpath renders through mi_render_sensor");
    else if (cfg->integrator != MI_INTEGRATOR_PATH)
        return fail(c, MI_ERR_INVALID, "render: unknown integrator %d", cfg->integrator);
    if (cfg->moment_pass < MI_MOMENT_OFF || cfg->moment_pass > MI_MOMENT_SQUARES) return fail(c, MI_ERR_INVALID, "render: moment_pass must be 0, 1 or 2");
#if MIW_SPECTRAL
    if (cfg->moment_pass) return fail(c, MI_ERR_INVALID, "render: the moment integrator is provided by the scalar_rgb library only");
#endif
    P.moment_pass = (uint32_t) cfg->moment_pass;
    render_params_prepare(P);
    return MI_OK;
}

// ---- which instantiation of the path kernels a scene gets ----------------------------------------------------------------------
// kernel_pick.h holds the RULES (scene facts -> tiny, material class, analytic); the lists here hold every tuple that EXISTS as an instantiation,
// once per kernel template. A launch matches its pick against its list (MIW_PICKED) and a pick outside the list is MI_ERR_STATE; nothing else
// names these kernels with literal class arguments, but the special cases in front of the tables in mi_render (the overlap's Groups = true pair,
// the four-wavefront shard kernel, the MATS_TRIO phase machine over the BVH2). A new class = a line in a rule + its tuples here (+ its
// part lists in device/class_instances.h when it is compiled beside the library).
static_assert(miw_pick::ALL == MATS_ALL && miw_pick::DIFFUSE == MATS_DIFFUSE && miw_pick::PLAIN == MATS_PLAIN && miw_pick::TRIO == MATS_TRIO &&
              miw_pick::NESTED == MATS_NESTED && miw_pick::LIGHTS == MATS_LIGHTS, "kernel_pick.h names the classes by miw/path.h's values");
// X(Tiny, Mats, Analytic, Integ): the sample-log film's k_path_resident<true, ...> (MIW_RESIDENT_LIST) and k_sample_rays (MIW_SAMPLE_LIST)
#define MIW_PATH_TUPLES(X)                                                                                                              \
    X(2, MATS_DIFFUSE, false, INTEG_PATH) X(1, MATS_DIFFUSE, false, INTEG_PATH)   /* 32-bit candidate masks up to 32 triangles (BASELINE config 2), else 64-bit */ \
    X(1, MATS_LIGHTS, false, INTEG_PATH) X(0, MATS_LIGHTS, true, INTEG_PATH) X(1, MATS_NESTED, false, INTEG_PATH) X(0, MATS_NESTED, true, INTEG_PATH) \
    X(1, MATS_ALL, false, INTEG_PATH) X(0, MATS_ALL, true, INTEG_PATH)                                                                  \
    X(2, MATS_PLAIN, false, INTEG_PATH) X(1, MATS_PLAIN, false, INTEG_PATH) X(0, MATS_PLAIN, false, INTEG_PATH) X(0, MATS_PLAIN, true, INTEG_PATH)
#define MIW_DIRECT_TUPLES(X)                                                                                                            \
    X(1, MATS_LIGHTS, false, INTEG_DIRECT) X(0, MATS_LIGHTS, true, INTEG_DIRECT) X(1, MATS_NESTED, false, INTEG_DIRECT) X(0, MATS_NESTED, true, INTEG_DIRECT) \
    X(1, MATS_ALL, false, INTEG_DIRECT) X(0, MATS_ALL, true, INTEG_DIRECT) X(1, MATS_PLAIN, false, INTEG_DIRECT) X(0, MATS_PLAIN, true, INTEG_DIRECT)
#define MIW_RESIDENT_LIST(X) MIW_PATH_TUPLES(X) MIW_DIRECT_TUPLES(X)
#define MIW_SAMPLE_LIST(X) MIW_PATH_TUPLES(X) X(0, MATS_TRIO, false, INTEG_PATH) MIW_DIRECT_TUPLES(X)
// ... and the float64-atomics film's k_path_resident<false, ...> (launched, and given its LDS attribute, from this list)
#define MIW_ATOMIC_LIST(X)                                                                                                              \
    X(1, MATS_LIGHTS, false, INTEG_PATH) X(0, MATS_LIGHTS, true, INTEG_PATH) X(1, MATS_NESTED, false, INTEG_PATH) X(0, MATS_NESTED, true, INTEG_PATH) \
    X(1, MATS_ALL, false, INTEG_PATH) X(0, MATS_ALL, true, INTEG_PATH)                                                                  \
    X(1, MATS_LIGHTS, false, INTEG_DIRECT) X(0, MATS_LIGHTS, true, INTEG_DIRECT) X(1, MATS_NESTED, false, INTEG_DIRECT) X(0, MATS_NESTED, true, INTEG_DIRECT) \
    X(1, MATS_ALL, false, INTEG_DIRECT) X(0, MATS_ALL, true, INTEG_DIRECT)
// X(Mats, Analytic, Waves, Wide, Placed): k_path_phased — the six tree classes, each over the 8-wide and the 4-wide tree at four wavefronts per
// SIMD, placed or not, and over the 4-wide tree at three
#define MIW_TREE_CLASSES(X, ...) X(MATS_LIGHTS, true, __VA_ARGS__) X(MATS_NESTED, true, __VA_ARGS__) X(MATS_ALL, true, __VA_ARGS__) \
    X(MATS_TRIO, false, __VA_ARGS__) X(MATS_PLAIN, false, __VA_ARGS__) X(MATS_PLAIN, true, __VA_ARGS__)
#define MIW_PHASED_LIST(X) MIW_TREE_CLASSES(X, 4, 2, true) MIW_TREE_CLASSES(X, 4, 2, false) MIW_TREE_CLASSES(X, 4, 1, true) MIW_TREE_CLASSES(X, 4, 1, false) MIW_TREE_CLASSES(X, 3, 1, false)
// X(Mats, Analytic, NW, PP): k_path_pooled (the 8 x 2 shape is instantiated for the MATS_TRIO class only — BASELINE configs 3 / 4)
#define MIW_POOLED_LIST(X) X(MATS_ALL, true, 12, 1) X(MATS_TRIO, false, 12, 1) X(MATS_TRIO, false, 8, 2) X(MATS_PLAIN, false, 12, 1) X(MATS_PLAIN, true, 12, 1)
// X(Tiny, Mats): the packet path kernels with the sample log that have a LEAN twin, k_path_resident<true, Tiny, Mats, false, INTEG_PATH, false, 0, FEAT_NONE> (miw/scene.h: FEAT_*;
// kernel_pick.h: packet_features, packet_lean_class) — and the four-wavefront shard form of the first, named where it is launched. Two masks per kernel, all and none:
// a scene with any of the four features runs the full kernel, which is correct for every scene. Each of the four also has a FRAME twin, k_path_resident<..., FEAT_FRAME>
// (resident_kernel.h; kernel_pick.h: frame_twin): the lean twin with the facts of a full frame's launch compiled in.
#define MIW_LEAN_LIST(X) X(2, MATS_DIFFUSE) X(1, MATS_DIFFUSE) X(2, MATS_PLAIN) X(1, MATS_PLAIN)
#define MIW_PICKED(T, M, A) (pick.tiny == (T) && pick.mats == (M) && pick.analytic == (A))
// MIW_DEBUG: every launch of a path kernel says on stderr which instantiation it is, "[miwave] kernel launched: NAME<ARG, ARG, ...>" with the template arguments as
// the launch site spells them. The text is the launch macro's own arguments, stringified beside the launch: it cannot name another kernel than
// the one launched. tests/test_instantiation_census_gpu.py reads these lines; tests/instantiation_cases.py is keyed by them.
// MIW_LAUNCH_NAMED launches `kernel_` — the template-id in parentheses, as hipLaunchKernelGGL takes it — and prints that very text (without the parentheses).
#define MIW_SAY_KERNEL_TEXT(opt_, text_) do { if ((opt_).get("MIW_DEBUG")) fprintf(stderr, "[miwave] kernel launched: %s\n", text_); } while (0)
#define MIW_LAUNCH_NAMED(opt_, kernel_, ...) do { if ((opt_).get("MIW_DEBUG")) fprintf(stderr, "[miwave] kernel launched: %.*s\n", (int) sizeof(#kernel_) - 3, #kernel_ + 1); \
    hipLaunchKernelGGL(kernel_, __VA_ARGS__); } while (0)

// the scene facts the rules read, from the context and the options of this call
static miw_pick::Facts pick_facts(const mi_ctx *c, const Options &opt) {
    miw_pick::Facts f;
    f.tiny = c->lds_cfg.brute != 0; f.small = c->view.tri_count <= 32u;
    f.diffuse_only = c->diffuse_only; f.trio = c->trio; f.nested = c->nested; f.textured = c->textured; f.lights_on = c->lights_on;
    f.no_rects = c->rects.empty(); f.trio_on = !opt.off("MIW_TRIO");
    return f;
}
// the 8-wide tree is there and not switched off (MIW_BVH8=0 keeps the 4-wide walk: A/B runs in one process)
static bool tree8_on(const mi_ctx *c, const Options &opt) { return c->view.nodes4 != nullptr && c->nodes8_count != 0u && !opt.off("MIW_BVH8"); }

// ---- mi_sample: SamplingIntegrator::sample for caller-supplied rays (device/sample_kernel.h) ------------------------------
// Rays per launch. Host-pointer calls stage one chunk at a time in a buffer the context keeps (88 + 4 N bytes per ray: 200 MB),
// so n is bounded by the caller's memory only; device-pointer calls are cut as well, so that mi_cancel is looked at in between
// (and the queue's 32-bit counter never wraps).
#define MIW_SAMPLE_CHUNK_HOST (1u << 21)
#define MIW_SAMPLE_CHUNK_DEVICE (1u << 26)
#if !MIW_SPECTRAL
static MediaView media_view(const mi_ctx *c) {
    MediaView mv;
    mv.media = c->media.empty() ? nullptr : c->d_media.p; mv.media_count = (uint32_t) c->media.size();
    mv.shape_media = c->shape_media.empty() ? nullptr : c->d_shape_media.p; mv.start_medium = c->start_medium;
    return mv;
}
// MI_INTEGRATOR_VOLPATH: k_sample_volpath (device/volpath_kernel.h) of the MATS_NESTED class, which holds every BSDF plugin; packets or
// the tree as the scene was built. Scenes of the two routes no float64 tier pins yet are refused by name.
static mi_status volpath_sample_launch(mi_ctx *c, const RenderParams &P, const SampleIO &io, hipStream_t s) {
    if (c->lights_on) return fail(c, MI_ERR_INVALID, "volpath: scenes with point / spot / directional / constant emitters are not served yet");
    if (!c->rects.empty()) return fail(c, MI_ERR_INVALID, "volpath: scenes with analytic shapes (rectangle, sphere) are not served yet");
    const bool tiny = c->lds_cfg.brute != 0;
    const dim3 grid(std::min<unsigned>((io.n + MIW_BLOCK - 1u) / MIW_BLOCK, (unsigned) c->cu_count * volpath_waves(tiny ? 1 : 0)));
    HIP_TRY(c, hipMemsetAsync(c->d_next_ray.p, 0, sizeof(uint32_t), s));
    const MediaView mv = media_view(c);
    const int mats = MATS_NESTED;
    const hipError_t e = volpath_launch(s, c->opt.get("MIW_DEBUG") != nullptr, tiny ? 1 : 0, mats, false, grid, c->lds_bytes, P, c->view, mv, io, c->lds_cfg,
                                        c->d_next_ray.p, c->d_volpath_capped.p);
    if (e == hipErrorInvalidValue) return fail(c, MI_ERR_STATE, "mi_sample: no k_sample_volpath<%d, %d, 0> in the library", tiny ? 1 : 0, mats);
    HIP_TRY(c, e);
    return MI_OK;
}
// the counter of rays ended by MIW_VOLPATH_MAX_TRIPS: cleared before the launches of a call, read into mi_counters after them
static mi_status volpath_capped_reset(mi_ctx *c, hipStream_t s) {
    HIP_TRY(c, c->d_volpath_capped.resize(1));
    HIP_TRY(c, hipMemsetAsync(c->d_volpath_capped.p, 0, sizeof(uint32_t), s));
    c->volpath_capped = 0;
    return MI_OK;
}
static mi_status volpath_capped_read(mi_ctx *c, hipStream_t s) {
    uint32_t n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, c->d_volpath_capped.p, sizeof n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->volpath_capped = n;
    return MI_OK;
}
#endif
static mi_status sample_launch(mi_ctx *c, const RenderParams &P, const SampleIO &io, hipStream_t s) {
#if !MIW_SPECTRAL
    if (P.integrator == INTEG_VOLPATH) return volpath_sample_launch(c, P, io, s);
#endif
    const bool tiny = c->lds_cfg.brute != 0, direct = P.integrator == INTEG_DIRECT;
    // persistent grid: as many workgroups per CU as the kernel is compiled for wavefronts per SIMD (sample_kernel.h), never more than the rays need
    const unsigned waves = direct ? (unsigned) MIW_DIRECT_WAVES : tiny ? 4u : (unsigned) MIW_TREE_WAVES;
    const dim3 grid(std::min<unsigned>((io.n + MIW_BLOCK - 1u) / MIW_BLOCK, (unsigned) c->cu_count * waves)), block(MIW_BLOCK);
    HIP_TRY(c, hipMemsetAsync(c->d_next_ray.p, 0, sizeof(uint32_t), s));
    // the instantiation mi_render picks for this scene (the same rule: no BSDF dispatch when every shape is plain diffuse, no texture lookups
    // without texture coordinates, no analytic shapes where there are none), plus the MATS_TRIO tree kernel mi_render leaves to its phase machine
    const miw_pick::Facts facts = pick_facts(c, c->opt);
    const miw_pick::Pick pick = direct ? miw_pick::resident_direct(facts) : miw_pick::resident_path(facts, true);
    const uint32_t integ = direct ? INTEG_DIRECT : INTEG_PATH;
#define MIW_SAMPLE_LAUNCH(T, M, A, I) if (integ == (I) && MIW_PICKED(T, M, A)) MIW_LAUNCH_NAMED(c->opt, (k_sample_rays<T, M, A, I>), grid, block, c->lds_bytes, s, P, c->view, io, c->lds_cfg, c->d_next_ray.p); else
    MIW_SAMPLE_LIST(MIW_SAMPLE_LAUNCH) return fail(c, MI_ERR_STATE, "mi_sample: no k_sample_rays<%d, %d, %d, %u> in the library", pick.tiny, pick.mats, (int) pick.analytic, integ);
#undef MIW_SAMPLE_LAUNCH
    HIP_TRY(c, hipGetLastError());
    return MI_OK;
}

static std::string sample_cfg_problem(const mi_sample_cfg *cfg) {
    char buf[160];
    if (cfg->struct_size != sizeof(mi_sample_cfg)) {
        snprintf(buf, sizeof buf, "mi_sample: unknown mi_sample_cfg::struct_size %u (this library: %zu)", cfg->struct_size, sizeof(mi_sample_cfg));
        return buf;
    }
    if (cfg->integrator == MI_INTEGRATOR_PATH) {
        if (cfg->rr_depth <= 0) return "\"rr_depth\" must be set to a value greater than zero!";
        if (cfg->max_depth < -1) return "\"max_depth\" must be set to -1 (infinite) or a value >= 0";
    } else if (cfg->integrator == MI_INTEGRATOR_DIRECT) {
        if (cfg->emitter_samples + cfg->bsdf_samples == 0) return "Must have at least 1 BSDF or emitter sample!";
    } else if (cfg->integrator == MI_INTEGRATOR_VOLPATH) {
#if MIW_SPECTRAL
        return "volpath is served by the scalar_rgb library";
#else
        if (cfg->rr_depth <= 0) return "\"rr_depth\" must be set to a value greater than zero!";
        if (cfg->max_depth < -1) return "\"max_depth\" must be set to -1 (infinite) or a value >= 0";
#endif
    } else {
        snprintf(buf, sizeof buf, "mi_sample: unknown integrator %d (served: MI_INTEGRATOR_PATH, MI_INTEGRATOR_DIRECT, MI_INTEGRATOR_VOLPATH)", cfg->integrator);
        return buf;
    }
    return std::string();
}

mi_status mi_sample(mi_ctx *c, const mi_sample_cfg *cfg, const mi_rays_soa *rays, const float *wavelengths,
                    uint64_t *rng_state, const uint64_t *rng_inc, float *spec_out, uint8_t *valid, uint64_t n) {
    if (!cfg) return MI_ERR_INVALID;
    {   // the job description first: a caller compiled against another header must hear so whatever else is wrong (no context needed)
        const std::string why = sample_cfg_problem(cfg);
        if (!why.empty()) { if (c) c->error = why; else g_global_error = why; return MI_ERR_INVALID; }
    }
    if (!c) return MI_ERR_INVALID;
    if (!rays || !rng_state || !spec_out || !valid) return fail(c, MI_ERR_INVALID, "mi_sample: null rays / rng_state / spec / valid");
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_sample: call mi_scene_upload and mi_bvh_build first");
    RenderParams P;
    memset(&P, 0, sizeof P);
    P.spp = 1u; P.max_depth = cfg->max_depth; P.rr_depth = cfg->rr_depth;
    if (cfg->integrator == MI_INTEGRATOR_DIRECT) {
        P.integrator = INTEG_DIRECT;
        direct_constants(P.direct, cfg->emitter_samples, cfg->bsdf_samples, cfg->hide_emitters != 0);
    }
    const bool volpath = cfg->integrator == MI_INTEGRATOR_VOLPATH;
    if (volpath) { P.integrator = INTEG_VOLPATH; P.direct.hide_emitters = cfg->hide_emitters != 0 ? 1u : 0u; }
    if (MIW_SPECTRAL && !wavelengths) return fail(c, MI_ERR_INVALID, "mi_sample: the scalar_spectral library needs wavelengths");
    const float *src[8] = { rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->mint, rays->maxt };
    for (int k = 0; k < 8; ++k) if (!src[k]) return fail(c, MI_ERR_INVALID, "mi_sample: null ray array");
    if (n == 0) return MI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->cancel.store(0);
    HIP_TRY(c, c->d_next_ray.resize(1));
#if !MIW_SPECTRAL
    if (volpath) MI_TRY(volpath_capped_reset(c, s));
#endif
    const bool dev = cfg->on_device != 0;
    const uint64_t chunk = dev ? MIW_SAMPLE_CHUNK_DEVICE : MIW_SAMPLE_CHUNK_HOST;
    // staged chunk of a host-pointer call: [8 ray arrays][wavelengths][rng state][rng inc][spec][valid], every array 16-byte aligned
    const uint64_t m_max = std::min<uint64_t>(n, chunk), m_pad = (m_max + 15u) & ~(uint64_t) 15u;
    const size_t off_wl = 8 * m_pad * 4, off_st = off_wl + (MIW_SPECTRAL ? 4 * m_pad * 4 : 0), off_inc = off_st + m_pad * 8,
                 off_spec = off_inc + m_pad * 8, off_valid = off_spec + MIW_SPEC_N * m_pad * 4, stage_bytes = off_valid + m_pad;
    if (!dev) HIP_TRY(c, c->d_sample_stage.resize(stage_bytes));
    for (uint64_t done = 0; done < n; done += chunk) {
        if (c->cancel.load()) return fail(c, MI_ERR_CANCELLED, "mi_sample: cancelled after %llu of %llu rays", (unsigned long long) done, (unsigned long long) n);
        const uint64_t m = std::min<uint64_t>(chunk, n - done);
        SampleIO io;
        io.n = (uint32_t) m;
        if (dev) {
            io.R = { src[0] + done, src[1] + done, src[2] + done, src[3] + done, src[4] + done, src[5] + done, src[6] + done, src[7] + done };
            io.wavelengths = wavelengths ? wavelengths + 4 * done : nullptr;
            io.rng_state = rng_state + done; io.rng_inc = rng_inc ? rng_inc + done : nullptr;
            io.spec = spec_out + MIW_SPEC_N * done; io.valid = valid + done;
        } else {
            unsigned char *b = c->d_sample_stage.p;
            float *f = reinterpret_cast<float *>(b);
            for (int k = 0; k < 8; ++k) HIP_TRY(c, hipMemcpyAsync(f + k * m_pad, src[k] + done, m * sizeof(float), hipMemcpyHostToDevice, s));
            io.R = { f, f + m_pad, f + 2 * m_pad, f + 3 * m_pad, f + 4 * m_pad, f + 5 * m_pad, f + 6 * m_pad, f + 7 * m_pad };
            io.wavelengths = nullptr;
            if (MIW_SPECTRAL) {
                HIP_TRY(c, hipMemcpyAsync(b + off_wl, wavelengths + 4 * done, 4 * m * sizeof(float), hipMemcpyHostToDevice, s));
                io.wavelengths = reinterpret_cast<const float *>(b + off_wl);
            }
            HIP_TRY(c, hipMemcpyAsync(b + off_st, rng_state + done, m * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            io.rng_state = reinterpret_cast<uint64_t *>(b + off_st);
            io.rng_inc = nullptr;
            if (rng_inc) {
                HIP_TRY(c, hipMemcpyAsync(b + off_inc, rng_inc + done, m * sizeof(uint64_t), hipMemcpyHostToDevice, s));
                io.rng_inc = reinterpret_cast<const uint64_t *>(b + off_inc);
            }
            io.spec = reinterpret_cast<float *>(b + off_spec); io.valid = b + off_valid;
        }
        const mi_status ls = sample_launch(c, P, io, s);
        if (ls != MI_OK) return ls;
        if (!dev) {
            HIP_TRY(c, hipMemcpyAsync(rng_state + done, io.rng_state, m * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(spec_out + MIW_SPEC_N * done, io.spec, MIW_SPEC_N * m * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(valid + done, io.valid, m, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(c, hipStreamSynchronize(s));
    }
#if !MIW_SPECTRAL
    if (volpath) MI_TRY(volpath_capped_read(c, s));
#endif
    return MI_OK;
}

// ---- per-launch timing of one mi_render: HIP events from the context's pool around every launch, summed per launch class into mi_counters ----
struct LaunchTimer {
    struct Stamp { int cls; size_t e0, e1; };
    mi_ctx *c; mi_counters &K; bool on;
    std::vector<Stamp> stamps; size_t ev_used = 0;
    hipError_t get_event(size_t &idx) {
        if (ev_used == c->ev_pool.size()) {
            hipEvent_t e; hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
            c->ev_pool.push_back(e);
        }
        idx = ev_used++;
        return hipSuccess;
    }
    void drain() {
        if (!on) return;
        for (const Stamp &t : stamps) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev_pool[t.e0], c->ev_pool[t.e1]) != hipSuccess) continue;
            switch (t.cls) {
                case 0: K.ms_trace_closest += ms; break;
                case 1: K.ms_trace_any += ms; break;
                case 2: K.ms_shade += ms; break;
                case 3: K.ms_init += ms; break;
                case 6: K.ms_path += ms; break;
                case 4: K.ms_film_blocks += ms; K.ms_resolve += ms; break;
                case 5: K.ms_film_merge += ms; K.ms_resolve += ms; break;
                default: K.ms_resolve += ms; break;
            }
        }
        stamps.clear(); ev_used = 0;
    }
};
// a launch on the stream `s` between two events of the timer `T` (both, and the context `c`, by those names where the macro is used)
#define MIW_TIMED(cls_, launch) do {                                                   \
        size_t e0_ = 0, e1_ = 0;                                                       \
        if (T.on) { HIP_TRY(c, T.get_event(e0_)); HIP_TRY(c, hipEventRecord(c->ev_pool[e0_], s)); } \
        launch;                                                                        \
        if (T.on) { HIP_TRY(c, T.get_event(e1_)); HIP_TRY(c, hipEventRecord(c->ev_pool[e1_], s)); \
                    T.stamps.push_back({ cls_, e0_, e1_ }); }                          \
    } while (0)

// ---- mi_render, phase "film plan": how ImageBlock::put is realised for this job (mi_render_cfg::film_mode), the sample log's record
// format (16-byte class records where film_classes.h covers the filter, 24-byte positions otherwise), its layout ([lane][sample], or interleaved
// over groups of 64 tiles for k_film_lanes) and its allocation ----
struct FilmPlan { int film_mode = 0; bool rec16 = false; int film_lanes = 0; bool film_chains = false; /* the replay outside the overlap route: k_film_chains */ uint32_t log_il = 0; size_t log_entries = 0, rec_bytes = 0; };
// ---- mi_render, what every phase reads: the job, this render's options and parameters, the frame's geometry (frame_geometry), the execution plan,
// the film plan, the lane queues as the kernels get them, the launch timer and the counters ----
struct RenderFrame {
    mi_ctx *c; const mi_render_cfg *cfg;
    Options ropt;                                                 // the context's options under the job's debug overrides (render_options)
    RenderParams P; hipStream_t s = nullptr;
    uint32_t bs = 0, bs2 = 0, bs2_log2 = 0, blocks_x = 0, blocks_y = 0, n_tiles = 0, n_lanes = 0; size_t film_n = 0;
    int plan = 0;                                                 // 1: wavefront (queue) plan, 2: resident plan
    FilmPlan FP; LaneQueues Q;
    LaunchTimer T;                                                // HIP-event time per launch class (mi_counters::ms_*)
    mi_counters &K;
    std::chrono::steady_clock::time_point wall0;
    RenderFrame(mi_ctx *c_, const mi_render_cfg *cfg_) : c(c_), cfg(cfg_), ropt(c_->opt), T{ c_, c_->counters, cfg_->profile != 0 }, K(c_->counters) {}
};
static mi_status plan_film_log(RenderFrame &F) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s;
    const uint32_t n_tiles = F.n_tiles, n_lanes = F.n_lanes, bs2 = F.bs2, bs2_log2 = F.bs2_log2; const size_t film_n = F.film_n; FilmPlan &FP = F.FP;
    // film mode: sample log + ordered gather if the log fits, else float64 atomics
    int film_mode = cfg->film_mode;
    const size_t nl = std::max<uint32_t>(n_lanes, 1);
    if (film_mode < 0 || film_mode > 2) return fail(c, MI_ERR_INVALID, "render: film_mode must be 0, 1 or 2");
    const size_t log_lanes_entries = (size_t) nl * std::max<uint32_t>(cfg->spp, 1);
    // The log format: 16-byte records with phase classes where the host enumeration covers the filter (film_classes.h: box, tent,
    // gaussian, mitchell, catmullrom), positions + values (24 bytes) otherwise. MIW_FILM_LEGACY=1 forces the latter (A/B runs).
    bool rec16 = false;
    if (film_mode != 2 && bs2 <= 65536u && !ropt.get("MIW_FILM_LEGACY")) {
        // the cache key: the filter's fields only, in a zero-filled record (padding bytes of a stack copy would make memcmp miss)
        FilmRec key; memset(&key, 0, sizeof key);
        key.border = P.film.border; key.radius = P.film.radius; key.scale_factor = P.film.scale_factor; memcpy(key.lut, P.film.lut, sizeof key.lut);
        // (a filter the enumeration refuses is remembered as well — classes_valid — instead of being enumerated again by every render)
        if (!c->classes_valid || memcmp(&key, &c->classes_of, sizeof key) != 0 || (c->classes.ok && !c->d_fc_thr.p)) {
            c->classes = film_classes_build(P.film);             // ~30 ms, once per filter
            c->classes_of = key; c->classes_valid = true;
            if (c->classes.ok) { HIP_TRY(c, c->d_fc_thr.upload(c->classes.thr, s)); HIP_TRY(c, c->d_fc_w.upload(c->classes.w, s)); HIP_TRY(c, hipStreamSynchronize(s)); }
        }
        rec16 = c->classes.ok;
    }
    // The replay kernel for the 16-byte records (device/film_kernels.h): k_film_lanes — one 4 x 4 texel block per lane, a wavefront = one
    // block position in 64 consecutive tiles — wants those tiles' logs interleaved record by record (path.h: log_index), so the
    // choice is made before the render kernels write the log. MIW_FILM_LANES = 0, or naming another kernel's shape
    // (MIW_FILM_QUADS / _COLUMNS / _GROUP), keeps [lane][sample] and the group kernels; MIW_FILM_LANES = 2: k_film_lanes over [lane][sample].
    // k_film_lanes' wavefronts are few and long (81 per 64 tiles, each the serial replay of 64 pixel runs: ~6 ms at 512 spp however few
    // there are), so shards of fewer than 7 x 64 tiles keep the group kernel: 255 tiles (a rank's eighth of a 1080p frame) 4.1 ms by
    // k_film_quads against 6.1, 510 tiles 7.1 against 6.65, 1 020 tiles 12.9 against 10.2 (gpurun q10)
    int film_lanes = rec16 && c->classes.reach <= 2 && n_tiles >= 448u && !ropt.get("MIW_FILM_COLUMNS") && !ropt.get("MIW_FILM_GROUP") && !ropt.get("MIW_FILM_QUADS") ? 1 : 0;
    if (const char *e = ropt.get("MIW_FILM_LANES")) film_lanes = rec16 && c->classes.reach <= 2 ? atoi(e) : 0;
    const uint32_t log_il = film_lanes == 1 ? bs2_log2 + 1u : 0u;
    const size_t log_entries = log_il ? log_capacity(log_il, n_tiles, bs2, std::max<uint32_t>(cfg->spp, 1)) : log_lanes_entries;
    const size_t rec_bytes = rec16 ? sizeof(U4) : sizeof(F2) + sizeof(F4);
    if (film_mode != 2) {
        size_t need = log_entries * rec_bytes;
        size_t have = c->q_log_pos.n * sizeof(F2) + c->q_log_val.n * sizeof(F4) + c->q_log_rec.n * sizeof(U4), free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        bool fits = need <= (size_t) ((double) (free_b + have) * 0.8);
        if (!fits) {
            if (film_mode == 1) return fail(c, MI_ERR_INVALID, "render: sample log needs %zu MiB, only %zu MiB free", need >> 20, free_b >> 20);
            film_mode = 2; rec16 = false;
        } else film_mode = 1;
    }
    if (film_mode == 1) {
        if (rec16) {
            if (c->q_log_rec.n < log_entries) { c->q_log_rec.release(); c->q_log_pos.release(); c->q_log_val.release(); }
            HIP_TRY(c, c->q_log_rec.resize(log_entries));
        } else {
            if (c->q_log_pos.n < log_entries) { c->q_log_pos.release(); c->q_log_val.release(); c->q_log_rec.release(); }
            HIP_TRY(c, c->q_log_pos.resize(log_entries)); HIP_TRY(c, c->q_log_val.resize(log_entries));
        }
    } else {
        HIP_TRY(c, c->d_accum.resize(film_n));
        HIP_TRY(c, hipMemsetAsync(c->d_accum.p, 0, film_n * sizeof(double), s));
    }
#if defined(MIW_DEBUG_POISON)
    // Debug tier (-DMIW_DEBUG_POISON=1 builds; the reference poisons its GPU interactions in debug builds the same way,
    // src/librender/scene_optix.inl:475-480): every buffer a render kernel is supposed to WRITE before anything reads it starts as
    // NaN bit patterns (0xff bytes) — the sample log, plan 1's queues, the block tiles — and mi_render fails when a NaN reaches the film.
    // A slot that is read without having been written (an indexing error, a lane that skipped its log write) then shows up as
    // MI_ERR_STATE instead of as a plausible-looking stale value from the previous frame.
    {
        auto poison = [&](void *p, size_t bytes) -> hipError_t { return p && bytes ? hipMemsetAsync(p, 0xff, bytes, s) : hipSuccess; };
        HIP_TRY(c, poison(c->q_log_rec.p, c->q_log_rec.n * sizeof(U4))); HIP_TRY(c, poison(c->q_log_pos.p, c->q_log_pos.n * sizeof(F2))); HIP_TRY(c, poison(c->q_log_val.p, c->q_log_val.n * sizeof(F4)));
        if (F.plan == 1) for (DevBuf<F4> *q : { &c->q_tp, &c->q_res, &c->q_ray_o, &c->q_ray_d, &c->q_hit, &c->q_sh_d, &c->q_sh_c }) HIP_TRY(c, poison(q->p, q->n * sizeof(F4)));
        HIP_TRY(c, poison(c->d_tiles.p, c->d_tiles.n * sizeof(float)));
    }
#endif
    c->counters.log_bytes = film_mode == 1 ? (uint64_t) log_entries * rec_bytes : 0u;
    c->counters.log_record_bytes = film_mode == 1 ? (uint32_t) rec_bytes : 0u;
    c->counters.film_kernel = 0u; c->counters.log_interleaved = film_mode == 1 && rec16 && log_il ? 1u : 0u;
    c->counters.film_mode = (uint32_t) film_mode;
    FP.film_mode = film_mode; FP.rec16 = rec16; FP.film_lanes = film_lanes; FP.film_chains = film_lanes == 1 && log_il != 0u && !ropt.off("MIW_FILM_CHAINS") && ropt.num("MIW_FL_NT", 1) != 0; FP.log_il = log_il; FP.log_entries = log_entries; FP.rec_bytes = rec_bytes;
    return MI_OK;
}

// ---- mi_render, debug builds: what the instrumented kernels counted (printed when the option MIW_DEBUG is set) ----
static void print_debug_statistics(mi_ctx *c, const Options &ropt, mi_counters &K) {
    (void) c; (void) ropt; (void) K;
#if defined(MIW_VERIFY_FILTER)
        {
            unsigned int n = 0; float buf[256];
            (void) hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_verify_n), sizeof n);
            (void) hipMemcpyFromSymbol(buf, HIP_SYMBOL(g_verify), sizeof buf);
            fprintf(stderr, "[miwave] filter verification: %u mismatching queries\n", n);
            for (unsigned i = 0; i < n && i < 16; ++i) {
                const float *r = buf + i * 16; uint32_t a, b; memcpy(&a, r + 9, 4); memcpy(&b, r + 10, 4);
                fprintf(stderr, "  kind %g o=(%.9g %.9g %.9g) mint=%.9g d=(%.9g %.9g %.9g) maxt=%.9g brute=%u filter=%u t_brute=%.9g t_filter=%.9g\n",
                        r[8], r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], a, b, r[11], r[12]);
            }
            n = 0; (void) hipMemcpyToSymbol(HIP_SYMBOL(g_verify_n), &n, sizeof n);
        }
#endif
#if defined(MIW_PHASE_STATS)
        if (ropt.get("MIW_DEBUG")) {
            unsigned long long ps[15];
            if (!K.pooled && hipMemcpyFromSymbol(ps, HIP_SYMBOL(g_phase_stats), sizeof ps) == hipSuccess) {
                static const char *names[5] = { "node step", "triangle test", "walk end", "shade", "vote" };
                unsigned long long tot = 0;
                for (int k = 0; k < 5; ++k) tot += ps[10 + k];
                for (int k = 0; k < 5; ++k)
                    fprintf(stderr, "[miwave] phase %-13s runs/segment %7.2f  lanes/run %5.1f  cycles/run %7.0f  share of wave cycles %5.1f %%\n", names[k],
                            64.0 * (double) ps[k] / std::max<double>((double) K.segments, 1), (double) ps[5 + k] / std::max<double>((double) ps[k], 1),
                            (double) ps[10 + k] / std::max<double>((double) ps[k], 1), 100.0 * (double) ps[10 + k] / std::max<double>((double) tot, 1));
                memset(ps, 0, sizeof ps);
                (void) hipMemcpyToSymbol(HIP_SYMBOL(g_phase_stats), ps, sizeof ps);
            }
        }
#endif
#if defined(MIW_PHASE_STATS) && !MIW_SPECTRAL
        if (ropt.get("MIW_DEBUG") && K.pooled) {
            unsigned long long ps[32];
            if (hipMemcpyFromSymbol(ps, HIP_SYMBOL(g_pool_stats), sizeof ps) == hipSuccess) {
                static const char *names[5] = { "vote", "node trip", "triangle trip", "shade", "idle" };
                unsigned long long tot = 0;
                for (int k = 0; k < 5; ++k) tot += ps[10 + k];
                for (int k = 0; k < 5; ++k)
                    fprintf(stderr, "[miwave] pooled %-13s runs per 64 segments %7.2f  lanes/run %5.1f  cycles/run %7.0f  share of wave cycles %5.1f %%\n", names[k],
                            64.0 * (double) ps[k] / std::max<double>((double) K.segments, 1), (double) ps[5 + k] / std::max<double>((double) ps[k], 1),
                            (double) ps[10 + k] / std::max<double>((double) ps[k], 1), 100.0 * (double) ps[10 + k] / std::max<double>((double) tot, 1));
                fprintf(stderr, "[miwave] pooled claims: %.2f tried per segment, %.1f %% won\n", (double) ps[15] / std::max<double>((double) K.segments, 1), 100.0 * (double) ps[16] / std::max<double>((double) ps[15], 1));
                memset(ps, 0, sizeof ps);
                (void) hipMemcpyToSymbol(HIP_SYMBOL(g_pool_stats), ps, sizeof ps);
            }
        }
#endif
#if defined(MIW_WALK_STATS)
        if (ropt.get("MIW_DEBUG")) {
            unsigned long long st[8]; float stf[8];
            if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_walk_stats), sizeof st) == hipSuccess && hipMemcpyFromSymbol(stf, HIP_SYMBOL(g_walk_statsf), sizeof stf) == hipSuccess) {
                for (int k = 0; k < 2; ++k) {
                    const unsigned long long *a = st + 4 * k; const float *f = stf + 4 * k;
                    fprintf(stderr, "[miwave] walk stats %s: rays %llu, node steps/ray %.2f (SIMT eff %.3f), triangle tests/ray %.2f (SIMT eff %.3f)\n",
                            k ? "any-hit" : "closest", a[2], (double) a[0] / std::max<double>(a[2], 1), (double) a[0] / (64.0 * std::max(f[0], 1.f)),
                            (double) a[1] / std::max<double>(a[2], 1), (double) a[1] / (64.0 * std::max(f[1], 1.f)));
                }
                memset(st, 0, sizeof st); memset(stf, 0, sizeof stf);
                (void) hipMemcpyToSymbol(HIP_SYMBOL(g_walk_stats), st, sizeof st); (void) hipMemcpyToSymbol(HIP_SYMBOL(g_walk_statsf), stf, sizeof stf);
            }
        }
#endif
#if defined(MIW_SECTION_PROFILE)
        if (ropt.get("MIW_DEBUG")) {
            unsigned long long sec[16];
            if (hipMemcpyFromSymbol(sec, HIP_SYMBOL(g_sections), sizeof sec) == hipSuccess) {
                static const char *names[13] = { "fetch/begin", "leaf boxes", "E candidates", "S candidates", "path_step", "finish+begin",
                                                 "walks + votes", "shade: surface interaction", "shade: emitter hit + MIS", "shade: RR + emitter sampling + bsdf eval",
                                                 "shade: bsdf sample", "shade: finish + next sample", "shade: pixel fetch + walk start" };
                unsigned long long tot = 0;
                for (int i = 0; i < 13; ++i) tot += sec[i];
                for (int i = 0; i < 13; ++i) if (sec[i]) fprintf(stderr, "[miwave] section %-40s %6.2f %%\n", names[i], 100.0 * (double) sec[i] / (double) std::max<unsigned long long>(tot, 1));
                memset(sec, 0, sizeof sec);
                (void) hipMemcpyToSymbol(HIP_SYMBOL(g_sections), sec, sizeof sec);
            }
        }
#endif
}

// ---- mi_render, what every replay kernel is handed: the log, the pixel states, the class tables, the block -> tile map of this shard (uploaded from a
// context-owned vector: nobody waits for that copy), the tile buffer ----
struct FilmReplay { BlockReplayArgs A; uint32_t side = 0; const uint32_t *chains = nullptr; uint32_t n_chains = 0; /* k_film_chains' table, where the replay takes it */ uint32_t beside = 0; /* groups of 64 tiles replayed beside the path kernel (overlap_enqueue); the launch after it takes the rest */ };
#ifndef MIW_FILM_CHAINS_U_DEFAULT
#define MIW_FILM_CHAINS_U_DEFAULT 8     /* records in flight per lane of k_film_chains: 8 at two wavefronts per SIMD replays C2 in 12.4 ms, 4 at three in 15.3 (k_film_lanes: 16.0) */
#endif
static mi_status film_replay_setup(RenderFrame &F, FilmReplay &R) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; hipStream_t s = F.s; const FilmPlan &FP = F.FP;
    const uint32_t n_tiles = F.n_tiles, bs = F.bs, bs2_log2 = F.bs2_log2, blocks_x = F.blocks_x, blocks_y = F.blocks_y;
    const bool rec16 = FP.rec16;
    std::vector<int32_t> &block_tile = c->h_block_tile;
    block_tile.assign(cfg->block_count, -1);
    for (uint32_t t = 0; t < n_tiles; ++t) block_tile[cfg->tile_list ? cfg->tile_list[t] : t] = (int32_t) t;
    HIP_TRY(c, c->d_block_tile.resize(cfg->block_count));
    HIP_TRY(c, hipMemcpyAsync(c->d_block_tile.p, block_tile.data(), block_tile.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    BlockReplayArgs &A = R.A;
    A.log_pos = c->q_log_pos.p; A.log_val = c->q_log_val.p; A.st = c->q_st.p; A.spp = cfg->spp;
    A.log_rec = rec16 ? c->q_log_rec.p : nullptr; A.log_il = rec16 ? FP.log_il : 0u;
    A.cls.thr = c->d_fc_thr.p; A.cls.w = c->d_fc_w.p; A.cls.count = rec16 ? c->classes.count : 0u; A.cls.reach = rec16 ? c->classes.reach : 0;
    A.block_ids = c->d_block_ids.p; A.block_tile = c->d_block_tile.p;
    A.tile_list = cfg->tile_list ? c->d_tile_list.p : nullptr;
    A.blocks_x = blocks_x; A.blocks_y = blocks_y; A.bs2_log2 = bs2_log2;
    R.side = bs + 2u * (uint32_t) cfg->filter_border;
    A.tile_stride = R.side * R.side * MIW_FILM_CHANNELS;
    HIP_TRY(c, c->d_tiles.resize((size_t) std::max<uint32_t>(n_tiles, 1) * A.tile_stride));
    if (FP.film_chains) {
        // the positions of a tile in chains of equal weight: a function of the tile's shape and the filter alone, so nearly every frame finds its table uploaded
        const uint32_t patches = (R.side + MIW_FL_BS - 1) / MIW_FL_BS;
        const int64_t key = (((int64_t) bs * 64 + cfg->filter_border) * 64 + c->classes.reach) * 4096 + patches;
        if (key != c->film_chains_key) {
            const miw_chains::Table t = miw_chains::build(patches, patches, MIW_FL_BS, (int) bs, cfg->filter_border, c->classes.reach);
            c->h_film_chains = t.packed();                       // (nothing of an earlier frame is in flight: mi_render ends with a wait; the vector outlives the copy)
            HIP_TRY(c, c->d_film_chains.upload(c->h_film_chains, s));
            c->film_chains_n = t.chains(); c->film_chains_key = key;
        }
        R.chains = c->d_film_chains.p; R.n_chains = c->film_chains_n;
    }
    return MI_OK;
}

// The film replay of a full frame BESIDE its render (round 6). k_film_lanes waits on memory (a quarter of its issue slots used), the path kernels on
// issue slots (0.14 TB/s of HBM), and a path kernel's last ~30 ms run at falling occupancy (a lane's last pixel is a serial stream of spp samples): so
// the replay is queued on a second stream BEFORE the path kernel has run, one launch per group of 64 tiles (the unit of the tile-interleaved log), each
// behind a stream-level wait (hipStreamWaitValue32: the command processor polls, no wavefront spins) for the flag the group's LAST finished pixel raises
// (resident_kernel.h: QueueWork::store counts finished pixels per group). The groups finish in queue order, so their replays run in the wave slots the
// path kernel's tail frees, and only the last groups' replay is left when the path kernel ends. Same kernels, same log, same additions: the same film.
// A raise-all launch behind the path kernel releases every wait whatever the counts said (a stream can never be left waiting).
__global__ void k_raise_flags(uint32_t *flag, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) __hip_atomic_store(flag + i, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static mi_status overlap_prepare(RenderFrame &F) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; hipStream_t s = F.s; LaneQueues &Q = F.Q;
    const uint32_t n_tiles = F.n_tiles, bs = F.bs, blocks_x = F.blocks_x, bs2_log2 = F.bs2_log2;
    const uint32_t n_groups = (n_tiles + 63u) / 64u;
    if (!c->ev_fork) {
        bool ok = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 3 && ok; ++i)
            ok = hipStreamCreateWithFlags(&c->stream2[i], hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) { (void) hipGetLastError(); c->overlap_state = 0; return MI_OK; }
    }
    if (c->group_flag_cap < n_groups) {
        if (c->h_group_flag) (void) hipHostFree(c->h_group_flag);
        c->h_group_flag = nullptr; c->group_flag_cap = 0;
        const uint32_t cap = std::max<uint32_t>(1024u, n_groups);
        if (hipHostMalloc((void **) &c->h_group_flag, cap * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { (void) hipGetLastError(); c->overlap_state = 0; return MI_OK; }
        c->group_flag_cap = cap;
    }
    // pixels per group: the pixels of its tiles that lie inside the film (k_init_pixels marks the others done: they are never fetched, never stored)
    std::vector<uint32_t> &expected = c->h_group_expected;
    expected.assign(n_groups, 0u);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t b = cfg->tile_list ? cfg->tile_list[t] : t, bx = b % blocks_x, by = b / blocks_x;
        const int32_t bw = std::min<int32_t>((int32_t) bs, cfg->crop_w - (int32_t) (bx * bs)), bh = std::min<int32_t>((int32_t) bs, cfg->crop_h - (int32_t) (by * bs));
        expected[t >> 6] += (uint32_t) (std::max(bw, 0) * std::max(bh, 0));
    }
    HIP_TRY(c, c->d_group_done.resize(n_groups)); HIP_TRY(c, c->d_group_expected.resize(n_groups));
    memset(c->h_group_flag, 0, n_groups * sizeof(uint32_t));     // (the previous frame's stream work is complete: mi_render ends with a wait)
    HIP_TRY(c, hipMemsetAsync(c->d_group_done.p, 0, n_groups * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemcpyAsync(c->d_group_expected.p, expected.data(), n_groups * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    Q.group_done = c->d_group_done.p; Q.group_expected = c->d_group_expected.p; Q.group_flag = c->h_group_flag; Q.group_shift = bs2_log2 + 6u;
    return MI_OK;
}
// after the path kernel has been launched on `s`: fork, the waits + launches on stream2, the release-all behind the path kernel, the join event
static mi_status overlap_enqueue(RenderFrame &F, FilmReplay &R, bool wait_flags) {
    mi_ctx *c = F.c; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s; LaunchTimer &T = F.T; const uint32_t n_tiles = F.n_tiles;
    const uint32_t n_all = (n_tiles + 63u) / 64u;
    // how many groups are replayed BESIDE the path kernel; the rest in one launch after it (assemble_film). What runs after it cannot take less than one
    // wavefront's chain (~8 - 10 ms) however little it is; measured at C2 (gpurun r6m): three quarters beside 263.6 ms, half 266.1, none 265.8
    uint32_t n_groups = n_all * 3u / 4u;
    if (const char *e = ropt.get("MIW_FILM_OVERLAP_BESIDE")) n_groups = (uint32_t) std::min<long>(std::max<long>(atol(e), 0), (long) n_all);
    const int prio = std::min(3, std::max(0, ropt.num("MIW_FILM_OVERLAP_PRIO", 0)));
    PatchArgs PC; PC.patches_x = PC.patches_y = (R.side + MIW_FL_BS - 1) / MIW_FL_BS; PC.reach = c->classes.reach;
    const uint32_t n_pos = PC.patches_x * PC.patches_y;
    const size_t lbytes = (size_t) (c->classes.count + 1u) * MIW_FQ_WSTRIDE(MIW_FL_BS) * sizeof(float);
    const int fl_nt = ropt.num("MIW_FL_NT", 1);
    // One launch replays a SET of groups (MIW_FILM_OVERLAP_SET, default 4: 324 wavefronts) behind the flags of all of them; the sets go round the three
    // replay streams — kernels of one stream run one after the other, and a replay kernel lasts as long as ONE of its wavefronts (64 pixel runs, a
    // serial chain of ~4 ms) however few there are: one launch per group on one stream would be a chain of 32 such kernels.
    uint32_t set = 4u;
    if (const char *e = ropt.get("MIW_FILM_OVERLAP_SET")) set = (uint32_t) std::max(1, atoi(e));
    const bool lean_ok = fl_nt != 0 && !ropt.off("MIW_FILM_OVERLAP_LEAN");
    for (int i = 0; i < 3; ++i) HIP_TRY(c, hipStreamWaitEvent(c->stream2[i], c->ev_fork, 0));
    uint32_t launches = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += set, ++launches) {
        hipStream_t b = c->stream2[launches % 3u];
        const uint32_t g1 = std::min(n_groups, g0 + set);
        if (wait_flags)
            for (uint32_t g = g0; g < g1; ++g) {
                const hipError_t e = hipStreamWaitValue32(b, c->h_group_flag + g, 1u, hipStreamWaitValueGte, 0xffffffffu);
                if (e != hipSuccess) {                           // the runtime refuses stream memory operations
                    (void) hipGetLastError();
                    c->overlap_state = 0;
                    if (g == 0) return MI_OK;                    // nothing has been launched: assemble_film replays as before
                    return fail(c, MI_ERR_DEVICE, "hipStreamWaitValue32 failed mid-frame: %s", hipGetErrorString(e));
                }
            }
        size_t e0 = 0, e1 = 0;
        if (T.on) { HIP_TRY(c, T.get_event(e0)); HIP_TRY(c, hipEventRecord(c->ev_pool[e0], b)); }
        // (a partial last group of tiles: the kernel's lanes past n_tiles idle, as in the one-launch replay)
        // these sets run while the path kernel does — in the wave slots mi_render keeps free of it (MIW_FILM_OVERLAP_ROOM: on that many CUs the path kernel
        // has three workgroups instead of four, which leaves 152 registers per SIMD) — as the 128-register form of the replay (two records in flight per lane)
        const bool lean = lean_ok;
        if (lean) hipLaunchKernelGGL((k_film_lanes<2, 1, 4>), dim3((g1 - g0) * n_pos), dim3(64), lbytes, b, P.film, R.A, PC, (uint32_t) n_tiles, c->d_tiles.p, g0, (uint32_t) prio);
        else if (fl_nt) hipLaunchKernelGGL((k_film_lanes<4, 1>), dim3((g1 - g0) * n_pos), dim3(64), lbytes, b, P.film, R.A, PC, (uint32_t) n_tiles, c->d_tiles.p, g0, (uint32_t) prio);
        else hipLaunchKernelGGL((k_film_lanes<4, 0>), dim3((g1 - g0) * n_pos), dim3(64), lbytes, b, P.film, R.A, PC, (uint32_t) n_tiles, c->d_tiles.p, g0, (uint32_t) prio);
        if (T.on) { HIP_TRY(c, T.get_event(e1)); HIP_TRY(c, hipEventRecord(c->ev_pool[e1], b)); T.stamps.push_back({ 4, e0, e1 }); }
    }
    for (int i = 0; i < 3; ++i) HIP_TRY(c, hipEventRecord(c->ev_join[i], c->stream2[i]));
    c->replay_launches = launches;
    R.beside = n_groups;
    hipLaunchKernelGGL(k_raise_flags, dim3((n_all + 255u) / 256u), dim3(256), 0, s, c->h_group_flag, n_all);   // behind the path kernel: no wait outlives it
    HIP_TRY(c, hipGetLastError());
    c->replay_enqueued = true;
    c->overlap_state = 1;
    return MI_OK;
}

// ---- mi_render, phase "film": the ordered replay of the sample log into block tiles (device/film_kernels.h; which kernel: the log
// format, the shard's tile count, the options) + the merge of the tiles into the film, or the resolve of the float64 sums ----
static mi_status assemble_film(RenderFrame &F, void *film, mi_status result, const FilmReplay *queued /* != nullptr: the replay's launches already sit in stream2 (overlap_enqueue) */) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s; LaunchTimer &T = F.T;
    const uint32_t n_tiles = F.n_tiles; const size_t film_n = F.film_n;
    const int film_mode = F.FP.film_mode; const bool rec16 = F.FP.rec16; const int film_lanes = F.FP.film_lanes;
    (void) result;
    {
        const size_t elem = cfg->film_f64 ? sizeof(double) : sizeof(float);
        void *dst = film;
        const bool staged = !cfg->film_on_device;
        if (staged) {
            HIP_TRY(c, c->d_out.resize(film_n * elem)); dst = c->d_out.p;
            if (cfg->accumulate) HIP_TRY(c, hipMemcpyAsync(c->d_out.p, film, film_n * elem, hipMemcpyHostToDevice, s));
        }
        float *dst32 = cfg->film_f64 ? nullptr : (float *) dst;
        double *dst64 = cfg->film_f64 ? (double *) dst : nullptr;
        if (film_mode == 1) {
            FilmReplay R;
            if (queued) R = *queued;                              // (set up before the path kernel was launched)
            else MI_TRY(film_replay_setup(F, R));
            BlockReplayArgs &A = R.A;
            const uint32_t side = R.side;
            if (n_tiles) {
                PatchArgs PA;
                PA.patches_x = PA.patches_y = (side + MIW_FP_SIDE - 1) / MIW_FP_SIDE;
                PA.reach = (int32_t) floorf(cfg->filter_radius + .5f);
                const dim3 fgrid(n_tiles * PA.patches_x * PA.patches_y);
                const bool wide = cfg->filter_radius > 0.5f + MIW_RAY_EPSILON;
                if (rec16) {
                    // 16-byte class records -> per-group pixel lists (k_film_groups). Group shape: 2x2 reads 6.25 sample rows per texel,
                    // 4x4 3.06 but spends 0.77 wave-iterations per sample; 4x2 (4.4 rows, 0.55) balances HBM reads against issue slots.
                    // MIW_FILM_GROUP = 2 | 3 | 4 overrides (2x2 / 4x2 / 4x4).
                    const int group = ropt.num("MIW_FILM_GROUP", 3);
                    const size_t wbytes = (size_t) (c->classes.count + 1u) * MIW_FG_WSTRIDE * sizeof(float);
#define MIW_FG_LAUNCH(GW, GH) MIW_TIMED(4, hipLaunchKernelGGL((k_film_groups<GW, GH>), fgrid, dim3(64), wbytes, s, P.film, A, PA, c->d_tiles.p))
                    // round 4: a column of GH texels per lane (k_film_columns; MIW_FILM_COLUMNS = 0: the one-texel-per-lane kernel, 42 / 44: 4 x 2 / 4 x 4 groups;
                    // round 5 measured 2 x 4 and 2 x 2 groups as well: 27.6 / 27.5 ms against 25.6 at C2, gpurun r5p — not kept)
#define MIW_FC_LAUNCH(GW, GH) do { PatchArgs PC = PA; PC.patches_x = (side + (GW) - 1) / (GW); PC.patches_y = (side + (GH) - 1) / (GH); \
                                   const uint32_t per_wave = 64u / (GW), wpt = (PC.patches_x * PC.patches_y + per_wave - 1u) / per_wave; \
                                   MIW_TIMED(4, hipLaunchKernelGGL((k_film_columns<GW, GH>), dim3(n_tiles * wpt), dim3(64), wbytes, s, P.film, A, PC, c->d_tiles.p)); } while (0)
                    // round 5: groups of 4 x 2 (2 x 4: MIW_FILM_QUADS = 24) texels inside DPP quads, the records broadcast by quad_perm operands instead of
                    // staged through LDS (k_film_quads; MIW_FILM_QUADS = 24 / 28 / 44: other group shapes, = 0: the kernels below — also taken when a tile
                    // has fewer groups than a wavefront takes, i.e. tiny blocks)
                    const int columns = ropt.num("MIW_FILM_COLUMNS", 42);
                    // (what runs here by default are shards of fewer than 448 tiles — k_film_lanes takes the rest —: 4 x 2 groups, twice as many and half as
                    // long wavefronts as 2 x 4: a rank's eighth of a 1080p frame 3.63 ms against 4.13, k_film_columns 4.19, gpurun q11; a whole frame 24.1 / 23.8)
                    int quads = ropt.get("MIW_FILM_COLUMNS") == nullptr && ropt.get("MIW_FILM_GROUP") == nullptr ? 42 : 0;
                    if (const char *e = ropt.get("MIW_FILM_QUADS")) quads = atoi(e) == 1 ? 42 : atoi(e);
                    if ((quads != 24 && quads != 42 && quads != 28 && quads != 44) || c->classes.reach > 2) quads = 0;   // (the kernel's LDS rows hold windows of <= 5 weights)
                    const uint32_t qw = (uint32_t) quads / 10u, qh = (uint32_t) quads % 10u;
                    if (quads && ((side + qw - 1) / qw) * ((side + qh - 1) / qh) < 64u / qw) quads = 0;
                    // round 5, the default: one 4 x 4 texel block per lane, a wavefront = one block position in 64 tiles, the sample loop specialised
                    // for the rows / column pairs a pixel's footprint covers (k_film_lanes; MIW_FILM_LANES = 0: the kernels below)
                    const bool lanes = film_lanes != 0;
                    c->counters.film_kernel = lanes ? 4u : quads ? 3u : (columns == 42 || columns == 44 || columns == 82) ? 2u : 1u;   // (mi_counters)
                    if (lanes) {
                        PatchArgs PC = PA; PC.patches_x = PC.patches_y = (side + MIW_FL_BS - 1) / MIW_FL_BS;
                        const size_t lbytes = (size_t) (c->classes.count + 1u) * MIW_FQ_WSTRIDE(MIW_FL_BS) * sizeof(float);
                        const int fl_nt = ropt.num("MIW_FL_NT", 1);       // the log read with streaming loads (16.8 vs 17.05 ms at C2); MIW_FL_NT = 0: plain loads
                        // (the groups of 64 tiles below `first` were replayed beside the path kernel, on the replay streams: overlap_enqueue)
                        const uint32_t first = queued ? queued->beside : 0u, groups_all = ((uint32_t) n_tiles + 63u) / 64u;
                        const uint32_t waves_rest = (groups_all - first) * PC.patches_x * PC.patches_y;
                        // round 11: outside the overlap route the positions of a tile are replayed in chains of equal weight (k_film_chains), with eight records
                        // in flight per lane at two wavefronts per SIMD or (MIW_FILM_CHAINS_U=4) four at three
                        const bool chains = !queued && R.chains != nullptr && R.n_chains != 0u;
                        const int chains_u = ropt.num("MIW_FILM_CHAINS_U", MIW_FILM_CHAINS_U_DEFAULT) == 4 ? 4 : 8;
                        if (ropt.get("MIW_DEBUG")) {
                            if (chains) fprintf(stderr, "[miwave] film replay: k_film_chains, %u chains of %u positions per group of 64 tiles, %d records in flight per lane\n", R.n_chains, PC.patches_x * PC.patches_y, chains_u);
                            else fprintf(stderr, "[miwave] film replay: k_film_lanes, %u positions per group of 64 tiles\n", PC.patches_x * PC.patches_y);
                        }
                        if (waves_rest == 0u) { }
                        else if (chains && chains_u == 8) MIW_TIMED(4, hipLaunchKernelGGL((k_film_chains<8, 1, 2>), dim3(groups_all * R.n_chains), dim3(64), lbytes, s, P.film, A, PC, (uint32_t) n_tiles, c->d_tiles.p, R.chains, R.n_chains));
                        else if (chains) MIW_TIMED(4, hipLaunchKernelGGL((k_film_chains<4, 1, 3>), dim3(groups_all * R.n_chains), dim3(64), lbytes, s, P.film, A, PC, (uint32_t) n_tiles, c->d_tiles.p, R.chains, R.n_chains));
                        else if (fl_nt) MIW_TIMED(4, hipLaunchKernelGGL((k_film_lanes<4, 1>), dim3(waves_rest), dim3(64), lbytes, s, P.film, A, PC, (uint32_t) n_tiles, c->d_tiles.p, first, 0u));
                        else MIW_TIMED(4, hipLaunchKernelGGL((k_film_lanes<4, 0>), dim3(waves_rest), dim3(64), lbytes, s, P.film, A, PC, (uint32_t) n_tiles, c->d_tiles.p, first, 0u));
                        if (queued) { for (int i = 0; i < 3; ++i) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join[i], 0)); }
                    } else if (quads) {
                        PatchArgs PC = PA; PC.patches_x = (side + qw - 1) / qw; PC.patches_y = (side + qh - 1) / qh;
                        const uint32_t per_wave = 64u / qw, waves = (uint32_t) (((size_t) n_tiles * PC.patches_x * PC.patches_y + per_wave - 1u) / per_wave);
                        const size_t qbytes = (size_t) (c->classes.count + 1u) * (size_t) (5u + 2u * qh) * sizeof(float);
#define MIW_FQ_LAUNCH(GW, GH, U) MIW_TIMED(4, hipLaunchKernelGGL((k_film_quads<GW, GH, U>), dim3(waves), dim3(64), qbytes, s, P.film, A, PC, (uint32_t) n_tiles, c->d_tiles.p))
                        const int fq_u = ropt.num("MIW_FQ_U", 4);
                        if (quads == 24) { if (fq_u == 8) MIW_FQ_LAUNCH(2, 4, 8); else if (fq_u == 2) MIW_FQ_LAUNCH(2, 4, 2); else MIW_FQ_LAUNCH(2, 4, 4); }
                        else if (quads == 42) { if (fq_u == 8) MIW_FQ_LAUNCH(4, 2, 8); else MIW_FQ_LAUNCH(4, 2, 4); }
                        else if (quads == 28) MIW_FQ_LAUNCH(2, 8, 4); else MIW_FQ_LAUNCH(4, 4, 4);
#undef MIW_FQ_LAUNCH
                    } else if (columns == 42) MIW_FC_LAUNCH(4, 2); else if (columns == 44) MIW_FC_LAUNCH(4, 4); else if (columns == 82) MIW_FC_LAUNCH(8, 2);
                    else if (group == 4) MIW_FG_LAUNCH(4, 4); else if (group == 2) MIW_FG_LAUNCH(2, 2); else MIW_FG_LAUNCH(4, 2);
#undef MIW_FC_LAUNCH
#undef MIW_FG_LAUNCH
                } else if (wide)
                    MIW_TIMED(4, hipLaunchKernelGGL(k_film_blocks<true>, fgrid, dim3(64), 0, s, P.film, A, PA, c->d_tiles.p));
                else
                    MIW_TIMED(4, hipLaunchKernelGGL(k_film_blocks<false>, fgrid, dim3(64), 0, s, P.film, A, PA, c->d_tiles.p));
            }
            MIW_TIMED(5, hipLaunchKernelGGL(k_film_merge, dim3(((uint32_t) cfg->crop_w + 255u) / 256u, (uint32_t) cfg->crop_h), dim3(256), 0, s,
                                            P.film, A, c->d_tiles.p, dst32, dst64, cfg->accumulate));
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(s));            // block_tile (host vector) must outlive the copy
        } else {
            dim3 block(256), grid((unsigned) ((film_n + 255) / 256));
            MIW_TIMED(4, hipLaunchKernelGGL(k_film_resolve, grid, block, 0, s, c->d_accum.p, dst32, dst64, film_n, cfg->accumulate));
        }
        if (staged) HIP_TRY(c, hipMemcpyAsync(film, c->d_out.p, film_n * elem, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(s));
        T.drain();
#if defined(MIW_DEBUG_POISON)
        if (result == MI_OK) {                                    // (a cancelled render leaves unwritten slots by design)
            std::vector<unsigned char> host(film_n * elem);
            HIP_TRY(c, hipMemcpy(host.data(), dst, film_n * elem, hipMemcpyDeviceToHost));
            size_t bad = 0;
            for (size_t i = 0; i < film_n; ++i) bad += cfg->film_f64 ? std::isnan(((const double *) host.data())[i]) : std::isnan(((const float *) host.data())[i]);
            if (bad) return fail(c, MI_ERR_STATE, "render (poisoned build): %zu film values are NaN - a log / queue / tile slot was read before it was written", bad);
        }
#endif
    }
    return MI_OK;
}

// ---- mi_render, phase "options": this render's options — the context's, under the job's debug overrides (include/miwave.h: mi_render_cfg::debug_*) ----
static mi_status render_options(mi_ctx *c, const mi_render_cfg *cfg, Options &ropt) {
    switch (cfg->debug_film_replay) {
        case MI_FILM_REPLAY_AUTO: break;
        case MI_FILM_REPLAY_BLOCKS: ropt.v["MIW_FILM_LEGACY"] = "1"; break;
        case MI_FILM_REPLAY_GROUPS: ropt.v.erase("MIW_FILM_LEGACY"); ropt.v["MIW_FILM_LANES"] = "0"; ropt.v["MIW_FILM_QUADS"] = "0"; ropt.v["MIW_FILM_COLUMNS"] = "0"; break;
        case MI_FILM_REPLAY_COLUMNS: ropt.v.erase("MIW_FILM_LEGACY"); ropt.v["MIW_FILM_LANES"] = "0"; ropt.v["MIW_FILM_QUADS"] = "0"; ropt.v.erase("MIW_FILM_COLUMNS"); ropt.v.erase("MIW_FILM_GROUP"); break;
        case MI_FILM_REPLAY_QUADS: ropt.v.erase("MIW_FILM_LEGACY"); ropt.v["MIW_FILM_LANES"] = "0"; ropt.v.erase("MIW_FILM_COLUMNS"); ropt.v.erase("MIW_FILM_GROUP"); if (ropt.off("MIW_FILM_QUADS")) ropt.v.erase("MIW_FILM_QUADS"); break;
        case MI_FILM_REPLAY_LANES: ropt.v.erase("MIW_FILM_LEGACY"); ropt.v["MIW_FILM_LANES"] = "1"; break;
        case MI_FILM_REPLAY_LANES_PLAIN_LOG: ropt.v.erase("MIW_FILM_LEGACY"); ropt.v["MIW_FILM_LANES"] = "2"; break;
        default: return fail(c, MI_ERR_INVALID, "render: debug_film_replay must be one of MI_FILM_REPLAY_*");
    }
    if (cfg->debug_tree_width == 4) ropt.v["MIW_BVH8"] = "0";
    else if (cfg->debug_tree_width == 8) ropt.v.erase("MIW_BVH8");
    else if (cfg->debug_tree_width != 0) return fail(c, MI_ERR_INVALID, "render: debug_tree_width must be 0, 4 or 8");
    switch (cfg->debug_path_kernel) {
        case MI_PATH_KERNEL_AUTO: break;
        case MI_PATH_KERNEL_LOCKSTEP: ropt.v["MIW_PHASED"] = "0"; break;
        case MI_PATH_KERNEL_PHASED: ropt.v.erase("MIW_PHASED"); ropt.v["MIW_POOLED"] = "0"; break;
        case MI_PATH_KERNEL_POOLED: ropt.v.erase("MIW_PHASED"); ropt.v["MIW_POOLED"] = "1"; break;
        default: return fail(c, MI_ERR_INVALID, "render: debug_path_kernel must be one of MI_PATH_KERNEL_*");
    }
    return MI_OK;
}

// ---- mi_render, phase "geometry": the job's parameters (fill_params), its validation, the sizes derived from it — blocks, tiles, lanes, film values —
// and the execution plan (mi_render_cfg::plan 0: chosen here) with the refusals of what only the resident plan serves ----
static mi_status frame_geometry(RenderFrame &F) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; RenderParams &P = F.P;
    MI_TRY(fill_params(c, cfg, P));
    const uint32_t bs = (uint32_t) cfg->block_size, bs2 = bs * bs;
    uint32_t bs2_log2 = 0; while ((1u << bs2_log2) < bs2) ++bs2_log2;
    const uint32_t blocks_x = (cfg->crop_w + bs - 1) / bs, blocks_y = (cfg->crop_h + bs - 1) / bs;
    if (!cfg->block_ids || cfg->block_count != blocks_x * blocks_y)
        return fail(c, MI_ERR_INVALID, "render: block_ids must hold %u entries", blocks_x * blocks_y);
    uint32_t n_tiles = cfg->tile_list ? cfg->tile_count : cfg->block_count;
    if (cfg->tile_list)
        for (uint32_t i = 0; i < n_tiles; ++i)
            if (cfg->tile_list[i] >= cfg->block_count) return fail(c, MI_ERR_INVALID, "render: tile_list entry out of range");
    uint64_t n_lanes64 = (uint64_t) n_tiles * bs2;
    if (n_lanes64 >= (1ull << 31)) return fail(c, MI_ERR_INVALID, "render: too many lanes");
    const uint32_t n_lanes = (uint32_t) n_lanes64;
    P.n_lanes = n_lanes;
    F.bs = bs; F.bs2 = bs2; F.bs2_log2 = bs2_log2; F.blocks_x = blocks_x; F.blocks_y = blocks_y; F.n_tiles = n_tiles; F.n_lanes = n_lanes;
    F.film_n = (size_t) cfg->crop_w * cfg->crop_h * MIW_FILM_CHANNELS;

    HIP_TRY(c, hipSetDevice(c->device));
    F.s = c->stream;
    F.wall0 = std::chrono::steady_clock::now();
    c->cancel.store(0);

    // execution plan
    int plan = cfg->plan;
    if (plan < 0 || plan > 2) return fail(c, MI_ERR_INVALID, "render: plan must be 0, 1 or 2");
    const bool lds_resident = c->lds_cfg.brute || (c->lds_cfg.nodes_staged >= c->view.node_count && c->lds_cfg.tris_staged >= c->view.tri_count);
    // measured on MI355X: the resident plan wins whenever the scene query runs out of LDS
    // (packets / staged tree) or with the LDS-stack walk; the queue plan remains for the stackless fallback
    if (plan == 0) plan = (lds_resident || c->lds_cfg.stack || c->nested) ? 2 : 1;
    if (plan == 1 && c->lights_on) return fail(c, MI_ERR_INVALID, "render: scenes with point / spot / directional / constant emitters run the resident plan only (plan 0 or 2)");
    if (plan == 1 && c->nested) return fail(c, MI_ERR_INVALID, "render: scenes with mask / blendbsdf / null / thindielectric records run the resident plan only (plan 0 or 2)");
#if MIW_SPECTRAL
    if (cfg->plan == 1) return fail(c, MI_ERR_INVALID, "render: the scalar_spectral library runs the resident plan only (plan 0 or 2)");
    plan = 2;
#endif
    if (P.integrator == INTEG_DIRECT) {                          // direct.h runs on the paired query of the resident plan
        if (cfg->plan == 1) return fail(c, MI_ERR_INVALID, "render: the direct integrator runs the resident plan only (plan 0 or 2)");
        plan = 2;
    }
    c->counters.plan = (uint32_t) plan;
    F.plan = plan;
    return MI_OK;
}

// ---- mi_render, phase "queues": the per-lane state of the plan, the film plan with its log (plan_film_log), the block and tile lists on the device,
// and the lane queues as the kernels get them ----
static mi_status frame_queues(RenderFrame &F) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; hipStream_t s = F.s; LaneQueues &Q = F.Q;
    const int plan = F.plan; const uint32_t n_lanes = F.n_lanes, n_tiles = F.n_tiles;
    size_t nl = std::max<uint32_t>(n_lanes, 1);
    HIP_TRY(c, c->q_st.resize(nl)); HIP_TRY(c, c->q_pixel.resize(nl));
    if (plan == 1) {
        HIP_TRY(c, c->q_tp.resize(nl)); HIP_TRY(c, c->q_res.resize(nl)); HIP_TRY(c, c->q_ray_o.resize(nl));
        HIP_TRY(c, c->q_ray_d.resize(nl)); HIP_TRY(c, c->q_hit.resize(nl)); HIP_TRY(c, c->q_sh_d.resize(nl));
        HIP_TRY(c, c->q_sh_c.resize(nl)); HIP_TRY(c, c->q_pos.resize(nl)); HIP_TRY(c, c->q_sh_vis.resize(nl));
    }
    HIP_TRY(c, c->d_cnt.resize(MIW_CNT_SHARDS));
    HIP_TRY(c, hipMemsetAsync(c->d_cnt.p, 0, sizeof(Counters) * MIW_CNT_SHARDS, s));

    // film mode: sample log + ordered gather if the log fits, else float64 atomics; the log's format and layout follow the replay kernel
    MI_TRY(plan_film_log(F));
    const int film_mode = F.FP.film_mode; const bool rec16 = F.FP.rec16; const uint32_t log_il = F.FP.log_il;
    HIP_TRY(c, c->d_block_ids.resize(cfg->block_count));
    HIP_TRY(c, hipMemcpyAsync(c->d_block_ids.p, cfg->block_ids, cfg->block_count * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (cfg->tile_list && n_tiles) {
        HIP_TRY(c, c->d_tile_list.resize(n_tiles));
        HIP_TRY(c, hipMemcpyAsync(c->d_tile_list.p, cfg->tile_list, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }

    Q.tp = c->q_tp.p; Q.res = c->q_res.p; Q.st = c->q_st.p; Q.pos = c->q_pos.p; Q.pixel = c->q_pixel.p;
    Q.ray_o = c->q_ray_o.p; Q.ray_d = c->q_ray_d.p; Q.hit = c->q_hit.p;
    Q.sh_d = c->q_sh_d.p; Q.sh_c = c->q_sh_c.p; Q.sh_vis = c->q_sh_vis.p;
    Q.log_pos = film_mode == 1 && !rec16 ? c->q_log_pos.p : nullptr; Q.log_val = film_mode == 1 && !rec16 ? c->q_log_val.p : nullptr;
    Q.lane_cost = nullptr; Q.lane_sorted = nullptr; Q.piece_list = nullptr; Q.simd_ids = nullptr; Q.piece_a = 64u; Q.piece_b = 1u;
    Q.log_rec = film_mode == 1 && rec16 ? c->q_log_rec.p : nullptr; Q.log_thr = rec16 ? c->d_fc_thr.p : nullptr; Q.log_rej = rec16 ? c->classes.count | ((film_mode == 1 ? log_il : 0u) << 8) : 0u;
    return MI_OK;
}

// ---- mi_render, phase "LDS layout" ----
// dynamic LDS of the render launches: [staged geometry | per-lane stack][256 phase thresholds (16-byte records)][the scene's
// small tables + the environment warp's smallest levels (trace.h: stage_tables)]. The kernels that stage the tables keep four
// workgroups per CU (160 KB / 4), so everything has to fit 40 KB less one allocation granule; a scene whose tables do not takes
// the lock-step tree kernels, which read them from global memory (tables_fit; mi_bvh_build applies the same bound before it
// declares a scene tiny). The 8-wide walk's stack is one 8-byte entry per LEVEL of its tree (miw/bvh8.h): a launch that will
// run it sizes the column by the tree's depth instead of the 4-wide walk's 32 x 4 bytes, and the bytes that frees go to more
// levels of the environment warp (round 5: the 0.9 M-triangle interior, depth 10 -> 20 KB of stack, warp levels down to 64 x 32).
struct LdsLayout { TraceLds cfg; size_t rlds, rlds_plain, table_bytes; bool tables_fit; };
// one layout: `base` bytes of staged geometry or stacks in front, at most `env_cap` bytes of environment warp levels, everything inside `lds_budget`
static LdsLayout lds_layout(const mi_ctx *c, const Options &ropt, bool rec16, size_t base, size_t env_cap, size_t lds_budget) {
    LdsLayout L; L.cfg = c->lds_cfg; L.rlds = base;
    L.cfg.thr16 = (uint32_t) ((L.rlds + 15) / 16);
    if (rec16) L.rlds = (size_t) L.cfg.thr16 * 16 + (MIW_FC_TABLE + 3) / 4 * 16;
    L.cfg.tab16 = (uint32_t) ((L.rlds + 15) / 16);
    L.table_bytes = lds_table_bytes(c, L.cfg.tab_words, c->lds_cfg.brute != 0);
    L.cfg.light_words = (uint32_t) (c->lights.size() * sizeof(LightRec) / 4);
    // (packet scenes always stage: mi_bvh_build bounded their tables by 24 KB, which with the packets, boxes and thresholds stays
    // inside the 64 KB a workgroup may ask for, less the kernels' static __shared__ and a granule — at fewer workgroups per CU past
    // what lds_workgroups() below allows)
    L.tables_fit = (size_t) L.cfg.tab16 * 16 + L.table_bytes <= (c->lds_cfg.brute ? 64u * 1024u - MIW_LDS_STATIC - MIW_LDS_GRANULE : lds_budget);
    L.cfg.env_top_count = L.cfg.env_top_base = L.cfg.env_top_words = 0;
    if (L.tables_fit && c->have_env && !ropt.off("MIW_ENV_TOP")) {
        // ... and as many of the environment warp's smallest levels as fit what is left (at most env_cap): levels are stored from
        // the largest (0) to the smallest (n_levels - 1), so the top `count` levels are the tail of the array
        const EnvmapRec &e = c->env_host;
        const size_t used = (size_t) L.cfg.tab16 * 16 + L.table_bytes;
        const size_t room = used < lds_budget ? std::min<size_t>(env_cap, lds_budget - used) : 0;
        uint32_t count = 0;
        while (count + 1 < e.n_levels && ((size_t) c->env_levels_total - e.level_offset[e.n_levels - 1 - count]) * 4 <= room) ++count;
        if (count) {
            L.cfg.env_top_count = count; L.cfg.env_top_base = e.level_offset[e.n_levels - count];
            L.cfg.env_top_words = (uint32_t) (c->env_levels_total - L.cfg.env_top_base);
            L.table_bytes += ((size_t) L.cfg.env_top_words + 3) / 4 * 16;
        }
    }
    // (only the kernels that call stage_tables ask for the table bytes: the phase machine and the packet kernels — `rlds`; the
    // lock-step tree kernels, which read the tables from global memory, launch with `rlds_plain`: ADVICE r04)
    L.rlds_plain = L.rlds;
    if (L.tables_fit) L.rlds = (size_t) L.cfg.tab16 * 16 + L.table_bytes;
    return L;
}
// the layouts a render may use: the default one — sized for the 8-wide tree's depth where the render may walk that tree (stack8_sized) — and the pooled kernel's
struct RenderLds { LdsLayout lay, layp; bool walk8 = false, stack8_sized = false, pooled_fits = false; int pool_nw = 12, pool_pp = 1; };
static mi_status render_lds(RenderFrame &F, const miw_pick::Facts &facts, RenderLds &L) {
    mi_ctx *c = F.c; const Options &ropt = F.ropt; const bool rec16 = F.FP.rec16;
    const size_t lds_budget4 = MIW_LDS_PER_WORKGROUP - MIW_LDS_STATIC - MIW_LDS_GRANULE;
    LdsLayout &lay = L.lay;
    lay = lds_layout(c, ropt, rec16, c->lds_bytes, 4096, lds_budget4);
    // may this render walk the 8-wide tree? Everything the route asks for it (path_route: phased8) but that the tables fit the layout chosen here; MIW_BVH8=0 keeps the 4-wide walk
    const bool pre8 = L.walk8 = F.plan == 2 && F.P.integrator != INTEG_DIRECT && !c->lds_cfg.brute && c->lds_cfg.stack && tree8_on(c, ropt) &&
                                !ropt.off("MIW_PHASED") && ropt.num("MIW_PHASED_WAVES", 4) == 4 && F.FP.film_mode == 1;
    bool &stack8_sized = L.stack8_sized;
    if (pre8 && !ropt.on("MIW_STACK8_FULL")) {
        const size_t base8 = (size_t) c->lds_cfg.stack16 * 16 + (size_t) std::max<uint32_t>(c->nodes8_depth, 2u) * MIW_BLOCK * sizeof(U2);
        const LdsLayout lay8 = lds_layout(c, ropt, rec16, base8, 12288, lds_budget4);
        if (lay8.tables_fit && base8 <= c->lds_bytes) { lay = lay8; stack8_sized = true; }
    }
    // The pooled phase machine (device/pooled_kernel.h, round 6): ONE workgroup of MIW_POOL_NW wavefronts per CU whose lanes share their walks
    // through LDS — per lane an 8-byte stack entry per tree level + an 80-byte job record + a status byte, then thresholds, tables and the
    // environment warp's levels once per CU: [stacks][job records][status][thresholds][tables]. All of the CU's 160 KB may be one workgroup's.
    // MIW_POOLED=0 keeps k_path_phased (A/B runs, and what shards with placed queues run).
    LdsLayout &layp = L.layp; layp = LdsLayout{}; bool &pooled_fits = L.pooled_fits;
    // shape of the workgroup: NW wavefronts x PP pixels per lane — 12 x 1 (three wavefronts per SIMD), or 8 x 2 (two per SIMD, 256 VGPRs, twice the
    // jobs per lane: MIW_POOL_SHAPE=8x2; needs 1024 job records + stacks in LDS: trees of up to 8 levels)
    int &pool_nw = L.pool_nw, &pool_pp = L.pool_pp;
    if (const char *e = ropt.get("MIW_POOL_SHAPE")) { int a = 0, b = 0; if (sscanf(e, "%dx%d", &a, &b) == 2 && ((a == 12 && b == 1) || (a == 8 && b == 2))) { pool_nw = a; pool_pp = b; } }
    // (the 8 x 2 shape is instantiated for the MATS_TRIO class only — BASELINE configs 3 / 4)
    if (!miw_pick::trio_kernel(facts)) { pool_nw = 12; pool_pp = 1; }
    if (pre8 && ropt.on("MIW_POOLED")) {
        const size_t NJ = (size_t) pool_nw * pool_pp * 64u;
        size_t base = (size_t) std::max<uint32_t>(c->nodes8_depth, 2u) * NJ * sizeof(U2);
        const uint32_t pool16 = (uint32_t) (base / 16); base += 5u * NJ * 16u;
        const uint32_t stat16 = (uint32_t) (base / 16); base += NJ;
        layp = lds_layout(c, ropt, rec16, base, 32768, (size_t) 160u * 1024u - 1024u);
        layp.cfg.stack16 = 0u; layp.cfg.pool16 = pool16; layp.cfg.stat16 = stat16; layp.cfg.nodes_staged = layp.cfg.tris_staged = 0u;
        pooled_fits = layp.tables_fit;
        if (ropt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] pooled phase machine: %d wavefronts per workgroup x %d pixels per lane, LDS %zu bytes (stacks %zu, job records %zu, tables %zu of which environment warp levels %u), fits %d\n",
                                         pool_nw, pool_pp, layp.rlds, (size_t) pool16 * 16, 5u * NJ * 16u, layp.table_bytes, layp.cfg.env_top_words * 4u, (int) pooled_fits);
    }
    const TraceLds &rcfg = lay.cfg; const size_t rlds = lay.rlds, rlds_plain = lay.rlds_plain, table_bytes = lay.table_bytes; const bool tables_fit = lay.tables_fit;
    if (MIW_LDS_TABLES && c->lds_cfg.brute && !tables_fit) return fail(c, MI_ERR_STATE, "render: the tables of this packet scene do not fit a workgroup's LDS");
    if (ropt.get("MIW_DEBUG")) fprintf(stderr, "[miwave] LDS per workgroup: %zu bytes dynamic with the scene tables (%zu without), tables %zu B of which environment warp levels %u B and built frame tables %u B, budget %zu%s; + %u static: %u workgroups per CU by LDS\n",
                                     rlds, rlds_plain, table_bytes, rcfg.env_top_words * 4u, (rcfg.tab_words[10] + rcfg.tab_words[11]) * 4u, lds_budget4, stack8_sized ? "; stack sized for the 8-wide tree's depth" : "",
                                     MIW_LDS_STATIC + 16u, miw_plan::lds_workgroups(rlds));
    return MI_OK;
}

// ---- mi_render: the counters of the render that begins; what a device counter shard holds summed into them; the job's time limit ----
static void counters_reset(RenderFrame &F) {
    mi_ctx *c = F.c; mi_counters &K = F.K;
    K.samples = K.segments = K.shadow_rays = K.iterations = 0; K.lanes = F.n_lanes;
    K.ms_trace_closest = K.ms_trace_any = K.ms_shade = K.ms_init = K.ms_resolve = K.ms_path = K.ms_film_blocks = K.ms_film_merge = K.ms_film_pack = 0;
    K.n_trace_closest = K.n_trace_any = K.n_shade = K.n_path = 0; K.path_kernel = 0; K.placed = 0; K.tree_width = 0; K.pooled = 0; K.pool_waves = 0; K.film_overlapped = 0; K.film_groups = 0; K.job_chunk = 0; K.job_chunks = 0; c->replay_enqueued = false; K.place_cost_max = K.place_cost_unit = K.place_max_pixel = K.place_measure_spp = 0; K.place_cost_mean = 0.0;

}
static mi_status read_counters(RenderFrame &F, Counters &sum) {
    mi_ctx *c = F.c; hipStream_t s = F.s; mi_counters &K = F.K;
    HIP_TRY(c, hipMemcpyAsync(c->h_cnt, c->d_cnt.p, sizeof(Counters) * MIW_CNT_SHARDS, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    sum.segments = sum.samples = sum.shadow_rays = sum.active_lanes = 0;
    for (int i = 0; i < MIW_CNT_SHARDS; ++i) {
        sum.segments += c->h_cnt[i].segments; sum.samples += c->h_cnt[i].samples;
        sum.shadow_rays += c->h_cnt[i].shadow_rays; sum.active_lanes += c->h_cnt[i].active_lanes;
    }
    K.samples = sum.samples; K.segments = sum.segments; K.shadow_rays = sum.shadow_rays;
    return MI_OK;
}
static bool out_of_time(const RenderFrame &F) {
    return F.cfg->timeout_s > 0.f &&
           std::chrono::duration<double>(std::chrono::steady_clock::now() - F.wall0).count() > F.cfg->timeout_s;
}
// the context's view with the 8-wide tree's nodes, and the triangles / vertex normals in that tree's order (hit records of its walks name triangles in it)
static SceneView view_over_tree8(const mi_ctx *c) {
    SceneView v = c->view;
    v.nodes8 = c->d_nodes8.p; v.tris = c->d_tris8.p; if (v.tri_vn) v.tri_vn = c->d_tri_vn8.p;
    return v;
}
// what k_init_pixels / k_init_lanes read of the frame's geometry
static InitArgs init_args(const RenderFrame &F) {
    InitArgs A; A.block_ids = F.c->d_block_ids.p; A.tile_list = F.cfg->tile_list ? F.c->d_tile_list.p : nullptr;
    A.blocks_x = F.blocks_x; A.blocks_y = F.blocks_y; A.bs = F.bs; A.bs2_log2 = F.bs2_log2; A.base_seed = F.cfg->base_seed;
    return A;
}

// ---- mi_render, resident plan, phase "route": which path kernel runs and how its pixels reach it — every flag decided once, before the first launch ----
struct PathRoute {
    bool direct, tiny;
    uint32_t n_simd, per_launch;                                  // placed queues: one per SIMD; samples per launch
    bool phased, phased_placeable, phased8; int ph_waves;         // the phase machine; its Placed instantiations; over the 8-wide tree; its wavefronts per SIMD
    bool packet_shard4; uint32_t feat, res_waves;                 // the four-wavefront shard kernel; the scene-feature mask; wavefronts per SIMD that ARE resident
    bool place; uint32_t measure_end, n_pieces;                   // measuring + placed launch; the measuring launch's samples; 64-lane pieces
    int overlap_mode; bool overlap;                               // the film replay beside the render (MIW_FILM_OVERLAP)
    bool pooled;                                                  // k_path_pooled
    bool twin_fits; uint32_t job_pool; size_t twin_rlds;   // a frame twin's launch: the render's layout ends before its blocks and no resident workgroup is lost; MIW_JOB_POOL as launched; its dynamic LDS
};
static mi_status path_route(RenderFrame &F, const miw_pick::Facts &facts, const RenderLds &L, PathRoute &R) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; const FilmPlan &FP = F.FP;
    const int film_mode = FP.film_mode; const uint32_t n_lanes = F.n_lanes, n_tiles = F.n_tiles;
    const bool direct = F.P.integrator == INTEG_DIRECT, tables_fit = L.lay.tables_fit; const size_t rlds = L.lay.rlds;
    const uint32_t n_simd = (uint32_t) c->cu_count * 4u;                                  // placed queues: one per SIMD
    const uint32_t per_launch = cfg->samples_per_launch > 0 ? (uint32_t) cfg->samples_per_launch : 128u;
    // Shards of at most one pixel per resident lane (an N-GPU frame at N >= 8): a short measuring launch (the first eighth of the
    // samples, at least 16) records what every 64-lane piece costs, the pieces are dealt to the SIMDs longest-first, and the
    // rest of the samples run with every wavefront taking its pixels from the queue of the SIMD it sits on (resident_kernel.h:
    // QueueWork). Same samples, same log slots: the film does not change. MIW_PLACE = 0 | 1 overrides.
    // (packet kernels only — QueueWork<Placed> — and only where every pixel of the shard can be resident at once: 4 wavefronts per SIMD
    // for the plain-diffuse packet kernel, 3 for the others — a shard larger than that is balanced by the queue itself)
    // Which path kernel runs (decided here because placement depends on it): tree scenes with the LDS-stack walk get the wave-level
    // phase machine (device/phased_kernel.h; MIW_PHASED=0 keeps the lock-step kernel, MIW_TRIO=0 the full BSDF table: A/B runs)
    const bool tiny = facts.tiny;
    const bool phased_on = !ropt.off("MIW_PHASED");
    const bool trio_kernel = miw_pick::trio_kernel(facts);
    const bool phased = phased_on && !direct && !tiny && c->lds_cfg.stack && (c->view.nodes4 != nullptr || trio_kernel) && (tables_fit || !MIW_LDS_TABLES);
    // 4 waves per SIMD for every tree (measured: 0.9 M triangles +7 - 11 %, 41 k triangles +-0 before the register diet, +8 % after); MIW_PHASED_WAVES = 3 | 4 overrides
    const int ph_waves = ropt.num("MIW_PHASED_WAVES", 4) == 4 ? 4 : 3;
    const bool phased_placeable = phased && c->view.nodes4 != nullptr && ph_waves == 4;     // (the Placed instantiations: the 4-wide tree at four waves per SIMD)
    // the 8-wide tree whenever mi_bvh_build produced one (four waves per SIMD only; MIW_BVH8=0 here keeps the 4-wide walk: A/B runs in one process)
    // (render_lds asked everything else of this — walk8 — before it chose the layout whose tables_fit `phased` reads)
    const bool phased8 = phased_placeable && L.walk8;
    if (L.stack8_sized && !phased8) return fail(c, MI_ERR_STATE, "render: the LDS stack was sized for the 8-wide walk, which this launch does not run");
    // wavefronts per SIMD of the path kernel this render launches (resident_kernel.h / phased_kernel.h / trace.h: what each is compiled for)
    // (the plain-diffuse packet kernel of <= 32 triangles: five — or, when the job's pixels fill no more than four wavefronts per SIMD (a rank's shard), the
    // 128-register instantiation for four: resident_kernel.h; MIW_PACKET_SHARD4=0 keeps five)
    bool packet_shard4 = !phased && tiny && c->diffuse_only && !MIW_SPECTRAL && !direct && c->view.tri_count <= 32u && MIW_PACKET_WAVES > 4 && film_mode == 1 && n_lanes <= 64u * 4u * n_simd;
    if (ropt.off("MIW_PACKET_SHARD4")) packet_shard4 = false;
    // the scene features compiled into the packet path kernel (miw/scene.h: FEAT_*): facts of the uploaded scene and of this render; MIW_LEAN=0 keeps them all
    const uint32_t feat = miw_pick::packet_features_kernel(miw_pick::packet_features(c->have_env, c->shape_normals, c->emitter_normals, cfg->moment_pass != 0), !ropt.off("MIW_LEAN"));
    const uint32_t res_waves_compiled = miw_plan::res_waves_compiled(phased, (uint32_t) ph_waves, tiny, c->diffuse_only && !MIW_SPECTRAL, c->view.tri_count <= 32u, packet_shard4,
                                                                     (uint32_t) MIW_TREE_WAVES, (uint32_t) MIW_PACKET_WAVES, (uint32_t) MIW_PACKET_WAVES_ALL);
    // ... of which a packet kernel keeps resident only the workgroups whose LDS — packets, boxes, thresholds, tables, its static 1 KB — a CU holds:
    // the grid, the placement and the replay's room below count what IS resident, not what the registers alone would allow
    const uint32_t res_waves = tiny && film_mode == 1 ? std::max(1u, std::min(res_waves_compiled, miw_plan::lds_workgroups(rlds))) : res_waves_compiled;
    // A frame twin (kernel_pick.h: frame_twin, chosen at the launch) keeps a block per wavefront in dynamic LDS: the cursor and ring of its job pool (MIW_JOB_POOL ids
    // drawn at a time, their state words read with the draw: resident_kernel.h) and the launch's three counters. It is launched with ONE size of dynamic LDS, the
    // blocks at its end (render_plan.h: MIW_TWIN_LDS, MIW_POOL_AT). That must not cost a resident workgroup, and this layout must end before the blocks: a launch
    // where either fails keeps the lean twin. 32: profiles/r12_job_pool.txt.
    // (Not the bytes the pool needs, counted into this layout: a block whose place depends on the scene or on the pool needs a register for its address through the
    // pixel loop, and the twin has none — every such form spilled past the bounds of tests/test_job_pool_kernel_budget.py. The fixed size is well inside a fifth of a
    // CU, so no launch loses a workgroup to it. MIW_JOB_POOL=0 takes the same launch: no batch is ever drawn and every job is drawn on its own, but fetch_job still
    // reads the (empty) cursor and the counters are the per-wavefront ones — it is the twin without batches, about 1 ms slower on C2 than the kernel before the pool.)
    R.job_pool = miw_plan::pool_size(ropt.num("MIW_JOB_POOL", 32));
    R.twin_fits = tiny && film_mode == 1 && rlds <= MIW_POOL_AT && std::min(res_waves_compiled, miw_plan::lds_workgroups(MIW_TWIN_LDS)) >= res_waves;
    R.twin_rlds = MIW_TWIN_LDS;
    bool place = film_mode == 1 && !direct && (tiny || phased_placeable) && miw_plan::place_window(n_lanes, res_waves, n_simd) &&
                 cfg->spp >= 128u && per_launch >= cfg->spp && cfg->timeout_s <= 0.f;
    if (ropt.off("MIW_PLACE")) place = false;
    uint32_t measure_div = (uint32_t) std::max(2, ropt.num("MIW_PLACE_MEASURE", 8));                                 // the measuring launch runs spp / 8 samples (MIW_PLACE_MEASURE = divisor)
    const uint32_t measure_end = place ? std::max<uint32_t>(16u, cfg->spp / measure_div) : 0u;
    const uint32_t n_pieces = (n_lanes + 63u) / 64u;
    // the film replay beside the render (overlap_prepare / overlap_enqueue above): frames replayed by k_film_lanes over the tile-interleaved log whose
    // samples all run in ONE launch (a pixel is complete when that launch stores it), no placement, no time limit
    // OPT-IN (MIW_FILM_OVERLAP=1): measured at C2 (gpurun r6k - r6m, profiles/r06_experiments.txt) it hides up to 3/4 of the replay and gains 0 - 1 % of the
    // frame — the wave slots it needs cost the path kernel in proportion (32 workgroups short: +6 ms), a replay wavefront beside three packet-kernel
    // wavefronts takes 20 - 30 ms instead of 5, and what is left after the path kernel cannot take less than one wavefront's chain (~8 - 10 ms)
    const int overlap_mode = ropt.num("MIW_FILM_OVERLAP", 0);
    const bool overlap = overlap_mode != 0 && c->overlap_state != 0 && film_mode == 1 && FP.rec16 && FP.film_lanes != 0 && FP.log_il != 0 && !place && !phased /* (QueueWork<..., Groups = false>) */ && tiny && c->diffuse_only && !MIW_SPECTRAL && !direct /* the 120-register packet kernel: the only one a replay wavefront fits beside */ &&
                         per_launch >= cfg->spp && cfg->timeout_s <= 0.f && n_tiles > 0;
#if MIW_SPECTRAL
    const bool pooled = false;
#else
    const bool pooled = phased8 && !place && L.pooled_fits;
#endif
    R.direct = direct; R.tiny = tiny; R.n_simd = n_simd; R.per_launch = per_launch;
    R.phased = phased; R.phased_placeable = phased_placeable; R.phased8 = phased8; R.ph_waves = ph_waves;
    R.packet_shard4 = packet_shard4; R.feat = feat; R.res_waves = res_waves;
    R.place = place; R.measure_end = measure_end; R.n_pieces = n_pieces;
    R.overlap_mode = overlap_mode; R.overlap = overlap; R.pooled = pooled;
    return MI_OK;
}

// ---- mi_render, resident plan, phase "placement" (shards of at most one pixel per resident lane: path_route's `place`) ----
// place_prepare, before the measuring launch: the cost, sort and queue buffers, cleared
static mi_status place_prepare(RenderFrame &F, const PathRoute &R, size_t &place_tmp_bytes) {
    mi_ctx *c = F.c; hipStream_t s = F.s; const uint32_t n_lanes = F.n_lanes, n_pieces = R.n_pieces, n_simd = R.n_simd;
    HIP_TRY(c, c->d_lane_cost.resize(n_lanes)); HIP_TRY(c, c->d_cost_sorted.resize(n_lanes)); HIP_TRY(c, c->d_lane_iota.resize(n_lanes));
    HIP_TRY(c, c->d_lane_sorted.resize((size_t) n_pieces * 64u));
    HIP_TRY(c, c->d_piece_list.resize((size_t) n_simd * MIW_PLACE_PIECES)); HIP_TRY(c, c->d_simd_ids.resize(1u + (1u << 14)));
    HIP_TRY(c, hipMemsetAsync(c->d_lane_cost.p, 0, n_lanes * sizeof(uint32_t), s));      // (lanes without a pixel never report: cost 0, sorted last)
    HIP_TRY(c, hipMemsetAsync(c->d_lane_sorted.p, 0xff, (size_t) n_pieces * 64u * sizeof(uint32_t), s));
    HIP_TRY(c, hipMemsetAsync(c->d_simd_ids.p, 0, c->d_simd_ids.n * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_iota, dim3((n_lanes + 255u) / 256u), dim3(256), 0, s, c->d_lane_iota.p, n_lanes);
    HIP_TRY(c, rocprim::radix_sort_pairs_desc(nullptr, place_tmp_bytes, c->d_lane_cost.p, c->d_cost_sorted.p, c->d_lane_iota.p, c->d_lane_sorted.p, (size_t) n_lanes, 0u, 32u, s));
    HIP_TRY(c, c->d_place_tmp.resize(place_tmp_bytes + 16));
    return MI_OK;
}
// place_deal, between the measuring launch and the placed one: sort the lanes by cost, read the SIMD registry, deal the pieces to the queues, upload
static mi_status place_deal(RenderFrame &F, const PathRoute &R, size_t place_tmp_bytes, TraceLds &rcfg, bool &place_stats_due) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; hipStream_t s = F.s; LaneQueues &Q = F.Q; mi_counters &K = F.K;
    const uint32_t n_lanes = F.n_lanes, n_pieces = R.n_pieces; const bool phased = R.phased, phased8 = R.phased8;
    // the lanes by what their pixel cost, dearest first (device radix sort), cut into pieces of 64: consecutive sorted lanes
    // (the pixels of a wavefront cost about the same and finish together), or every pieces-th one (one pixel of every cost
    // stratum per wavefront). Either way a piece's cost is that of its first (dearest) lane.
    HIP_TRY(c, rocprim::radix_sort_pairs_desc(c->d_place_tmp.p, place_tmp_bytes, c->d_lane_cost.p, c->d_cost_sorted.p, c->d_lane_iota.p, c->d_lane_sorted.p, (size_t) n_lanes, 0u, 32u, s));
    // Which cut: measured on rank 0's 1/8 shard (gpurun r4b, path kernel ms at 256 / 128 / 512 spp; no placement -> consecutive
    // -> spread): material balls 99.3 -> 90.7 -> 104.9, 0.9 M-triangle interior 130.8 -> 131.0 -> 120.9, Cornell packets
    // 40.0 -> 36.7 -> 44.3. Consecutive pieces keep the dear pixels in few wavefronts, which the priorities then favour; the
    // interior — every pixel dear, its walks bound by memory latency, tree and triangles beyond the L2s — gains from every
    // wavefront carrying the same mix. Rule: spread when the tree does not fit the aggregate L2 (32 MB). MIW_PLACE_SPREAD = 0 | 1 overrides.
    bool spread = phased && ((phased8 ? (size_t) c->nodes8_count * sizeof(Bvh8Node) : (size_t) c->nodes4_count * sizeof(Bvh4Node)) + (size_t) c->view.tri_count * sizeof(Tri)) > ((size_t) 32 << 20);
    if (const char *e = ropt.get("MIW_PLACE_SPREAD")) spread = atoi(e) != 0;
    Q.piece_a = spread ? 1u : 64u; Q.piece_b = spread ? n_pieces : 1u;
    // one host round trip between the measuring launch and the placed one, and only for the SIMD registry: the pieces' costs stay on the
    // device (the dealing below needs their ORDER only, which the sort fixed; round 6 — the statistics of the measuring launch,
    // mi_counters::place_*, are read after the frame's last launch, below)
    // the SIMDs the measuring launch ran on, numbered 0 .. nqueues - 1 (simd_ids[1 + hardware key]; word 0 = the "all dry" flag)
    std::vector<uint32_t> &ids = c->h_simd_ids;
    ids.resize(c->d_simd_ids.n);
    HIP_TRY(c, hipMemcpyAsync(ids.data(), c->d_simd_ids.p, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    place_stats_due = cfg->profile != 0;
    uint32_t nqueues = 0;
    for (size_t k = 1; k < ids.size(); ++k) ids[k] = ids[k] ? nqueues++ : 0xffffffffu;
    ids[0] = 0u;
    // the pieces dealt to the queues in alternating rounds (render_plan.h: deal_pieces); fewer than two SIMDs, or more pieces than slots: one queue (cannot happen on a whole device)
    std::vector<uint32_t> &list = c->h_piece_list;                                          // (context-owned: the upload below is not waited for)
    nqueues = miw_plan::deal_pieces(n_pieces, nqueues, MIW_PLACE_PIECES, list);
    if (nqueues) {
        HIP_TRY(c, c->d_piece_list.resize(list.size()));
        HIP_TRY(c, hipMemcpyAsync(c->d_piece_list.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(c->d_simd_ids.p, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        rcfg.queues = nqueues; Q.piece_list = c->d_piece_list.p; Q.lane_sorted = c->d_lane_sorted.p; Q.simd_ids = c->d_simd_ids.p;
        K.placed = 1u;
    }
    return MI_OK;
}
// place_statistics, after the frame's last launch: what the measuring launch found (profile runs) and how the placed launch went (MIW_DEBUG)
static mi_status place_statistics(RenderFrame &F, const PathRoute &R, bool place_stats_due) {
    mi_ctx *c = F.c; const Options &ropt = F.ropt; hipStream_t s = F.s; const LaneQueues &Q = F.Q; mi_counters &K = F.K;
    const uint32_t n_lanes = F.n_lanes, n_pieces = R.n_pieces, n_simd = R.n_simd, measure_end = R.measure_end; const bool phased = R.phased;
    if (place_stats_due) {             // what the measuring launch found (mi_counters::place_*): the shard's dearest pixel and the mean
        std::vector<uint32_t> all(n_lanes); uint32_t first_lane = 0, px = 0;
        HIP_TRY(c, hipMemcpyAsync(all.data(), c->d_cost_sorted.p, (size_t) n_lanes * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(&first_lane, c->d_lane_sorted.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (first_lane < n_lanes) HIP_TRY(c, hipMemcpy(&px, c->q_pixel.p + first_lane, sizeof(uint32_t), hipMemcpyDeviceToHost));
        double csum = 0.0; uint32_t with = 0;
        for (uint32_t v : all) if (v) { csum += (double) v; ++with; }
        K.place_cost_max = all.empty() ? 0u : all[0]; K.place_cost_mean = with ? csum / with : 0.0; K.place_max_pixel = px;
        K.place_cost_unit = phased ? 1u : 0u; K.place_measure_spp = measure_end;
    }
    if (K.placed && ropt.get("MIW_DEBUG")) {                     // how the placed launch went: SIMDs that registered, lanes handed out per queue
        std::vector<uint32_t> cur(n_simd), ids(1u + (1u << 14)), cost(n_pieces);
        (void) hipMemcpy(cur.data(), c->d_next_pixel.p, n_simd * sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void) hipMemcpy(ids.data(), c->d_simd_ids.p, ids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void) hipMemcpy2D(cost.data(), sizeof(uint32_t), c->d_cost_sorted.p, Q.piece_a * sizeof(uint32_t), sizeof(uint32_t), n_pieces, hipMemcpyDeviceToHost);
        uint32_t keys = 0, key_or = 0, full = 0, over = 0; uint64_t csum = 0; uint32_t cmin = ~0u, cmax = 0;
        for (uint32_t k = 0; k < (1u << 14); ++k) if (ids[1 + k] != 0xffffffffu) { ++keys; key_or |= k; }
        ids[0] = keys;
        for (uint32_t v : cur) { full += v >= 64u * MIW_PLACE_PIECES; over += v > 64u * MIW_PLACE_PIECES; }
        for (uint32_t v : cost) { csum += v; cmin = std::min(cmin, v); cmax = std::max(cmax, v); }
        fprintf(stderr, "[miwave] placed queues: %u SIMDs numbered, %u distinct hardware keys (bits used 0x%x), %u of %u queues drained (%u asked beyond their end), "
                        "cost of the dearest pixel of a piece min / mean / max = %u / %.0f / %u (iterations, or 256-cycle units)\n", ids[0], keys, key_or, full, n_simd, over, cmin, (double) csum / n_pieces, cmax);
    }
    return MI_OK;
}

// the rule of the frame twins with the library's switch, asked where the chunks are cut and where the kernel is launched
static bool takes_frame_twin(const Options &ropt, const miw_pick::Pick &pick, bool direct, uint32_t feat, const miw_pick::LaunchFacts &lf) {
    return miw_pick::frame_twin(pick, direct, feat, lf, !ropt.off("MIW_FRAME_TWIN"));
}
// ---- mi_render, resident plan, phase "chunk jobs": LaneQueues::job_* and mi_counters::job_chunk* of the launch that begins at sample `done` ----
static void chunk_jobs(RenderFrame &F, const miw_pick::Facts &facts, const PathRoute &R, const RenderLds &L, uint32_t done) {
    const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; LaneQueues &Q = F.Q; mi_counters &K = F.K; const uint32_t n_lanes = F.n_lanes;
    const bool tiny = R.tiny, phased = R.phased, place = R.place, overlap = R.overlap, pooled_fits = L.pooled_fits;
    const uint32_t per_launch = R.per_launch, res_waves = R.res_waves, n_simd = R.n_simd;
    // chunk jobs (resident_kernel.h: QueueWork::fetch): full frames of the packet kernels, all samples in one launch. Without them a frame of N pixels
    // on L resident lanes lasts ceil(N / L) rounds of one PIXEL (every lane starts at once, a pixel's samples are one serial job, the jobs are about
    // equally long): C2 = 6.33 -> 7; with chunks of spp / 8 samples ceil(8 N / L) / 8 = 6.375.
    Q.job_chunk = Q.job_pow = Q.job_total = 0u; Q.job_min = 0x80000000u;
    // Every job costs one atomic on ONE address (the queue's counter) and a hand-over (a 16-byte state word out and in, past the L2): uniform chunks of
    // 8 / 16 / 32 samples ran C2 in 702 / 496 / 305 ms, 64 / 128 / 256 in 226.8 / 226.5 / 230.6, whole pixels in 239.3 (gpurun r6p). So the chunks
    // HALVE — a chunk ends where the samples still to do are a power of two — down to job_min samples (512 spp: 256 + 128 + 64 + 64): four hand-overs
    // per pixel instead of eight, the tail as long as the smallest. The phase machine's full frames (C3, C4) take the same queue.
    if ((tiny || (phased && MIW_PHASED_JOBS != 0)) && !pooled_fits && !place && !overlap && done == 0 && per_launch >= cfg->spp && cfg->timeout_s <= 0.f) {
        uint32_t jmin = tiny ? 64u : 32u;                                 // (gpurun r6s, halving chunks: C2 4 461 / 4 316 / 4 389 Msamples/s at 64 / 32 / 128; C3 1 298 / 1 305, C4 522 / 528 at 64 / 32)
        // A frame twin with its job pool draws `pool` jobs per atomic, so the queue's counter no longer bounds the chunk: 16 (C2, pool 32: path kernel 192.94 - 193.01 ms
        // at 16, 193.42 - 193.46 at 32, 195.41 - 195.46 at 64, the parent's 195.18 - 195.46: profiles/r12_job_pool.txt, visit 3). Asked of the rule the launch asks (kernel_pick.h: frame_twin), with the facts
        // that launch will have: chunk jobs, one queue and no group counts by the condition above, no tail priorities unless MIW_TAIL_PRIO turns them on.
        // (only a frame that takes chunk jobs for its own size: one that has them forced — MIW_JOB_CHUNK_FORCE, the tests of the hand-over — keeps 64)
        if (tiny && R.twin_fits && R.job_pool && miw_plan::chunks_enough(n_lanes, res_waves, n_simd)) {
            miw_pick::LaunchFacts lf;
            lf.job_chunks = true; lf.log_rec16 = Q.log_rec != nullptr; lf.one_queue = true; lf.tail_prio = ropt.on("MIW_TAIL_PRIO");
            lf.leaf_filter = F.c->lds_cfg.leaves != 0u; lf.group_counts = false;
            if (takes_frame_twin(ropt, miw_pick::resident_path(facts, false), R.direct, R.feat, lf)) jmin = 16u;
        }
        if (const char *e = ropt.get("MIW_JOB_CHUNK")) jmin = (uint32_t) std::max(0, atoi(e));   // (a value that is no power of two: off — render_plan.h: chunk_schedule)
        // from 1.2 pixels per resident lane on (render_plan.h: chunks_enough)
        bool enough = miw_plan::chunks_enough(n_lanes, res_waves, n_simd);
        if (ropt.on("MIW_JOB_CHUNK_FORCE")) enough = true;
        const miw_plan::ChunkSchedule cs = miw_plan::chunk_schedule(cfg->spp, jmin);
        if (cs.job_min && enough && cs.chunks >= 2u && (uint64_t) n_lanes * cs.chunks < (1ull << 31)) {
            Q.job_chunk = cs.job_min; Q.job_min = cs.job_min; Q.job_pow = cs.job_pow; Q.job_total = (uint32_t) ((uint64_t) n_lanes * cs.chunks);
            K.job_chunk = cs.job_min; K.job_chunks = (uint32_t) cs.chunks;
        }
    }
}

// ---- mi_render, resident plan, phase "launch": one launch of the path kernel up to sample `end` — the dispatch over every kernel class, with the
// launch's constants (rcfg / ph_cfg / pcfg) and grid ----
struct PathLaunch {
    dim3 grid;                                                    // one workgroup per MIW_BLOCK lanes: the persistent grids are cut from it
    TraceLds rcfg;                                                // the render's layout; queues: 1, or the SIMD count for the placed launch (place_deal)
    SceneView view8;                                              // the context's view over the 8-wide tree's nodes and triangle order (path_route: phased8)
    TileArgs TA; size_t tile_bytes = 0;                           // film_mode 2: the workgroup-local float64 tile (atomic_film_tile)
    uint32_t end = 0;
    uint32_t feat_launched = FEAT_ALL;                            // the mask of the instantiation this launch IS: set where a lean twin is launched (MIW_DEBUG prints it)
    bool frame_launched = false;                                  // ... and whether it is a frame twin: set where one is launched
};
// film_mode 2: workgroup-local float64 tile in LDS (needs 16x16-pixel workgroups: block_size >= 16)
static mi_status atomic_film_tile(RenderFrame &F, const InitArgs &A, PathLaunch &PK) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const int film_mode = F.FP.film_mode; const uint32_t bs = F.bs, blocks_x = F.blocks_x, bs2_log2 = F.bs2_log2;
    TileArgs &TA = PK.TA; size_t &tile_bytes = PK.tile_bytes;
    memset(&TA, 0, sizeof TA);
    tile_bytes = 0;
    if (film_mode == 2 && bs >= 16) {
        TA.tile_list = A.tile_list; TA.blocks_x = blocks_x; TA.bs = bs; TA.bs2_log2 = bs2_log2;
        TA.side = 16u + 2u * std::max<uint32_t>((uint32_t) cfg->filter_border, (uint32_t) floorf(cfg->filter_radius + .5f));
        TA.geom16 = (uint32_t) ((c->lds_bytes + 15) / 16);
        tile_bytes = (size_t) TA.geom16 * 16 - c->lds_bytes + (size_t) TA.side * TA.side * MIW_FILM_CHANNELS * sizeof(double);
        if (c->lds_bytes + tile_bytes > 64 * 1024) {
#define MIW_ATOMIC_ATTR(T, M, A, I) HIP_TRY(c, hipFuncSetAttribute((const void *) k_path_resident<false, T, M, A, I>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (c->lds_bytes + tile_bytes)));
            MIW_ATOMIC_LIST(MIW_ATOMIC_ATTR)
#undef MIW_ATOMIC_ATTR
        }
    }
    return MI_OK;
}
static mi_status launch_path_kernel(RenderFrame &F, const miw_pick::Facts &facts, const PathRoute &R, const RenderLds &L, PathLaunch &PK) {
    mi_ctx *c = F.c; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s; const LaneQueues &Q = F.Q; LaunchTimer &T = F.T; mi_counters &K = F.K;
    const uint32_t integ = R.direct ? INTEG_DIRECT : INTEG_PATH, feat = R.feat, res_waves = R.res_waves, end = PK.end;
    const bool direct = R.direct, tiny = R.tiny, phased = R.phased, phased8 = R.phased8, place = R.place, packet_shard4 = R.packet_shard4, pooled = R.pooled;
    const int ph_waves = R.ph_waves;
    const size_t rlds = L.lay.rlds, rlds_plain = L.lay.rlds_plain, tile_bytes = PK.tile_bytes;
    const dim3 grid = PK.grid, block(MIW_BLOCK); TraceLds &rcfg = PK.rcfg; const SceneView &view8 = PK.view8; const TileArgs &TA = PK.TA;
    uint32_t &feat_launched = PK.feat_launched; bool &frame_launched = PK.frame_launched;
    if (F.FP.film_mode == 1) {
        // persistent grid: as many workgroups per CU as the kernel is compiled for wavefronts per SIMD — the plain-diffuse packet kernel FIVE since
        // round 6 (96 registers: 248.1 -> 238.3 ms at C2, resident_kernel.h), the other scalar_rgb packet kernels four. (Round 2 launched 3 per CU for shards of about one pixel per resident lane; with the
        // least-progress-first priorities below every pixel of such a shard should start at once: 42.3 vs 49.6 ms on the 1/8
        // shard of C2, profiles/r03.)
        unsigned wg_per_cu = miw_plan::persistent_wg_per_cu(direct, (unsigned) res_waves);   // (never fewer than four: a kernel compiled for three keeps a fourth workgroup queued behind them)
        if (const char *e = ropt.get("MIW_WG_PER_CU")) wg_per_cu = (unsigned) std::max(1, atoi(e));
        unsigned room = 0u;                                // wave slots kept free for the replay that runs beside this launch (overlap_enqueue)
        if (Q.group_done) { room = 32u; if (const char *e = ropt.get("MIW_FILM_OVERLAP_ROOM")) room = (unsigned) std::max(0, atoi(e)); }
        // (room is counted from what is RESIDENT — the kernels compiled for three wavefronts per SIMD get a fourth workgroup per CU queued behind the
        // first three, which would take every slot a shorter grid leaves)
        const dim3 pgrid(miw_plan::persistent_grid(grid.x, (unsigned) c->cu_count, wg_per_cu, room, direct ? (unsigned) MIW_DIRECT_WAVES : (unsigned) res_waves));
        // (`phased`, `ph_waves`: path_route; MIW_BVH4=0 keeps the BVH2 node body for the MATS_TRIO class: A/B runs)
        K.path_kernel = phased ? (c->view.nodes4 ? 1u : 3u) : 0u;
        const dim3 phgrid(std::min<unsigned>(grid.x, (unsigned) c->cu_count * (unsigned) ph_waves));
        // the shade vote (phased_kernel.h): shade once n_shade * num >= den * (lanes of the busier walk body). Measured on the
        // 4-wide tree (gpurun r2f / r2g, Msamples/s at 1 : 1 -> 3 : 2 -> 2 : 1): balls 844 -> 873 -> 860; interior with its
        // environment-map lookups 338 -> 348 -> 361. MIW_SHADE_VOTE=num:den overrides (A/B runs).
        // (per-XCD pixel queues — each XCD's workgroups taking their pixels from their own eighth of the image, so that the rays of
        // one L2 stay in one region — measured neutral on the material balls, 883 vs 879 Msamples/s, and -2 % on the interior,
        // 362 vs 370: the secondary rays of a closed room go everywhere. Removed again.)
        // (rcfg.queues: 1, or the SIMD count for the placed launch of a small shard, set above)
        // least-progress-first wave priorities (QueueWork::tick): the wavefronts of a SIMD finish together instead of the most
        // expensive one running on alone. Made for shards of about one pixel per resident lane (1/8 of C2: path kernel 50.1 ->
        // 42.3 ms; 1/8 of the material balls -14 %), it also shortens the drain of a full frame (C2 275.9 -> 268.7 ms), so it is
        // always on — but for a packet kernel's launch of chunk jobs, whose tail is one chunk long: with and without them it took the same time in every configuration
        // (r6t: C2 path kernel 222.01 221.47 ms with / 221.17 220.93 without, C5 573.9 / 573.5, direct 79.7 / 79.8), and the frame twins compile them out
        // (kernel_pick.h: frame_twin). MIW_TAIL_PRIO = 0 | 1 overrides.
        rcfg.tail_prio = tiny && Q.job_chunk ? 0u : 1u;
        if (const char *e = ropt.get("MIW_TAIL_PRIO")) rcfg.tail_prio = atoi(e) != 0 ? 1u : 0u;
        TraceLds ph_cfg = rcfg;
        ph_cfg.shade_num = 2; ph_cfg.shade_den = c->have_env ? 4 : 3;
        if (const char *e = ropt.get("MIW_SHADE_VOTE")) { int a = 0, b = 0; if (sscanf(e, "%d:%d", &a, &b) == 2 && a > 0 && b > 0) { ph_cfg.shade_num = (uint32_t) a; ph_cfg.shade_den = (uint32_t) b; } }
        // when the walk loops hand over (phased_kernel.h): a loop runs on until its lanes are outnumbered 2 : 1 by the other walk body's, or
        // node_exit : 1 / tri_exit : 1 by the lanes waiting for another body. Measured on the 8-wide walk (gpurun r5f - r5h, Msamples/s,
        // material balls / interior): rounds 3 - 4's rule (1 : 1 against the other body, waiting + half the lanes that left) 1 119 / 463;
        // 2 : 1 with node 1, triangle 1 -> 1 161 / 471; triangle 2 -> 1 174 / 472; node 2 -> 1 147 / 478; node 2, triangle 3 -> . / 481
        // (the interior's shade runs are long: loops that wait for them less often win there). MIW_LOOP_EXIT=node:triangle overrides.
        ph_cfg.node_exit = c->have_env ? 2u : 1u; ph_cfg.tri_exit = c->have_env ? 3u : 2u;
        if (const char *e = ropt.get("MIW_LOOP_EXIT")) { int a = 0, b = 0; if (sscanf(e, "%d:%d", &a, &b) == 2 && a >= 0 && b >= 0) { ph_cfg.node_exit = (uint32_t) a; ph_cfg.tri_exit = (uint32_t) b; } }
// (the Spec argument is a constant of the build, phased_kernel.h: MIW_DEBUG's line gives its value, the other five arguments as the macro got them)
#define MIW_PHASED_LAUNCH_(M, A, WV, W, PL) do { MIW_SAY_KERNEL_TEXT(ropt, MIW_PHASE_SPEC != 0 ? "k_path_phased<" #M ", " #A ", true, " #WV ", " #W ", " #PL ">" : "k_path_phased<" #M ", " #A ", false, " #WV ", " #W ", " #PL ">"); \
    MIW_TIMED(6, hipLaunchKernelGGL((k_path_phased<M, A, MIW_PHASE_SPEC != 0, WV, W, PL>), phgrid, block, rlds, s, P, (W) == 2 ? view8 : c->view, Q, c->d_cnt.p, ph_cfg, end, c->d_next_pixel.p)); } while (0)
#define MIW_PHASED_LAUNCH(M, A, W) do { if (ph_waves == 4) MIW_PHASED_LAUNCH_(M, A, 4, W, false); else MIW_PHASED_LAUNCH_(M, A, 3, W, false); } while (0)
        K.tree_width = phased ? (phased8 ? 8u : (c->view.nodes4 ? 4u : 2u)) : 0u;
#if MIW_SPECTRAL
        if (pooled) { }
#else
        if (pooled) {
            const int pool_nw = L.pool_nw, pool_pp = L.pool_pp; const LdsLayout &layp = L.layp;
            // one workgroup per CU; the vote's constants travel in the fields the old kernel's vote used (pooled_kernel.h: shade_min, walk_min, node_min, tri_min)
            // + pool_claim_min; MIW_POOL_VOTE=shade_min:walk_min:node_min:tri_min:claim_min overrides (A/B runs)
            TraceLds pcfg = layp.cfg; pcfg.queues = 1u; pcfg.tail_prio = ph_cfg.tail_prio;
            pcfg.shade_num = 48; pcfg.shade_den = 16; pcfg.node_exit = 40u; pcfg.tri_exit = 20u; pcfg.pool_claim_min = 8u;
            if (const char *e = ropt.get("MIW_POOL_VOTE")) { int a = 0, b = 0, n = 0, t = 0, m = 0; if (sscanf(e, "%d:%d:%d:%d:%d", &a, &b, &n, &t, &m) == 5 && a > 0 && b >= 0) { pcfg.shade_num = (uint32_t) a; pcfg.shade_den = (uint32_t) b; pcfg.node_exit = (uint32_t) n; pcfg.tri_exit = (uint32_t) t; pcfg.pool_claim_min = (uint32_t) std::max(m, 1); } }
            const unsigned NL = (unsigned) pool_nw * 64u;
            const dim3 qgrid(std::min<unsigned>((F.n_lanes + NL - 1u) / NL, (unsigned) c->cu_count)), qblock(NL);
            if (c->lights_on) return fail(c, MI_ERR_INVALID, "render: the pooled kernel (MI_PATH_KERNEL_POOLED) does not serve scenes with point / spot / directional / constant emitters");
            if (c->nested) return fail(c, MI_ERR_INVALID, "render: the pooled kernel (MI_PATH_KERNEL_POOLED) does not serve scenes with mask / blendbsdf / null / thindielectric records");
            const miw_pick::Pick pick = miw_pick::tree_class(facts);
#define MIW_POOLED_LAUNCH(M, A, NW_, PP_) if (pick.mats == (M) && pick.analytic == (A) && pool_nw == (NW_) && pool_pp == (PP_)) { \
                HIP_TRY(c, hipFuncSetAttribute((const void *) k_path_pooled<M, A, NW_, PP_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) layp.rlds)); \
                MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (k_path_pooled<M, A, NW_, PP_>), qgrid, qblock, layp.rlds, s, P, view8, Q, c->d_cnt.p, pcfg, end, c->d_next_pixel.p)); } else
            MIW_POOLED_LIST(MIW_POOLED_LAUNCH) return fail(c, MI_ERR_STATE, "render: no k_path_pooled<%d, %d, %d, %d> in the library", pick.mats, (int) pick.analytic, pool_nw, pool_pp);
#undef MIW_POOLED_LAUNCH
            K.pooled = 1u; K.pool_waves = (uint32_t) pool_nw;
        }
#endif
        else
        if (phased && !c->view.nodes4) MIW_PHASED_LAUNCH(MATS_TRIO, false, 0);    // (MIW_BVH4=0: the phase machine steps through the BVH2, the MATS_TRIO class only)
        else if (phased) {
            // the tree's width, and the Placed instantiations for a shard of about one pixel per resident lane (measuring, then placed launch)
            const miw_pick::Pick pick = miw_pick::tree_class(facts);
            const int wide = phased8 ? 2 : 1;
#define MIW_PHASED_PICKED(M, A, WV, W, PL) if (pick.mats == (M) && pick.analytic == (A) && ph_waves == (WV) && wide == (W) && place == (PL)) MIW_PHASED_LAUNCH_(M, A, WV, W, PL); else
            MIW_PHASED_LIST(MIW_PHASED_PICKED) return fail(c, MI_ERR_STATE, "render: no k_path_phased<%d, %d, ., %d, %d, %d> in the library", pick.mats, (int) pick.analytic, ph_waves, wide, (int) place);
#undef MIW_PHASED_PICKED
        }
#undef MIW_PHASED_LAUNCH
#undef MIW_PHASED_LAUNCH_
        // (MIW_DEBUG's line is the text of the template-id the launch instantiates: MIW_LAUNCH_NAMED)
#define MIW_PACKET_SPECIAL(...) MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (__VA_ARGS__), pgrid, block, rlds, s, P, c->view, Q, (double *) nullptr, c->d_cnt.p, rcfg, end, TA, c->d_next_pixel.p))
        // the special instantiations of the packet kernel, in front of its table (none of them is ever the direct integrator's: `overlap` and `packet_shard4` above)
        else if (Q.group_done && c->view.tri_count <= 32u)     // (overlap: tiny && diffuse_only) the instantiation that counts finished pixels per group of 64 tiles
            MIW_PACKET_SPECIAL(k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, true>);
        else if (Q.group_done)
            MIW_PACKET_SPECIAL(k_path_resident<true, 1, MATS_DIFFUSE, false, INTEG_PATH, true>);
        else if (packet_shard4 && !Q.group_done && feat == FEAT_NONE) {
            feat_launched = FEAT_NONE;
            MIW_PACKET_SPECIAL(k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 4, FEAT_NONE>);
        }
        else if (packet_shard4 && !Q.group_done)
            MIW_PACKET_SPECIAL(k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 4>);
#undef MIW_PACKET_SPECIAL
        else {
            // kernel variants (kernel_pick.h): no BSDF dispatch when every shape is plain diffuse (64-bit candidate masks: that variant fits 4 waves per
            // SIMD without spills); else 32-bit candidate masks up to 32 triangles. The packet kernels stage the scene's tables (rlds), the lock-step tree kernels do not.
            const miw_pick::Pick pick = direct ? miw_pick::resident_direct(facts) : miw_pick::resident_path(facts, false);
            // (the lean twins in front of the table: a mask that is no instantiation has become FEAT_ALL above, a class without a twin keeps the full kernel)
            // (... and the frame twins in front of those: a lean twin's launch whose facts are the ones the twin has compiled in — chunk jobs from one queue, the 16-byte
            // log, no tail priorities, the leaf filter on, no group counts; MIW_FRAME_TWIN=0 keeps the lean twin)
            miw_pick::LaunchFacts lf;
            lf.job_chunks = Q.job_chunk != 0u; lf.log_rec16 = Q.log_rec != nullptr; lf.one_queue = rcfg.queues == 1u; lf.tail_prio = rcfg.tail_prio != 0u;
            lf.leaf_filter = c->lds_cfg.leaves != 0u; lf.group_counts = Q.group_done != nullptr;
            const bool frame = R.twin_fits && takes_frame_twin(ropt, pick, direct, feat, lf);
            // (the twin's job pool — path_route — goes in the film tile's arguments, which a sample-log launch does not read)
            TileArgs TW = TA; TW.side = R.job_pool;
#define MIW_FRAME_LAUNCH(T, M) if (frame && MIW_PICKED(T, M, false)) { feat_launched = FEAT_NONE; frame_launched = true; MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (k_path_resident<true, T, M, false, INTEG_PATH, false, 0, FEAT_FRAME>), pgrid, block, R.twin_rlds, s, P, c->view, Q, (double *) nullptr, c->d_cnt.p, rcfg, end, TW, c->d_next_pixel.p)); } else
            MIW_LEAN_LIST(MIW_FRAME_LAUNCH)
#undef MIW_FRAME_LAUNCH
#define MIW_LEAN_LAUNCH(T, M) if (feat == FEAT_NONE && !direct && MIW_PICKED(T, M, false)) { feat_launched = FEAT_NONE; MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (k_path_resident<true, T, M, false, INTEG_PATH, false, 0, FEAT_NONE>), pgrid, block, rlds, s, P, c->view, Q, (double *) nullptr, c->d_cnt.p, rcfg, end, TA, c->d_next_pixel.p)); } else
            MIW_LEAN_LIST(MIW_LEAN_LAUNCH)
#undef MIW_LEAN_LAUNCH
#define MIW_RESIDENT_LAUNCH(T, M, A, I) if (integ == (I) && MIW_PICKED(T, M, A)) MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (k_path_resident<true, T, M, A, I>), pgrid, block, (T) != 0 ? rlds : rlds_plain, s, P, c->view, Q, (double *) nullptr, c->d_cnt.p, rcfg, end, TA, c->d_next_pixel.p)); else
            MIW_RESIDENT_LIST(MIW_RESIDENT_LAUNCH) return fail(c, MI_ERR_STATE, "render: no k_path_resident<true, %d, %d, %d, %u> in the library", pick.tiny, pick.mats, (int) pick.analytic, integ);
#undef MIW_RESIDENT_LAUNCH
        }
    } else {
        // the float64-atomics film: one workgroup per 16 x 16 pixels, three classes (kernel_pick.h: resident_atomic)
        const miw_pick::Pick pick = miw_pick::resident_atomic(facts);
#define MIW_ATOMIC_LAUNCH(T, M, A, I) if (integ == (I) && MIW_PICKED(T, M, A)) MIW_TIMED(6, MIW_LAUNCH_NAMED(ropt, (k_path_resident<false, T, M, A, I>), grid, block, c->lds_bytes + tile_bytes, s, P, c->view, Q, c->d_accum.p, c->d_cnt.p, c->lds_cfg, end, TA, (uint32_t *) nullptr)); else
        MIW_ATOMIC_LIST(MIW_ATOMIC_LAUNCH) return fail(c, MI_ERR_STATE, "render: no k_path_resident<false, %d, %d, %d, %u> in the library", pick.tiny, pick.mats, (int) pick.analytic, integ);
#undef MIW_ATOMIC_LAUNCH
    }
    return MI_OK;
}

// ---- mi_render, the resident plan: every pixel advances `per_launch` samples per launch ----
static mi_status render_resident(RenderFrame &F, const miw_pick::Facts &facts, const RenderLds &L, FilmReplay &replay, mi_status &result) {
    mi_ctx *c = F.c; const mi_render_cfg *cfg = F.cfg; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s;
    LaneQueues &Q = F.Q; LaunchTimer &T = F.T; mi_counters &K = F.K; const int film_mode = F.FP.film_mode;
    PathLaunch PK; PK.grid = dim3((F.n_lanes + MIW_BLOCK - 1) / MIW_BLOCK);
    const InitArgs A = init_args(F);
    MIW_TIMED(3, hipLaunchKernelGGL(k_init_pixels, PK.grid, dim3(MIW_BLOCK), 0, s, P, c->q_st.p, c->q_pixel.p, A));
    HIP_TRY(c, hipGetLastError());
    PathRoute R;
    MI_TRY(path_route(F, facts, L, R));
    HIP_TRY(c, c->d_next_pixel.resize(std::max<uint32_t>(8u, R.n_simd)));
    PK.rcfg = L.lay.cfg;
    PK.view8 = R.phased8 ? view_over_tree8(c) : c->view;
    size_t place_tmp_bytes = 0;
    if (R.place) MI_TRY(place_prepare(F, R, place_tmp_bytes));
    MI_TRY(atomic_film_tile(F, A, PK));
    const uint32_t sync_every = 8;
    uint32_t launches = 0;
    bool place_stats_due = false;                              // (profile runs) the measuring launch's statistics, fetched after the last launch
    for (uint32_t done = 0; done < cfg->spp; ) {
        PK.end = cfg->spp - done < R.per_launch ? cfg->spp : done + R.per_launch;
        PK.feat_launched = FEAT_ALL; PK.frame_launched = false;
        if (film_mode == 1) {
            // persistent grid: <= 4 workgroups per CU, fed from the shared pixel queue
            HIP_TRY(c, hipMemsetAsync(c->d_next_pixel.p, 0, c->d_next_pixel.n * sizeof(uint32_t), s));
            PK.rcfg.queues = 1u; Q.lane_cost = nullptr; Q.lane_sorted = nullptr; Q.piece_list = nullptr; Q.simd_ids = nullptr;
            if (R.overlap && done == 0) {                        // the replay's arguments and the per-group counters, in front of the path kernel
                MI_TRY(film_replay_setup(F, replay));
                MI_TRY(overlap_prepare(F));
                if (Q.group_done) HIP_TRY(c, hipEventRecord(c->ev_fork, s));
            }
            chunk_jobs(F, facts, R, L, done);
            if (R.place && done == 0) { PK.end = R.measure_end; Q.lane_cost = c->d_lane_cost.p; Q.simd_ids = c->d_simd_ids.p; }   // the measuring launch
            else if (R.place) MI_TRY(place_deal(F, R, place_tmp_bytes, PK.rcfg, place_stats_due));                               // the placed launch
        }
        MI_TRY(launch_path_kernel(F, facts, R, L, PK));
        if (Q.group_done) {                                      // the path kernel is in `s`: queue the replay beside it
            MI_TRY(overlap_enqueue(F, replay, R.overlap_mode != 2));
            if (c->replay_enqueued) { K.film_overlapped = 1u; K.film_groups = c->replay_launches; }
            Q.group_done = nullptr; Q.group_expected = nullptr; Q.group_flag = nullptr;
        }
        // which instantiation this launch was, said after the launch site set it: 0x0 only where a lean twin (FEAT_NONE) was launched — not for a class without
        // a twin, the overlap's Groups = true pair, the direct integrator or the float64-atomics film, which run the full kernel whatever mask was chosen
        if (ropt.get("MIW_DEBUG") && R.tiny && !R.phased) fprintf(stderr, "[miwave] packet path kernel launched: scene features 0x%x of 0x%x compiled in (mask chosen for the render: 0x%x)\n", PK.feat_launched, (uint32_t) FEAT_ALL, R.feat);
        if (ropt.get("MIW_DEBUG") && R.tiny && !R.phased && !PK.frame_launched) fprintf(stderr, "[miwave] packet path kernel launched: frame twin no\n");
        if (ropt.get("MIW_DEBUG") && R.tiny && !R.phased && PK.frame_launched) fprintf(stderr, "[miwave] packet path kernel launched: frame twin yes (chunk jobs, one queue, 16-byte log, no tail priorities, leaf filter compiled in), job pool %u, smallest chunk %u, %zu bytes of LDS per workgroup\n", R.job_pool, Q.job_min, R.twin_rlds);
        K.n_path++; K.iterations++;
        done = PK.end;
        // cancel() / timeout take effect at launch granularity (the reference checks should_stop() per block)
        if ((++launches % sync_every == 0 || cfg->timeout_s > 0.f || c->cancel.load()) && done < cfg->spp) {
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(s));
            T.drain();
            if (c->cancel.load() || out_of_time(F)) { result = MI_ERR_CANCELLED; break; }
        }
    }
    HIP_TRY(c, hipGetLastError());
    Counters sum;
    MI_TRY(read_counters(F, sum));
    MI_TRY(place_statistics(F, R, place_stats_due));
    print_debug_statistics(c, ropt, K);                      // (debug builds only: -DMIW_PHASE_STATS / _WALK_STATS / _SECTION_PROFILE / _VERIFY_FILTER)
    T.drain();
    return MI_OK;
}

#if !MIW_SPECTRAL
// ---- mi_render, the wavefront (queue) plan: one launch per stage and iteration over work lists; the stackless fallback ----
static mi_status render_wavefront(RenderFrame &F, mi_status &result) {
    mi_ctx *c = F.c; const Options &ropt = F.ropt; const RenderParams &P = F.P; hipStream_t s = F.s;
    const LaneQueues &Q = F.Q; LaunchTimer &T = F.T; mi_counters &K = F.K; const int film_mode = F.FP.film_mode; const uint32_t n_lanes = F.n_lanes;
    dim3 grid((n_lanes + MIW_BLOCK - 1) / MIW_BLOCK), block(MIW_BLOCK);
    const InitArgs A = init_args(F);
    // work lists (stream compaction + material sorting), double-buffered by iteration parity
    const size_t n_wg = grid.x, seg_lanes = n_wg * MIW_BLOCK;
    HIP_TRY(c, c->d_lists.resize((size_t) 2 * WL_LISTS * seg_lanes));
    HIP_TRY(c, c->d_list_counts.resize(2 * WL_LISTS * n_wg));
    HIP_TRY(c, hipMemsetAsync(c->d_list_counts.p, 0, 2 * WL_LISTS * n_wg * sizeof(uint32_t), s));
    WorkLists WL[2];
    for (int p = 0; p < 2; ++p) {
        for (int l = 0; l < WL_LISTS; ++l) WL[p].list[l] = c->d_lists.p + ((size_t) p * WL_LISTS + l) * seg_lanes;
        WL[p].count = c->d_list_counts.p + (size_t) p * WL_LISTS * n_wg;
    }
    MIW_TIMED(3, hipLaunchKernelGGL(k_init_lanes, grid, block, 0, s, P, Q, c->q_pixel.p, A, WL[0]));
    HIP_TRY(c, hipGetLastError());

    // trees walked with the LDS stack: one persistent stream kernel serves the E and the S rays of an iteration
    // (device/stream_trace.h); MIW_STREAM=0 keeps the slice-per-workgroup kernels (A/B runs)
    const bool stream_on = !ropt.off("MIW_STREAM");
    const bool stream = stream_on && c->lds_cfg.stack && !c->lds_cfg.brute && c->lds_cfg.nodes_staged == 0;
    K.path_kernel = stream ? 2u : 0u;
    // round 6: the stream kernel walks the 8-wide tree (the phase machine's two walk bodies) wherever mi_bvh_build produced it; its hit records then
    // name triangles in that tree's order, so k_sort_hits and k_shade get the view with the triangles / vertex normals of that order
    const bool stream8 = stream && tree8_on(c, ropt);
    const SceneView pview = stream8 ? view_over_tree8(c) : c->view;
    K.tree_width = stream8 ? 8u : 0u;
    if (stream) {
        HIP_TRY(c, c->d_next_pixel.resize(1));
        HIP_TRY(c, hipMemsetAsync(c->d_next_pixel.p, 0, sizeof(uint32_t), s));
    }
    const dim3 sgrid(std::min<unsigned>(grid.x, (unsigned) c->cu_count * (stream8 ? 4u : (unsigned) MIW_STREAM_WAVES)));
    const int check_every = 16;
    bool first = true;
    unsigned long long active_prev = 0;
    uint32_t parity = 0;
    for (;;) {
        for (int it = 0; it < check_every; ++it, parity ^= 1u) {
            const WorkLists &cur = WL[parity], &nxt = WL[parity ^ 1u];
            if (stream) {
                if (stream8) MIW_TIMED(0, hipLaunchKernelGGL(k_trace_stream<2>, sgrid, block, c->lds_bytes, s, pview, Q, c->lds_cfg, cur, (uint32_t) n_wg, c->d_next_pixel.p));
                else MIW_TIMED(0, hipLaunchKernelGGL(k_trace_stream<0>, sgrid, block, c->lds_bytes, s, pview, Q, c->lds_cfg, cur, (uint32_t) n_wg, c->d_next_pixel.p));
                MIW_TIMED(1, hipLaunchKernelGGL(k_sort_hits, grid, block, 0, s, pview, Q, cur, c->d_next_pixel.p));
                K.n_trace_closest++; K.n_trace_any++;
            } else {
                if (!first) {
                    MIW_TIMED(1, hipLaunchKernelGGL(k_trace<true>, grid, block, c->lds_bytes, s, c->view, Q, c->lds_cfg, cur));
                    K.n_trace_any++;
                }
                MIW_TIMED(0, hipLaunchKernelGGL(k_trace<false>, grid, block, c->lds_bytes, s, c->view, Q, c->lds_cfg, cur));
                K.n_trace_closest++;
            }
            const uint32_t count_active = it == check_every - 1 ? 1u : 0u;
            if (film_mode == 1)
                MIW_TIMED(2, hipLaunchKernelGGL(k_shade<true>, grid, block, 0, s, P, pview, Q, (double *) nullptr, c->d_cnt.p, count_active, cur, nxt));
            else
                MIW_TIMED(2, hipLaunchKernelGGL(k_shade<false>, grid, block, 0, s, P, pview, Q, c->d_accum.p, c->d_cnt.p, count_active, cur, nxt));
            K.n_shade++; K.iterations++;
            first = false;
        }
        HIP_TRY(c, hipGetLastError());
        Counters sum;
        MI_TRY(read_counters(F, sum));
        T.drain();
        // active_lanes accumulates over the counting launches: the last one's share is the delta
        unsigned long long active_now = sum.active_lanes - active_prev;
        active_prev = sum.active_lanes;
        if (active_now == 0) break;
        if (c->cancel.load()) { result = MI_ERR_CANCELLED; break; }
        if (out_of_time(F)) { result = MI_ERR_CANCELLED; break; }
    }
    return MI_OK;
}
#endif

mi_status mi_render(mi_ctx *c, const mi_render_cfg *cfg, void *film) {
    if (!c || !cfg || !film) return MI_ERR_INVALID;
    if (!c->have_bvh) return fail(c, MI_ERR_STATE, "mi_render: call mi_scene_upload and mi_bvh_build first");
    RenderFrame F(c, cfg);
    MI_TRY(render_options(c, cfg, F.ropt));
    MI_TRY(frame_geometry(F));
    MI_TRY(frame_queues(F));                                      // (with the film plan: sample log + ordered gather if the log fits, else float64 atomics)
    const miw_pick::Facts facts = pick_facts(c, F.ropt);        // what the kernel-class rules read (kernel_pick.h)
    RenderLds L;
    MI_TRY(render_lds(F, facts, L));
    counters_reset(F);
    mi_status result = MI_OK;                                     // (MI_ERR_CANCELLED: the film is assembled from what ran)
    FilmReplay replay;                                            // (filled before the path kernel when the replay is queued beside it)
    if (F.n_lanes > 0 && F.plan == 2) MI_TRY(render_resident(F, facts, L, replay, result));
#if !MIW_SPECTRAL
    else if (F.n_lanes > 0) MI_TRY(render_wavefront(F, result));
#endif
    // film assembly -> caller's buffer (device pointer, or staged through d_out for a host pointer)
    const mi_status fs = assemble_film(F, film, result, c->replay_enqueued ? &replay : nullptr);
    c->replay_enqueued = false;
    if (fs != MI_OK) return fs;
    F.K.ms_render = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - F.wall0).count();
    if (result == MI_ERR_CANCELLED) c->error = "render cancelled";
    return result;
}

// ---- mi_eval -----------------------------------------------------------------------------
mi_status mi_eval(mi_ctx *c, int32_t op, const mi_render_cfg *cfg, const float *in, int32_t is, float *out, int32_t os, uint64_t n) {
    if (!c || !in || !out || is <= 0 || os <= 0) return MI_ERR_INVALID;
    if (n == 0) return MI_OK;
    RenderParams P; memset(&P, 0, sizeof P);
    if (op == MI_EVAL_CAMERA_RAY) {
        if (!cfg) return fail(c, MI_ERR_INVALID, "mi_eval: camera ray needs a render cfg");
        mi_status st = fill_params(c, cfg, P);
        if (st != MI_OK) return st;
    }
    if ((op == MI_EVAL_BSDF || op == MI_EVAL_EMITTER_SAMPLE || op == MI_EVAL_ENVMAP || op == MI_EVAL_TEXTURE) && !c->have_bvh)
        return fail(c, MI_ERR_STATE, "mi_eval: scene required");
    const bool medium_op = op == MI_EVAL_MEDIUM || op == MI_EVAL_PHASE;
    if (medium_op) {
#if MIW_SPECTRAL
        return fail(c, MI_ERR_INVALID, "mi_eval: media are served by the scalar_rgb library");
#else
        if (!c->have_scene) return fail(c, MI_ERR_STATE, "mi_eval: scene required");
        if (is < (op == MI_EVAL_MEDIUM ? 12 : 9) || os < (op == MI_EVAL_MEDIUM ? 22 : 5)) return fail(c, MI_ERR_INVALID, "mi_eval: strides too small for op %d", op);
        for (uint64_t i = 0; i < n; ++i) {
            const float m = in[i * (uint64_t) is];
            if (!(m >= 0.f && m < (float) c->media.size()) || m != (float) (uint32_t) m)
                return fail(c, MI_ERR_INVALID, "mi_eval: entry %llu: medium %g out of range (%zu media)", (unsigned long long) i, (double) m, c->media.size());
            if (op == MI_EVAL_MEDIUM) {
                const float ch = in[i * (uint64_t) is + 10];
                if (!(ch == 0.f || ch == 1.f || ch == 2.f)) return fail(c, MI_ERR_INVALID, "mi_eval: entry %llu: channel %g must be 0, 1 or 2", (unsigned long long) i, (double) ch);
            }
        }
#endif
    }
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<float> din, dout;
    HIP_TRY(c, din.resize(n * is)); HIP_TRY(c, dout.resize(n * os));
    HIP_TRY(c, hipMemcpyAsync(din.p, in, n * is * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(dout.p, 0, n * os * sizeof(float), c->stream));
#if !MIW_SPECTRAL
    if (medium_op) {
        HIP_TRY(c, volpath_launch_eval(c->stream, op, media_view(c), din.p, is, dout.p, os, n));
        HIP_TRY(c, hipMemcpyAsync(out, dout.p, n * os * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return MI_OK;
    }
#endif
    hipLaunchKernelGGL(k_eval, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, c->stream, op, P, c->view, din.p, is, dout.p, os, n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, dout.p, n * os * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MI_OK;
}

// ---- mi_selftest -------------------------------------------------------------------------
__global__ void k_selftest_rcp(unsigned long long *mismatches) {
    unsigned long long bad = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = u2f((uint32_t) i);
        volatile float one = 1.f;                               // keeps the division a division
        const float ref = one / x, got = miw::rcp(x), got_l = miw::rcp_loop(x);
        if (f2u(ref) != f2u(got) && !(ref != ref && got != got)) ++bad;
        if (f2u(ref) != f2u(got_l) && !(ref != ref && got_l != got_l)) ++bad;
    }
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mismatches, bad);
}

mi_status mi_selftest(mi_ctx *c, int32_t which, uint64_t *mismatches) {
    if (!c || !mismatches) return MI_ERR_INVALID;
    if (which != MI_SELFTEST_RCP) return fail(c, MI_ERR_INVALID, "mi_selftest: unknown test %d", which);
    HIP_TRY(c, hipSetDevice(c->device));
    TmpBuf<unsigned long long> d;
    HIP_TRY(c, d.resize(1));
    HIP_TRY(c, hipMemsetAsync(d.p, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_selftest_rcp, dim3(4096), dim3(256), 0, c->stream, d.p);
    HIP_TRY(c, hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(c, hipMemcpyAsync(&h, d.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *mismatches = h;
    return MI_OK;
}

#include "aov_host.h"                  /* mi_render_aov, mi_aov_channel_count */
#include "sensor_host.h"               /* mi_render_sensor, mi_sensor_sample_ray */

} // extern "C"
#endif // !MIW_KERNELS_ONLY
