// The launch arithmetic of mi_render (csrc/miwave.hip) that reads plain numbers only: the chunk-job schedule, the dealing of placed pieces to SIMD
// queues, the workgroups a CU holds by LDS, the persistent grid, the wavefronts per SIMD a path kernel is compiled for and the size window of the
// placed route. Plain C++17 without HIP types, so that a host program can print them (tests/test_render_plan_cpu.py); mi_render's phases call them
// with the context's and the job's values.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#define MIW_LDS_PER_CU (160u * 1024u)
#define MIW_LDS_PER_WORKGROUP (MIW_LDS_PER_CU / 4u) /* 160 KB per CU / four workgroups of 256 (four wavefronts per SIMD) */
#define MIW_LDS_STATIC 1024u                      /* static __shared__ of k_path_phased and of the packet kernels: s_job_pend (QueueWork: a word per lane); s_prog, 16 bytes, inside the granule below */
#define MIW_LDS_GRANULE 512u                      /* LDS is handed out in granules: dynamic + static, rounded up, must stay inside 40 KB */

namespace miw_plan {

// ---- chunk jobs (device/resident_kernel.h: QueueWork::fetch) ----
// The chunks HALVE — a chunk ends where the samples still to do are a power of two — down to jmin samples (512 spp, jmin 64: 256 + 128 + 64 + 64).
// `jmin` is the option's value as given: one that is no power of two means off (0), as does 0.
struct ChunkSchedule { uint32_t job_min, job_pow; uint64_t chunks; };   // job_pow: the largest power of two below spp; chunks: per pixel (1: no chunk jobs)
inline ChunkSchedule chunk_schedule(uint32_t spp, uint32_t jmin) {
    jmin = (jmin & (jmin - 1u)) ? 0u : jmin;
    uint32_t pow2 = 1u;
    while (pow2 * 2u < spp) pow2 *= 2u;                          // the largest power of two below spp
    uint64_t chunks = 1u;
    for (uint32_t r = pow2; jmin && r >= jmin && r < spp; r >>= 1) ++chunks;
    return { jmin, pow2, chunks };
}
// from 1.2 pixels per resident lane on (gpurun r6z, a rank's shard of C2 with / without: 4 ranks = 1.6 pixels per lane 67.8 / 79.1 ms, 5 ranks = 1.3: 58.7 / 67.5,
// 6 ranks = 1.06: 54.9 / 54.6; at about ONE pixel per lane every pixel is in flight all the time and no lane finds a second job: 8 ranks 47.1 against the placed launches' 41.4)
inline bool chunks_enough(uint32_t n_lanes, uint32_t res_waves, uint32_t n_simd) { return (uint64_t) n_lanes * 5u >= (uint64_t) 6u * 64u * res_waves * n_simd; }

// ---- the job pool of a frame twin's wavefront (device/resident_kernel.h: QueueWork<..., Frame>::refill / fetch_job) ----
// A wavefront draws `pool` consecutive ids from the queue at a time and keeps the half-open range [next, end) of those nobody has taken yet; the state word
// and the pixel word of id sit in ring slot id & (pool - 1) of its LDS block, read when the batch was drawn. The device calls these very functions.
struct JobCursor { uint32_t next, end; };
#define MIW_POOL_DRY 0xffffffffu                     /* next == end == MIW_POOL_DRY: a batch began at or past job_total — the queue is empty for good, no further draw */
// MIW_JOB_POOL as given -> the pool: a power of two from 2 to 32 (a lane reads one word of a batch; MIW_POOL_MAX below), anything else is 0 = every job drawn on its own
constexpr uint32_t pool_size(int given) { return given >= 2 && given <= 32 && (given & (given - 1)) == 0 ? (uint32_t) given : 0u; }
// the cursor after a draw that returned `base`: ids at or above job_total are dropped
constexpr JobCursor pool_batch(uint32_t base, uint32_t pool, uint32_t job_total) {
    return base >= job_total ? JobCursor{ MIW_POOL_DRY, MIW_POOL_DRY } : JobCursor{ base, job_total - base < pool ? job_total : base + pool };
}
constexpr bool pool_dry(JobCursor c) { return c.next == MIW_POOL_DRY; }
constexpr bool pool_empty(JobCursor c) { return c.next == c.end; }                      // (a dry pool is empty too: test pool_dry first)
// `asking` lanes ask at once, ranked 0 .. asking - 1: the first pool_take() of them get id next + rank, the cursor moves past those; the others draw for themselves
constexpr uint32_t pool_take(JobCursor c, uint32_t asking) { return pool_dry(c) ? 0u : (c.end - c.next < asking ? c.end - c.next : asking); }
constexpr JobCursor pool_after(JobCursor c, uint32_t asking) { return JobCursor{ c.next + pool_take(c, asking), c.end }; }
constexpr uint32_t pool_ring_slot(uint32_t id, uint32_t pool) { return id & (pool - 1u); }
// a wavefront's block in the dynamic LDS behind the render's layout: cursor (8 B), the pool's size (4 B of 8), the three counters of the launch (3 x 8 B), 8 B spare, `pool` state words (16 B), `pool` pixel words
#define MIW_POOL_HEAD 48u
constexpr uint32_t pool_wave_bytes(uint32_t pool) { return MIW_POOL_HEAD + 20u * pool; }
constexpr uint32_t pool_lds_bytes(uint32_t pool, uint32_t waves_per_workgroup) { return waves_per_workgroup * pool_wave_bytes(pool); }
// A frame twin is launched with ONE size of dynamic LDS whatever the scene, the most that still lets a CU hold five workgroups, and the blocks stand at its end at the
// stride of the largest pool: a wavefront finds its block from its number alone (no register holds the address through the pixel loop: the twin has none to spare,
// tests/test_job_pool_kernel_budget.py). A scene whose own layout reaches into the blocks keeps the lean twin (miwave.hip: path_route).
#define MIW_POOL_MAX 32u
#define MIW_POOL_STRIDE 688u                         /* pool_wave_bytes(MIW_POOL_MAX) */
#define MIW_POOL_FRONT 2752u                         /* pool_lds_bytes(MIW_POOL_MAX, 4 wavefronts of a workgroup): a multiple of 16 */
#define MIW_TWIN_LDS 26624u                          /* 26 KB: with the static 1 040 well inside a fifth of a CU (32 KB) whatever granule the LDS is handed out in */
#define MIW_POOL_AT (MIW_TWIN_LDS - MIW_POOL_FRONT)  /* where the blocks begin */
static_assert(pool_wave_bytes(MIW_POOL_MAX) == MIW_POOL_STRIDE && pool_lds_bytes(MIW_POOL_MAX, 4u) == MIW_POOL_FRONT && MIW_POOL_FRONT % 16u == 0u && MIW_TWIN_LDS % 16u == 0u, "the twin's blocks");

// ---- placed queues: the pieces of 64 sorted lanes dealt to `nqueues` SIMD queues of `slots` pieces each ----
// The pieces arrive in descending cost (they are cuts of the sorted lane list), so "longest piece first onto the emptiest queue" is dealt
// in rounds, alternating direction (round 0: piece i to queue i; round 1: piece N + i to queue N - 1 - i; ...): every queue gets one
// piece of every cost stratum, dear and cheap strata paired. O(pieces) on the host between the two launches — the heap-based
// longest-first dealing of rounds 3 - 5 took 0.3 ms there (4 096 pieces, 1 024 queues) with the GPU idle; any dealing renders the same film.
// Returns the queue count the launch uses — 0 (one queue; `list` untouched) where fewer than two SIMDs registered or the pieces do not fit their
// slots (cannot happen on a whole device) — and list[queue * slots + round] = piece, 0xffffffff where a slot stays empty.
inline uint32_t deal_pieces(uint32_t n_pieces, uint32_t nqueues, uint32_t slots, std::vector<uint32_t> &list) {
    if (nqueues < 2u || (uint64_t) nqueues * slots < n_pieces) return 0u;
    list.assign((size_t) nqueues * slots, 0xffffffffu);
    for (uint32_t i = 0; i < n_pieces; ++i) {
        const uint32_t round = i / nqueues, k = i % nqueues, qd = (round & 1u) ? nqueues - 1u - k : k;
        list[(size_t) qd * slots + round] = i;
    }
    return nqueues;
}

// workgroups of a kernel with `dyn` bytes of dynamic LDS (+ its static __shared__, in granules) that one CU holds
// KNOWN ERROR at the edge: the part hands LDS out in larger granules than MIW_LDS_GRANULE. A launch of 31 232 dynamic bytes, five workgroups per CU by this count,
// ran with four (profiles/r12_job_pool.txt, visit 2). Every launch sized by it so far asks for what its scene needs, far from a boundary; a size chosen to sit AT a
// boundary must keep a margin (MIW_TWIN_LDS does: 26 KB where 31 KB counts as five). The true granule has not been measured.
inline uint32_t lds_workgroups(size_t dyn) {
    const size_t per = (dyn + MIW_LDS_STATIC + 16u + MIW_LDS_GRANULE - 1u) / MIW_LDS_GRANULE * MIW_LDS_GRANULE;
    return (uint32_t) (MIW_LDS_PER_CU / per);
}

// ---- the persistent grid of the sample-log film's path kernels ----
// `wg_per_cu` workgroups per CU (persistent_wg_per_cu, or the option's value); `room` wave slots are kept free for the replay that runs beside the
// launch (overlap_enqueue), counted from what is RESIDENT — `resident_waves` per SIMD: the kernels compiled for three wavefronts per SIMD get a fourth
// workgroup per CU queued behind the first three, which would take every slot a shorter grid leaves. Never more workgroups than `grid_x`, what the lanes need.
inline unsigned persistent_wg_per_cu(bool direct, unsigned res_waves) { return std::max(4u, direct ? 4u : res_waves); }   // (never fewer than four: a kernel compiled for three keeps a fourth workgroup queued behind them)
inline unsigned persistent_grid(unsigned grid_x, unsigned cu_count, unsigned wg_per_cu, unsigned room, unsigned resident_waves) {
    const unsigned resident = cu_count * resident_waves;
    const unsigned full = room ? std::min(cu_count * wg_per_cu, resident) : cu_count * wg_per_cu;
    return std::min<unsigned>(grid_x, full > 2u * room ? full - room : full);
}

// wavefronts per SIMD of the path kernel a render launches (resident_kernel.h / phased_kernel.h / trace.h: what each is compiled for); the *_waves arguments
// are those headers' MIW_*_WAVES. `plain_diffuse`: diffuse_only in the scalar_rgb library; `small`: <= 32 triangles.
inline uint32_t res_waves_compiled(bool phased, uint32_t ph_waves, bool tiny, bool plain_diffuse, bool small, bool packet_shard4,
                                   uint32_t tree_waves, uint32_t packet_waves, uint32_t packet_waves_all) {
    return phased ? ph_waves : !tiny ? tree_waves : (plain_diffuse ? (small && !packet_shard4 ? packet_waves : 4u) : packet_waves_all);
}
// the size window of the placed route: from half a pixel per SIMD lane up to every pixel of the shard resident at once
inline bool place_window(uint32_t n_lanes, uint32_t res_waves, uint32_t n_simd) { return n_lanes >= 64u * n_simd / 2u && n_lanes <= 64u * res_waves * n_simd; }

}  // namespace miw_plan
