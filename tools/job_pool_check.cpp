// Host check of the frame twin's job pool (csrc/render_plan.h: miw_plan::pool_*; device/resident_kernel.h: QueueWork<..., Frame>::refill / fetch_job), on the
// functions the device calls. Three models, each printing one row per configuration and counting violations:
//
//   C  coverage   `waves` wavefronts ask the one queue in a fixed pseudo-random order, 1 .. 64 lanes at a time: the askers take ids from the wavefront's cursor,
//                 the rest draw for themselves (one add of their count to the queue's counter), and a wavefront whose cursor is empty draws a batch. Every id in
//                 [0, job_total) is served exactly once, none at or above it; with a pool, a served id's ring slot holds what its batch wrote there.
//   P  progress   lanes that run jobs of chunk-major ids over `n_lanes` pixel slots, chunk j of a slot ready when chunk j - 1 has finished; a lane whose job is not
//                 ready parks it and asks again on its wavefront's next trip; a batch is drawn only by a trip in which a lane of the wavefront is running (the
//                 device draws in tick(), which running lanes execute). Every wavefront takes one trip (the launch starts them together: with more lanes than
//                 slots the later ones draw chunks whose predecessors have not run); from then on the scheduler is adversarial: it always steps the wavefront holding the largest id —
//                 in its cursor, parked or running — that can change anything. The run must end with every job run exactly once.
//
//   g++ -O2 -std=c++17 -I . tools/job_pool_check.cpp -o job_pool_check && ./job_pool_check        (also under -fsanitize=address,undefined)
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "mitsuba2_amd/csrc/render_plan.h"

using miw_plan::JobCursor;
static unsigned long long violations = 0;
#define CHECK(cond) do { if (!(cond)) { if (violations++ < 20) fprintf(stderr, "violated at line %d: %s\n", __LINE__, #cond); } } while (0)

static uint32_t rnd(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (s >> 33); }

struct Wave {
    JobCursor cur{ 0u, 0u };
    std::vector<uint32_t> ring;          // ring slot (MIW_POOL_MAX of them whatever the pool, as on the device) -> the id whose words the batch read into it
    bool exhausted = false;
};

// a batch: `pool` ids from the queue, each id's words into its ring slot
static void draw_batch(Wave &w, uint32_t &queue, uint32_t pool, uint32_t job_total) {
    const uint32_t base = queue; queue += pool;
    w.cur = miw_plan::pool_batch(base, pool, job_total);
    if (miw_plan::pool_dry(w.cur)) return;
    CHECK(w.cur.next == base && w.cur.end <= job_total && w.cur.end - w.cur.next <= pool);
    for (uint32_t id = w.cur.next; id < w.cur.end; ++id) w.ring[miw_plan::pool_ring_slot(id, MIW_POOL_MAX)] = id;
}

static void coverage(uint32_t job_total, uint32_t pool, uint32_t waves) {
    std::vector<uint8_t> served(job_total, 0);
    std::vector<Wave> W(waves);
    for (Wave &w : W) w.ring.assign(MIW_POOL_MAX, 0xffffffffu);
    uint32_t queue = 0, live = waves; unsigned long long asks = 0, beyond = 0, from_pool = 0;
    uint64_t seed = 0x9e3779b97f4a7c15ull ^ ((uint64_t) job_total << 20) ^ ((uint64_t) pool << 8) ^ waves;
    while (live) {
        Wave &w = W[rnd(seed) % waves];
        if (w.exhausted) continue;
        const uint32_t asking = 1u + rnd(seed) % 64u; ++asks;
        uint32_t took = 0;
        if (pool) {
            if (miw_plan::pool_dry(w.cur)) { w.exhausted = true; --live; continue; }
            took = miw_plan::pool_take(w.cur, asking);
            for (uint32_t rank = 0; rank < took; ++rank) {
                const uint32_t id = w.cur.next + rank;
                CHECK(id < job_total);
                if (id < job_total) { CHECK(served[id] == 0); served[id]++; }
                CHECK(w.ring[miw_plan::pool_ring_slot(id, MIW_POOL_MAX)] == id);       // the slot a lane reads is the one its batch wrote
                ++from_pool;
            }
            const JobCursor after = miw_plan::pool_after(w.cur, asking);
            CHECK(after.next == w.cur.next + took && after.end == w.cur.end && after.next <= after.end);
            w.cur = after;
        }
        if (took < asking) {                                    // the others draw for themselves: one add of their count
            const uint32_t base = queue; queue += asking - took;
            for (uint32_t rank = 0; rank < asking - took; ++rank) {
                const uint32_t id = base + rank;
                // (that lane is exhausted. Without a pool the model retires its wavefront; with one, the wavefront's other lanes go on asking until a batch comes back dry)
                if (id >= job_total) { ++beyond; if (!pool && !w.exhausted) { w.exhausted = true; --live; } continue; }
                CHECK(served[id] == 0); served[id]++;
            }
        }
        // (the device draws at the top of the next trip: the cursor is empty, the queue not known to be dry)
        if (pool && !w.exhausted && miw_plan::pool_empty(w.cur) && !miw_plan::pool_dry(w.cur)) draw_batch(w, queue, pool, job_total);
    }
    for (Wave &w : W) if (pool) CHECK(miw_plan::pool_dry(w.cur));         // no wavefront retires with ids in its cursor
    unsigned long long once = 0;
    for (uint32_t id = 0; id < job_total; ++id) once += served[id] == 1;
    CHECK(once == job_total);
    printf("C %u %u %u %llu %llu %llu %llu\n", job_total, pool, waves, once, asks, from_pool, beyond);
}

// ---- progress ----
struct Lane { int state = 0; uint32_t id = 0, left = 0; };       // 0: asking, 1: parked with id, 2: running id for `left` more trips, 3: exhausted
struct PWave { JobCursor cur{ 0u, 0u }; Lane lane[64]; };

static void progress(uint32_t n_lanes, uint32_t chunks, uint32_t pool, uint32_t waves) {
    const uint32_t job_total = n_lanes * chunks;
    std::vector<uint32_t> done(n_lanes, 0), runs(job_total, 0);
    std::vector<PWave> W(waves);
    uint32_t queue = 0; unsigned long long trips = 0, parks = 0, finished = 0;
    auto length = [&](uint32_t j) { const uint32_t l = 8u >> j; return l ? l : 1u; };       // halving chunks: 8, 4, 2, 1, 1 trips
    auto ready = [&](uint32_t id) { return done[id % n_lanes] == id / n_lanes; };
    auto held = [&](const PWave &w) {                           // the largest id the wavefront holds, + 1 (0: none)
        uint32_t m = 0;
        if (pool && !miw_plan::pool_dry(w.cur) && !miw_plan::pool_empty(w.cur)) m = w.cur.end;
        for (const Lane &l : w.lane) if ((l.state == 1 || l.state == 2) && l.id + 1u > m) m = l.id + 1u;
        return m;
    };
    // one trip of a wavefront; false: nothing changed
    auto trip = [&](PWave &w) {
        bool changed = false;
        // fetch_job: the lanes that ask — fresh ones from the cursor, the rest of them drawing for themselves; parked ones look at their job again
        uint32_t fresh = 0;
        for (Lane &l : w.lane) fresh += l.state == 0;
        uint32_t took = 0, base = 0;
        const bool dry = pool && miw_plan::pool_dry(w.cur);
        if (fresh && pool && !dry) { took = miw_plan::pool_take(w.cur, fresh); base = w.cur.next; w.cur = miw_plan::pool_after(w.cur, fresh); }
        uint32_t own = 0;
        if (fresh > took && !dry) { own = queue; queue += fresh - took; }
        uint32_t rank = 0;
        for (Lane &l : w.lane) {
            if (l.state == 0) {
                changed = true;
                if (dry) { l.state = 3; continue; }
                l.id = rank < took ? base + rank : own + (rank - took); ++rank;
                if (l.id >= job_total) { l.state = 3; continue; }
                l.state = 1;
            }
            if (l.state == 1) {
                if (ready(l.id)) { l.state = 2; l.left = length(l.id / n_lanes); CHECK(runs[l.id] == 0); runs[l.id]++; changed = true; }
                else ++parks;
            }
        }
        // the body: running lanes advance; tick() at its top draws a batch when the cursor is empty
        bool running = false;
        for (Lane &l : w.lane) running |= l.state == 2;
        if (running && pool && miw_plan::pool_empty(w.cur) && !miw_plan::pool_dry(w.cur)) { const uint32_t b = queue; queue += pool; w.cur = miw_plan::pool_batch(b, pool, job_total); changed = true; }
        for (Lane &l : w.lane) if (l.state == 2) {
            changed = true;
            if (--l.left == 0) { done[l.id % n_lanes]++; ++finished; l.state = 0; }
        }
        return changed;
    };
    bool stuck = false;
    for (PWave &w : W) trip(w);                                 // the launch starts every wavefront: each draws before any job has finished
    for (;;) {
        if (++trips > 50000000ull) { stuck = true; break; }
        // the adversary: the wavefront holding the largest id first; the next one only where that trip would change nothing
        std::vector<uint32_t> order(waves);
        for (uint32_t i = 0; i < waves; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return held(W[a]) > held(W[b]); });
        bool moved = false;
        for (uint32_t i : order) if (trip(W[i])) { moved = true; break; }
        if (!moved) break;
    }
    bool all_out = true;
    for (const PWave &w : W) for (const Lane &l : w.lane) all_out &= l.state == 3;
    unsigned long long once = 0;
    for (uint32_t id = 0; id < job_total; ++id) once += runs[id] == 1;
    CHECK(!stuck); CHECK(all_out); CHECK(once == job_total && finished == job_total);
    for (uint32_t s = 0; s < n_lanes; ++s) CHECK(done[s] == chunks);
    printf("P %u %u %u %u %llu %llu %d %d\n", n_lanes, chunks, pool, waves, once, parks, (int) stuck, (int) all_out);
}

int main() {
    const uint32_t totals[] = { 1u, 63u, 64u, 65u, 1000u, 8294400u }, pools[] = { 0u, 8u, 16u, 32u };
    // MIW_JOB_POOL as given -> the pool
    const int given[] = { -1, 0, 1, 2, 3, 8, 16, 24, 32, 64, 65, 128 };
    for (int g : given) printf("S %d %u\n", g, miw_plan::pool_size(g));
    for (uint32_t p : pools) printf("B %u %u %u\n", p, miw_plan::pool_wave_bytes(p), miw_plan::pool_lds_bytes(p, 4u));
    // a batch at and around job_total, then `asking` lanes at its cursor: base pool job_total asking -> next end dry take next-after slot-of-next
    const uint32_t batches[][4] = { { 0, 32, 192, 1 }, { 160, 32, 192, 64 }, { 176, 32, 192, 3 }, { 191, 32, 192, 2 }, { 192, 32, 192, 1 }, { 200, 8, 192, 5 }, { 0, 8, 1, 64 },
                                    { 8294368, 32, 8294400, 40 }, { 8294392, 16, 8294400, 7 }, { 4294967200u, 32, 4294967295u, 64 } };
    for (const uint32_t *b : batches) {
        const JobCursor c = miw_plan::pool_batch(b[0], b[1], b[2]), a = miw_plan::pool_after(c, b[3]);
        printf("T %u %u %u %u %u %u %d %u %u %u\n", b[0], b[1], b[2], b[3], c.next, c.end, (int) miw_plan::pool_dry(c), miw_plan::pool_take(c, b[3]), a.next, miw_plan::pool_ring_slot(c.next, b[1]));
    }
    for (uint32_t t : totals) for (uint32_t p : pools) for (uint32_t w = 1; w <= 40u; ++w) coverage(t, p, w);
    for (uint32_t n : { 64u, 320u }) for (uint32_t c = 2; c <= 5u; ++c) for (uint32_t p : pools) for (uint32_t w : { 1u, 2u, n / 64u, n / 64u + 3u }) progress(n, c, p, w);
    printf("violations %llu\n", violations);
    return violations ? 1 : 0;
}
