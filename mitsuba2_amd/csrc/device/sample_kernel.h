// mi_sample: SamplingIntegrator::sample for caller-supplied rays — k_sample_rays and its ray queue.
// Part of the single translation unit csrc/miwave.hip (included there, in this order; not a stand-alone header).
//
// Persistent lanes, ONE queue of ray indices (`next_ray`). Paths end at very different depths (Cornell box: 3.37 segments per
// sample on average, tails beyond 30), so a lane that finishes its ray draws the next index inside the loop
// (miw/path.h: ray_stream_sample), a wavefront at a time: the lanes that ask are counted by a ballot, their leader adds the count to
// the queue with one atomic, v_mbcnt hands every asking lane its rank. Indices drawn together are consecutive, so the SoA reads of
// those lanes and the stores of their results coalesce. The grid is sized to the device (miwave.hip: mi_sample); workgroups that
// start late find the queue empty and retire.
//
// Scene queries: the paired extension + shadow query of the resident plan (trace.h: trace2) — packet scenes out of the staged
// triangle packets and leaf boxes (Tiny = 1: 64-bit candidate masks, 2: 32-bit), tree scenes by the lock-step LDS-stack walk
// (Tiny = 0). The scene's small tables are read from global memory (the layout mi_trace launches with: no stage_tables).
struct SampleIO {
    SoaRays R;
    const float *wavelengths;         // 4 per ray (spectral builds), else unused
    uint64_t *rng_state;              // in / out
    const uint64_t *rng_inc;          // nullptr: MIW_PCG32_SCALAR_INC
    float *spec;                      // MIW_SPEC_N per ray
    uint8_t *valid;
    uint32_t n;
};

struct RayFeed {
    SampleIO io; uint32_t *next_ray; uint32_t i;
    __device__ __forceinline__ bool fetch(LaneRegs &L) {
        // (called from divergent code: the ballot counts the lanes that are here)
        const unsigned long long b = __ballot(1);
        const uint32_t me = threadIdx.x & 63u, leader = (uint32_t) __ffsll((long long) b) - 1u;
        uint32_t base = 0;
        if (me == leader) base = atomicAdd(next_ray, (uint32_t) __popcll(b));
        base = (uint32_t) __shfl((int) base, (int) leader, 64);
        i = base + __builtin_amdgcn_mbcnt_hi((uint32_t) (b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) b, 0u));
        if (i >= io.n) return false;
        const SoaRays &R = io.R;
        L.ray.o = v3(R.ox[i], R.oy[i], R.oz[i]); L.ray.d = v3(R.dx[i], R.dy[i], R.dz[i]);
        L.ray.mint = R.mint[i]; L.ray.maxt = R.maxt[i];
#if MIW_SPECTRAL
        for (int k = 0; k < 4; ++k) L.wl.l[k] = io.wavelengths[4 * (size_t) i + k];
#endif
        L.rng.state = io.rng_state[i];
        L.rng.inc = io.rng_inc ? io.rng_inc[i] : MIW_PCG32_SCALAR_INC;
        return true;
    }
    __device__ __forceinline__ void store(const LaneRegs &L) const {
        const float *v = reinterpret_cast<const float *>(&L.res);
        for (int k = 0; k < MIW_SPEC_N; ++k) io.spec[(size_t) MIW_SPEC_N * i + k] = v[k];
        io.valid[i] = (L.flags & LF_VALID_RAY) ? 1 : 0;
        io.rng_state[i] = L.rng.state;
    }
};

// Wavefronts per SIMD: what the resident kernels of the same class are compiled for (resident_kernel.h), except that the
// plain-diffuse packet kernel stays at four (128 registers, no scratch).
template <int Tiny, int Mats, bool Analytic, uint32_t Integ>
__global__ __launch_bounds__(MIW_BLOCK, Integ == INTEG_DIRECT ? MIW_DIRECT_WAVES : Tiny ? 4 : MIW_TREE_WAVES)
void k_sample_rays(RenderParams P, SceneView sc, SampleIO io, TraceLds cfg, uint32_t *next_ray) {
    extern __shared__ uint4 smem[];
    stage_to_lds(sc, cfg, smem);
    auto tr2 = [&](V3 o, float mint, V3 dE, float maxtE, bool hasE, V3 dS, float maxtS, bool hasS, F4 &hE, bool &occS) {
        trace2<Tiny, Analytic>(sc, cfg, smem, o, mint, dE, maxtE, hasE, dS, maxtS, hasS, hE, occS);
    };
    RayFeed feed; feed.io = io; feed.next_ray = next_ray; feed.i = 0;
    if constexpr (Integ == INTEG_DIRECT) ray_stream_sample_direct<Mats, Analytic>(P, sc, feed, tr2, (LaneCounters *) nullptr);
    else ray_stream_sample<Mats, Analytic>(P, sc, feed, tr2, (LaneCounters *) nullptr);
}
