// k_sample_volpath: VolumetricPathIntegrator::sample for caller-supplied rays (mi_sample and, through it, mi_render_sensor), and
// its launch function (device/volpath_launch.h). Compiled in csrc/miwave_volpath.hip (a split build) or in csrc/miwave.hip; not
// a stand-alone header.
//
// The launch shape of k_sample_rays (device/sample_kernel.h): persistent lanes, the wave-level ray queue (RayFeed), sampler state
// in and out, trace2 (device/trace.h) as the one scene query per loop trip — packet scenes out of the staged triangle packets
// (Tiny = 1), tree scenes by the lock-step LDS-stack walk (Tiny = 0). What runs per lane is the state machine of miw/volpath.h:
// lanes in the main loop, in an emitter walk and in a direct-light walk share a trip, each asking for at most one closest-hit
// query (hasS = false). Values are written with plain vector stores; the only atomics are the queue's counter and the counter of
// rays ended by MIW_VOLPATH_MAX_TRIPS.
//
// Wavefronts per SIMD: a lane carries more than k_sample_rays' (the medium, channel, state, the carried hit record and its ray
// origin, a walk's ray, hit record, transmittance, emitter value and distances), so the kernels are compiled for two (256
// registers) — DESIGN.md records registers, scratch and occupancy per instantiation.
#if !MIW_SPECTRAL
#ifndef MIW_VOLPATH_WAVES
#define MIW_VOLPATH_WAVES 2
#endif

template <int Tiny, int Mats, bool Analytic>
__global__ __launch_bounds__(MIW_BLOCK, MIW_VOLPATH_WAVES)
void k_sample_volpath(RenderParams P, SceneView sc, MediaView mv, SampleIO io, TraceLds cfg, uint32_t *next_ray, uint32_t *capped) {
    extern __shared__ uint4 smem[];
    stage_to_lds(sc, cfg, smem);
    auto tr2 = [&](V3 o, float mint, V3 dE, float maxtE, bool hasE, V3 dS, float maxtS, bool hasS, F4 &hE, bool &occS) {
        trace2<Tiny, Analytic>(sc, cfg, smem, o, mint, dE, maxtE, hasE, dS, maxtS, hasS, hE, occS);
    };
    RayFeed feed; feed.io = io; feed.next_ray = next_ray; feed.i = 0;
    ray_stream_sample_volpath<Mats, Analytic>(P, sc, mv, feed, tr2, capped);
}

// X(Tiny, Mats, Analytic): packet scenes and tree scenes of triangle meshes with area emitters and an environment map. Scenes with
// shapeless emitters (MATS_LIGHTS) or analytic shapes are refused by name (miwave.hip: volpath_sample_launch) until a float64 tier pins
// those routes; the state machine itself is written for them (Lights, Analytic).
#define MIW_VOLPATH_LIST(X) X(1, MATS_NESTED, false) X(0, MATS_NESTED, false)

// MI_EVAL_MEDIUM / MI_EVAL_PHASE (include/miwave.h): the leaves of miw/medium.h on the device, one work item per entry
__global__ void k_eval_medium(int op, MediaView mv, const float *in, int is, float *out, int os, uint64_t n) {
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + i * (uint64_t) is;
    float *o = out + i * (uint64_t) os;
    const MediumRec &m = mv.media[(uint32_t) a[0]];
    if (op == MI_EVAL_MEDIUM) {
        Ray ray; ray.o = v3(a[1], a[2], a[3]); ray.d = v3(a[4], a[5], a[6]); ray.mint = a[7]; ray.maxt = a[8];
        const float si_t = a[11];
        MediumInteraction mi = medium_sample_interaction(m, ray, a[9], (uint32_t) a[10]);
        o[0] = mi.t; o[1] = mi.mint; o[2] = mi.p.x; o[3] = mi.p.y; o[4] = mi.p.z;
        o[5] = mi.sigma_s.x; o[6] = mi.sigma_s.y; o[7] = mi.sigma_s.z;
        o[8] = mi.sigma_t.x; o[9] = mi.sigma_t.y; o[10] = mi.sigma_t.z;
        o[11] = mi.sigma_t.x; o[12] = mi.sigma_t.y; o[13] = mi.sigma_t.z; o[14] = mi.ts; o[15] = 0.f;
        if (si_t < mi.t) mi.t = MIW_INFINITY;                            // volpath.cpp:112
        Spec tr, pdf;
        medium_eval_tr_and_pdf(mi, si_t, tr, pdf);
        o[16] = tr.x; o[17] = tr.y; o[18] = tr.z; o[19] = pdf.x; o[20] = pdf.y; o[21] = pdf.z;
    } else {
        const V3 ray_d = v3(a[1], a[2], a[3]);
        float pdf;
        const V3 wo = phase_sample(m, ray_d, v2(a[4], a[5]), pdf);
        o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = pdf;
        o[4] = phase_eval(m, ray_d, v3(a[6], a[7], a[8]));
    }
}
hipError_t volpath_launch_eval(hipStream_t s, int op, const MediaView &mv, const float *in, int is, float *out, int os, uint64_t n) {
    hipLaunchKernelGGL(k_eval_medium, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, op, mv, in, is, out, os, n);
    return hipGetLastError();
}

unsigned volpath_waves(int) { return (unsigned) MIW_VOLPATH_WAVES; }
hipError_t volpath_launch(hipStream_t s, bool say, int tiny, int mats, bool analytic, dim3 grid, size_t lds_bytes, const RenderParams &P,
                          const SceneView &sc, const MediaView &mv, const SampleIO &io, const TraceLds &cfg, uint32_t *next_ray, uint32_t *capped) {
#define MIW_VOLPATH_LAUNCH(T, M, A) if (tiny == (T) && mats == (M) && analytic == (A)) { \
        if (say) fprintf(stderr, "[miwave] kernel launched: k_sample_volpath<" #T ", " #M ", " #A ">\n"); \
        hipLaunchKernelGGL((k_sample_volpath<T, M, A>), grid, dim3(MIW_BLOCK), lds_bytes, s, P, sc, mv, io, cfg, next_ray, capped); \
        return hipGetLastError(); }
    MIW_VOLPATH_LIST(MIW_VOLPATH_LAUNCH)
#undef MIW_VOLPATH_LAUNCH
    return hipErrorInvalidValue;
}
#endif
