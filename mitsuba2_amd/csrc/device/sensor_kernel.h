// The general sensor route's kernels: k_sensor_step, k_sensor_rays and their launch functions (device/sensor_launch.h).
// Compiled in csrc/miwave_sensor.hip (a split build) or in csrc/miwave.hip; not a stand-alone header.
//
// A frame of mi_render_sensor advances one sample per round: k_sensor_step, then k_sample_rays (mi_sample's launch, as it stands).
// A lane is a pixel of a group of tiles, seeded and mapped by k_init_pixels. k_sensor_step sits BETWEEN two k_sample_rays launches:
// in one pass over the lanes it finishes sample j - 1 (integrator.cpp:264-287: X Y Z A as lane_finish_sample forms them,
// ImageBlock::put's validity test, one log record for k_aov_film) and begins sample j (integrator.cpp:242-258: the draws of
// render_sample in the ledger's order — jitter, aperture [thinlens], time [shutter_open_time > 0], wavelength — and
// Sensor::sample_ray through miw/lens.h). What a lane carries between launches lives in HBM: the 16-byte state word, the film
// position of the sample under way and, in scalar_spectral, its wavelengths and ray weight. No LDS, no atomics; plain vector stores.
#define MIW_SENSOR_FINISH 1u
#define MIW_SENSOR_BEGIN 2u

__device__ __forceinline__ void sensor_store_ray(float *const *ray, uint32_t i, const Ray &r) {
    ray[0][i] = r.o.x; ray[1][i] = r.o.y; ray[2][i] = r.o.z; ray[3][i] = r.d.x; ray[4][i] = r.d.y; ray[5][i] = r.d.z;
    ray[6][i] = r.mint; ray[7][i] = r.maxt;
}

__global__ __launch_bounds__(MIW_BLOCK) void k_sensor_step(SensorStepArgs A, uint32_t j, uint32_t what) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= A.n_lanes) return;
    U4 st = A.st[lane];
    if (st.z & LF_DONE) {
        // a lane outside the film (integrator.cpp:201-202) draws nothing and logs nothing. k_sample_rays runs every index of its
        // SoA, so the frame's first launch hands it the ray through the film's centre, once: traced for nothing, its result never read
        if (what == MIW_SENSOR_BEGIN) {
            sensor_store_ray(A.ray, lane, sensor_sample(A.sensor, A.lens, v2(.5f, .5f), v2(.5f, .5f)));
            A.rng_state[lane] = 0ull;
#if MIW_SPECTRAL
            Wavelengths wl; Spec w;
            sample_wavelengths(.5f, wl, w);
            F4 q; q.x = wl.l[0]; q.y = wl.l[1]; q.z = wl.l[2]; q.w = wl.l[3];
            A.wl[lane] = q;
#endif
        }
        return;
    }
    PCG32 rng;
    rng.state = (uint64_t) st.x | ((uint64_t) st.y << 32); rng.inc = MIW_PCG32_SCALAR_INC;
    if (what & MIW_SENSOR_FINISH) {
        rng.state = A.rng_state[lane];                               // the sampler as the integrator's sample() left it
        const F2 pos = A.pos[lane];
#if MIW_SPECTRAL
        const F4 r4 = reinterpret_cast<const F4 *>(A.spec)[lane], w4 = A.weight[lane], l4 = A.wl[lane];
        Spec res, weight; Wavelengths wl;
        res.c[0] = r4.x; res.c[1] = r4.y; res.c[2] = r4.z; res.c[3] = r4.w;
        weight.c[0] = w4.x; weight.c[1] = w4.y; weight.c[2] = w4.z; weight.c[3] = w4.w;
        wl.l[0] = l4.x; wl.l[1] = l4.y; wl.l[2] = l4.z; wl.l[3] = l4.w;
        const V3 xyz = spectrum_to_xyz(weight * res, wl);            // integrator.cpp:266-271
#else
        const V3 xyz = srgb_to_xyz(v3(A.spec[3 * (size_t) lane], A.spec[3 * (size_t) lane + 1], A.spec[3 * (size_t) lane + 2]));   // :272-273 (ray_weight == 1)
#endif
        const float aovs[5] = { xyz.x, xyz.y, xyz.z, A.valid[lane] ? 1.f : 0.f, 1.f };
        F2 *rec = reinterpret_cast<F2 *>(A.log + ((size_t) lane * A.spp + (j - 1u)) * MIW_AOV_LOG_HEAD);
        F2 a, b, c;
        a.x = sample_is_valid(aovs, A.warn_negative != 0u) ? pos.x : __builtin_nanf(""); a.y = pos.y;   // imageblock.cpp:85-109
        b.x = aovs[0]; b.y = aovs[1]; c.x = aovs[2]; c.y = aovs[3];
        rec[0] = a; rec[1] = b; rec[2] = c;
    }
    if (what & MIW_SENSOR_BEGIN) {
        const uint32_t pixel = A.pixel[lane];
        const V2 jit = next_2d(rng);                                 // integrator.cpp:242
        F2 pos; pos.x = (float) (pixel & 0xffffu) + jit.x; pos.y = (float) (pixel >> 16) + jit.y;
        V2 aperture = v2(.5f, .5f);
        if (lens_needs_aperture_sample(A.lens)) aperture = next_2d(rng);   // :244-246
        if (A.lens.draw_time) (void) next_1d(rng);                   // :248-250 (no animated transform reads the time)
        const float wavelength_sample = next_1d(rng);               // :252, always drawn
#if MIW_SPECTRAL
        Wavelengths wl; Spec w;
        sample_wavelengths(wavelength_sample, wl, w);
        F4 q; q.x = wl.l[0]; q.y = wl.l[1]; q.z = wl.l[2]; q.w = wl.l[3];
        A.wl[lane] = q;
        q.x = w.c[0]; q.y = w.c[1]; q.z = w.c[2]; q.w = w.c[3];
        A.weight[lane] = q;
#else
        (void) wavelength_sample;
#endif
        const V2 adjusted = v2((pos.x - A.crop_f[0]) / A.crop_f[2], (pos.y - A.crop_f[1]) / A.crop_f[3]);   // :254-256
        sensor_store_ray(A.ray, lane, sensor_sample(A.sensor, A.lens, adjusted, aperture));
        A.pos[lane] = pos;
        A.rng_state[lane] = rng.state;
    }
    st.x = (uint32_t) rng.state; st.y = (uint32_t) (rng.state >> 32); st.w = j;
    A.st[lane] = st;
}

// Sensor::sample_ray for n samples (mi_sensor_sample_ray)
__global__ __launch_bounds__(MIW_BLOCK) void k_sensor_rays(SensorRaysArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const V2 pos = v2(A.position[2 * (size_t) i], A.position[2 * (size_t) i + 1]);
    const V2 aperture = A.aperture ? v2(A.aperture[2 * (size_t) i], A.aperture[2 * (size_t) i + 1]) : v2(.5f, .5f);
    sensor_store_ray(A.ray, i, sensor_sample(A.sensor, A.lens, pos, aperture));
#if MIW_SPECTRAL
    if (A.wavelength_sample) {
        Wavelengths wl; Spec w;
        sample_wavelengths(A.wavelength_sample[i], wl, w);
        for (int k = 0; k < 4; ++k) {
            if (A.wavelengths) A.wavelengths[4 * (size_t) i + k] = wl.l[k];
            if (A.weights) A.weights[4 * (size_t) i + k] = w.c[k];
        }
    }
#else
    if (A.weights) for (int k = 0; k < MIW_SPEC_N; ++k) A.weights[(size_t) MIW_SPEC_N * i + k] = 1.f;
#endif
}

// ---- launch functions (device/sensor_launch.h) ----
hipError_t sensor_launch_step(hipStream_t s, const SensorStepArgs &A, uint32_t j, bool finish, bool begin) {
    const uint32_t what = (finish ? MIW_SENSOR_FINISH : 0u) | (begin ? MIW_SENSOR_BEGIN : 0u);
    hipLaunchKernelGGL(k_sensor_step, dim3((A.n_lanes + MIW_BLOCK - 1) / MIW_BLOCK), dim3(MIW_BLOCK), 0, s, A, j, what);
    return hipGetLastError();
}
hipError_t sensor_launch_rays(hipStream_t s, const SensorRaysArgs &A) {
    hipLaunchKernelGGL(k_sensor_rays, dim3((A.n + MIW_BLOCK - 1) / MIW_BLOCK), dim3(MIW_BLOCK), 0, s, A);
    return hipGetLastError();
}
