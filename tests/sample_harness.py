"""Reassembling the checker's film from per-ray SamplingIntegrator::sample results (shared by test_integrator_sample*.py).

The checker renders whole frames and exports no per-ray sample(); so the tests rebuild everything AROUND the integrator from the
checker's own exports and compare films:

    per pixel   seed = base_seed + block_id * block_size^2 + morton_i (integrator.cpp:198), PCG32 seeded as sampler.cpp:83-96 — the
                numpy PCG32 below, because the tests need the STATE (pinned against orc_pcg32_* in a CPU test)
    per sample  jitter = next_2d, wavelength sample = next_1d (integrator.cpp:242-252), camera ray = the checker's MI_EVAL_CAMERA_RAY,
                (spectral: wavelengths and weights = orc_spectral op 2), then `sample_fn` — the integrator under test — returns
                (Spectrum, valid, sampler state after), and the state feeds sample j + 1
    to X Y Z    with the checker's fused multiply-adds (MI_EVAL_FP_SEMANTICS), not numpy's arithmetic
    film        box filter of radius 0.5: ImageBlock::put adds a sample to exactly one texel with weight 1, every texel gets the samples of
                its own pixel in sample order, so film64[texel] = sum_j (double) aovs_j — the checker's float64 film, bit for bit
A jitter component of exactly 0.0 (or lost in the float32 sum pixel + jitter) would move a sample to the neighbour texel: chain()
asserts that none occurs."""
import ctypes as C

import numpy as np

# The sampler seed of the reassembly jobs (96 x 64, up to 7 samples per pixel). Where a pixel's later samples fall depends on how many
# numbers the integrator drew for the earlier ones, so the seed is chosen per set of jobs: with this one every sample of every job of
# test_integrator_sample_gpu.py stays in its own texel — the weight channel of the checker's film is the sample count in every texel,
# which test_integrator_sample.py checks on the CPU (seeds 0, 10000 ... 40000 each put a few samples on a pixel edge in some job).
BASE_SEED = 50000
GPU_W, GPU_H, GPU_SPP = 96, 64, 6
GPU_SCENES = ["cornell_box", "plugin_box", "rect_box", "sphere_box", "open_box"]
GPU_INTEGRATORS = [("path", dict(max_depth=-1, rr_depth=5)), ("path", dict(max_depth=3, rr_depth=2)),
                   ("direct", dict(emitter_samples=1, bsdf_samples=1)), ("direct", dict(emitter_samples=2, bsdf_samples=0))]


def gpu_scene(scenes, which, spp):
    """(scene description only, sensor) of a reassembly job: box filter, BASE_SEED"""
    kw = dict(device=-1, rfilter="box", seed=BASE_SEED)
    if which == "glass_block":
        return scenes.cornell_box(GPU_W, GPU_H, spp, diffuse_only=False, ball_level=1, glass_block=True, **kw)
    return getattr(scenes, which)(GPU_W, GPU_H, spp, **kw)


def every_sample_in_its_texel(film64, spp):
    """the checker's film of a box-filter job: a sample that left its pixel's texel shows in the weight channel"""
    return bool((film64[..., 4] == spp).all())


DEFAULT_STREAM = 0xda3e39cb94b95bdb
MULT = np.uint64(0x5851f42d4c957f2d)
SCALAR_INC = np.uint64(((DEFAULT_STREAM << 1) | 1) & 0xffffffffffffffff)


def pcg32_next_u32(state, inc=SCALAR_INC):
    """-> (uint32 outputs, states after) for an array of uint64 states"""
    state = np.asarray(state, np.uint64)
    with np.errstate(over="ignore"):
        new = state * MULT + np.uint64(inc)
    xorshifted = (((state >> np.uint64(18)) ^ state) >> np.uint64(27)).astype(np.uint32)
    rot = (state >> np.uint64(59)).astype(np.uint32)
    out = (xorshifted >> rot) | (xorshifted << ((~rot + np.uint32(1)) & np.uint32(31)))
    return out, new


def pcg32_next_f32(state, inc=SCALAR_INC):
    u, new = pcg32_next_u32(state, inc)
    return ((u >> np.uint32(9)) | np.uint32(0x3f800000)).view(np.float32) - np.float32(1), new


def pcg32_seed(initstate, initseq=DEFAULT_STREAM):
    """-> (states, inc) for an array of seeds (pcg32_seed of miw/rng.h)"""
    initstate = np.asarray(initstate, np.uint64)
    inc = np.uint64(((initseq << 1) | 1) & 0xffffffffffffffff)
    state = np.zeros_like(initstate)
    _, state = pcg32_next_u32(state, inc)
    with np.errstate(over="ignore"):
        state = state + initstate
    _, state = pcg32_next_u32(state, inc)
    return state, inc


def _compact1(x):
    x = x & 0x55555555
    x = (x ^ (x >> 1)) & 0x33333333
    x = (x ^ (x >> 2)) & 0x0f0f0f0f
    x = (x ^ (x >> 4)) & 0x00ff00ff
    x = (x ^ (x >> 8)) & 0x0000ffff
    return x


def pixels_and_seeds(job):
    """every pixel of the job's crop window -> (px, py, seed): integrator.cpp:196-202"""
    cfg = job.cfg
    bs = cfg.block_size
    nbx, nby = (cfg.crop_w + bs - 1) // bs, (cfg.crop_h + bs - 1) // bs
    i = np.arange(bs * bs, dtype=np.int64)
    x, y = _compact1(i), _compact1(i >> 1)
    px, py, seed = [], [], []
    for b in range(nbx * nby):
        bx, by = b % nbx, b // nbx
        bw, bh = min(bs, cfg.crop_w - bx * bs), min(bs, cfg.crop_h - by * bs)
        keep = (x < bw) & (y < bh)
        px.append(cfg.crop_x + bx * bs + x[keep]); py.append(cfg.crop_y + by * bs + y[keep])
        seed.append(np.uint64(cfg.base_seed) + np.uint64(int(job.block_ids[b])) * np.uint64(bs * bs) + i[keep].astype(np.uint64))
    px, py, seed = np.concatenate(px), np.concatenate(py), np.concatenate(seed)
    assert len(px) == cfg.crop_w * cfg.crop_h
    return px, py, seed


def _fp_sem(oracle, a, b, c):
    """the checker's a * b and fma(a, b, c), vectorised"""
    out = oracle.eval(7, np.stack([a, b, c], 1).astype(np.float32))
    return out[:, 1], out[:, 4]


def srgb_to_xyz(oracle, rgb):
    """miw/base.h: srgb_to_xyz — per channel fma(m2, b, fma(m1, g, m0 * r))"""
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float32)
    n = len(rgb)
    zero = np.zeros(n, np.float32)
    cols = []
    for k in range(3):
        m0, m1, m2 = (np.full(n, M[k, i], np.float32) for i in range(3))
        t, _ = _fp_sem(oracle, m0, rgb[:, 0], zero)
        _, t = _fp_sem(oracle, m1, rgb[:, 1], t)
        _, t = _fp_sem(oracle, m2, rgb[:, 2], t)
        cols.append(t)
    return np.stack(cols, 1)


def _orc_spectral(oracle, op, inp, n_out):
    x = np.ascontiguousarray(inp, np.float32); out = np.zeros(n_out, np.float32)
    oracle.L.orc_spectral(op, x.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def sample_wavelengths(oracle, u):
    """orc_spectral op 2 per wavelength sample -> (wavelengths [n, 4], weights [n, 4])"""
    r = np.stack([_orc_spectral(oracle, 2, [v], 8) for v in u])
    return np.ascontiguousarray(r[:, :4]), np.ascontiguousarray(r[:, 4:])


def spectrum_to_xyz(oracle, value, wl):
    """miw/spectrum.h: spectrum_to_xyz — cie1931_xyz (orc_spectral op 0) per wavelength, products and hmean4's ((a + b) + (c + d)) * 0.25
    through the checker's own multiply / add (MI_EVAL_FP_SEMANTICS: a + b, a * b)"""
    n = len(value)
    lam, inv = np.unique(wl.reshape(-1), return_inverse=True)
    cie = np.stack([_orc_spectral(oracle, 0, [v], 3) for v in lam])[inv].reshape(n, 4, 3)
    add = lambda a, b: oracle.eval(7, np.stack([a, b, np.zeros(n, np.float32)], 1).astype(np.float32))[:, 0]
    mul = lambda a, b: oracle.eval(7, np.stack([a, b, np.zeros(n, np.float32)], 1).astype(np.float32))[:, 1]
    cols = []
    for k in range(3):
        p = [mul(cie[:, i, k], value[:, i]) for i in range(4)]
        cols.append(mul(add(add(p[0], p[1]), add(p[2], p[3])), np.full(n, 0.25, np.float32)))
    return np.stack(cols, 1)


def chain(oracle, job, sample_fn, n_samples, spectral=False):
    """Runs n_samples camera samples of every pixel through sample_fn(o [n, 3], d [n, 3], mint [n], maxt [n], wavelengths [n, 4] | None,
    rng_state [n] uint64) -> (Spectrum [n, N], valid [n], rng_state after [n]) and yields after every sample j the float64 film
    [crop_h, crop_w, 5] accumulated so far (a view: copy it to keep it)."""
    cfg = job.cfg
    # (the box filter's radius is 0.5 + the ray epsilon, like the reference's: still ImageBlock::put's one-texel branch)
    assert cfg.filter_border == 0 and 0.5 <= cfg.filter_radius < 0.5002, "the reassembly holds for the box filter of radius 0.5"
    px, py, seed = pixels_and_seeds(job)
    n = len(px)
    state, inc = pcg32_seed(seed)
    assert inc == SCALAR_INC
    film = np.zeros((cfg.crop_h, cfg.crop_w, 5), np.float64)
    ty, tx = py - cfg.crop_y, px - cfg.crop_x
    for j in range(n_samples):
        jx, state = pcg32_next_f32(state)
        jy, state = pcg32_next_f32(state)
        wsample, state = pcg32_next_f32(state)
        pos = np.stack([px.astype(np.float32) + jx, py.astype(np.float32) + jy], 1)
        # the texel is ceil(position - 1): a jitter of exactly 0.0 — or one so small that the float32 sum is the pixel's own coordinate —
        # puts the sample into the neighbour texel. Deterministic per seed: a job for which this fires needs another base seed.
        assert (jx != 0).all() and (jy != 0).all() and (pos[:, 0] > px).all() and (pos[:, 1] > py).all(), "a sample falls on its pixel's edge: pick another seed"
        ray = oracle.eval(5, pos, cfg=cfg)
        wl = weight = None
        if spectral:
            wl, weight = sample_wavelengths(oracle, wsample)
        spec, valid, state = sample_fn(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), np.ascontiguousarray(ray[:, 6]),
                                       np.ascontiguousarray(ray[:, 7]), wl, state)
        spec = np.asarray(spec, np.float32); state = np.asarray(state, np.uint64)
        if spectral:
            zero = np.zeros(n, np.float32)
            weighted = np.stack([_fp_sem(oracle, weight[:, i], spec[:, i], zero)[0] for i in range(4)], 1)
            xyz = spectrum_to_xyz(oracle, weighted, wl)
        else:
            xyz = srgb_to_xyz(oracle, spec)
        aovs = np.concatenate([xyz, np.asarray(valid, bool).astype(np.float32)[:, None], np.ones((n, 1), np.float32)], 1)
        film[ty, tx] += aovs.astype(np.float64)                  # (every pixel once per sample: no repeated index)
        yield film


def first_hit_emission(oracle, desc):
    """PathIntegrator::sample with max_depth = 1 out of the checker's scene queries: emitter->eval(si) of the first hit, valid = a hit,
    no random number drawn (path.cpp:121-149)."""
    def fn(o, d, mint, maxt, wl, state):
        si = oracle.ray_intersect(desc, o, d, mint, maxt)
        return oracle.emitter_eval(desc, si, wavelengths=wl), np.isfinite(si["t"]), state
    return fn
