"""SamplingIntegrator::sample for caller-supplied rays (mi_sample, k_sample_rays) on the GPU.

The oracle check: the checker's float64 film of a small box-filter job is reassembled from mi_sample results (sample_harness.py —
proved on the CPU by test_integrator_sample.py) and must come out BIT FOR BIT, all five channels, every texel. Sample j + 1 of a
pixel starts from the sampler state mi_sample returned for sample j, so a wrong returned state is a wrong film; the state after
the last sample is checked by running the chain one sample further against the checker's film of spp + 1."""
import ctypes as C

import numpy as np
import pytest

import sample_harness as H

pytestmark = pytest.mark.gpu

W, HGT, SPP = H.GPU_W, H.GPU_H, H.GPU_SPP
SCENES, INTEGRATORS = H.GPU_SCENES, H.GPU_INTEGRATORS


def _scene(scenes, which, spp):
    return H.gpu_scene(scenes, which, spp)


def _integrator(api, kind, kw):
    return api.PathIntegrator(**kw) if kind == "path" else api.DirectIntegrator(**kw)


def _host_fn(dev, cfg):
    def fn(o, d, mint, maxt, wl, state):
        return dev.sample(o, d, state, mint, maxt, wavelengths=wl, cfg=cfg)
    return fn


def _device_fn(dev, cfg):
    import torch

    def fn(o, d, mint, maxt, wl, state):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        rays = [t(o[:, k]) for k in range(3)] + [t(d[:, k]) for k in range(3)] + [t(mint), t(maxt)]
        st = t(state.view(np.int64))
        spec, valid = dev.sample_device(rays, st, wavelengths=None if wl is None else t(wl), cfg=cfg)
        return spec.cpu().numpy(), valid.cpu().numpy() != 0, st.cpu().numpy().view(np.uint64)
    return fn


def _check_films(oracle, job6, job7, want6, want7, fn, spectral=False):
    films = [f.copy() for f in H.chain(oracle, job7, fn, SPP + 1, spectral=spectral)]
    for got, want, what in ((films[SPP - 1], want6, "spp"), (films[SPP], want7, "spp + 1")):
        bad = got.view(np.uint64) != want.view(np.uint64)
        assert not bad.any(), "%s: %d of %d film words differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


@pytest.mark.parametrize("kind,ikw", INTEGRATORS, ids=["path", "path_d3_rr2", "direct_1_1", "direct_2_0"])
@pytest.mark.parametrize("which", SCENES)
def test_gpu_sample_reassembles_the_checkers_film_bit_exact(native, oracle, which, kind, ikw):
    from mitsuba2_amd import scenes, _capi
    scene, sensor6 = _scene(scenes, which, SPP)
    sensor7 = scenes.cornell_sensor(W, HGT, SPP + 1, seed=H.BASE_SEED, rfilter="box")
    integ = _integrator(native, kind, ikw)
    job6, job7 = integ.render_job(sensor6), integ.render_job(sensor7)
    _, want6, _ = oracle.render(scene.desc(), job6, threads=8, want_f64=True)
    _, want7, _ = oracle.render(scene.desc(), job7, threads=8, want_f64=True)
    assert H.every_sample_in_its_texel(want6, SPP) and H.every_sample_in_its_texel(want7, SPP + 1)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):         # the scene's own route (packets for the small boxes), and the tree walk forced
            dev.upload(scene.desc(), quality)
            for fn in (_host_fn(dev, cfg), _device_fn(dev, cfg)):
                _check_films(oracle, job6, job7, want6, want7, fn)
    finally:
        dev.close()


def test_gpu_sample_spectral_glass_block_bit_exact(spectral, oracle_spectral):
    from mitsuba2_amd import scenes, _capi
    scene, sensor6 = _scene(scenes, "glass_block", SPP)
    sensor7 = scenes.cornell_sensor(W, HGT, SPP + 1, seed=H.BASE_SEED, rfilter="box")
    integ = spectral.PathIntegrator()
    job6, job7 = integ.render_job(sensor6), integ.render_job(sensor7)
    _, want6, _ = oracle_spectral.render(scene.desc(), job6, threads=8, want_f64=True)
    _, want7, _ = oracle_spectral.render(scene.desc(), job7, threads=8, want_f64=True)
    assert H.every_sample_in_its_texel(want6, SPP) and H.every_sample_in_its_texel(want7, SPP + 1)
    cfg = integ.sample_cfg()
    dev = spectral.Device(0)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            for fn in (_host_fn(dev, cfg), _device_fn(dev, cfg)):
                _check_films(oracle_spectral, job6, job7, want6, want7, fn, spectral=True)
        # a spectral ray without wavelengths is refused
        with pytest.raises(RuntimeError, match="needs wavelengths"):
            dev.sample([[278, 273, -800]], [[0, 0, 1]], [1], cfg=cfg)
    finally:
        dev.close()


def _camera_rays(dev, job, n, seed=11):
    """n camera rays through random film positions + a PCG32 state each"""
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2)) * [job.cfg.crop_w, job.cfg.crop_h]).astype(np.float32)
    ray = dev.eval(5, pos, cfg=job.cfg)
    state, _ = H.pcg32_seed(rng.integers(0, 2 ** 63, n, dtype=np.uint64))
    return np.ascontiguousarray(ray[:, :3]), np.ascontiguousarray(ray[:, 3:6]), np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), state


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["cornell_box", "plugin_box"])
def test_gpu_sample_sizes_order_and_chunks(native, which):
    """n = 0, 1, not a multiple of 64, and a call of more than 2^22 rays (several staged chunks, the queue drawn from millions of
    times): a ray's result depends on its own inputs only — a strided subset run alone, and the rays permuted, give the same bits."""
    from mitsuba2_amd import scenes, _capi
    scene, sensor = _scene(scenes, which, 1)
    job = native.PathIntegrator().render_job(sensor)
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            cfg = native.sample_cfg("path")
            empty = dev.sample(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.uint64), cfg=cfg)
            assert empty[0].shape == (0, 3) and len(empty[1]) == 0 and len(empty[2]) == 0
            n = (1 << 22) + 1237 if quality == 0 else 200003
            o, d, mint, maxt, state = _camera_rays(dev, job, n)
            full = dev.sample(o, d, state, mint, maxt, cfg=cfg)
            assert full[1].any() and np.isfinite(full[0]).all() and (full[2] != state).any()
            for idx in (np.arange(0, n, 4099), np.array([n - 1]), np.arange(1000, 1000 + 777)):
                part = dev.sample(o[idx], d[idx], state[idx], mint[idx], maxt[idx], cfg=cfg)
                assert _same(part, [x[idx] for x in full]), len(idx)
            perm = np.random.default_rng(3).permutation(n)
            shuffled = dev.sample(o[perm], d[perm], state[perm], mint[perm], maxt[perm], cfg=cfg)
            assert _same(shuffled, [x[perm] for x in full])
    finally:
        dev.close()


def test_gpu_sample_host_class_route_and_no_state_left_behind(native):
    """integrator.sample(scene, ...) (host class) == Device.sample (C ABI), ray by ray and batched, with the sampler advanced to the
    returned state; mi_render gives the same film before and after mi_sample calls; MI_ERR_STATE before mi_bvh_build."""
    from mitsuba2_amd import scenes, _capi
    scene, sensor = scenes.plugin_box(W, HGT, 4, device=0)
    for integ in (native.PathIntegrator(max_depth=6, rr_depth=3), native.DirectIntegrator(emitter_samples=2, bsdf_samples=1)):
        dev = native.Device(0)
        try:
            cfg = integ.sample_cfg()
            r = native.mi_rays_soa()
            assert dev.L.mi_sample(dev.ctx, C.byref(cfg), C.byref(r), None, None, None, None, None, 4) == _capi.MI_ERR_INVALID
            one = np.zeros(1, np.float32); st = np.zeros(1, np.uint64); spec = np.zeros(3, np.float32); valid = np.zeros(1, np.uint8)
            p = lambda a: C.c_void_p(a.ctypes.data)
            assert dev.L.mi_sample(dev.ctx, C.byref(cfg), C.byref(r), None, p(st), None, p(spec), p(valid), 1) == _capi.MI_ERR_STATE
            dev.upload(scene.desc())
            job = integ.render_job(sensor)
            before, st0 = dev.render(job)
            o, d, mint, maxt, state = _camera_rays(dev, job, 3001)
            abi = dev.sample(o, d, state, mint, maxt, cfg=cfg)
            after, st1 = dev.render(job)
            assert st0 == 0 and st1 == 0 and np.array_equal(before.view(np.uint32), after.view(np.uint32))
            batch = integ.sample_batch(scene, o, d, state, mint, maxt)
            assert _same(batch, abi)
            sampler = native.Sampler(sample_count=1)
            _, inc = sampler.state()
            for i in range(0, 3001, 500):
                sampler.set_state(int(state[i]), inc)
                spec, valid = integ.sample(scene, sampler, np.concatenate([o[i], d[i], [mint[i], maxt[i]]]))
                assert np.array_equal(spec.view(np.uint32), abi[0][i].view(np.uint32)) and valid == abi[1][i]
                assert sampler.state() == (int(abi[2][i]), inc)
        finally:
            dev.close()


def test_gpu_sample_custom_increment_without_draws(native):
    """rng_inc: with max_depth = 1 the integrator draws nothing, so every state comes back unchanged whatever the stream — and with
    draws, the default stream passed explicitly is the default."""
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, "cornell_box", 1)
    job = native.PathIntegrator().render_job(sensor)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        o, d, mint, maxt, state = _camera_rays(dev, job, 1000)
        inc = np.random.default_rng(9).integers(0, 2 ** 63, 1000, dtype=np.uint64) | np.uint64(1)
        spec, valid, after = dev.sample(o, d, state, mint, maxt, rng_inc=inc, cfg=native.sample_cfg("path", max_depth=1))
        assert np.array_equal(after, state) and valid.any()
        a = dev.sample(o, d, state, mint, maxt, cfg=native.sample_cfg("path"))
        b = dev.sample(o, d, state, mint, maxt, rng_inc=np.full(1000, H.SCALAR_INC, np.uint64), cfg=native.sample_cfg("path"))
        c = dev.sample(o, d, state, mint, maxt, rng_inc=inc, cfg=native.sample_cfg("path"))
        assert _same(a, b) and (a[2] != state).any() and not np.array_equal(a[2], c[2])
    finally:
        dev.close()
