"""Point, spot, directional and constant emitters on the GPU (MATS_LIGHTS kernels).

The CPU checker cannot render a shapeless emitter, so nothing here compares against its film. The yardsticks are the float64
restatement of tests/f64_lights.py through mi_sample (k_sample_rays: packet route and forced tree walk), closed forms of the
direct integrator, the scene query surface against the same restatement, and the refusals that need a device."""
import math

import numpy as np
import pytest

import f64_integrators as F
import f64_lights as FL
from test_independent_integrators import RTOL, report
import sample_harness as H
from test_independent_integrators import xyz_of
from test_lights import restated, spectral_restated

LOCKSTEP, PHASED, POOLED = 1, 2, 3                # MI_PATH_KERNEL_*

pytestmark = pytest.mark.gpu


# ---- 1. mi_sample against the float64 restatement ---------------------------------------------------------------------------------
def _host(dev, cfg, ray, state):
    o, d = np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6])
    return dev.sample(o, d, state, np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), cfg=cfg)


def _device(dev, cfg, ray, state):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = t(state.view(np.int64))
    spec, valid = dev.sample_device([t(ray[:, k]) for k in range(8)], st, cfg=cfg)
    return spec.cpu().numpy(), valid.cpu().numpy() != 0, st.cpu().numpy().view(np.uint64)


def _check(name, res, call):
    for j in range(FL.JOB_SPP):
        spec, valid, after = call(res["ray"][j], res["state_before"][j].copy())
        checked, bad, dev = F.compare(spec, valid, res, j, RTOL, to_xyz=False)
        msg = report(name, res, checked, dev)
        print("sample %d: %s" % (j, msg))
        assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            pytest.fail("%s\nsample %d: %d rays differ; first: pixel (%d, %d): device %s valid %s, restatement %s valid %s, margin %.3g (%s)"
                        % (msg, j, bad.sum(), res["px"][i], res["py"][i], spec[i], valid[i], res["L"][j, i], res["valid"][j, i], res["margin"][j, i], res["what"][j][i]))
        wrong = checked & (after != res["state_after"][j])
        assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count; first: ray %d, %d draws" % (
            msg, j, wrong.sum(), np.flatnonzero(wrong)[0], res["n_draws"][j, np.flatnonzero(wrong)[0]])


@pytest.mark.parametrize("name", list(FL.JOBS))
def test_gpu_sample_against_float64_restatement(native, oracle, name):
    """the scene's own route (packet kernels: the boxes hold at most 64 triangles) and the forced tree walk, each through host
    arrays and through arrays resident on the device; L, valid and the sampler state after every ray"""
    from mitsuba2_amd import _capi
    scene, integ, job, res = restated(name, native, oracle)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            _check(name, res, lambda ray, st: _host(dev, cfg, ray, st))
            _check(name, res, lambda ray, st: _device(dev, cfg, ray, st))
    finally:
        dev.close()


# ---- 2. closed forms of the direct integrator ---------------------------------------------------------------------------------------
RHO = (0.5, 0.25, 0.75)


def _floor(native, half=4.0):
    v = np.array([[-half, 0, -half], [-half, 0, half], [half, 0, half], [half, 0, -half]], np.float32)      # normal +y
    return native.Mesh("floor", v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), bsdf=native.BSDF("diffuse", reflectance=RHO))


def _rays_down(n, seed):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-3, 3, n), np.full(n, 5.0), rng.uniform(-3, 3, n)], 1).astype(np.float32)
    t = np.stack([rng.uniform(-3.5, 3.5, n), np.zeros(n), rng.uniform(-3.5, 3.5, n)], 1)
    d = t - o
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    return o, d


def _direct(native, scene, o, d, quality, **kw):
    cfg = native.DirectIntegrator(**kw).sample_cfg()
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), quality)
        state = np.arange(1, len(o) + 1, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
        spec, valid, _ = dev.sample(o, d, state, np.zeros(len(o), np.float32), np.full(len(o), np.inf, np.float32), cfg=cfg)
        si = dev.ray_intersect(o, d)
    finally:
        dev.close()
    return spec.astype(np.float64), valid, si


EPS32 = 2.0 ** -23       # the closed-form bounds below are in float32 epsilons, relative: twice the largest deviation measured on the MI355X


@pytest.mark.parametrize("quality", [0, 0x11])
def test_point_light_over_a_diffuse_floor_is_the_closed_form(native, quality):
    """direct, emitter_samples = 1, bsdf_samples = 0: every result is rho / pi * I * cos(theta) / d^2 from the hit point, in float64.
    The device evaluates it in about a dozen correctly rounded float32 operations (d = p_light - p, its norm and reciprocal, the
    frame's dot product, the products with rho / pi, cos and I / d^2). Largest relative deviation measured over the 512 rays, on
    both routes: 3.86 float32 epsilons (4.6e-7); the bound is twice that, 7.72 epsilons. The test prints what it sees."""
    I, P = np.array([30.0, 20.0, 10.0]), np.array([0.5, 3.0, -0.25])
    scene = native.Scene([_floor(native)], lights=[native.PointLight(position=tuple(P), intensity=tuple(I))]).build(-1)
    o, d = _rays_down(512, 3)
    spec, valid, si = _direct(native, scene, o, d, quality, emitter_samples=1, bsdf_samples=0)
    assert valid.all()
    p = si["p"].astype(np.float64)
    v = P - p
    d2 = (v * v).sum(1)
    cos = v[:, 1] / np.sqrt(d2)
    want = np.array(RHO, np.float32).astype(np.float64)[None, :] / math.pi * I[None, :] * (cos / d2)[:, None]
    rel = np.abs(spec - want) / want
    print("point: largest relative deviation %.3g = %.2f float32 epsilons" % (rel.max(), rel.max() / EPS32))
    assert rel.max() <= 7.72 * EPS32


@pytest.mark.parametrize("quality", [0, 0x11])
def test_directional_light_over_a_diffuse_floor_is_the_closed_form(native, quality):
    """rho / pi * E * cos(theta), the same for every hit point. Largest relative deviation measured, on both routes: 0.60 float32
    epsilons (7.16e-8); the bound is twice that, 1.2 epsilons."""
    E, D = np.array([3.0, 2.0, 1.0]), np.array([0.0, -0.8, 0.6])
    scene = native.Scene([_floor(native)], lights=[native.DirectionalEmitter(direction=tuple(D), irradiance=tuple(E))]).build(-1)
    o, d = _rays_down(512, 4)
    spec, valid, si = _direct(native, scene, o, d, quality, emitter_samples=1, bsdf_samples=0)
    assert valid.all()
    want = np.array(RHO, np.float32).astype(np.float64) / math.pi * E * 0.8
    rel = np.abs(spec - want[None, :]) / want[None, :]
    print("directional: largest relative deviation %.3g = %.2f float32 epsilons" % (rel.max(), rel.max() / EPS32))
    assert rel.max() <= 1.2 * EPS32


@pytest.mark.parametrize("quality", [0, 0x11])
def test_a_miss_returns_the_constant_radiance_bit_for_bit(native, quality):
    """an open scene: rays that leave it return the radiance exactly (direct.cpp:119-123 on a miss), valid = false; with
    hide_emitters they return zero"""
    R = (0.3, 0.7, 1.1)
    scene = native.Scene([_floor(native)], lights=[native.ConstantBackgroundEmitter(radiance=R)]).build(-1)
    o, d = _rays_down(256, 5)
    d = -d                                                      # upwards: every ray misses
    spec, valid, si = _direct(native, scene, o, d, quality, emitter_samples=1, bsdf_samples=0)
    assert not valid.any() and np.array_equal(spec.astype(np.float32), np.tile(np.array(R, np.float32), (256, 1)))
    assert (si["emitter_index"] == 0).all()                     # si.emitter(scene) of a miss: the constant emitter
    spec, valid, _ = _direct(native, scene, o, d, quality, emitter_samples=1, bsdf_samples=0, hide_emitters=True)
    assert not valid.any() and (spec == 0).all()
    cfg = native.PathIntegrator().sample_cfg()
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), quality)
        spec, valid, _ = dev.sample(o, d, np.arange(1, 257, dtype=np.uint64), np.zeros(256, np.float32), np.full(256, np.inf, np.float32), cfg=cfg)
    finally:
        dev.close()
    assert not valid.any() and np.array_equal(spec, np.tile(np.array(R, np.float32), (256, 1)))


# ---- 4. the scene query surface ---------------------------------------------------------------------------------------------------------
def test_scene_queries_on_the_new_types(native):
    """mi_sample_emitter_direction / mi_pdf_emitter_direction / mi_emitter_eval per emitter of the mixed scene and of each lit box
    against the restatement; the visibility test on a point light behind the short block"""
    from mitsuba2_amd import _capi, scenes
    rng = np.random.default_rng(11)
    n = 64
    for which in ("point", "spot", "directional", "constant", "mixed"):
        scene, _ = FL.job_scene(scenes, which, 1)
        s64 = FL.from_api_scene(scene)
        ref = np.stack([rng.uniform(60, 500, n), rng.uniform(20, 400, n), rng.uniform(60, 500, n)], 1).astype(np.float32)
        smp = rng.random((n, 2)).astype(np.float32)
        dev = native.Device(0)
        try:
            dev.upload(scene.desc(), 0)
            for e, em in enumerate(s64.emitters):
                ds, spec = dev.sample_emitter_direction(ref, smp, test_visibility=False, emitter=e)
                pdf = dev.pdf_emitter_direction(ref, ds, emitter=e)
                if isinstance(em, FL._Light):                # Endpoint::eval: the radiance for constant, zero for the delta lights
                    si = np.zeros(4, _capi.SI_DTYPE)
                    si["emitter_index"] = e; si["wi"] = (0, 0, 1); si["t"] = np.inf
                    got = dev.emitter_eval(si)
                    want = em.eval_direction(np.array([0.0, 0.0, -1.0]))
                    assert np.array_equal(np.asarray(got, np.float32), np.tile(np.asarray(want, np.float32), (4, 1))), (which, e, got, want)
                    assert (np.asarray(want) > 0).all() == isinstance(em, FL.Constant)
                for i in range(n):
                    M = F.Margin()
                    d, dist, p, val, nrm = em.sample_direction(ref[i].astype(np.float64), smp[i].astype(np.float64), M)
                    if M.value < 1.0:
                        continue
                    assert np.allclose(ds["d"][i], d, atol=2e-6) and abs(ds["dist"][i] - dist) <= 2e-6 * dist and abs(ds["pdf"][i] - p) <= 1e-5 * max(p, 1e-30), (which, e, i)
                    # (a spot's falloff goes to zero at the cutoff: the absolute bound is relative to the unattenuated intensity / d^2)
                    peak = float(np.abs(em.radiance).max()) / dist ** 2 if isinstance(em, (FL.Point, FL.Spot)) else float(np.abs(val).max())
                    assert np.allclose(spec[i], val, rtol=2e-4, atol=1e-5 * peak + 1e-30), (which, e, i, spec[i], val)
                    assert ds["emitter_index"][i] == e
                    if isinstance(em, FL._Light):
                        want = em.pdf_direction(d, dist, nrm, M)
                        assert abs(pdf[i] - want) <= 1e-6 * max(want, 1e-30), (which, e, i)      # 0 for the delta lights, 1 / (4 pi) for constant
        finally:
            dev.close()
    # visibility: a point light seen from the floor under the short block's shadow side comes back black, from the open floor lit
    scene, _ = FL.job_scene(scenes, "point", 1)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), 0)
        lit = np.array([[450.0, 0.1, 60.0]], np.float32)        # open floor: the segment to the light passes neither block
        inside = np.array([[185.0, 0.1, 169.0]], np.float32)     # on the floor inside the short block's footprint
        _, a = dev.sample_emitter_direction(lit, np.zeros((1, 2), np.float32), test_visibility=True)
        _, b = dev.sample_emitter_direction(inside, np.zeros((1, 2), np.float32), test_visibility=True)
        _, c = dev.sample_emitter_direction(inside, np.zeros((1, 2), np.float32), test_visibility=False)
        assert (a > 0).all() and (b == 0).all() and (c > 0).all()
    finally:
        dev.close()


# ---- 5. refusals, 6. no change for scenes without lights --------------------------------------------------------------------------------
def test_plan_1_and_the_pooled_kernel_refuse_lights(native):
    from mitsuba2_amd import _capi, scenes
    scene, sensor = scenes.lit_box("point", 32, 24, 1)
    integ = native.PathIntegrator()
    integ.set_plan(1)
    with pytest.raises(RuntimeError, match="point / spot / directional / constant"):
        integ.render(scene, sensor)
    scene, sensor = scenes.lit_box("point", 32, 24, 1, diffuse_only=False, ball_level=2)
    integ = native.PathIntegrator()
    integ.set_plan(0)
    assert integ.render(scene, sensor) is True
    c = integ.counters()
    assert c.plan == 2 and c.path_kernel == 1 and c.samples == 32 * 24 and np.isfinite(sensor.film.data((24, 32, 5))).all()
    job = native.PathIntegrator().render_job(sensor)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        with pytest.raises(RuntimeError, match="pooled kernel.*point / spot / directional / constant"):
            dev.render(job, path_kernel=POOLED)
        with pytest.raises(RuntimeError, match="point / spot / directional / constant"):
            dev.render(job, plan=1)
    finally:
        dev.close()


def test_upload_refusals(native):
    """records the host layer cannot produce: built by hand and handed to mi_scene_upload"""
    import copy
    import ctypes as C
    from mitsuba2_amd import _capi, scenes
    scene, _ = scenes.mixed_light_box(16, 16, 1, device=-1)
    d = scene.desc().contents
    dev = native.Device(0)

    def refused(edit, match):
        desc = _capi.mi_scene_desc.from_buffer_copy(d)
        lights = (_capi.mi_light * d.light_count)(*[_capi.mi_light.from_buffer_copy(d.lights[k]) for k in range(d.light_count)])
        desc.lights = lights
        edit(desc, lights)
        st = dev.L.mi_scene_upload(dev.ctx, C.byref(desc))
        msg = dev.L.mi_last_error(dev.ctx).decode()
        assert st == _capi.MI_ERR_INVALID and match in msg, (st, msg)
    try:
        def collide(desc, l): l[1].emitter_index = l[0].emitter_index
        refused(collide, "collides")
        def gap(desc, l): l[1].emitter_index = 7
        refused(gap, "gap")
        def two_constants(desc, l): l[0].type = _capi.MI_LIGHT_CONSTANT
        refused(two_constants, "second constant")
        def directional(desc, l): l[0].type = _capi.MI_LIGHT_DIRECTIONAL; l[0].direction[0], l[0].direction[1], l[0].direction[2] = 0.0, 0.0, 2.0
        refused(directional, "unit length")
        def spot_texture(desc, l): l[0].type = _capi.MI_LIGHT_SPOT; l[0].value_tex.type = 5
        refused(spot_texture, "texture")
        dev.upload(scene.desc(), 0)                               # the record as the host layer built it is accepted
    finally:
        dev.close()


def test_scenes_without_lights_keep_their_kernels(native):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(32, 24, 1)
    integ = native.PathIntegrator()
    assert integ.render(scene, sensor) is True
    c = integ.counters()
    assert c.plan == 2 and c.path_kernel == 0 and c.tree_width == 0          # packets, as before
    scene, sensor = scenes.cornell_box(32, 24, 1, diffuse_only=False, ball_level=2)
    integ = native.PathIntegrator()
    assert integ.render(scene, sensor) is True
    c = integ.counters()
    assert c.plan == 2 and c.path_kernel == 1 and c.tree_width == 8


# ---- 1b. the scalar_spectral job -----------------------------------------------------------------------------------------------------
def test_gpu_sample_spectral_against_float64_restatement(spectral, oracle_spectral):
    """scalar_spectral: the mixed scene (area + point + constant, srgb_d65 spectra) through spectral.Device.sample on both routes;
    both sides compared after spectrum_to_xyz in float64, the sampler state after every checked ray exactly"""
    from mitsuba2_amd import _capi
    scene, integ, job, res, model = spectral_restated(spectral, oracle_spectral)
    cfg = integ.sample_cfg()
    dev = spectral.Device(0)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            for j in range(FL.JOB_SPP):
                ray, wl = res["ray"][j], np.ascontiguousarray(res["wl"][j])
                spec, valid, after = dev.sample(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), res["state_before"][j].copy(),
                                                np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), wavelengths=wl, cfg=cfg)
                checked, bad, dv = F.compare(xyz_of(spec, wl, model.cie, False), valid, res, j, RTOL, to_xyz=False, want=xyz_of(res["L"][j], wl, model.cie, False))
                msg = report("mixed-spectral-path", res, checked, dv)
                print("sample %d: %s" % (j, msg))
                assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
                assert not bad.any(), "%s\nsample %d: %d rays differ, first ray %d: device %s, restatement %s" % (
                    msg, j, bad.sum(), np.flatnonzero(bad)[0], spec[np.flatnonzero(bad)[0]], res["L"][j, np.flatnonzero(bad)[0]])
                wrong = checked & (after != res["state_after"][j])
                assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count" % (msg, j, wrong.sum())
    finally:
        dev.close()


# ---- 3. render() against the film reassembled from chained mi_sample results ------------------------------------------------------------
RW, RH, RSPP = 32, 24, 3


def _render_scene(scenes, which, balls):
    kw = dict(device=-1, rfilter="box", seed=FL.SEED, diffuse_only=not balls, ball_level=2)
    return scenes.mixed_light_box(RW, RH, RSPP, **kw) if which == "mixed" else scenes.lit_box(which, RW, RH, RSPP, **kw)


def _reassembled(oracle, dev, job, cfg):
    """-> (float64 film, float32 film) of the job from chained mi_sample results of `dev`: the float64 film sums every texel's
    samples exactly; the float32 film adds them in sample order in float32, as ImageBlock::put does. The checker serves camera
    rays and the X Y Z fused multiply-adds only (no scene is handed to it)."""
    fn = lambda o, d, mint, maxt, wl, state: dev.sample(o, d, state, mint, maxt, cfg=cfg)
    films = [f.copy() for f in H.chain(oracle, job, fn, RSPP)]
    f32 = np.zeros(films[0].shape, np.float32)
    prev = np.zeros_like(films[0])
    for f in films:
        sample = f - prev
        assert np.array_equal(sample.astype(np.float32).astype(np.float64), sample)      # one float32 sample per texel
        f32 = f32 + sample.astype(np.float32)
        prev = f
    return films[-1], f32


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


@pytest.mark.parametrize("kind,ikw", [("path", dict()), ("direct", dict(emitter_samples=1, bsdf_samples=1))], ids=["path", "direct"])
@pytest.mark.parametrize("which", ["point", "mixed"])
def test_render_equals_the_reassembled_film_on_packets_and_the_lock_step_tree(native, oracle, which, kind, ikw):
    """k_path_resident<MATS_LIGHTS>: packets (the box's 30-odd triangles) and the lock-step tree walk (MI_BVH_FORCE_TREE), logging
    film (film_mode 1: bit for bit) and float64-atomics film (film_mode 2: equal after rounding to float32 — largest distance
    seen on the MI355X: 0 ulps), path and direct"""
    from mitsuba2_amd import _capi, scenes
    scene, sensor = _render_scene(scenes, which, False)
    integ = (native.PathIntegrator if kind == "path" else native.DirectIntegrator)(**ikw)
    job, cfg = integ.render_job(sensor), integ.sample_cfg()
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            want64, want32 = _reassembled(oracle, dev, job, cfg)
            g, st = dev.render(job, film_mode=1)
            c = dev.counters()
            assert st == 0 and c.plan == 2 and c.path_kernel == 0 and c.samples == RW * RH * RSPP
            bad = g.view(np.uint32) != want32.view(np.uint32)
            assert not bad.any(), "film_mode 1, quality %#x: %d film words differ, first at %s" % (quality, bad.sum(), np.argwhere(bad)[0])
            g, st = dev.render(job, film_mode=2, f64=True)
            u = _ulps(g.astype(np.float32), want64.astype(np.float32))
            print("%s %s quality %#x film_mode 2: largest distance %d ulps" % (which, kind, quality, u))
            assert st == 0 and u == 0
    finally:
        dev.close()


@pytest.mark.parametrize("which", ["point", "mixed"])
def test_render_equals_the_reassembled_film_on_the_phase_machine(native, oracle, which):
    """past 64 triangles (the two 320-triangle balls): k_path_phased<MATS_LIGHTS> over the 8-wide and the 4-wide tree and its
    lock-step twin through the debug_* fields, each bit for bit against the film reassembled from k_sample_rays' results"""
    from mitsuba2_amd import scenes
    scene, sensor = _render_scene(scenes, which, True)
    integ = native.PathIntegrator()
    job, cfg = integ.render_job(sensor), integ.sample_cfg()
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        want64, want32 = _reassembled(oracle, dev, job, cfg)
        for kernel, width, want_kernel, want_width in ((0, 0, 1, 8), (PHASED, 4, 1, 4), (LOCKSTEP, 0, 0, None)):
            g, st = dev.render(job, film_mode=1, path_kernel=kernel, tree_width=width)
            c = dev.counters()
            assert st == 0 and c.plan == 2 and c.path_kernel == want_kernel and (want_width is None or c.tree_width == want_width), (kernel, width, c.path_kernel, c.tree_width)
            bad = g.view(np.uint32) != want32.view(np.uint32)
            assert not bad.any(), "kernel %d width %d: %d film words differ, first at %s" % (kernel, width, bad.sum(), np.argwhere(bad)[0])
    finally:
        dev.close()
