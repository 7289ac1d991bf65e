"""The volpath integrator, the tier that needs no GPU: the float64 restatement of tests/f64_volpath.py pinned by closed forms, the
conditions of the jobs the GPU tier compares against it, the host leaves (the host compile of csrc/miw/medium.h) against the
restatement's leaves, the records the classes flatten into, and the ABI mirrors."""
import ctypes as C
import math

import numpy as np
import pytest

import f64_integrators as F
import f64_nested_bsdfs as N
import f64_volpath as V
import sample_harness as H

_cache = {}


def restated(name, native, oracle):
    """the restatement of job `name`, once per session (the GPU tier reads the same results) -> (scene, integ, job, res)"""
    if name not in _cache:
        from mitsuba2_amd import scenes
        which, kw, seed = V.JOBS[name]
        scene, sensor = V.job_scene(scenes, which, F.JOB_SPP, seed)
        integ = native.VolPathIntegrator(**kw)
        job = integ.render_job(sensor)
        V.PANES.clear()
        with np.errstate(all="ignore"):
            res = F.restate_job(H, oracle, N.Scene(scene.shapes), job, V.integrator_fn(V.Media(scene), kw), F.JOB_SPP)
        res["stats"]["panes"] = dict(V.PANES)
        _cache[name] = (scene, integ, job, res, sensor)
    return _cache[name][:4]


# ---------------------------------------------------------------- the restatement pinned by closed forms
class _OneStream:
    """an Rng over numpy's generator (the closed forms need numbers, not the renderer's streams)"""

    def __init__(self, seed):
        self.g, self.count, self.log = np.random.default_rng(seed), 0, []

    def next_1d(self):
        self.count += 1
        v = float(np.float32(self.g.random()))
        v = min(v, float(np.float32(1) - np.float32(2.0 ** -24)))
        self.log.append(v)
        return v

    def next_2d(self):
        a = self.next_1d()
        return (a, self.next_1d())


def _slab_scene(native, albedo, sigma_t, with_light, envmap=None):
    """a null cube [-1, 1]^3 holding a medium; behind it (z = 3) a square light facing the camera at z = -5"""
    from mitsuba2_amd import api, scenes
    v, f = scenes._cube((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    medium = api.HomogeneousMedium(sigma_t=sigma_t, albedo=albedo, has_spectral_extinction=True)
    meshes = [api.Mesh("slab", v, f, bsdf=api.BSDF("null"), interior=medium)]
    if with_light:
        q, qf = scenes._quad([(-4, -4, 3), (4, -4, 3), (4, 4, 3), (-4, 4, 3)], inward_point=(0, 0, 0))
        meshes.append(api.Mesh("light", q, qf, emitter=api.AreaLight((2.0, 3.0, 5.0))))
    return api.Scene(meshes, envmap=envmap)


def test_absorbing_slab_is_le_or_zero(native):
    """albedo 0: a camera ray through the slab of thickness 2 sees the light behind it exactly when the free flight
    -log(1 - u) / sigma_t leaves the slab, and nothing at all otherwise"""
    sigma = 0.7
    api_scene = _slab_scene(native, 0.0, sigma, True)
    scene, media = N.Scene(api_scene.shapes), V.Media(api_scene)
    n_le = n_zero = 0
    for k in range(400):
        rng = _OneStream(k)
        ox, oy = 0.5 * math.sin(k), 0.5 * math.cos(3 * k)
        ray = (np.array([ox, oy, -5.0]), np.array([0.0, 0.0, 1.0]), 0.0, math.inf)
        with np.errstate(all="ignore"):
            L, valid, nd, M = V.volpath_sample(scene, media, ray, rng, max_depth=-1, rr_depth=5)
        # ledger of this path: [channel] [roulette] [null BSDF: s1, s2.x, s2.y] [roulette] [free flight] ...
        u = rng.log[6]
        leaves = -math.log1p(-u) / float(np.float32(sigma)) > 2.0
        if leaves:
            assert np.array_equal(L, np.array([2.0, 3.0, 5.0])), (k, L)
            n_le += 1
        else:
            assert not L.any(), (k, L)
            n_zero += 1
    assert n_le > 40 and n_zero > 40, (n_le, n_zero)


def test_white_furnace_mean_is_one(native):
    """albedo 1 under a constant environment of radiance 1, max_depth = -1: every path estimates 1; the mean over the run is 1
    within four standard errors of the run"""
    from mitsuba2_amd import api
    env = api.EnvMap(np.ones((4, 8, 3), np.float32))
    api_scene = _slab_scene(native, 1.0, 1.5, False, envmap=env)
    scene, media = N.Scene(api_scene.shapes), V.Media(api_scene)
    scene.env = F.make_envmap(env)                               # (f64_nested_bsdfs.Scene takes meshes only)
    scene.env.index = 0
    scene.emitters.append(scene.env)
    scene.env.set_scene(np.full(3, -1.0), np.full(3, 1.0))
    vals = []
    for k in range(600):
        rng = _OneStream(1000 + k)
        ray = (np.array([0.3 * math.sin(k), 0.3 * math.cos(2 * k), -5.0]), np.array([0.0, 0.0, 1.0]), 0.0, math.inf)
        with np.errstate(all="ignore"):
            L, valid, nd, M = V.volpath_sample(scene, media, ray, rng, max_depth=-1, rr_depth=5)
        vals.append(L.mean())
    vals = np.array(vals)
    se = vals.std(ddof=1) / math.sqrt(len(vals))
    print("white furnace: mean %.4f, standard error %.4f" % (vals.mean(), se))
    assert abs(vals.mean() - 1.0) <= 4 * se, (vals.mean(), se)


# ---------------------------------------------------------------- the jobs
def jitters(job, res, j):
    """the jitter of camera sample j of every pixel: the two numbers its sampler hands out after the draws of sample j - 1"""
    if j == 0:
        state, _ = H.pcg32_seed(H.pixels_and_seeds(job)[2])
    else:
        state = res["state_after"][j - 1]
    jx, state = H.pcg32_next_f32(state)
    jy, state = H.pcg32_next_f32(state)
    return jx, jy


@pytest.mark.parametrize("name", list(V.JOBS))
def test_job_conditions(native, oracle, name):
    """the restatement ALONE keeps at most MAX_EXCLUDED of a job's samples on a margin, every sample stays in its texel, and the
    job reaches what it is there for"""
    scene, integ, job, res = restated(name, native, oracle)
    checked = res["margin"] >= 1.0
    st = res["stats"]
    msg = "%s: %.2f %% of the samples on a margin, draws per sample %.1f (max %d), stats %s" % (
        name, 100.0 * (1 - checked.mean()), res["n_draws"].mean(), res["n_draws"].max(), st)
    print(msg)
    assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
    # every sample in its own texel: the jitter the restatement drew moves no sample onto its pixel's edge
    for j in range(F.JOB_SPP):
        jx, jy = jitters(job, res, j)
        px, py = res["px"].astype(np.float32), res["py"].astype(np.float32)
        assert (jx != 0).all() and (jy != 0).all() and (px + jx > px).all() and (py + jy > py).all(), "a sample left its texel: pick another base seed"
    if name == "cornell-nomedia":
        assert "medium_scatter" not in st and st["hit"] > 1000, msg
        return
    assert st.get("medium_scatter", 0) > 500, msg
    if name == "fog-panes":
        assert st["hit"] > 1000 and st.get("null_pass", 0) > 100 and st["panes"].get("mask", 0) > 100 and st["panes"].get("thindielectric", 0) > 100, msg
    elif name.startswith("fog-cornell"):
        assert st["hit"] > 1000, msg
    else:
        assert st.get("transition_in", 0) > 100 and st.get("transition_out", 0) > 100, msg
    if name in ("smoke-cube-gray", "bubble-cube"):
        assert st.get("null_pass", 0) > 500, msg


def test_hide_emitters_changes_the_fog_job(native, oracle):
    a, b = restated("fog-cornell", native, oracle)[3], restated("fog-cornell-hide", native, oracle)[3]
    assert np.array_equal(a["n_draws"], b["n_draws"])            # the ledger does not depend on the flag
    assert (a["L"] >= b["L"]).all() and (a["L"] > b["L"]).any()  # the directly visible light is gone


# ---------------------------------------------------------------- host leaves against the restatement's leaves
def test_host_medium_leaves_against_restatement(native):
    from mitsuba2_amd import api
    rng = np.random.default_rng(5)
    med = api.HomogeneousMedium(sigma_t=(0.5, 1.25, 3.0), albedo=(0.2, 0.5, 0.9), scale=0.7)
    ref = V.Medium(med)
    # the sampler hands out multiples of 2^-23 (pcg32's float conversion), so 1 - u is exact in float32, as in the renderer
    samples = list(rng.random(200)) + [0.0, 2.0 ** -23, 3 * 2.0 ** -23, 1 - 2.0 ** -23, 0.5]
    for i, u in enumerate(samples):
        u = math.floor(u * 2.0 ** 23) / 2.0 ** 23
        o, d = rng.normal(size=3).astype(np.float32), rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(np.float32)
        ch = i % 3
        mint = float(np.float32(rng.random() * 0.1)) if i % 4 else 0.0
        want0 = ref.sample_interaction(o.astype(np.float64), d.astype(np.float64), mint, math.inf, u, ch, F.Margin())
        # the seams of t against maxt and against the surface: maxt = the sampled distance itself, just below, just above
        for maxt in (math.inf, want0.ts, want0.ts * (1 - 1e-3), want0.ts * (1 + 1e-3)):
            maxt32 = float(np.float32(maxt))
            si_t = float(np.float32(want0.ts * (0.5 if i % 2 else 2.0)))
            got = med.sample_interaction(np.concatenate([o, d, [mint, maxt32]]), u, ch, si_t)
            want = ref.sample_interaction(o.astype(np.float64), d.astype(np.float64), mint, maxt32, u, ch, F.Margin())
            assert got["sampled_t"] == pytest.approx(want.ts, rel=2e-6, abs=1e-12)
            if abs(want.ts / maxt32 - 1) > 1e-5:
                assert math.isinf(got["t"]) == math.isinf(want.t)
            assert got["mint"] == pytest.approx(want.mint)
            assert np.allclose(got["p"], want.p, rtol=1e-5, atol=1e-5)
            assert np.allclose(got["sigma_t"], want.sigma_t, rtol=1e-6) and np.allclose(got["sigma_s"], want.sigma_s, rtol=1e-6)
            assert np.array_equal(got["combined_extinction"], got["sigma_t"])
            if abs(want.ts / maxt32 - 1) > 1e-5 and abs(want.ts / si_t - 1) > 1e-5:
                if si_t < want.t:
                    want.t = math.inf
                tr, pdf = V.Medium.eval_tr_and_pdf(want, si_t)
                assert np.allclose(got["tr"], tr, rtol=2e-5, atol=1e-30) and np.allclose(got["pdf"], pdf, rtol=2e-5, atol=1e-30)


@pytest.mark.parametrize("g", [None, 0.0, 0.6, -0.4, 0.99, -0.99])
def test_host_phase_leaves_against_restatement(native, g):
    from mitsuba2_amd import api
    phase = api.IsotropicPhase() if g is None else api.HGPhase(g=g)
    ref = V.make_phase(phase)
    rng = np.random.default_rng(11)
    pairs = [rng.random(2) for _ in range(200)] + [(0.0, 0.0), (1 - 2.0 ** -23, 1 - 2.0 ** -23), (0.0, 0.5), (0.5, 0.0)]
    for u in pairs:
        u = np.asarray(u, np.float32)
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(np.float32)
        if abs(d[2]) < 1e-3:
            continue
        wo_eval = rng.normal(size=3)
        wo_eval = (wo_eval / np.linalg.norm(wo_eval)).astype(np.float32)
        wo, pdf, ev = phase.sample_eval(d, u, wo_eval)
        want_wo, want_pdf = ref.sample(d.astype(np.float64), u.astype(np.float64), F.Margin())
        # hg: 1 - g + 2 g u cancels near |g| = 1 — the float32 1 - g is off by 6e-8 / (1 - |g|) relative and enters cos(theta) squared
        tol = 2e-5 + (0.0 if g is None else 2e-7 / (1 - abs(g)) ** 2)
        # sin(theta) = sqrt(1 - cos^2) is ill-conditioned at the poles: a float32 cos(theta), off by a few 1e-7, moves it by that over sin(theta)
        sin_ref = math.sqrt(max(0.0, 1 - float(want_wo @ d.astype(np.float64)) ** 2))
        assert np.allclose(wo, want_wo, atol=tol + 1e-6 / max(sin_ref, 1e-3)), (g, u, wo, want_wo)
        assert pdf == pytest.approx(want_pdf, rel=50 * tol)
        assert ev == pytest.approx(ref.eval(d.astype(np.float64), wo_eval.astype(np.float64)), rel=50 * tol)
        assert abs(np.linalg.norm(wo) - 1) < 1e-5


def test_hg_refuses_g_outside_the_open_interval(native):
    from mitsuba2_amd import api
    for g in (1.0, -1.0, 1.5):
        with pytest.raises(RuntimeError, match="asymmetry parameter must lie in the interval"):
            api.HGPhase(g=g)


# ---------------------------------------------------------------- records and flattening
def test_medium_record_through_the_classes(native):
    from mitsuba2_amd import api, _capi
    m = api.HomogeneousMedium(sigma_t=(1.0, 2.0, 4.0), albedo=(0.1, 0.2, 0.3), scale=0.5, phase=api.HGPhase(g=0.6), sample_emitters=False,
                              has_spectral_extinction=False)
    r = m.record()
    assert list(r.sigma_t) == [0.5, 1.0, 2.0] and np.allclose(list(r.albedo), [0.1, 0.2, 0.3])
    assert (r.has_spectral_extinction, r.sample_emitters, r.phase) == (0, 0, _capi.MI_PHASE_HG) and r.g == pytest.approx(0.6)
    d = api.HomogeneousMedium().record()                         # the reference's defaults
    assert list(d.sigma_t) == [1.0, 1.0, 1.0] and list(d.albedo) == [0.75, 0.75, 0.75]
    assert (d.has_spectral_extinction, d.sample_emitters, d.phase) == (1, 1, _capi.MI_PHASE_ISOTROPIC)


def test_scene_flattens_media_into_references(native):
    from mitsuba2_amd import api, scenes
    a, b = api.HomogeneousMedium(sigma_t=2.0), api.HomogeneousMedium(sigma_t=3.0, phase=api.HGPhase(g=0.3))
    v, f = scenes._cube((0, 0, 0), (1, 1, 1))
    v2, f2 = scenes._cube((2, 0, 0), (3, 1, 1))
    m0 = api.Mesh("in", v, f, bsdf=api.BSDF("null"), interior=a, exterior=b)
    m1 = api.Mesh("plain", v2, f2)
    m2 = api.Mesh("out", v2 + 3, f2, bsdf=api.BSDF("null"), exterior=a)
    assert m0.is_medium_transition() and not m1.is_medium_transition() and m2.is_medium_transition()
    scene = api.Scene([m0, m1, m2], start_medium=b).build(-1)
    d = scene.desc().contents
    assert d.media_count == 2 and d.start_medium == 1             # the sensor's medium is met first
    assert [d.shape_media[i] for i in range(6)] == [2, 1, 0, 0, 0, 2]
    assert d.media[0].sigma_t[0] == 3.0 and d.media[1].sigma_t[0] == 2.0 and d.media[0].phase == 1
    plain = api.Scene([api.Mesh("plain", v2, f2)]).build(-1).desc().contents
    assert plain.media_count == 0 and not plain.shape_media and plain.start_medium == 0 and not plain.media


def test_path_job_description_differs_only_in_the_appended_members(native):
    """the description of a scene with media records and of the same scene without: every member up to `lights` is equal"""
    from mitsuba2_amd import _capi, scenes
    with_media = scenes.volpath_scene("smoke-cube-gray").build(-1)
    without = scenes.volpath_scene("smoke-cube-gray")
    for m in without.shapes:
        m.set_media(None, None)
    without = without.build(-1)
    a, b = with_media.desc().contents, without.desc().contents
    appended = ("media", "media_count", "shape_media", "start_medium")
    for name, typ in _capi.mi_scene_desc._fields_:
        if name in appended:
            continue
        va, vb = getattr(a, name), getattr(b, name)
        if isinstance(va, int):
            assert va == vb, name
    n = a.shape_count
    assert bytes(C.string_at(a.shapes, n * C.sizeof(_capi.mi_shape))) == bytes(C.string_at(b.shapes, n * C.sizeof(_capi.mi_shape)))
    assert bytes(C.string_at(a.bsdfs, a.bsdf_count * C.sizeof(_capi.mi_bsdf))) == bytes(C.string_at(b.bsdfs, b.bsdf_count * C.sizeof(_capi.mi_bsdf)))
    assert bytes(C.string_at(a.vertex_positions, 12 * a.vertex_count)) == bytes(C.string_at(b.vertex_positions, 12 * b.vertex_count))
    assert a.media_count == 1 and b.media_count == 0
    assert _capi.mi_scene_desc.media.offset >= _capi.mi_scene_desc.light_count.offset + 4


# ---------------------------------------------------------------- the ABI mirrors
def test_mi_medium_mirror_and_appended_members(native):
    from mitsuba2_amd import _capi, api
    assert C.sizeof(_capi.mi_medium) == 40
    offs = {n: getattr(_capi.mi_medium, n).offset for n, _ in _capi.mi_medium._fields_}
    assert offs == dict(sigma_t=0, albedo=12, has_spectral_extinction=24, sample_emitters=28, phase=32, g=36)
    assert C.sizeof(_capi.mi_sample_cfg) == 32 and api.VolPathIntegrator().sample_cfg().struct_size == 32
    assert _capi.MI_INTEGRATOR_VOLPATH == 2 and api.VolPathIntegrator(max_depth=7, rr_depth=3, hide_emitters=True).sample_cfg().integrator == 2
    cfg = api.VolPathIntegrator(max_depth=7, rr_depth=3, hide_emitters=True).sample_cfg()
    assert (cfg.max_depth, cfg.rr_depth, cfg.hide_emitters) == (7, 3, 1)
    # appended: the members before them keep their offsets
    d = _capi.mi_scene_desc
    assert d.media.offset == d.lights.offset + 16 and d.shape_media.offset == d.media.offset + 16 and d.start_medium.offset == d.shape_media.offset + 8
    assert [f[0] for f in _capi.mi_counters._fields_][-2:] == ["job_chunk", "job_chunks"]      # mi_counters is as it was: the count has an entry point
    assert "mi_volpath_capped" in _capi.MI_SYMBOLS


def test_volpath_integrator_checks_its_properties(native):
    from mitsuba2_amd import api
    with pytest.raises(RuntimeError, match="rr_depth"):
        api.VolPathIntegrator(rr_depth=0)
    with pytest.raises(RuntimeError, match="max_depth"):
        api.VolPathIntegrator(max_depth=-2)
    with pytest.raises(RuntimeError, match="volpath"):
        api.MomentIntegrator(api.VolPathIntegrator())
    with pytest.raises(RuntimeError, match="volpath"):
        api.AOVIntegrator("depth", nested=api.VolPathIntegrator())
