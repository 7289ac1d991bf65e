"""k_sample_volpath (mi_sample and mi_render_sensor with MI_INTEGRATOR_VOLPATH) on the GPU.

The jobs and the restatement results of test_volpath.py (computed once per job): Device.sample returns L, `valid` and the sampler
state per ray, checked under the rule of f64_integrators.compare with the project's RTOL; the state after every checked ray must be
EXACTLY the state advanced by the restatement's draw count. Films: render_sensor against the film reassembled from chained
mi_sample calls (lens_harness.chain_lens), bit for bit. mi_volpath_capped answers 0 everywhere."""
import numpy as np
import pytest

import f64_integrators as F
import f64_volpath as V
import lens_harness as LH
from test_independent_integrators import RTOL, report
from test_volpath import restated

pytestmark = pytest.mark.gpu

W, HGT, BASE_SEED = 64, 48, 50000
LENS = dict(type="thinlens", aperture_radius=8.0, focus_distance=1000.0)


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_film(got, want, what):
    bad = _words(got) != _words(want)
    assert not bad.any(), "%s: %d of %d film words differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def _host(dev, cfg, ray, state):
    o, d = np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6])
    return dev.sample(o, d, state, np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), cfg=cfg)


def _device(dev, cfg, ray, state):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = t(state.view(np.int64))
    spec, valid = dev.sample_device([t(ray[:, k]) for k in range(8)], st, cfg=cfg)
    return spec.cpu().numpy(), valid.cpu().numpy() != 0, st.cpu().numpy().view(np.uint64)


def _check(name, res, dev, call):
    assert (res["margin"] >= 1.0).mean() >= 1 - F.MAX_EXCLUDED              # the job's condition (test_volpath.py asserts it on the CPU)
    for j in range(F.JOB_SPP):
        spec, valid, after = call(res["ray"][j], res["state_before"][j].copy())
        assert dev.volpath_capped() == 0
        checked, bad, dev_max = F.compare(spec, valid, res, j, RTOL, to_xyz=False)
        msg = report(name, res, checked, dev_max)
        print("sample %d: %s" % (j, msg))
        assert checked.mean() >= 0.9, msg
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            pytest.fail("%s\nsample %d: %d rays differ; first: pixel (%d, %d): device %s valid %s, restatement %s valid %s, margin %.3g (%s), draws %d"
                        % (msg, j, bad.sum(), res["px"][i], res["py"][i], spec[i], valid[i], res["L"][j, i], res["valid"][j, i], res["margin"][j, i],
                           res["what"][j][i], res["n_draws"][j, i]))
        wrong = checked & (after != res["state_after"][j])
        assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count; first: ray %d, %d draws" % (
            msg, j, wrong.sum(), np.flatnonzero(wrong)[0], res["n_draws"][j, np.flatnonzero(wrong)[0]])


@pytest.mark.parametrize("name", list(V.JOBS))
def test_gpu_volpath_sample_against_float64_restatement(native, oracle, name):
    """both routes — the scene's own (packet kernels for these small boxes) and the forced tree walk — each through host arrays and
    through arrays resident on the device"""
    from mitsuba2_amd import _capi
    scene, integ, job, res = restated(name, native, oracle)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        for call in (_host, _device):
            for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
                dev.upload(scene.desc(), quality)
                _check(name, res, dev, lambda ray, st: call(dev, cfg, ray, st))
    finally:
        dev.close()


# ---- device leaf == host leaf, word for word (MI_EVAL_MEDIUM, MI_EVAL_PHASE) ---------------------------------------------------------
def _leaf_scene(api, scenes):
    """one cube per medium, so that medium k of the uploaded description is media[k]: rgb sigma_t with a scale, isotropic, and hg with
    g = 0 (the |g| < Epsilon branch), 0.6, -0.4 and +-0.99"""
    media = [api.HomogeneousMedium(sigma_t=(0.5, 1.25, 3.0), albedo=(0.2, 0.5, 0.9), scale=0.7, phase=api.IsotropicPhase())]
    media += [api.HomogeneousMedium(sigma_t=(0.002 * (k + 1), 0.5, 40.0), albedo=0.75, phase=api.HGPhase(g=g)) for k, g in enumerate((0.0, 0.6, -0.4, 0.99, -0.99))]
    meshes = []
    for k, m in enumerate(media):
        v, f = scenes._cube((3.0 * k, 0, 0), (3.0 * k + 1, 1, 1))
        meshes.append(api.Mesh("cube%d" % k, v, f, bsdf=api.BSDF("null"), interior=m))
    return media, api.Scene(meshes).build(-1)


def test_device_leaf_equals_host_leaf(native):
    from mitsuba2_amd import scenes, _capi
    media, scene = _leaf_scene(native, scenes)
    d = scene.desc().contents
    assert d.media_count == len(media) and all(d.media[k].g == np.float32(m.record().g) for k, m in enumerate(media))
    rng = np.random.default_rng(23)
    grid = lambda u: np.floor(np.asarray(u) * 2.0 ** 23) / 2.0 ** 23          # what the sampler hands out
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), 0)
        # -- MI_EVAL_MEDIUM: random inputs plus the seams — sample at 0, one step above, one step below 1; t at maxt; a surface before / behind
        rows, want = [], []
        for k, med in enumerate(media):
            for i, u in enumerate(list(grid(rng.random(40))) + [0.0, 2.0 ** -23, 1 - 2.0 ** -23, 0.5]):
                o = rng.normal(size=3).astype(np.float32) * 100
                dd = rng.normal(size=3); dd = (dd / np.linalg.norm(dd)).astype(np.float32)
                ch = i % 3
                mint = np.float32(rng.random() * 0.1) if i % 4 else np.float32(0)
                ts = np.float32(med.sample_interaction(np.concatenate([o, dd, [mint, np.inf]]), float(u), ch)["sampled_t"])
                for maxt in (np.float32(np.inf), ts, np.nextafter(ts, np.float32(0)), np.nextafter(ts, np.float32(np.inf))):
                    for si_t in (np.float32(np.inf), np.float32(ts * np.float32(0.5)), np.float32(ts * np.float32(2))):
                        ray8 = np.concatenate([o, dd, [mint, maxt]]).astype(np.float32)
                        h = med.sample_interaction(ray8, float(u), ch, float(si_t))
                        rows.append(np.concatenate([[k], ray8, [u, ch, si_t]]).astype(np.float32))
                        want.append(np.concatenate([[h["t"], h["mint"]], h["p"], h["sigma_s"], h["sigma_t"], h["combined_extinction"], [h["sampled_t"], 0.0],
                                                    h["tr"], h["pdf"]]).astype(np.float32))
        got = dev.eval(_capi.MI_EVAL["MEDIUM"], np.stack(rows))
        want = np.stack(want)
        assert np.isinf(want[:, 0]).any() and np.isfinite(want[:, 0]).any()
        same = (_words(got) == _words(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), "MI_EVAL_MEDIUM: %d of %d words differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])
        # -- MI_EVAL_PHASE: random inputs plus the corners of the sample square
        rows, want = [], []
        for k, med in enumerate(media):
            for u in [grid(rng.random(2)) for _ in range(60)] + [(0.0, 0.0), (1 - 2.0 ** -23, 1 - 2.0 ** -23), (0.0, 0.5), (0.5, 0.0)]:
                dd = rng.normal(size=3); dd = (dd / np.linalg.norm(dd)).astype(np.float32)
                wo_e = rng.normal(size=3); wo_e = (wo_e / np.linalg.norm(wo_e)).astype(np.float32)
                wo, pdf, ev = med.phase.sample_eval(dd, np.asarray(u, np.float32), wo_e)
                rows.append(np.concatenate([[k], dd, u, wo_e]).astype(np.float32))
                want.append(np.concatenate([wo, [pdf, ev]]).astype(np.float32))
        got = dev.eval(_capi.MI_EVAL["PHASE"], np.stack(rows))
        same = _words(got) == _words(np.stack(want))
        assert same.all(), "MI_EVAL_PHASE: %d of %d words differ, first at %s" % ((~same).sum(), same.size, np.argwhere(~same)[0])
        bad = np.stack(rows)[:2].copy(); bad[1, 0] = len(media)
        with pytest.raises(RuntimeError, match="entry 1: medium 6 out of range"):
            dev.eval(_capi.MI_EVAL["PHASE"], bad)
    finally:
        dev.close()


def test_routes_without_a_float64_tier_are_refused_by_name(native):
    """scenes with shapeless emitters or analytic shapes: volpath refuses them until a restatement pins those routes; path serves them"""
    from mitsuba2_amd import scenes
    ray = (np.array([[278.0, 273.0, -800.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32), np.zeros(1, np.uint64))
    dev = native.Device(0)
    try:
        for scene, msg in ((scenes.lit_box("point", W, HGT, 1, device=-1)[0], "point / spot / directional / constant emitters are not served yet"),
                           (scenes.sphere_box(W, HGT, 1, device=-1)[0], r"analytic shapes \(rectangle, sphere\) are not served yet")):
            dev.upload(scene.desc(), 0)
            with pytest.raises(RuntimeError, match=msg):
                dev.sample(*ray, cfg=native.sample_cfg("volpath"))
            spec, valid, _ = dev.sample(*ray, cfg=native.sample_cfg("path"))                     # ... and the context works on
            assert valid.all()
    finally:
        dev.close()


def _fog_job(native, scenes, spp, lens=None, w=W, h=HGT, **film_kw):
    scene = scenes.volpath_scene("fog-cornell")
    sensor = scenes.cornell_sensor(w, h, spp, seed=BASE_SEED, rfilter="box", sensor=dict(lens or {}, medium=scene.start_medium), **film_kw)
    return scene, sensor


@pytest.mark.parametrize("lens", [None, LENS], ids=["perspective", "thinlens"])
def test_sensor_film_is_the_reassembled_film(native, oracle, lens):
    """render_sensor's film at spp and spp + 1 == the film chained from mi_sample calls with the volpath cfg, bit for bit"""
    from mitsuba2_amd import scenes, _capi
    spp = 2
    integ = native.VolPathIntegrator(max_depth=6)
    scene, s0 = _fog_job(native, scenes, spp, lens)
    _, s1 = _fog_job(native, scenes, spp + 1, lens)
    scene.build(-1)
    desc = s0.desc()
    jobs = [integ.render_job(s0), integ.render_job(s1)]
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            cfg = integ.sample_cfg()
            fn = lambda o, d, mint, maxt, wl, state: dev.sample(o, d, state, mint, maxt, cfg=cfg)
            films = [f.copy() for f in LH.chain_lens(oracle, jobs[1], desc, s0.sample_rays, fn, spp + 1)]
            for job, want, what in ((jobs[0], films[spp - 1], "spp"), (jobs[1], films[spp], "spp + 1")):
                got, st = dev.render_sensor(job, desc)
                assert st == 0 and dev.volpath_capped() == 0
                assert want[..., 4].min() == job.cfg.spp and want[..., :3].max() > 0
                _same_film(got, want, what)
    finally:
        dev.close()


def test_passes_small_film_and_the_public_class(native):
    """a 40 x 24 film (lanes outside the film): api.VolPathIntegrator.render == the ABI film, in one pass and in two passes of 2 spp,
    the second accumulated onto the first (integrator.cpp:75-86; the passes carry other seeds than the one-pass frame)"""
    from mitsuba2_amd import scenes
    scene, sensor = _fog_job(native, scenes, 4, w=40, h=24)
    scene.build(0)
    one, passes = native.VolPathIntegrator(max_depth=5), native.VolPathIntegrator(max_depth=5, samples_per_pass=2)
    assert passes.pass_count(sensor) == 2
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), 0)
        want, st = dev.render_sensor(one.render_job(sensor), sensor.desc())
        assert st == 0 and want[..., 4].min() == 4 and want[..., :3].max() > 0 and dev.volpath_capped() == 0
        g0, _ = dev.render_sensor(passes.render_job(sensor, pass_index=0), sensor.desc())
        g1, _ = dev.render_sensor(passes.render_job(sensor, pass_index=1), sensor.desc(), onto=g0)
        assert g1[..., 4].min() == 4 and not np.array_equal(g1, want) and dev.volpath_capped() == 0
    finally:
        dev.close()
    assert one.render(scene, sensor)
    _same_film(sensor.film.data((24, 40, 5)), want, "VolPathIntegrator.render")
    assert one.volpath_capped() == 0
    assert passes.render(scene, sensor)
    _same_film(sensor.film.data((24, 40, 5)), g1, "VolPathIntegrator.render, two passes")
    other = scenes.cornell_sensor(40, 24, 4, seed=BASE_SEED, rfilter="box")       # a sensor outside the fog the scene starts in
    with pytest.raises(RuntimeError, match="sensor's medium"):
        one.render(scene, other)


def test_without_media_volpath_agrees_with_path(native, oracle):
    """no media in the scene (the job cornell-nomedia, whose L the job test above pins to the restatement within RTOL): `valid`
    equals path's on the same rays; with max_depth = 1 both return the emission the camera ray sees, bit for bit. The draw ledgers
    differ — volpath draws the channel and a roulette number per bounce — so deeper paths are other paths and a per-ray comparison of L
    with path's within RTOL, as the issue words it, has no meaning: in its place the job's L is pinned per ray to the restatement (the
    job test) and here the MEANS of the two estimators over the job's 3072 rays agree within four standard errors of their difference."""
    scene, integ, job, res = restated("cornell-nomedia", native, oracle)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), 0)
        ray, st = res["ray"][0], res["state_before"][0].copy()
        v_spec, v_valid, _ = _host(dev, integ.sample_cfg(), ray, st)
        p_spec, p_valid, _ = _host(dev, native.PathIntegrator(max_depth=3, rr_depth=2).sample_cfg(), ray, st)
        assert dev.volpath_capped() == 0
        assert np.array_equal(v_valid, p_valid) and p_valid.any() and not p_valid.all()
        n = len(v_spec)
        se = np.sqrt(v_spec.var(0, ddof=1) / n + p_spec.var(0, ddof=1) / n)
        print("mean L: volpath %s, path %s, standard error of the difference %s" % (v_spec.mean(0), p_spec.mean(0), se))
        assert (np.abs(v_spec.mean(0) - p_spec.mean(0)) <= 4 * se).all()
        v1, v1_valid, _ = _host(dev, native.VolPathIntegrator(max_depth=1).sample_cfg(), ray, st)
        p1, p1_valid, _ = _host(dev, native.PathIntegrator(max_depth=1).sample_cfg(), ray, st)
        assert np.array_equal(v1, p1) and np.array_equal(v1_valid, p1_valid) and v1.max() > 0
    finally:
        dev.close()


def test_path_ignores_media_records(native):
    """a `path` render of a scene with media records gives the same film, word for word, as without them"""
    from mitsuba2_amd import scenes
    sensor = scenes.cornell_sensor(W, HGT, 2, seed=BASE_SEED, rfilter="box")
    with_media = scenes.volpath_scene("smoke-cube-gray").build(-1)
    without = scenes.volpath_scene("smoke-cube-gray")
    for m in without.shapes:
        m.set_media(None, None)
    without.build(-1)
    integ = native.PathIntegrator(max_depth=4)
    dev = native.Device(0)
    try:
        films = []
        for scene in (with_media, without):
            dev.upload(scene.desc(), 0)
            film, st = dev.render(integ.render_job(sensor), film_mode=1)
            assert st == 0
            films.append(film)
        _same_film(films[0], films[1], "path with media records")
        assert films[0][..., :3].max() > 0
    finally:
        dev.close()


def test_refusals_by_message_and_the_context_renders_on(native):
    from mitsuba2_amd import scenes, _capi, api
    import ctypes as C
    scene, sensor = _fog_job(native, scenes, 1)
    scene.build(-1)
    integ = native.VolPathIntegrator(max_depth=4)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc(), 0)
        want, st = dev.render_sensor(integ.render_job(sensor), sensor.desc())
        assert st == 0
        with pytest.raises(RuntimeError, match="volpath renders through mi_render_sensor"):
            dev.render(integ.render_job(sensor))
        job = integ.render_job(sensor); job.cfg.moment_pass = 1
        with pytest.raises(RuntimeError, match="moment"):
            dev.render_sensor(job, sensor.desc())
        shard = native.VolPathIntegrator(max_depth=4); shard.set_shard(0, 2)
        with pytest.raises(RuntimeError, match="tile_list"):
            dev.render_sensor(shard.render_job(sensor), sensor.desc())
        bad = api.sample_cfg("volpath", rr_depth=0)
        with pytest.raises(RuntimeError, match="rr_depth"):
            dev.sample(np.zeros((1, 3)), np.array([[0, 0, 1.0]]), np.zeros(1, np.uint64), cfg=bad)
        again, st = dev.render_sensor(integ.render_job(sensor), sensor.desc())      # ... and the context renders on
        assert st == 0
        _same_film(again, want, "after the refusals")
        # upload refusals name the record; the context keeps working after them
        d = scene.desc().contents
        for field, value, msg in (("sigma_t", (0.0, 1.0, 1.0), r"medium 0: sigma_t\[0\]"), ("sigma_t", (1.0, float("inf"), 1.0), r"medium 0: sigma_t\[1\]"),
                                  ("albedo", (0.5, 0.5, 1.5), r"medium 0: albedo\[2\]"), ("g", 1.0, "medium 0: The asymmetry parameter")):
            rec = _capi.mi_medium.from_buffer_copy(d.media[0])
            if field == "g":
                rec.phase, rec.g = _capi.MI_PHASE_HG, value
            else:
                setattr(rec, field, (C.c_float * 3)(*value))
            bad_desc = _capi.mi_scene_desc.from_buffer_copy(d)
            bad_desc.media = C.pointer(rec)
            with pytest.raises(RuntimeError, match=msg):
                dev.upload(C.pointer(bad_desc), 0)
        bad_desc = _capi.mi_scene_desc.from_buffer_copy(d)
        bad_desc.start_medium = 2
        with pytest.raises(RuntimeError, match="start_medium 2 out of range"):
            dev.upload(C.pointer(bad_desc), 0)
        refs = (C.c_uint32 * (2 * d.shape_count))(*([0] * (2 * d.shape_count)))
        refs[3] = 5
        bad_desc = _capi.mi_scene_desc.from_buffer_copy(d)
        bad_desc.shape_media = C.cast(refs, _capi.c_u32_p)
        with pytest.raises(RuntimeError, match="shape 1: exterior medium 5 out of range"):
            dev.upload(C.pointer(bad_desc), 0)
        dev.upload(scene.desc(), 0)
        again, st = dev.render_sensor(integ.render_job(sensor), sensor.desc())
        assert st == 0
        _same_film(again, want, "after the refused uploads")
    finally:
        dev.close()
    multi, sensor = _fog_job(native, scenes, 1)
    multi.build([0, 0])
    with pytest.raises(RuntimeError, match="one device and without tile shards"):
        native.VolPathIntegrator().render(multi, sensor)
