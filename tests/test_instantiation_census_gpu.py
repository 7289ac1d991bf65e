"""Every instantiation of the path kernels, once on the GPU: tests/instantiation_cases.py has one case per instantiation of k_path_resident /
k_path_phased / k_path_pooled / k_sample_rays the library can launch (test_instantiation_census.py proves the table complete on the CPU), and
each case is one pytest id here, so that a failure names one kernel.

A case uploads its scene, sets its options and MIW_DEBUG=1, renders, and reads the library's "[miwave] kernel launched: NAME<...>" lines
(printed by the launch macro from its own arguments): the SET of instantiations launched must be exactly the case's
key (a placed launch runs the measuring launch and the placed one through the same Placed instantiation), the status 0 and the counters
the case expects. Then, by the case's kind and reference:

  log      the sample-log film (film_mode 1) equals the CPU checker's film of the same job in every uint32 word; samples and segments equal.
  atomic   the float64-atomics film (film_mode 2), rounded to float32, against the checker's float64 film rounded to float32. With the
           gaussian filter every weight is >= 0, so two float64 sums of the same non-negative float32 products in different orders differ by
           far less than half a float32 ulp and the rounded values by at most 1 ulp, only where a sum sits on a rounding boundary: <= 1 ulp
           asserted, and at most 1 word in 1 000 different at all (the condition that keeps a systematically offset kernel from hiding
           behind the first bound). The largest distance is printed per case.
  placed   256 x 128 @ 128 spp in one launch; counters().placed == 1 and n_path == 2; the same context renders the job again with
           MIW_PLACE=0 and the two films are equal bit for bit. (The checker needs about 20 s on 8 threads for this job, so it is not
           asked: the unplaced kernel of every class is pinned to it by its own case at 64 x 64.)
  sample   k_sample_rays: sample_harness.chain reassembles the checker's float64 film from Device.sample results (host arrays), bit for
           bit at spp and at spp + 1 — which pins the returned sampler state.

The checker cannot render a shapeless emitter (test_lights_gpu.py), so the MATS_LIGHTS cases have no checker film: their films are compared
bit for bit (atomics: as above) with the film reassembled from the device's own mi_sample results by the method of test_lights_gpu.py (box
filter), and k_sample_rays<..., MATS_LIGHTS, ...> with the float64 restatement of tests/f64_lights.py, state after every ray included, at that
test's tolerance.
"""
import re

import numpy as np
import pytest

import instantiation_cases as IC
import sample_harness as H

pytestmark = pytest.mark.gpu

LINE = re.compile(r"\[miwave\] kernel launched: (k_[a-z_]+<[^>]*>)")
_scenes, _oracle_films, _chain_films = {}, {}, {}


def _launched(capfd):
    return set(LINE.findall(capfd.readouterr().err))


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.view(u) != b.view(u)


def _assert_same_bits(got, want, what):
    bad = _bits_differ(got, want)
    assert not bad.any(), "%s: %d of %d film words differ, first at texel (y, x, channel) %s: %r against %r" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def _scene(api, variant, name):
    if (variant, name) not in _scenes:
        from mitsuba2_amd import scenes
        _scenes[variant, name] = IC.build_scene(name, api, scenes)
    return _scenes[variant, name]


def _oracle(orc, variant, case, scene, job, extra_spp=0):
    """one checker render per (scene, job), shared by the cases that use it and left unchanged"""
    k = IC.job_key(case, variant, extra_spp)
    if k not in _oracle_films:
        o32, o64, st = orc.render(scene.desc(), job, threads=8, want_f64=True)
        assert float(np.nanmax(o32[..., :3])) > 0 and o32[..., 4].min() > 0
        o32.setflags(write=False); o64.setflags(write=False)
        _oracle_films[k] = (o32, o64, st.samples, st.segments)
    return _oracle_films[k]


def _chain_reference(orc, dev, variant, case, job, cfg):
    """MATS_LIGHTS: (float64 film, float32 film) of the job from chained mi_sample results (test_lights_gpu.py: _reassembled), once per job"""
    k = IC.job_key(case, variant)
    if k not in _chain_films:
        spectral = variant == "scalar_spectral"
        fn = lambda o, d, mint, maxt, wl, state: dev.sample(o, d, state, mint, maxt, wavelengths=wl, cfg=cfg)
        films = [f.copy() for f in H.chain(orc, job, fn, case.film[2], spectral=spectral)]
        f32 = np.zeros(films[0].shape, np.float32)
        prev = np.zeros_like(films[0])
        for f in films:                                           # ImageBlock::put: one texel per sample (box filter), added in sample order in float32
            f32 += (f - prev).astype(np.float32)
            prev = f
        assert float(films[-1][..., :3].max()) > 0 and (films[-1][..., 4] == case.film[2]).all()
        _chain_films[k] = (films[-1], f32)
    return _chain_films[k]


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _lights_sample(api, orc, dev, variant, case, capfd):
    """k_sample_rays<..., MATS_LIGHTS, ...> against the float64 restatement of the point-light job (tests/f64_lights.py), every ray's state included"""
    import f64_integrators as F
    import f64_lights as FL
    from test_independent_integrators import RTOL, report, xyz_of
    from test_lights import restated
    name = "point-direct-1-1" if case.integrator == "direct" else "point-path"
    if variant == "scalar_rgb":
        scene, integ, job, res = restated(name, api, orc)
        model = None
    else:
        k = ("f64", variant, name)
        if k not in _chain_films:
            from conftest import SRGB_COEFF
            from mitsuba2_amd import scenes
            from test_independent_leaves import _reference_tables
            which, kind, kw = FL.JOBS[name]
            cie, d65 = _reference_tables()
            model = F.SrgbModel(SRGB_COEFF, cie, d65)
            scene, sensor = FL.job_scene(scenes, which, FL.JOB_SPP)
            integ = (api.PathIntegrator if kind == "path" else api.DirectIntegrator)(**kw)
            job = integ.render_job(sensor)
            res = F.restate_job(H, orc, FL.from_api_scene(scene), job, F.integrator_fn(kind, kw), FL.JOB_SPP, model=model)
            excluded = 1.0 - float((res["margin"] >= 1.0).mean())
            assert excluded <= F.MAX_EXCLUDED and np.isfinite(res["L"]).all() and res["L"].max() > 0
            _chain_films[k] = (scene, integ, job, res, model)
        scene, integ, job, res, model = _chain_films[k]
    assert scene.desc().contents.face_count == IC.SCENES[case.scene][1] and (job.cfg.crop_w, job.cfg.crop_h, FL.JOB_SPP) == case.film
    cfg = integ.sample_cfg()
    dev.upload(scene.desc(), case.quality)
    dev.set_option("MIW_DEBUG", "1")
    capfd.readouterr()
    for j in range(FL.JOB_SPP):
        ray = res["ray"][j]
        wl = None if model is None else np.ascontiguousarray(res["wl"][j])
        spec, valid, after = dev.sample(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), res["state_before"][j].copy(),
                                        np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), wavelengths=wl, cfg=cfg)
        if model is None:
            checked, bad, dv = F.compare(spec, valid, res, j, RTOL, to_xyz=False)
        else:
            checked, bad, dv = F.compare(xyz_of(spec, wl, model.cie, False), valid, res, j, RTOL, to_xyz=False, want=xyz_of(res["L"][j], wl, model.cie, False))
        msg = report(name, res, checked, dv)
        print("sample %d: %s" % (j, msg))
        assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
        assert not bad.any(), "%s\nsample %d: %d rays differ, first ray %d: device %s, restatement %s" % (
            msg, j, bad.sum(), np.flatnonzero(bad)[0], spec[np.flatnonzero(bad)[0]], res["L"][j, np.flatnonzero(bad)[0]])
        wrong = checked & (after != res["state_after"][j])
        assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count" % (msg, j, wrong.sum())
    assert _launched(capfd) == {case.key}


def _sample(api, orc, dev, variant, case, capfd):
    from mitsuba2_amd import scenes
    spp = case.film[2]
    scene = _scene(api, variant, case.scene)
    integ = IC.integrator(api, case)
    jobs = [integ.render_job(IC.sensor(scenes, case, variant, extra)) for extra in (0, 1)]
    want = [_oracle(orc, variant, case, scene, jobs[extra], extra)[1] for extra in (0, 1)]
    assert H.every_sample_in_its_texel(want[0], spp) and H.every_sample_in_its_texel(want[1], spp + 1)      # (a condition of the job: asserted on the CPU as well)
    cfg = integ.sample_cfg()
    dev.upload(scene.desc(), case.quality)
    dev.set_option("MIW_DEBUG", "1")
    for k, v in case.options:
        dev.set_option(k, v)
    capfd.readouterr()
    fn = lambda o, d, mint, maxt, wl, state: dev.sample(o, d, state, mint, maxt, wavelengths=wl, cfg=cfg)
    films = [f.copy() for f in H.chain(orc, jobs[1], fn, spp + 1, spectral=variant == "scalar_spectral")]
    assert _launched(capfd) == {case.key}
    _assert_same_bits(films[spp - 1], want[0], "spp")
    _assert_same_bits(films[spp], want[1], "spp + 1")


def _render(api, orc, dev, variant, case, capfd):
    from mitsuba2_amd import scenes
    scene = _scene(api, variant, case.scene)
    integ = IC.integrator(api, case)
    job = integ.render_job(IC.sensor(scenes, case, variant), n_threads=case.n_threads)
    w, h, spp = case.film
    for k, v in case.build_options:
        dev.set_option(k, v)
    dev.upload(scene.desc(), case.quality)
    assert dev.counters().bvh_tris == IC.SCENES[case.scene][1], dev.counters().bvh_tris
    if case.reference == "oracle":
        o32, o64, o_samples, o_segments = _oracle(orc, variant, case, scene, job)
    elif case.reference == "chain":
        o64, o32 = _chain_reference(orc, dev, variant, case, job, integ.sample_cfg())
        o_samples, o_segments = w * h * spp, None
    for k, v in case.options:
        dev.set_option(k, v)
    dev.set_option("MIW_DEBUG", "1")
    capfd.readouterr()
    g, st = dev.render(job, **case.render)
    c = dev.counters()
    launched = _launched(capfd)
    assert st == 0
    assert launched == {case.key}, "launched %s" % sorted(launched)
    assert c.plan == 2
    for field, value in case.expect.items():
        assert getattr(c, field) == value, (field, getattr(c, field), value)
    if case.kind == "placed":
        assert case.reference == "unplaced" and float(g[..., :3].max()) > 0 and g[..., 4].min() > 0 and c.samples == w * h * spp
        dev.set_option("MIW_PLACE", "0")
        plain, st = dev.render(job, **case.render)
        c1 = dev.counters()
        unplaced = case.key[:-len("true>")] + "false>"
        assert st == 0 and (c1.placed, c1.n_path) == (0, 1) and _launched(capfd) == {unplaced}
        assert (c1.samples, c1.segments) == (c.samples, c.segments)
        _assert_same_bits(g, plain, "placed against MIW_PLACE=0")
        return
    assert c.samples == o_samples and (o_segments is None or c.segments == o_segments), (c.samples, o_samples, c.segments, o_segments)
    if case.kind == "log":
        assert c.film_mode == 1
        _assert_same_bits(g, o32, "film_mode 1")
    else:
        assert case.kind == "atomic" and g.dtype == np.float64
        u = _ulps(g.astype(np.float32), o64.astype(np.float32))
        print("%s %s: float64-atomics film against the reference, both rounded to float32: largest distance %d ulps, %d of %d words differ" % (
            variant, case.key, u.max(), (u != 0).sum(), u.size))
        assert np.isfinite(g).all() and u.max() <= 1, "first beyond 1 ulp at %s" % (tuple(np.argwhere(u > 1)[0]),)
        assert (u != 0).sum() * 1000 <= u.size


def _run(api, orc, capfd, variant, key):
    case = IC.cases(variant)[key]
    assert case.unreachable is None, case.unreachable
    dev = api.Device(0)
    try:
        if variant == "scalar_spectral":
            assert dev.L.mi_spectrum_channels() == 4
        if case.kind == "sample":
            (_lights_sample if case.reference == "f64" else _sample)(api, orc, dev, variant, case, capfd)
        else:
            _render(api, orc, dev, variant, case, capfd)
    finally:
        dev.close()


def _ids(variant):
    c = IC.cases(variant)
    return dict(argvalues=list(c), ids=[c[k].pytest_id() for k in c])


@pytest.mark.parametrize("key", **_ids("scalar_rgb"))
def test_scalar_rgb(native, oracle, capfd, key):
    _run(native, oracle, capfd, "scalar_rgb", key)


@pytest.mark.parametrize("key", **_ids("scalar_spectral"))
def test_scalar_spectral(spectral, oracle_spectral, capfd, key):
    _run(spectral, oracle_spectral, capfd, "scalar_spectral", key)
