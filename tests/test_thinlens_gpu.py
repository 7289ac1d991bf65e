"""The general sensor route (mi_render_sensor, mi_sensor_sample_ray: k_sensor_step, k_sensor_rays) on the GPU.

The yardsticks: the device compile of the shared leaf equals the host compile word for word; for the sensor both routes know the
route's film is mi_render's film word for word; a thinlens film is the float32 film reassembled, sample after sample, from host-leaf
rays and chained mi_sample results (lens_harness.chain_lens — k_sample_rays is pinned against tests/f64_integrators.py elsewhere).
The shapes are the smallest at which the route can go wrong: a 40 x 24 film with block size 32 has two blocks, both clipped, one of
them 8 pixels wide, so lanes exist outside the film."""
import ctypes as C

import numpy as np
import pytest

import lens_harness as LH
import sample_harness as H

from conftest import has_gpu

pytestmark = pytest.mark.gpu
# (asked at collection, as the suite's other GPU modules do: torch opens the GPU before the library does, also when this file runs alone —
# the on_device cases hand the library torch tensors)
HAS_GPU = has_gpu()

W, HGT = 40, 24
# The sampler seed of the reassembly jobs of this file (40 x 24, 3 samples per pixel + one more): where a pixel's later samples fall
# depends on how many numbers the integrator drew for the earlier ones, so chain_lens asserts per job that no sample sits on its
# pixel's edge; with this seed the assertion holds in every job below.
BASE_SEED = 50000
LENS = dict(type="thinlens", aperture_radius=8.0, focus_distance=1000.0)


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_film(got, want, what):
    bad = _words(got) != _words(want)
    assert not bad.any(), "%s: %d of %d film words differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def _integrator(api, kind, **kw):
    return api.PathIntegrator(**kw) if kind == "path" else api.DirectIntegrator(emitter_samples=1, bsdf_samples=1, **kw)


def _scene(scenes, which, spp, **kw):
    kw = dict(dict(device=-1), **kw)
    if which == "cornell_box":
        return scenes.cornell_box(W, HGT, spp, **kw)
    if which == "balls":
        return scenes.cornell_box(W, HGT, spp, diffuse_only=False, ball_level=2, **kw)
    if which == "glass_block":
        return scenes.cornell_box(W, HGT, spp, diffuse_only=False, ball_level=1, glass_block=True, **kw)
    assert which == "point"
    return scenes.lit_box("point", W, HGT, spp, **kw)


# ---- 1. device leaf == host leaf -----------------------------------------------------------------------------------------------------
def _leaf_cases(api):
    from test_thinlens import make_camera
    yield make_camera(api, [1.0, 4.0, 1.5], [1.0, 0.0, 0.0], kind="perspective", principal_point_offset_x=0.1)
    yield make_camera(api, [1.0, 0.0, 1.5], [0.0, 0.0, 1.0], aperture=0.25, focus=15.0)
    yield make_camera(api, [1.0, 4.0, 1.5], [1.0, 0.0, 0.0], aperture=0.01, focus=1.0,
                      film_kw=dict(crop_width=200, crop_height=100, crop_offset_x=37, crop_offset_y=11))


def test_device_leaf_equals_host_leaf(native):
    rng = np.random.default_rng(1)
    dev = native.Device(0)
    try:
        for cam in _leaf_cases(native):
            job = native.PathIntegrator().render_job(cam)
            pos = rng.random((4096, 2)).astype(np.float32); ap = rng.random((4096, 2)).astype(np.float32)
            pos[:4] = [[0, 0], [1, 1], [.5, .5], [0, 1]]; ap[:4] = [[.5, .5], [0, 0], [1, 1], [.5, 0]]      # corners, the centre, the seams of the disk map
            want = cam.sample_rays(pos, ap)
            for on_device in (False, True):
                rays, wl, wt = dev.sensor_sample_ray(job, cam.desc(), pos, ap, on_device=on_device)
                assert np.array_equal(_words(rays), _words(want)), (cam.desc().type, on_device)
                assert wl is None and np.array_equal(wt, np.ones((4096, 3), np.float32))
            centred, _, _ = dev.sensor_sample_ray(job, cam.desc(), pos)                                 # no aperture array: (.5, .5)
            assert np.array_equal(_words(centred), _words(cam.sample_rays(pos)))
    finally:
        dev.close()


def test_device_leaf_spectral(spectral, oracle_spectral):
    """libmiwave_spectral: the rays as above, the wavelengths and weights against the checker's sample_wavelength (orc_spectral op 2)"""
    rng = np.random.default_rng(4)
    dev = spectral.Device(0)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        cam = list(_leaf_cases(spectral))[1]
        job = spectral.PathIntegrator().render_job(cam)
        n = 1024
        pos = rng.random((n, 2)).astype(np.float32); ap = rng.random((n, 2)).astype(np.float32); ws = rng.random(n).astype(np.float32)
        want_wl, want_wt = H.sample_wavelengths(oracle_spectral, ws)
        for on_device in (False, True):
            rays, wl, wt = dev.sensor_sample_ray(job, cam.desc(), pos, ap, wavelength_sample=ws, on_device=on_device)
            assert np.array_equal(_words(rays), _words(cam.sample_rays(pos, ap)))
            assert np.array_equal(_words(wl), _words(want_wl)) and np.array_equal(_words(wt), _words(want_wt))
    finally:
        dev.close()


# ---- 2. the route is mi_render's film for the sensor both know -------------------------------------------------------------------------
@pytest.mark.parametrize("which,kind", [("cornell_box", "path"), ("cornell_box", "direct"), ("balls", "path"), ("point", "path")])
def test_perspective_through_the_route_is_mi_renders_film(native, which, kind):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, which, 4)
    integ = _integrator(native, kind)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        want, st = dev.render(integ.render_job(sensor), film_mode=1)
        assert st == 0 and want[..., 4].sum() > 0
        got, st = dev.render_sensor(integ.render_job(sensor), sensor.desc(), profile=True)
        assert st == 0
        _same_film(got, want, "%s %s" % (which, kind))
        c = dev.counters()
        assert c.samples == W * HGT * 4 and c.ms_path > 0 and 0 < c.ms_init < c.ms_path and c.ms_film_blocks > 0 and c.ms_film_merge > 0 and c.ms_render > 0
    finally:
        dev.close()


def test_perspective_groups_passes_and_crop(native):
    from mitsuba2_amd import scenes
    dev = native.Device(0)
    try:
        scene, sensor = _scene(scenes, "cornell_box", 4)
        dev.upload(scene.desc())
        integ = native.PathIntegrator()
        want, _ = dev.render(integ.render_job(sensor), film_mode=1)
        desc = sensor.desc(); desc.debug_group_tiles = 1                                                # two groups of one tile
        got, st = dev.render_sensor(integ.render_job(sensor), desc)
        assert st == 0
        _same_film(got, want, "two groups")
        # two passes of 2 spp, the second accumulated onto the first (integrator.cpp:75-86)
        passes = native.PathIntegrator(samples_per_pass=2)
        assert passes.pass_count(sensor) == 2
        w0, _ = dev.render(passes.render_job(sensor, pass_index=0), film_mode=1)
        w1, _ = dev.render(passes.render_job(sensor, pass_index=1), film_mode=1, onto=w0)
        g0, _ = dev.render_sensor(passes.render_job(sensor, pass_index=0), sensor.desc())
        g1, _ = dev.render_sensor(passes.render_job(sensor, pass_index=1), sensor.desc(), onto=g0)
        _same_film(g0, w0, "pass 0"); _same_film(g1, w1, "pass 0 + pass 1")
        assert not np.array_equal(w1, want)                                                             # (other seeds than the one-pass frame)
        # a 48 x 32 film cropped to 40 x 24 at (5, 3)
        cropped = scenes.cornell_sensor(48, 32, 4, crop_width=W, crop_height=HGT, crop_offset_x=5, crop_offset_y=3)
        job = integ.render_job(cropped)
        assert (job.cfg.crop_x, job.cfg.crop_y, job.cfg.crop_w, job.cfg.crop_h) == (5, 3, W, HGT)
        want, _ = dev.render(integ.render_job(cropped), film_mode=1)
        got, st = dev.render_sensor(job, cropped.desc())
        assert st == 0
        _same_film(got, want, "crop")
    finally:
        dev.close()


# ---- 3. thinlens frames are the reassembled film -----------------------------------------------------------------------------------
def _host_fn(dev, cfg):
    def fn(o, d, mint, maxt, wl, state):
        return dev.sample(o, d, state, mint, maxt, wavelengths=wl, cfg=cfg)
    return fn


def _check_reassembly(api, oracle, dev, scene, integ, lens, spp=3, spectral=False):
    """render_sensor's film at spp and at spp + 1 (the sampler state after the last sample matters too) == chain_lens' film"""
    from mitsuba2_amd import scenes
    sensors = [scenes.cornell_sensor(W, HGT, n, seed=BASE_SEED, rfilter="box", sensor=lens) for n in (spp, spp + 1)]
    desc = sensors[0].desc()
    assert desc.type == 1 and sensors[0].needs_aperture_sample()
    jobs = [integ.render_job(s) for s in sensors]
    films = [f.copy() for f in LH.chain_lens(oracle, jobs[1], desc, sensors[0].sample_rays, _host_fn(dev, integ.sample_cfg()), spp + 1, spectral=spectral)]
    for job, want, what in ((jobs[0], films[spp - 1], "spp"), (jobs[1], films[spp], "spp + 1")):
        got, st = dev.render_sensor(job, desc)
        assert st == 0 and want[..., 4].min() == job.cfg.spp and want[..., :3].max() > 0
        _same_film(got, want, what)
    return films[spp - 1]


@pytest.mark.parametrize("kind", ["path", "direct"])
@pytest.mark.parametrize("which", ["cornell_box", "balls"])
def test_thinlens_film_is_the_reassembled_film(native, oracle, which, kind):
    from mitsuba2_amd import scenes, _capi
    scene, _ = _scene(scenes, which, 3)
    integ = _integrator(native, kind)
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):         # the scene's own route, and the tree walk forced
            dev.upload(scene.desc(), quality)
            _check_reassembly(native, oracle, dev, scene, integ, LENS)
    finally:
        dev.close()


def test_thinlens_film_with_a_shutter_time_and_against_the_pinhole(native, oracle):
    """shutter_open_time = 1: one more next_1d per sample shifts every later draw (integrator.cpp:248-250) — the film is the
    reassembled one again, and another film than without the shutter; the lens changes the film at all (aperture 8 against the pinhole)"""
    from mitsuba2_amd import scenes
    scene, pinhole = _scene(scenes, "cornell_box", 3, seed=BASE_SEED, rfilter="box")
    integ = native.PathIntegrator()
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        closed = _check_reassembly(native, oracle, dev, scene, integ, LENS)
        timed = _check_reassembly(native, oracle, dev, scene, integ, dict(LENS, shutter_open=0.5, shutter_close=1.5))
        assert not np.array_equal(closed, timed)
        plain, _ = dev.render(integ.render_job(pinhole), film_mode=1)
        assert not np.array_equal(plain, closed)
    finally:
        dev.close()


# ---- 4. spectral ------------------------------------------------------------------------------------------------------------------------
def test_thinlens_film_spectral_glass_block(spectral, oracle_spectral):
    from mitsuba2_amd import scenes, _capi
    scene, _ = _scene(scenes, "glass_block", 3)
    dev = spectral.Device(0)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        dev.upload(scene.desc(), 1 | _capi.MI_BVH_FORCE_TREE)
        _check_reassembly(spectral, oracle_spectral, dev, scene, spectral.PathIntegrator(), LENS, spectral=True)
    finally:
        dev.close()


# ---- 5. through the public classes -------------------------------------------------------------------------------------------------
XML = """<scene version="2.0.0">
    <integrator type="path"><integer name="max_depth" value="5"/><integer name="rr_depth" value="3"/></integrator>
    <sensor type="thinlens">
        <float name="fov" value="39.3"/>
        <float name="aperture_radius" value="8"/>
        <float name="focus_distance" value="1000"/>
        <transform name="to_world"><lookat origin="278, 273, -800" target="278, 273, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sample_count" value="4"/><integer name="seed" value="7"/></sampler>
        <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/><rfilter type="gaussian"/></film>
    </sensor>
    <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.725, 0.71, 0.68"/></bsdf>
    <shape type="rectangle">
        <transform name="to_world"><scale x="278" y="280" z="1"/><rotate x="1" angle="-90"/><translate x="278" y="0" z="280"/></transform>
        <ref id="white"/>
    </shape>
    <shape type="rectangle">
        <transform name="to_world"><scale value="278"/><rotate y="1" angle="180"/><translate x="278" y="278" z="559"/></transform>
        <ref id="white"/>
    </shape>
    <shape type="obj">
        <string name="filename" value="%s"/>
        <bsdf type="diffuse"><spectrum name="reflectance" value="0"/></bsdf>
        <emitter type="area"><rgb name="radiance" value="17, 12, 4"/></emitter>
    </shape>
</scene>"""
SERVED = "thinlens sensor is served for the path and direct integrators only"


def test_public_classes_and_refusals(native, tmp_path):
    from mitsuba2_amd import scenes, _capi
    (tmp_path / "light.obj").write_text("v 343 548 227\nv 343 548 332\nv 213 548 332\nv 213 548 227\nf 4 3 2 1\n")
    scene, sensor, integ = native.load_string(XML % (tmp_path / "light.obj"))
    assert isinstance(sensor, native.ThinLensCamera)
    scene.build(0)
    assert integ.render(scene, sensor) is True
    from_xml = sensor.film.data((HGT, W, 5)).copy()
    by_hand = native.ThinLensCamera(native.Film(rfilter="gaussian", width=W, height=HGT), native.Sampler(sample_count=4, seed=7), fov=39.3,
                                    aperture_radius=8.0, focus_distance=1000.0, to_world=dict(origin=(278, 273, -800), target=(278, 273, 0), up=(0, 1, 0)))
    path = native.PathIntegrator(max_depth=5, rr_depth=3)
    assert path.render(scene, by_hand) is True and path.counters().samples == W * HGT * 4
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        want, st = dev.render_sensor(path.render_job(by_hand), by_hand.desc())
        assert st == 0 and want[..., :3].max() > 0
        _same_film(from_xml, want, "xml"); _same_film(by_hand.film.data((HGT, W, 5)), want, "classes")
        # two passes through the classes == two passes through the ABI
        passes = native.PathIntegrator(max_depth=5, rr_depth=3, samples_per_pass=2)
        assert passes.render(scene, by_hand) is True
        g0, _ = dev.render_sensor(passes.render_job(by_hand, pass_index=0), by_hand.desc())
        g1, _ = dev.render_sensor(passes.render_job(by_hand, pass_index=1), by_hand.desc(), onto=g0)
        _same_film(by_hand.film.data((HGT, W, 5)), g1, "passes")

        # what the route does not serve says so
        with pytest.raises(RuntimeError, match=SERVED):
            native.MomentIntegrator(native.PathIntegrator()).render(scene, by_hand)
        with pytest.raises(RuntimeError, match=SERVED):
            native.AOVIntegrator("dd:depth", nested=native.PathIntegrator()).render(scene, by_hand)
        shard = native.PathIntegrator(); shard.set_shard(0, 2)
        with pytest.raises(RuntimeError, match=SERVED):
            shard.render(scene, by_hand)
        job = shard.render_job(by_hand)
        assert job.cfg.tile_list
        with pytest.raises(RuntimeError, match="tile_list"):
            dev.render_sensor(job, by_hand.desc())
        job = path.render_job(by_hand); job.cfg.film_f64 = 1
        with pytest.raises(RuntimeError, match="film_f64"):
            dev.render_sensor(job, by_hand.desc())
        for field, value in (("film_mode", 2), ("plan", 1), ("moment_pass", 1)):
            job = path.render_job(by_hand); setattr(job.cfg, field, value)
            with pytest.raises(RuntimeError, match=field):
                dev.render_sensor(job, by_hand.desc())
        bad = by_hand.desc(); bad.type = 7
        with pytest.raises(RuntimeError, match="type 7"):
            dev.render_sensor(path.render_job(by_hand), bad)
        job = path.render_job(by_hand); job.cfg.timeout_s = 1e-6
        _, st = dev.render_sensor(job, by_hand.desc())
        assert st == _capi.MI_ERR_CANCELLED
        again, st = dev.render_sensor(path.render_job(by_hand), by_hand.desc())                         # ... and the context renders on
        assert st == 0
        _same_film(again, want, "after a cancelled frame")
    finally:
        dev.close()
    multi, _ = scenes.cornell_box(W, HGT, 4, device=-1)
    multi.build([0, 0])
    with pytest.raises(RuntimeError, match=SERVED):
        native.PathIntegrator().render(multi, by_hand)


# ---- 6. nothing else moved ----------------------------------------------------------------------------------------------------------
def test_perspective_frames_keep_their_kernels(native):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(32, 24, 1)
    integ = native.PathIntegrator()
    assert integ.render(scene, sensor) is True
    c = integ.counters()
    assert c.plan == 2 and c.path_kernel == 0 and c.tree_width == 0
