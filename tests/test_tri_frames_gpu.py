"""The per-triangle frame tables of the packet kernels (device/trace.h: stage_tables builds SceneView::tri_frames / emit_face_n in
LDS; miw/shape.h: TriFrame) on the GPU: every case renders 64 x 64 @ 16 spp on the device and through the oracle, which runs the
classic per-hit code; the film must be bit-identical and the sample and segment counts equal.

The cases are the smallest that reach every branch of the new code:
  * the diffuse Cornell box (32 triangles: 32-bit candidate masks, MATS_DIFFUSE, five wavefronts per SIMD), path and direct
    (the direct integrator's packet kernels stage the copies and build no tables — device/resident_kernel.h says why — so under
    `direct` every scene here runs the classic entry points next to the path kernels' tables);
  * the box with a level-0 icosphere (vertex normals) in place of the short block — 42 triangles: the 64-bit-mask kernel, flat and
    smooth shapes in one table (the smooth ones take n and dp_du from the record and build their frame per hit);
  * a packet scene with a texture-mapped flat panel (scenes._panel): dp_du from the uv determinant, the MATS_ALL kernel;
  * the glass-block box under scalar_spectral (libmiwave_spectral.so's packet kernel);
  * an area light that is a mesh of four non-coplanar faces plus a second emitter with vertex normals: emit_face_n is read for
    the one and not for the other, under path and direct;
  * the first case through mi_sample (its packet kernel stages no tables and builds none: it runs the classic entry points).
The oracle renders each of these scenes without a NaN pixel (checked on the CPU when the cases were chosen, and asserted here)."""
import numpy as np
import pytest

import sample_harness as H
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 64, 16


def _sensor(scenes, **kw):
    return scenes.cornell_sensor(W, HGT, SPP, **kw)


def smooth_ball_box_meshes(api, scenes):
    """the diffuse box, a level-0 icosphere with exact vertex normals in place of the short block: 32 - 10 + 20 = 42 triangles"""
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "short_block"]
    v, f, n = scenes.icosphere((185.0, 82.5, 169.0), 82.5, 0)
    meshes.append(api.Mesh("ball", v, f, normals=n, bsdf=api.BSDF("diffuse", reflectance=scenes.WHITE)))
    return meshes


def panel_box_meshes(api, scenes):
    """the diffuse box plus one free-standing quad with texture coordinates and a bitmap reflectance, seen from its front"""
    y, x = np.mgrid[0:8, 0:8]
    img = np.stack([0.2 + 0.6 * ((x + y) & 1), 0.15 + 0.1 * x, 0.8 - 0.09 * y], -1).astype(np.float32)
    tex = api.BitmapTexture(img, filter_type="nearest", wrap_mode="clamp")
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "tall_block"]
    meshes.append(scenes._panel("panel", [(470, 0, 300), (300, 0, 420), (300, 330, 420), (470, 330, 300)],
                                api.TwoSided(api.BSDF("diffuse", reflectance=tex))))
    return meshes


def two_emitter_box_meshes(api, scenes):
    """the box without its blocks; the ceiling light becomes a shallow four-sided pyramid (four faces, four different normals, all
    pointing down) and a small level-0 icosphere with vertex normals glows above the floor: 10 + 4 + 20 = 34 triangles"""
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name not in ("short_block", "tall_block", "light")]
    rim = np.array([(343, 548.0, 227), (343, 548.0, 332), (213, 548.0, 332), (213, 548.0, 227)], np.float32)
    apex = np.array([(278, 530.0, 279.5)], np.float32)
    v = np.concatenate([rim, apex])
    f = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], np.uint32)
    n = np.cross(v[1] - v[0], v[4] - v[0])
    if n[1] > 0:                                                 # geometric normals towards the room
        f = f[:, ::-1].copy()
    meshes.append(api.Mesh("light", v, f, emitter=api.AreaLight(scenes.LIGHT_RADIANCE)))
    bv, bf, bn = scenes.icosphere((150.0, 120.0, 200.0), 40.0, 0)
    meshes.append(api.Mesh("glow", bv, bf, normals=bn, emitter=api.AreaLight((2.0, 3.0, 5.0))))
    return meshes


def _scene(api, scenes, which):
    if which == "cornell":
        return api.Scene(scenes.cornell_box_meshes(diffuse_only=True)).build(-1)
    if which == "smooth_ball":
        return api.Scene(smooth_ball_box_meshes(api, scenes)).build(-1)
    if which == "panel":
        return api.Scene(panel_box_meshes(api, scenes)).build(-1)
    if which == "two_emitters":
        return api.Scene(two_emitter_box_meshes(api, scenes)).build(-1)
    if which == "glass_block":
        return api.Scene(scenes.cornell_box_meshes(diffuse_only=True, glass_block=True)).build(-1)
    raise ValueError(which)


TRIANGLES = {"cornell": 32, "smooth_ball": 42, "panel": 24, "two_emitters": 34, "glass_block": 34}


def _device_equals_oracle(api, orc, scene, job):
    """every film mode and launch shape of the resident plan against the oracle's film of the same job"""
    o32, o64, ost = orc.render(scene.desc(), job, threads=8)
    assert np.isfinite(o32).all() and o32[..., 4].min() > 0      # the reference side is clean
    d = api.Device(0)
    try:
        d.upload(scene.desc())
        for spl in (0, 3):
            g32, st = d.render(job, samples_per_launch=spl)
            c = d.counters()
            assert st == 0 and c.plan == 2 and c.film_mode == 1 and c.path_kernel == 0     # k_path_resident: the packet kernel
            assert c.samples == ost.samples == W * HGT * SPP and c.segments == ost.segments
            assert np.array_equal(g32, o32), "rel L2 %g" % parity.rel_l2(g32, o32)
    finally:
        d.close()


@pytest.mark.parametrize("which", ["cornell", "smooth_ball", "panel", "two_emitters"])
def test_path_film_bit_identical(native, oracle, which):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(native, scenes, which), _sensor(scenes)
    assert scene.desc().contents.face_count == TRIANGLES[which]
    dev = native.Device(0)
    try:
        # the comparison helper of test_gpu_parity.py: plans 1 / 2, one launch or several, both film modes
        g64, o32, o64, cnt, ost = parity._render_both(native, oracle, dev, scene, sensor)
    finally:
        dev.close()
    assert cnt.samples == ost.samples == W * HGT * SPP and cnt.segments == ost.segments
    assert np.isfinite(o32).all() and o32[..., 4].min() > 0


@pytest.mark.parametrize("which,kw", [("cornell", dict()), ("cornell", dict(emitter_samples=2, bsdf_samples=2)), ("two_emitters", dict(emitter_samples=3, bsdf_samples=1)),
                                      ("smooth_ball", dict()), ("panel", dict())])
def test_direct_film_bit_identical(native, oracle, which, kw):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(native, scenes, which), _sensor(scenes)
    _device_equals_oracle(native, oracle, scene, native.DirectIntegrator(**kw).render_job(sensor))


def test_spectral_glass_block_film_bit_identical(spectral, oracle_spectral):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(spectral, scenes, "glass_block"), _sensor(scenes)
    assert scene.desc().contents.face_count == TRIANGLES["glass_block"]
    _device_equals_oracle(spectral, oracle_spectral, scene, spectral.PathIntegrator().render_job(sensor))


def test_cornell_through_mi_sample(native, oracle):
    """mi_sample's packet kernel on the first case: the checker's float64 film of a box-filter job, reassembled from its results"""
    from mitsuba2_amd import scenes
    scene = _scene(native, scenes, "cornell")
    sensor = scenes.cornell_sensor(W, HGT, SPP, seed=H.BASE_SEED, rfilter="box")
    integ = native.PathIntegrator()
    job = integ.render_job(sensor)
    _, want, _ = oracle.render(scene.desc(), job, threads=8, want_f64=True)
    assert H.every_sample_in_its_texel(want, SPP)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        fn = lambda o, d, mint, maxt, wl, state: dev.sample(o, d, state, mint, maxt, wavelengths=wl, cfg=cfg)
        got = None
        for film in H.chain(oracle, job, fn, SPP):
            got = film
        bad = got.view(np.uint64) != want.view(np.uint64)
        assert not bad.any(), "%d of %d film words differ" % (bad.sum(), bad.size)
    finally:
        dev.close()
