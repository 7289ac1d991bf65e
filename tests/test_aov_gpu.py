"""The aov integrator on the GPU (mi_render_aov: k_aov_samples, k_sample_rays, k_aov_finish, k_aov_film).

Everything is compared against code that is itself pinned to the checker: the geometric channels against mi_ray_intersect on the
camera rays rebuilt in numpy (sample_harness.py: the numpy PCG32, pixels_and_seeds, the checker's camera-ray export), channels
0 .. 4 of a frame with a nested integrator against mi_render's film of that integrator, the child's raw spectrum against chained
mi_sample calls, the filtered channels against a float64 accumulation of ImageBlock::put with the checker's weights."""
import ctypes as C

import numpy as np
import pytest

import f64_aov as F
import sample_harness as H
from test_independent_integrators import RTOL

pytestmark = pytest.mark.gpu

W, HGT, SPP = H.GPU_W, H.GPU_H, 4
# The sampler seed of the box-filter jobs: the aov integrator draws three numbers per camera sample and nothing else, so where a
# pixel's samples fall follows from the seed alone; with this one no sample of the 96 x 64 x 4 job sits on its pixel's lower edge
# (_positions asserts it — on the CPU, from the numpy stream).
AOV_SEED = 0
GEO = ["depth", "position", "uv", "geo_normal", "sh_normal"]
ALL = GEO + ["dp_du", "dp_dv", "duv_dx", "duv_dy"]


def _scene(scenes, which, spp, w=W, h=HGT, rfilter="box", seed=AOV_SEED):
    kw = dict(device=-1, rfilter=rfilter, seed=seed)
    if which == "balls":
        return scenes.cornell_box(w, h, spp, diffuse_only=False, ball_level=1, **kw)
    if which.startswith("cutout"):                             # panels with texture coordinates, nested BSDF records; with the ball: a tree
        return scenes.cutout_box(w, h, spp, proxy=False, ball_level=1 if which == "cutout_ball" else None, **kw)
    return getattr(scenes, which)(w, h, spp, **kw)


def _positions(job, spp):
    """per sample j: (positions [n, 2] float32, sampler states after the three camera draws)"""
    px, py, seed = H.pixels_and_seeds(job)
    state, inc = H.pcg32_seed(seed)
    out = []
    for j in range(spp):
        jx, state = H.pcg32_next_f32(state)
        jy, state = H.pcg32_next_f32(state)
        _, state = H.pcg32_next_f32(state)
        pos = np.stack([px.astype(np.float32) + jx, py.astype(np.float32) + jy], 1)
        assert (jx != 0).all() and (jy != 0).all() and (pos[:, 0] > px).all() and (pos[:, 1] > py).all(), "a sample falls on its pixel's edge: pick another seed"
        out.append((pos, state.copy()))
    return px, py, out


def _offsets(types):
    off, k = {}, 5
    for t in types:
        off[t] = k; k += F.CHANNELS[t]
    return off, k


# ---------------------------------------------------------------- 1. geometric channels, box filter
@pytest.mark.parametrize("which", ["cornell_box", "rect_box", "sphere_box", "plugin_box", "balls", "cutout", "cutout_ball"])
def test_geometric_channels_equal_ray_intersect(native, oracle, which):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, which, SPP)
    job = native.PathIntegrator().render_job(sensor)
    px, py, samples = _positions(job, SPP)
    off, nch = _offsets(ALL)
    arr = F.scene_arrays(scene.desc().contents)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        film, st = dev.render_aov(job, native.aov_cfg(ALL))
        assert st == 0 and film.shape == (HGT, W, nch)
        want = np.zeros((HGT, W, nch), np.float32)
        du64, dv64, mag = np.zeros((HGT, W, 3)), np.zeros((HGT, W, 3)), np.zeros((HGT, W, 2))
        ty, tx = py - job.cfg.crop_y, px - job.cfg.crop_x
        hits = 0
        for pos, _ in samples:
            ray = oracle.eval(5, pos, cfg=job.cfg)
            o, d = np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6])
            si = dev.ray_intersect(o, d, ray[:, 6], ray[:, 7])
            hit = np.isfinite(si["t"])
            hits += hit.sum()
            z = lambda v: np.where(hit if v.ndim == 1 else hit[:, None], v, np.float32(0)).astype(np.float32)
            want[ty, tx, off["depth"]] += z(si["t"])                              # float32 running sums, in sample order
            want[ty, tx, off["position"]:off["position"] + 3] += z(si["p"])
            want[ty, tx, off["uv"]:off["uv"] + 2] += z(si["uv"])
            want[ty, tx, off["geo_normal"]:off["geo_normal"] + 3] += z(si["n"])
            want[ty, tx, off["sh_normal"]:off["sh_normal"] + 3] += z(si["sh_n"])
            want[ty, tx, 4] += np.float32(1)
            du, dv = F.partials_at(arr, si, o, d)
            du64[ty, tx] += du; dv64[ty, tx] += dv
            mag[ty, tx, 0] += np.linalg.norm(du, axis=1); mag[ty, tx, 1] += np.linalg.norm(dv, axis=1)
        assert 0.5 * SPP * W * HGT < hits
        assert (film[..., 0:4] == 0).all() and (film[..., 4] == SPP).all()
        lo, hi = off["depth"], off["sh_normal"] + 3
        bad = film[..., lo:hi] != want[..., lo:hi]
        assert not bad.any(), "%d of %d texel channels differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])
        assert (film[..., off["duv_dx"]:off["duv_dy"] + 2] == 0).all()
        # the partials: float32 on the device against the float64 restatement at the same primitive; a float32 vector errs relative to
        # its length, so the bound is RTOL x the summed lengths of the texel's terms
        for name, ref, m in (("dp_du", du64, mag[..., 0]), ("dp_dv", dv64, mag[..., 1])):
            err = np.abs(film[..., off[name]:off[name] + 3].astype(np.float64) - ref).max(-1)
            print("%s %s: max err / bound = %.3g" % (which, name, (err / np.maximum(RTOL * m, 1e-300)).max()))
            assert (err <= RTOL * m).all(), (name, np.argwhere(err > RTOL * m)[0])
    finally:
        dev.close()


# ---------------------------------------------------------------- 2. nested path / direct
def _integrator(api, kind):
    return api.PathIntegrator() if kind == "path" else api.DirectIntegrator(emitter_samples=1, bsdf_samples=1)


@pytest.mark.parametrize("size", [(70, 45), (96, 64)], ids=["70x45", "96x64"])
@pytest.mark.parametrize("kind", ["path", "direct"])
@pytest.mark.parametrize("which", ["cornell_box", "plugin_box"])
def test_nested_integrator_reproduces_mi_render(native, which, kind, size):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, which, SPP, size[0], size[1], rfilter="gaussian")
    integ = _integrator(native, kind)
    aov = native.AOVIntegrator(aovs="dd:depth,nn:sh_normal", nested=integ, name="img")
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        want, st = dev.render(integ.render_job(sensor))
        assert st == 0
        film, st = dev.render_aov(aov.render_job(sensor), aov.aov_cfg())
        assert st == 0 and film.shape == (size[1], size[0], 13)
        bad = film[..., :5].view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%d of %d film words differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])
        assert np.array_equal(film[..., 12].view(np.uint32), film[..., 3].view(np.uint32))       # img.A == A
        assert film[..., 9:12].sum() > 0 and film[..., 5].max() > 0
    finally:
        dev.close()


@pytest.mark.parametrize("kind", ["path", "direct"])
def test_child_spectrum_equals_chained_mi_sample(native, oracle, kind):
    """box filter: img.R .G .B .A are the float32 running sums of what mi_sample returns for the same rays, every sample starting from
    the sampler state the one before it left (sample_harness.BASE_SEED: the seed that module chose for these two integrators)"""
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, "cornell_box", SPP, seed=H.BASE_SEED)
    integ = _integrator(native, kind)
    aov = native.AOVIntegrator(aovs="", nested=integ, name="img")
    job = aov.render_job(sensor)
    px, py, seed = H.pixels_and_seeds(job)
    ty, tx = py - job.cfg.crop_y, px - job.cfg.crop_x
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        film, st = dev.render_aov(job, aov.aov_cfg())
        assert st == 0 and film.shape == (HGT, W, 9)
        want = np.zeros((HGT, W, 4), np.float32)
        state, _ = H.pcg32_seed(seed)
        for j in range(SPP):
            jx, state = H.pcg32_next_f32(state); jy, state = H.pcg32_next_f32(state); _, state = H.pcg32_next_f32(state)
            pos = np.stack([px.astype(np.float32) + jx, py.astype(np.float32) + jy], 1)
            assert (jx != 0).all() and (jy != 0).all() and (pos[:, 0] > px).all() and (pos[:, 1] > py).all(), "a sample falls on its pixel's edge: pick another seed"
            ray = oracle.eval(5, pos, cfg=job.cfg)
            spec, valid, state = dev.sample(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), state, ray[:, 6], ray[:, 7], cfg=integ.sample_cfg())
            want[ty, tx, 0:3] += spec.astype(np.float32)
            want[ty, tx, 3] += valid.astype(np.float32)
        assert np.array_equal(film[..., 5:9], want) and (film[..., 4] == SPP).all() and want[..., :3].sum() > 0
    finally:
        dev.close()


# ---------------------------------------------------------------- 3. gaussian AOV channels
def test_gaussian_channels_against_float64_put(native, oracle):
    from mitsuba2_amd import scenes
    from test_film_classes import _weights
    w, h, spp = 70, 45, 3
    scene, sensor = _scene(scenes, "cornell_box", spp, w, h, rfilter="gaussian")
    types = ["depth", "sh_normal"]
    job = native.PathIntegrator().render_job(sensor)
    px, py, seed = H.pixels_and_seeds(job)
    state, _ = H.pcg32_seed(seed)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        film, st = dev.render_aov(job, native.aov_cfg(types))
        assert st == 0 and film.shape == (h, w, 9)
        acc, mag = np.zeros((h, w, 5)), np.zeros((h, w, 5))                      # W, depth, sh_normal
        for j in range(spp):
            jx, state = H.pcg32_next_f32(state); jy, state = H.pcg32_next_f32(state); _, state = H.pcg32_next_f32(state)
            pos = np.stack([px.astype(np.float32) + jx, py.astype(np.float32) + jy], 1)
            ray = oracle.eval(5, pos, cfg=job.cfg)
            si = dev.ray_intersect(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), ray[:, 6], ray[:, 7])
            hit = np.isfinite(si["t"])
            val = np.concatenate([np.ones((len(px), 1)), np.where(hit, si["t"], 0)[:, None], np.where(hit[:, None], si["sh_n"], 0)], 1).astype(np.float64)
            _, _, wts, _ = _weights(native, oracle, sensor, 1, pos, np.stack([px, py], 1))
            reach = 2
            for b in range(8):
                for a in range(8):
                    wt = wts[:, b * 8 + a].astype(np.float64)
                    fx, fy = px - job.cfg.crop_x - reach + a, py - job.cfg.crop_y - reach + b
                    ok = (wt != 0) & (fx >= 0) & (fy >= 0) & (fx < w) & (fy < h)
                    np.add.at(acc, (fy[ok], fx[ok]), val[ok] * wt[ok, None])
                    np.add.at(mag, (fy[ok], fx[ok]), np.abs(val[ok] * wt[ok, None]))
        got = np.concatenate([film[..., 4:5], film[..., 5:9]], -1).astype(np.float64)
        err = np.abs(got - acc)
        print("gaussian channels: max err / (RTOL x sum |terms|) = %.3g" % (err / np.maximum(RTOL * mag, 1e-300)).max())
        assert (mag[..., 0] > 0).all() and (err <= RTOL * mag).all()
        assert (film[..., 0:4] == 0).all()
    finally:
        dev.close()


# ---------------------------------------------------------------- 4. determinism
def test_determinism_and_sample_by_sample_launches(native):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, "plugin_box", SPP, 70, 45, rfilter="gaussian")
    job = native.PathIntegrator().render_job(sensor)
    cfg = native.aov_cfg(ALL)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        a, _ = dev.render_aov(job, cfg)
        b, _ = dev.render_aov(job, cfg)
        c, _ = dev.render_aov(job, cfg, samples_per_launch=1)
        assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes() and np.abs(a).sum() > 0
        nested = native.aov_cfg(["depth"], "path")
        d, _ = dev.render_aov(job, nested)
        e, _ = dev.render_aov(job, nested)
        assert d.tobytes() == e.tobytes()
    finally:
        dev.close()


# ---------------------------------------------------------------- 5. refusals, the spectral library; 6. no state left behind
def test_refusals_leave_the_context_usable(native):
    from mitsuba2_amd import scenes
    scene, sensor = _scene(scenes, "cornell_box", SPP, 70, 45, rfilter="gaussian")
    path = native.PathIntegrator()
    job = path.render_job(sensor)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        before, _ = dev.render(job)
        shard = native.PathIntegrator(); shard.set_shard(1, 2)
        with pytest.raises(RuntimeError, match="tile shards"):
            dev.render_aov(shard.render_job(sensor), native.aov_cfg(["depth"]))
        for bad, msg in ((dict(n=33), "at most 32"), (dict(t=9), "Invalid AOV type"), (dict(size=4), "struct_size")):
            cfg = native.aov_cfg(["depth"])
            cfg.n_types = bad.get("n", 1); cfg.types[0] = bad.get("t", 0); cfg.struct_size += bad.get("size", 0)
            with pytest.raises(RuntimeError, match=msg):
                dev.render_aov(job, cfg)
        film, st = dev.render_aov(job, native.aov_cfg(["depth", "uv"], "direct"))
        assert st == 0
        after, _ = dev.render(path.render_job(sensor))
        assert before.tobytes() == after.tobytes()                                # 6: a path render before and after
    finally:
        dev.close()


def test_spectral_library_serves_the_geometric_channels_only(native, spectral):
    from mitsuba2_amd import scenes
    native.set_variant("scalar_rgb")
    scene, sensor = _scene(scenes, "plugin_box", SPP, 70, 45, rfilter="gaussian")
    job = native.PathIntegrator().render_job(sensor)
    dev = native.Device(0)
    try:
        dev.upload(scene.desc())
        rgb, _ = dev.render_aov(job, native.aov_cfg(ALL))
    finally:
        dev.close()
    native.set_variant("scalar_spectral")
    scene, sensor = _scene(scenes, "plugin_box", SPP, 70, 45, rfilter="gaussian")
    path = native.PathIntegrator()
    job = path.render_job(sensor)
    dev = native.Device(0)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        dev.upload(scene.desc())
        before, _ = dev.render(job)
        with pytest.raises(RuntimeError, match="scalar_rgb library only"):
            dev.render_aov(job, native.aov_cfg(["depth"], "path"))
        film, st = dev.render_aov(job, native.aov_cfg(ALL))
        assert st == 0 and film[..., 5:].tobytes() == rgb[..., 5:].tobytes() and film[..., :5].tobytes() == rgb[..., :5].tobytes()
        after, _ = dev.render(path.render_job(sensor))
        assert before.tobytes() == after.tobytes()
    finally:
        dev.close()


def test_host_class_renders_the_named_channels(native):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(48, 32, 2, device=0, seed=3)
    aov = native.AOVIntegrator(aovs="dd:depth,nn:sh_normal", nested=native.PathIntegrator(), name="img")
    assert aov.render(scene, sensor) is True
    film = sensor.film.data((32, 48, 13))
    path = native.PathIntegrator()
    scene2, sensor2 = scenes.cornell_box(48, 32, 2, device=0, seed=3)
    assert path.render(scene2, sensor2) is True
    assert film[..., :5].tobytes() == sensor2.film.data((32, 48, 5)).tobytes()
    names, img = sensor.film.bitmap()
    assert names == ["R", "G", "B", "A", "dd", "nn.X", "nn.Y", "nn.Z", "img.R", "img.G", "img.B", "img.A"]
    assert np.allclose(img[..., :3], sensor2.film.develop(), rtol=1e-6, atol=1e-7) and img[..., 4].max() > 100
