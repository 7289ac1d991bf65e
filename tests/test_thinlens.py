"""The thinlens sensor on the CPU tier: the shared leaf (csrc/miw/lens.h) as the host library compiles it against the float64
restatement of tests/f64_sensors.py, the reference's own properties of the sensor (src/sensors/tests/test_thinlens.py), the
constructor and the XML loader, and the ABI mirror of mi_sensor_desc."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import f64_sensors as F
from f64_integrators import disk_concentric
from conftest import ROOT

EPS = 2.0 ** -23                                                 # float32 epsilon
ORIGINS = [[1.0, 0.0, 1.5], [1.0, 4.0, 1.5]]
DIRECTIONS = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
APERTURES = [0.01, 0.1, 0.25]
FOCUS = [1.0, 15.0, 25.0]
N = 4096


def make_camera(api, o, d, fov=34.0, fov_axis="x", aperture=0.1, focus=15.0, film_kw=None, kind="thinlens", **kw):
    """create_camera of the reference's test (:6-37): film 512 x 256, near 1, far 35, shutter 1.5 .. 5"""
    film = api.Film(rfilter="gaussian", width=512, height=256, **(film_kw or {}))
    sampler = api.Sampler(sample_count=4, seed=0)
    t = [o[0] + d[0], o[1] + d[1], o[2] + d[2]]
    p = dict(near_clip=1.0, far_clip=35.0, fov=float(fov), fov_axis=fov_axis, to_world=dict(origin=o, target=t, up=(0, 1, 0)))
    if kind == "perspective":
        return api.Sensor(film, sampler, **p, **kw)
    return api.ThinLensCamera(film, sampler, focus_distance=float(focus), aperture_radius=float(aperture), shutter_open=1.5, shutter_close=5.0, **p, **kw)


def grid():
    for o, d, a, f in itertools.product(ORIGINS, DIRECTIONS, APERTURES, FOCUS):
        yield o, d, a, f, None
    yield ORIGINS[0], DIRECTIONS[0], 0.1, 15.0, dict(crop_width=200, crop_height=100, crop_offset_x=37, crop_offset_y=11)


# what test_host_leaf_against_float64 measured on an x86-64 CPU (glibc libm, numpy float64), in float32 epsilons (2^-23), the largest
# over the 37 cameras x 4096 pairs; the test asserts twice these (the margin is for another libm or compiler on the FLOAT64 side —
# the float32 leaf is deterministic):
MEASURED_EPS = dict(o=205.980, d=1.119, t=1.852)


def test_host_leaf_against_float64(native):
    """ThinLensCamera.sample_rays (the host compile of thinlens_sample_ray) against f64_sensors.Camera.thinlens_sample_ray on the
    reference's grid of cameras and one cropped film, 4 096 random (position, aperture) pairs each, none excluded.
    Measured (float32 epsilons): |o - o64| / aperture_radius 205.980 (the origin is rounded at the size of the world coordinates, up to 4, and divided by radii down to 0.01), |d - d64| 1.119, relative mint / maxt 1.852."""
    rng = np.random.default_rng(1)
    worst = dict(o=0.0, d=0.0, t=0.0)
    for o, d, a, f, film_kw in grid():
        cam = make_camera(native, o, d, aperture=a, focus=f, film_kw=film_kw)
        kw = {} if film_kw is None else dict(crop_size=(film_kw["crop_width"], film_kw["crop_height"]), crop_offset=(film_kw["crop_offset_x"], film_kw["crop_offset_y"]))
        ref = F.Camera((512, 256), o, d, aperture_radius=a, focus_distance=f, **kw)
        pos = rng.random((N, 2)).astype(np.float32); ap = rng.random((N, 2)).astype(np.float32)
        got = cam.sample_rays(pos, ap).astype(np.float64)
        for i in range(N):
            o64, d64, mint64, maxt64 = ref.thinlens_sample_ray(pos[i].astype(np.float64), ap[i].astype(np.float64))
            worst["o"] = max(worst["o"], np.linalg.norm(got[i, 0:3] - o64) / a)
            worst["d"] = max(worst["d"], np.linalg.norm(got[i, 3:6] - d64))
            worst["t"] = max(worst["t"], abs(got[i, 6] - mint64) / mint64, abs(got[i, 7] - maxt64) / maxt64)
    seen = {k: v / EPS for k, v in worst.items()}
    print("thinlens host leaf vs float64, float32 epsilons: |o - o64| / r %.3f, |d - d64| %.3f, relative mint / maxt %.3f" % (seen["o"], seen["d"], seen["t"]))
    for k in seen:
        assert seen[k] <= 2.0 * MEASURED_EPS[k], (k, seen[k], MEASURED_EPS[k])


@pytest.mark.parametrize("o,d,a,f", list(itertools.product(ORIGINS, DIRECTIONS, APERTURES, FOCUS)))
def test_reference_properties(native, o, d, a, f):
    """src/sensors/tests/test_thinlens.py:88-110"""
    cam = make_camera(native, o, d, aperture=a, focus=f)
    assert cam.needs_aperture_sample()
    centre = cam.sample_ray(.5, .5, .5, .5)
    assert np.allclose(centre[3:6], d, atol=1e-7, rtol=0)
    assert np.allclose(centre[0:3], o)
    to_world = F.look_at(o, np.add(o, d), (0, 1, 0))
    for ax, ay in zip([0.9, 0.4, 0.2], [0.6, 0.9, 0.7]):
        ray = cam.sample_ray(.5, .5, ax, ay)
        tx, ty = disk_concentric((ax, ay))
        aperture_v = to_world[:3, :3] @ np.array([a * tx, a * ty, 0.0])
        assert np.allclose(ray[0:3], centre[0:3] + aperture_v)
        want = centre[3:6].astype(np.float64) * f - aperture_v            # (near_clip = 1)
        assert np.allclose(ray[3:6], want / np.linalg.norm(want))


@pytest.mark.parametrize("d", DIRECTIONS)
@pytest.mark.parametrize("fov", [34, 80])
def test_fov_axis(native, d, fov):
    """:190-218 — the extremities of the unit square along the fov axis make the angle fov / 2 with the camera direction"""
    o = ORIGINS[0]

    def check(cam, sample):
        ray = cam.sample_ray(sample[0], sample[1], .5, .5)
        assert np.allclose(math.degrees(math.acos(float(np.dot(ray[3:6], d)))), fov / 2)

    for axis in ("x", "larger"):                                  # aspect 2: `larger` is x
        for s in ([0.0, 0.5], [1.0, 0.5]):
            check(make_camera(native, o, d, fov=fov, fov_axis=axis), s)
    for axis in ("y", "smaller"):
        for s in ([0.5, 0.0], [0.5, 1.0]):
            check(make_camera(native, o, d, fov=fov, fov_axis=axis), s)
    for s in ([0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]):
        check(make_camera(native, o, d, fov=fov, fov_axis="diagonal"), s)


def test_rays_of_one_position_meet_on_the_focus_plane(native):
    """Every ray of one position sample passes through the same point of the plane z = focus_distance (camera space): the points
    o_cam + d_cam * (focus / d_cam.z) of 256 aperture samples spread by less than 64 * 2^-23 * focus — focus_p carries one rounding
    of the quotient and one of the product, the difference focus_p - aperture_p one, normalize three (dot, rsqrt, product), and
    the reconstruction here one division and a product-sum in float64 of float32 inputs: half a dozen roundings of relative size
    2^-24 on a quantity of the size of focus, times the conditioning of the intersection (d_cam.z close to 1), far below 64."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for a, f in itertools.product(APERTURES, FOCUS):
        cam = make_camera(native, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], aperture=a, focus=f)      # camera space = world space up to the sign of x
        for px, py in rng.random((8, 2)):
            ap = rng.random((256, 2)).astype(np.float32)
            rays = cam.sample_rays(np.tile(np.float32([px, py]), (256, 1)), ap).astype(np.float64)
            hit = rays[:, 0:3] + rays[:, 3:6] * ((f - rays[:, 2:3]) / rays[:, 5:6])
            spread = np.linalg.norm(hit - hit.mean(0), axis=1).max()
            worst = max(worst, spread / f)
            assert spread < 64 * EPS * f, (a, f, spread)
    print("focus-plane spread, largest over the cameras: %.3f float32 epsilons of the focus distance" % (worst / EPS))


def test_sensor_sample_with_the_perspective_kind(native):
    """sensor_sample(PERSPECTIVE) is Sensor.sample_ray bit for bit, whatever the aperture sample"""
    rng = np.random.default_rng(3)
    cam = make_camera(native, ORIGINS[1], DIRECTIONS[1], kind="perspective", principal_point_offset_x=0.1)
    assert not cam.needs_aperture_sample() and cam.desc().type == 0 and cam.desc().struct_size == C.sizeof(cam.desc())
    pos = rng.random((N, 2)).astype(np.float32); ap = rng.random((N, 2)).astype(np.float32)
    got = cam.sample_rays(pos, ap)
    want = np.stack([cam.sample_ray(x, y) for x, y in pos])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cam.sample_rays(pos).view(np.uint32), want.view(np.uint32))
    ref = F.Camera((512, 256), ORIGINS[1], DIRECTIONS[1])         # ... and the float64 perspective camera agrees to a few epsilons
    plain = make_camera(native, ORIGINS[1], DIRECTIONS[1], kind="perspective")
    for i in range(0, N, 64):
        o64, d64, mint64, maxt64 = ref.perspective_sample_ray(pos[i].astype(np.float64))
        r = plain.sample_ray(pos[i, 0], pos[i, 1]).astype(np.float64)
        assert np.linalg.norm(r[3:6] - d64) < 8 * EPS and abs(r[6] - mint64) < 8 * EPS * mint64 and np.array_equal(r[0:3], o64)


XML = """<scene version="2.0.0">
    <integrator type="path"/>
    <sensor type="%s">
        %s
        <float name="fov" value="39.3"/>
        <transform name="to_world">%s<lookat origin="278, 273, -800" target="278, 273, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sample_count" value="4"/></sampler>
        <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/><rfilter type="box"/></film>
    </sensor>
    <shape type="rectangle"/>
</scene>"""


def test_constructor_and_xml(native):
    film = lambda: native.Film(rfilter="box", width=40, height=24)
    sampler = lambda: native.Sampler(sample_count=4, seed=0)
    scene, sensor, integ = native.load_string(XML % ("thinlens", '<float name="aperture_radius" value="0.25"/><float name="far_clip" value="900"/>', ""))
    assert isinstance(sensor, native.ThinLensCamera) and sensor.needs_aperture_sample()
    d = sensor.desc()
    assert (d.struct_size, d.type, d.aperture_radius, d.focus_distance, d.shutter_open, d.shutter_open_time) == (C.sizeof(d), 1, 0.25, 900.0, 0.0, 0.0)   # focus_distance = far_clip
    job = integ.render_job(sensor)
    assert (job.cfg.crop_w, job.cfg.crop_h, job.cfg.spp, job.cfg.far_clip) == (40, 24, 4, 900.0)
    _, sensor, _ = native.load_string(XML % ("thinlens", '<float name="aperture_radius" value="2"/><float name="focus_distance" value="7"/>'
                                             '<float name="shutter_open" value="1"/><float name="shutter_close" value="3.5"/>', ""))
    d = sensor.desc()
    assert (d.aperture_radius, d.focus_distance, d.shutter_open, d.shutter_open_time) == (2.0, 7.0, 1.0, 2.5)
    _, sensor, _ = native.load_string(XML % ("perspective", "", ""))
    assert type(sensor) is native.Sensor and not sensor.needs_aperture_sample() and sensor.desc().type == 0
    with pytest.raises(RuntimeError, match='Property "aperture_radius" has not been specified'):
        native.ThinLensCamera(film(), sampler(), fov=40.0)
    with pytest.raises(RuntimeError, match='Property "aperture_radius" has not been specified'):
        native.load_string(XML % ("thinlens", "", ""))
    zero = native.ThinLensCamera(film(), sampler(), fov=40.0, aperture_radius=0.0)
    assert zero.desc().aperture_radius == 2.0 ** -24
    with pytest.raises(RuntimeError, match="Shutter opening time must be less than or equal to the shutter closing time"):
        native.ThinLensCamera(film(), sampler(), fov=40.0, aperture_radius=1.0, shutter_open=2.0, shutter_close=1.0)
    with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed"):
        native.load_string(XML % ("thinlens", '<float name="aperture_radius" value="1"/>', '<scale value="2"/>'))
    with pytest.raises(RuntimeError, match='Plugin "orthographic" not found'):
        native.load_string(XML % ("orthographic", "", ""))
    # the scene builders' sensor= keyword: a dict or a callable; without it nothing changes
    from mitsuba2_amd import scenes
    s = scenes.cornell_sensor(40, 24, 4, sensor=dict(type="thinlens", aperture_radius=8.0, focus_distance=1000.0))
    assert isinstance(s, native.ThinLensCamera) and s.desc().focus_distance == 1000.0
    s = scenes.cornell_sensor(40, 24, 4, sensor=lambda film, sampler: native.ThinLensCamera(film, sampler, fov=20.0, aperture_radius=1.0))
    assert s.desc().aperture_radius == 1.0
    assert type(scenes.cornell_sensor(40, 24, 4)) is native.Sensor
    job = native.DirectIntegrator().render_job(s)
    assert job.cfg.integrator == 1 and job.cfg.principal_point_offset[0] == 0.0


def test_sensor_desc_mirror_matches_the_header(tmp_path):
    """mi_sensor_desc of _capi.py has the header's size and offsets, and the library's two new entry points are declared"""
    from mitsuba2_amd import _capi
    cls = _capi.mi_sensor_desc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "miwave.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(mi_sensor_desc));']
    lines += ['  printf("%s %%zu\\n", offsetof(mi_sensor_desc, %s));' % (f[0], f[0]) for f in cls._fields_]
    lines += ['  printf("enum %d\\n", MI_SENSOR_PERSPECTIVE + 10 * MI_SENSOR_THINLENS);', '  return 0;', '}']
    src = tmp_path / "desc.c"; src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "desc")])
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "desc")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(cls) == 28
    assert int(out.pop("enum")) == _capi.MI_SENSOR_PERSPECTIVE + 10 * _capi.MI_SENSOR_THINLENS == 10
    assert len(out) == 7 and all(int(v) == getattr(cls, k).offset for k, v in out.items())
    assert "mi_render_sensor" in _capi.MI_SYMBOLS and "mi_sensor_sample_ray" in _capi.MI_SYMBOLS
    lib = _capi.load_device_lib()
    assert lib.mi_render_sensor and lib.mi_sensor_sample_ray
    # the description is checked before the context: an unknown size or type is MI_ERR_INVALID with no context at all
    d = cls(struct_size=C.sizeof(cls) + 4, type=0)
    assert lib.mi_render_sensor(None, None, C.byref(d), None) == _capi.MI_ERR_INVALID and b"struct_size" in lib.mi_last_error(None)
    d = cls(struct_size=C.sizeof(cls), type=7)
    assert lib.mi_render_sensor(None, None, C.byref(d), None) == _capi.MI_ERR_INVALID and b"type 7" in lib.mi_last_error(None)
    for bad in (dict(aperture_radius=0.0, focus_distance=1.0), dict(aperture_radius=1.0, focus_distance=float("nan")), dict(aperture_radius=float("inf"), focus_distance=1.0)):
        d = cls(struct_size=C.sizeof(cls), type=1, **bad)
        assert lib.mi_sensor_sample_ray(None, None, C.byref(d), None, None, None, None, None, None, 0, 0) == _capi.MI_ERR_INVALID
        assert b"aperture_radius" in lib.mi_last_error(None) or b"focus_distance" in lib.mi_last_error(None)
