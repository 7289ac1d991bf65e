"""Point, spot, directional and constant emitters — the tier that needs no GPU: the C ABI record (mi_light) against its ctypes
mirror, XML / Python / description packing with the emitter order, the refusals the host layer raises, the float32 leaves of
csrc/miw/light.h against closed forms (a host program compiled from the header), and the share of samples the float64
restatement (tests/f64_lights.py) excludes in the jobs of the GPU tier.

No description with light_count > 0 is handed to the CPU checker: it has no record for a shapeless emitter."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import f64_integrators as F
import f64_lights as FL
import sample_harness as H
from conftest import ROOT


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_mi_light_mirror_matches_the_header(tmp_path):
    from mitsuba2_amd import _capi
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "miwave.h"', 'int main(void) {']
    for n in ("mi_light", "mi_scene_desc"):
        cls = getattr(_capi, n)
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (n, n))
        for f in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (n, f[0], n, f[0]))
    lines += ['  printf("enum point %d\\n", MI_LIGHT_POINT); printf("enum spot %d\\n", MI_LIGHT_SPOT);',
              '  printf("enum directional %d\\n", MI_LIGHT_DIRECTIONAL); printf("enum constant %d\\n", MI_LIGHT_CONSTANT);', '  return 0;', '}']
    src = tmp_path / "abi.c"; src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi")])
    out = subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        n, field, value = line.split()
        if n == "enum":
            assert getattr(_capi, "MI_LIGHT_" + field.upper()) == int(value)
            continue
        cls = getattr(_capi, n)
        mine = C.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert mine == int(value), "%s.%s: header %s, ctypes %d" % (n, field, value, mine)
        seen += 1
    assert seen == 2 + len(_capi.mi_light._fields_) + len(_capi.mi_scene_desc._fields_)
    # appended: the members every earlier caller knows keep their offsets, `lights` comes after all of them
    d = _capi.mi_scene_desc
    assert d.lights.offset > d.bsdf_table_floats.offset and d.light_count.offset > d.lights.offset


# ---- records from Python -------------------------------------------------------------------------------------------------
def _rec(light):
    return light.record()


def test_point_record(native):
    from mitsuba2_amd import _capi
    r = _rec(native.PointLight(position=(1.0, 2.0, 3.0), intensity=(4.0, 5.0, 6.0)))
    assert r.type == _capi.MI_LIGHT_POINT and list(r.position) == [1.0, 2.0, 3.0] and list(r.value) == [4.0, 5.0, 6.0]
    m = np.eye(4, dtype=np.float32); m[:3, 3] = (7, 8, 9)
    r = _rec(native.PointLight(to_world=m))
    assert list(r.position) == [7.0, 8.0, 9.0] and list(r.value) == [1.0, 1.0, 1.0]       # default intensity: D65(1) ~ white
    with pytest.raises(RuntimeError, match="position.*to_world"):
        native.PointLight(position=(0.0, 0.0, 0.0), to_world=m)


def test_spot_record_and_defaults(native):
    from mitsuba2_amd import _capi
    f32 = np.float32
    r = _rec(native.SpotLight(to_world=dict(origin=(1, 2, 3), target=(1, 0, 3), up=(0, 0, 1))))
    assert r.type == _capi.MI_LIGHT_SPOT and list(r.position) == [1.0, 2.0, 3.0]
    cutoff, beam = f32(20.0) * f32(math.pi / 180.0), f32(20.0) * f32(3.0) / f32(4.0) * f32(math.pi / 180.0)     # spot.cpp:88-91
    assert r.cutoff_angle == cutoff and r.beam_width == beam
    assert r.inv_transition_width == f32(1.0) / (cutoff - beam)
    assert abs(r.cos_cutoff_angle - math.cos(cutoff)) < 1e-7 and abs(r.cos_beam_width - math.cos(beam)) < 1e-7 and abs(r.uv_factor - math.tan(cutoff)) < 1e-7
    tw, to = np.array(r.to_world).reshape(4, 4).T, np.array(r.to_object).reshape(4, 4).T
    assert np.allclose(tw @ to, np.eye(4), atol=1e-5) and np.allclose(tw[:3, 2], (0, -1, 0), atol=1e-6)    # points along +z of its frame
    r = _rec(native.SpotLight(cutoff_angle=40.0, beam_width=10.0))
    assert r.cutoff_angle == f32(40.0) * f32(math.pi / 180.0) and r.beam_width == f32(10.0) * f32(math.pi / 180.0)
    with pytest.raises(RuntimeError, match="cutoff_angle"):
        native.SpotLight(cutoff_angle=10.0, beam_width=20.0)


def test_spot_with_a_texture_child_is_refused(native):
    tex = native.BitmapTexture(np.ones((2, 2, 3), np.float32))
    with pytest.raises(RuntimeError, match="texture"):
        native.SpotLight(texture=tex)


def test_directional_record(native):
    from mitsuba2_amd import _capi
    r = _rec(native.DirectionalEmitter(direction=(0.0, -3.0, 4.0), irradiance=(2.0, 2.0, 2.0)))
    assert r.type == _capi.MI_LIGHT_DIRECTIONAL and np.allclose(list(r.direction), (0.0, -0.6, 0.8), atol=1e-6) and list(r.value) == [2.0, 2.0, 2.0]
    assert abs(np.linalg.norm(list(r.direction)) - 1) < 1e-6
    r = _rec(native.DirectionalEmitter(to_world=dict(origin=(0, 0, 0), target=(0, -1, 0), up=(0, 0, 1))))
    assert np.allclose(list(r.direction), (0, -1, 0), atol=1e-6)
    with pytest.raises(RuntimeError, match="direction.*to_world"):
        native.DirectionalEmitter(direction=(0.0, 0.0, 1.0), to_world=np.eye(4, dtype=np.float32))


def test_constant_record(native):
    from mitsuba2_amd import _capi
    r = _rec(native.ConstantBackgroundEmitter(radiance=(0.25, 0.5, 0.75)))
    assert r.type == _capi.MI_LIGHT_CONSTANT and list(r.value) == [0.25, 0.5, 0.75]


# ---- the scene: emitter order, bounding sphere, one environment emitter -----------------------------------------------------
def _quad_mesh(native, name, y, emitter=None):
    v = np.array([[-1, y, -1], [1, y, -1], [1, y, 1], [-1, y, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return native.Mesh(name, v, f, bsdf=None if emitter else native.BSDF("diffuse"), emitter=emitter)


def test_emitter_order_with_envmap_and_area_lights_in_between(native):
    """children in declaration order: point | area a | envmap, spot | area b | constant-free tail directional"""
    from mitsuba2_amd import _capi
    shapes = [_quad_mesh(native, "a", 0.0, native.AreaLight((1.0, 1.0, 1.0))), _quad_mesh(native, "floor", -1.0),
              _quad_mesh(native, "b", 2.0, native.AreaLight((2.0, 2.0, 2.0)))]
    env = native.EnvMap(np.ones((4, 8, 3), np.float32))
    point, spot, direc = native.PointLight(position=(0.0, 5.0, 0.0)), native.SpotLight(), native.DirectionalEmitter(direction=(0.0, -1.0, 0.0))
    scene = native.Scene(shapes, envmap=env, envmap_after=1, lights=[(point, 0), (spot, 1), direc]).build(-1)
    d = scene.desc().contents
    assert d.light_count == 3 and d.emitter_count == 2 and scene.emitter_count() == 6
    by_type = {d.lights[k].type: d.lights[k].emitter_index for k in range(3)}
    # point, area a, envmap, spot, area b, directional
    assert by_type == {_capi.MI_LIGHT_POINT: 0, _capi.MI_LIGHT_SPOT: 3, _capi.MI_LIGHT_DIRECTIONAL: 5}
    assert d.envmap.contents.emitter_index == 2
    assert [d.shapes[i].emitter for i in range(3)] == [0, -1, 1]           # mi_shape::emitter indexes mi_scene_desc::emitters, unshifted
    # the bounding sphere of the scene's box, for the emitters that need it (set_scene)
    lo, hi = scene.bbox()
    c = (lo + hi) / 2
    for k in range(3):
        assert np.allclose(list(d.lights[k].bsphere_center), c) and abs(d.lights[k].bsphere_radius - np.linalg.norm(c - hi)) < 1e-5
    assert abs(d.envmap.contents.bsphere_radius - d.lights[0].bsphere_radius) == 0


def test_scene_without_lights_packs_as_before(native):
    from mitsuba2_amd import scenes
    scene, _ = scenes.cornell_box(16, 16, 1, device=-1)
    d = scene.desc().contents
    assert d.light_count == 0 and not d.lights and d.emitter_count == 1


def test_one_environment_emitter_per_scene(native):
    shapes = [_quad_mesh(native, "floor", 0.0)]
    const = native.ConstantBackgroundEmitter()
    with pytest.raises(RuntimeError, match="Only one environment emitter"):
        native.Scene(shapes, envmap=native.EnvMap(np.ones((4, 8, 3), np.float32)), lights=[const])
    with pytest.raises(RuntimeError, match="Only one environment emitter"):
        native.Scene(shapes, lights=[native.ConstantBackgroundEmitter(), native.ConstantBackgroundEmitter()])


XML = """<scene version="2.0.0">
    <emitter type="point"><point name="position" x="1" y="2" z="3"/><rgb name="intensity" value="10, 20, 30"/></emitter>
    <shape type="rectangle"><bsdf type="diffuse"/><emitter type="area"><rgb name="radiance" value="1, 1, 1"/></emitter></shape>
    <emitter type="spot"><transform name="to_world"><lookat origin="0, 4, 0" target="0, 0, 0" up="0, 0, 1"/></transform>
        <float name="cutoff_angle" value="30"/><float name="beam_width" value="15"/></emitter>
    <emitter type="directional"><vector name="direction" x="0" y="-1" z="0"/><rgb name="irradiance" value="2, 2, 2"/></emitter>
    <emitter type="constant"><rgb name="radiance" value="0.5, 0.5, 0.5"/></emitter>
</scene>"""


def test_xml_scene_level_emitters(native):
    from mitsuba2_amd import _capi
    scene, _, _ = native.load_string(XML)
    scene.build(-1)
    d = scene.desc().contents
    assert d.light_count == 4 and d.emitter_count == 1 and scene.emitter_count() == 5
    L = {d.lights[k].type: d.lights[k] for k in range(4)}
    assert [L[t].emitter_index for t in range(4)] == [0, 2, 3, 4] and d.shapes[0].emitter == 0
    assert list(L[_capi.MI_LIGHT_POINT].position) == [1.0, 2.0, 3.0] and list(L[_capi.MI_LIGHT_POINT].value) == [10.0, 20.0, 30.0]
    assert abs(L[_capi.MI_LIGHT_SPOT].cutoff_angle - math.radians(30)) < 1e-6 and abs(L[_capi.MI_LIGHT_SPOT].beam_width - math.radians(15)) < 1e-6
    assert np.allclose(list(L[_capi.MI_LIGHT_DIRECTIONAL].direction), (0, -1, 0), atol=1e-6)
    assert list(L[_capi.MI_LIGHT_CONSTANT].value) == [0.5, 0.5, 0.5]
    with pytest.raises(RuntimeError, match="Only one environment emitter"):
        native.load_string(XML.replace("</scene>", '<emitter type="constant"/></scene>'))
    with pytest.raises(RuntimeError, match="top level"):
        native.load_string(XML.replace('type="constant"', 'type="area"'))


@pytest.mark.parametrize("kind", ["point", "spot", "directional", "constant", "mixed"])
def test_lit_box_scenes(native, kind):
    from mitsuba2_amd import scenes
    scene, sensor = FL.job_scene(scenes, kind, 1)
    d = scene.desc().contents
    if kind == "mixed":
        assert d.light_count == 2 and d.emitter_count == 1 and [d.lights[k].emitter_index for k in range(2)] == [0, 2]
    else:
        assert d.light_count == 1 and d.emitter_count == 0 and d.lights[0].emitter_index == 0
        assert all(d.shapes[i].emitter == -1 for i in range(d.shape_count))


# ---- the float32 leaves of csrc/miw/light.h against closed forms ---------------------------------------------------------------
LEAF_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "mitsuba2_amd/csrc/miw/light.h"
using namespace miw;
int main() {
    Wavelengths wl;
    LightRec l; memset(&l, 0, sizeof l);
    l.value.type = TEX_RGB; l.value.v[0] = 8.f; l.value.v[1] = 4.f; l.value.v[2] = 2.f;
    LightSample ds;
    // point at (0, 2, 0) seen from the origin and from (3, 2, 4)
    l.type = EMITTER_POINT; l.position[1] = 2.f;
    Spec v = light_sample_direction(l, v3(0.f, 0.f, 0.f), v2(.3f, .7f), ds, wl);
    printf("point %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", v.x, v.y, v.z, ds.d.x, ds.d.y, ds.d.z, ds.dist, ds.pdf, (int) ds.delta);
    v = light_sample_direction(l, v3(3.f, 2.f, 4.f), v2(.3f, .7f), ds, wl);
    printf("point %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d\n", v.x, v.y, v.z, ds.d.x, ds.d.y, ds.d.z, ds.dist, ds.pdf, (int) ds.delta);
    printf("pointpdf %.9g %.9g\n", light_pdf_direction(l), light_eval(l, wl).x);
    // spot at the origin of its own frame (to_object = identity), cutoff 40 degrees, beam 20 degrees: reference points at angle a below it
    l.type = EMITTER_SPOT; l.position[1] = 0.f;
    for (int k = 0; k < 16; ++k) l.to_object[k] = (k % 5 == 0) ? 1.f : 0.f;
    const float cutoff = 40.f * (MIW_PI / 180.f), beam = 20.f * (MIW_PI / 180.f);
    l.cutoff_angle = cutoff; l.cos_cutoff_angle = cosf(cutoff); l.cos_beam_width = cosf(beam); l.inv_transition_width = 1.f / (cutoff - beam);
    for (int a = 0; a <= 50; a += 5) {
        const float t = (float) a * (MIW_PI / 180.f);
        v = light_sample_direction(l, v3(2.f * sinf(t), 0.f, 2.f * cosf(t)), v2(0.f, 0.f), ds, wl);
        printf("spot %d %.9g %.9g %.9g %.9g %.9g %d\n", a, v.x, v.y, v.z, ds.dist, ds.pdf, (int) ds.delta);
    }
    // directional along (0, -0.6, 0.8), bounding sphere radius 5
    l.type = EMITTER_DIRECTIONAL; l.direction[0] = 0.f; l.direction[1] = -.6f; l.direction[2] = .8f; l.dist = 2.f * light_bsphere_radius(5.f);
    v = light_sample_direction(l, v3(1.f, 2.f, 3.f), v2(.1f, .2f), ds, wl);
    printf("directional %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %.9g %.9g %.9g %.9g %.9g %.9g\n", v.x, v.y, v.z, ds.d.x, ds.d.y, ds.d.z, ds.dist, ds.pdf, (int) ds.delta,
           ds.p.x, ds.p.y, ds.p.z, ds.n.x, ds.n.y, ds.n.z);
    // constant, radius 5
    l.type = EMITTER_CONSTANT;
    for (int k = 0; k < 5; ++k) {
        v = light_sample_direction(l, v3(1.f, 2.f, 3.f), v2(.1f + .2f * k, .9f - .2f * k), ds, wl);
        printf("constant %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %.9g %.9g\n", v.x, v.y, v.z, ds.d.x, ds.d.y, ds.d.z, ds.dist, ds.pdf, (int) ds.delta,
               light_pdf_direction(l), light_eval(l, wl).x);
    }
    printf("radius %.9g %.9g\n", light_bsphere_radius(5.f), light_bsphere_radius(0.f));
    return 0;
}
"""


@pytest.fixture(scope="module")
def leaf_lines(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("light_leaves")
    (d / "main.cpp").write_text(LEAF_MAIN)
    flags = [f for f in build.CXX_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.CXX] + flags + ["-I", ROOT, str(d / "main.cpp"), "-o", str(d / "leaves")])
    out = subprocess.run([str(d / "leaves")], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        k, *v = line.split()
        rows.setdefault(k, []).append([float(x) for x in v])
    return rows


EPS = 2.0 ** -23         # float32 epsilon: each closed form below is a handful of correctly rounded float32 operations


def test_leaf_point(leaf_lines):
    a, b = leaf_lines["point"]
    # I / d^2, pdf 1, delta; d = 2 and d = 5 (3-4-5)
    assert np.allclose(a[0:3], np.array([8, 4, 2]) / 4.0, rtol=4 * EPS) and a[3:6] == [0, 1, 0] and a[6] == 2 and a[7] == 1 and a[8] == 1
    assert np.allclose(b[0:3], np.array([8, 4, 2]) / 25.0, rtol=4 * EPS) and np.allclose(b[3:6], [-0.6, 0, -0.8], atol=2 * EPS) and abs(b[6] - 5) <= 5 * EPS
    assert leaf_lines["pointpdf"][0] == [0.0, 0.0]               # never hit: pdf_direction and eval are zero


def test_leaf_spot_falloff(leaf_lines):
    cutoff, beam = math.radians(40), math.radians(20)
    for a, x, y, z, dist, pdf, delta in leaf_lines["spot"]:
        t = math.radians(a)
        want = 1.0 if t <= beam else (0.0 if t >= cutoff else (cutoff - t) / (cutoff - beam))     # 1 inside the beam, 0 outside the cutoff, linear in the angle between
        got = np.array([x, y, z]) / (np.array([8, 4, 2]) / 4.0)                                    # distance 2: intensity / 4
        if a in (20, 40):                                        # on a branch point the float32 cosine decides the side: either neighbour value
            assert np.all(np.abs(got - want) <= 1e-5)
        else:
            assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (a, got, want)
        assert abs(dist - 2) <= 4 * EPS and pdf == 1 and delta == 1


def test_leaf_directional(leaf_lines):
    r = leaf_lines["directional"][0]
    f32 = np.float32
    radius = f32(5) * (f32(1) + f32(2.0 ** -24) * f32(1500))
    assert r[0:3] == [8, 4, 2] and r[7] == 1 and r[8] == 1        # the irradiance, undivided; pdf 1, delta
    assert np.array_equal(np.array(r[3:6], f32), -np.array([0, -.6, .8], f32))    # ds.d = -direction, exactly
    assert f32(r[6]) == f32(2) * radius                           # dist = 2 r (r enlarged by set_scene)
    assert np.allclose(r[9:12], np.array([1, 2, 3]) - np.array([0, -.6, .8]) * float(r[6]), rtol=4 * EPS) and np.array_equal(np.array(r[12:15], f32), np.array([0, -.6, .8], f32))
    assert [f32(x) for x in leaf_lines["radius"][0]] == [radius, f32(2.0 ** -24) * f32(1500)]     # (printed with nine digits: a float32 round-trips)


def test_leaf_constant(leaf_lines):
    f32 = np.float32
    inv4pi = f32(1 / (4 * math.pi))
    for k, r in enumerate(leaf_lines["constant"]):
        u = (f32(.1) + f32(.2) * f32(k), f32(.9) - f32(.2) * f32(k))
        assert f32(r[7]) == inv4pi and f32(r[9]) == inv4pi and r[8] == 0 and r[10] == 8      # pdf = 1 / (4 pi), not delta, eval = the radiance
        assert np.allclose(np.array(r[0:3]) * r[7], [8, 4, 2], rtol=4 * EPS)       # value x pdf = radiance
        z = 1 - 2 * float(u[1]); rr = math.sqrt(max(0, 1 - z * z)); phi = 2 * math.pi * float(u[0])
        assert np.allclose(r[3:6], [rr * math.cos(phi), rr * math.sin(phi), z], atol=1e-6) and abs(np.linalg.norm(r[3:6]) - 1) < 1e-6
        assert f32(r[6]) == f32(2) * f32(leaf_lines["radius"][0][0])


# ---- the float64 restatement: the share of samples its margins exclude ----------------------------------------------------------
_cache = {}


def restated(name, native, oracle):
    """the restatement of job `name`, once per session (the GPU tier reads the same results). The checker serves the camera rays
    (MI_EVAL_CAMERA_RAY: no scene involved) and nothing else."""
    if name not in _cache:
        from mitsuba2_amd import scenes
        which, kind, kw = FL.JOBS[name]
        scene, sensor = FL.job_scene(scenes, which, FL.JOB_SPP)
        integ = (native.PathIntegrator if kind == "path" else native.DirectIntegrator)(**kw)
        job = integ.render_job(sensor)
        res = F.restate_job(H, oracle, FL.from_api_scene(scene), job, F.integrator_fn(kind, kw), FL.JOB_SPP)
        _cache[name] = (scene, integ, job, res)
    return _cache[name]


@pytest.mark.parametrize("name", list(FL.JOBS))
def test_restatement_excludes_at_most_five_percent(native, oracle, name):
    scene, integ, job, res = restated(name, native, oracle)
    excluded = 1.0 - float((res["margin"] >= 1.0).mean())
    print("%s: %.2f %% of %d samples excluded, stats %s" % (name, 100 * excluded, res["margin"].size, res["stats"]))
    assert excluded <= F.MAX_EXCLUDED, (name, excluded)
    assert res["stats"]["hit"] > 300 and res["stats"]["miss"] > 5
    assert np.isfinite(res["L"]).all() and (res["L"] >= 0).all() and res["L"].max() > 0


SPECTRAL_JOB = ("mixed", "path", dict())          # scalar_spectral: area + point + constant, every value a srgb_d65 spectrum


def spectral_restated(spectral, oracle_spectral):
    """the restatement of the scalar_spectral job, once per session -> (scene, integ, job, res, model). Called with the `spectral`
    fixture active: the scene's records are the spectral variant's."""
    if "spectral" not in _cache:
        from conftest import SRGB_COEFF
        from mitsuba2_amd import scenes
        from test_independent_leaves import _reference_tables
        which, kind, kw = SPECTRAL_JOB
        cie, d65 = _reference_tables()
        model = F.SrgbModel(SRGB_COEFF, cie, d65)
        scene, sensor = FL.job_scene(scenes, which, FL.JOB_SPP)
        integ = spectral.PathIntegrator(**kw)
        job = integ.render_job(sensor)
        res = F.restate_job(H, oracle_spectral, FL.from_api_scene(scene), job, F.integrator_fn(kind, kw), FL.JOB_SPP, model=model)
        _cache["spectral"] = (scene, integ, job, res, model)
    return _cache["spectral"]


def test_spectral_restatement_excludes_at_most_five_percent(spectral, oracle_spectral):
    scene, integ, job, res, model = spectral_restated(spectral, oracle_spectral)
    d = scene.desc().contents
    assert d.light_count == 2 and all(d.lights[k].value_tex.type == _capi_tex_srgb_d65() for k in range(2))      # <rgb> inside an emitter: srgb_d65
    excluded = 1.0 - float((res["margin"] >= 1.0).mean())
    print("mixed-spectral-path: %.2f %% of %d samples excluded, stats %s" % (100 * excluded, res["margin"].size, res["stats"]))
    assert excluded <= F.MAX_EXCLUDED and res["L"].shape[-1] == 4 and np.isfinite(res["L"]).all() and res["L"].max() > 0


def _capi_tex_srgb_d65():
    return 4                                      # MI_TEX_SRGB_D65 (include/miwave.h)
