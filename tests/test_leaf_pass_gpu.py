"""The leaf-box pass of the render kernels' trace2 with the widening of the exit distance hoisted out of its loop (device/trace.h: LeafRay,
leaf_ray, leaf_box_test_octant on LeafRay operands) on the GPU. The pass is a conservative filter in front of the exact triangle test, so the film
must not move: every case renders 64 x 64 @ 16 spp on the device and through the oracle (which has no such filter) and the two films
must be equal bit for bit, the sample and segment counts equal.

  i    the diffuse Cornell box — 32 triangles: 32-bit candidate masks (Tiny == 2), the headline instantiation
  ii   the material balls at tessellation level 0 — 52 triangles: 64-bit masks (Tiny == 1), the BSDF-dispatch kernel
  iii  the glass-block box under scalar_spectral — the other variant's packet kernel
  iv   scene i under the direct integrator — its packet kernels keep the old leaf test (their register budget, device/resident_kernel.h): the two forms
       side by side in one library
  v    scene i seen from 100 scene extents away (a field of view that still frames the box): |plane - o| large against the box
  vi   scene i scaled by 1e3 and by 1e-3 (camera and clip planes with it): the widening is relative
  vii  scene i with 4-sample chunk jobs forced, the way tests/test_job_chunks.py forces them: pixels change lanes inside the launch
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 64, 16
EXTENT = 559.2                                                   # the box's largest side


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _device_equals_oracle(api, orc, scene, job, options=(), expect=None):
    o32, _, ost = orc.render(scene.desc(), job, threads=8)
    assert np.isfinite(o32).all() and o32[..., 4].min() > 0      # the reference side is clean
    assert float(o32[..., :3].max()) > 0                         # ... and sees the scene
    d = api.Device(0)
    try:
        d.upload(scene.desc())
        for k, v in options:
            d.set_option(k, v)
        g32, st = d.render(job)
        c = d.counters()
        assert st == 0 and c.plan == 2 and c.path_kernel == 0    # k_path_resident: the packet kernel
        if expect:
            expect(c)
        assert c.samples == ost.samples == W * HGT * SPP and c.segments == ost.segments
        assert _same_bits(g32, o32), "%d of %d film words differ" % ((g32.view(np.uint32) != o32.view(np.uint32)).sum(), g32.size)
    finally:
        d.close()


def _scaled_box(api, scenes, s, distance=1.0, **mesh_kw):
    """the Cornell box scaled by s about the origin; the camera backs away to `distance` x its usual 800 units from the front opening
    and narrows its field of view to keep the box in frame"""
    meshes = [api.Mesh(m.name, m.vertices * np.float32(s), m.faces, normals=m.normals, bsdf=m.bsdf, emitter=m.emitter)
              for m in scenes.cornell_box_meshes(**mesh_kw)]
    fov = float(np.degrees(2.0 * np.arctan(np.tan(np.radians(39.3 / 2.0)) / distance)))
    film = api.Film(rfilter="gaussian", width=W, height=HGT)
    sensor = api.Sensor(film, api.Sampler(sample_count=SPP, seed=0), fov=fov, near_clip=1e-2 * s, far_clip=1e4 * s * distance,
                        to_world=dict(origin=(278 * s, 273 * s, -800.0 * s * distance), target=(278 * s, 273 * s, 0), up=(0, 1, 0)))
    return api.Scene(meshes).build(-1), sensor


def test_i_diffuse_cornell_box(native, oracle):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)
    assert scene.desc().contents.face_count == 32
    _device_equals_oracle(native, oracle, scene, native.PathIntegrator().render_job(sensor))


def test_ii_material_balls_52_triangles(native, oracle):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1, diffuse_only=False, ball_level=0)
    assert scene.desc().contents.face_count == 52
    _device_equals_oracle(native, oracle, scene, native.PathIntegrator().render_job(sensor))


def test_iii_spectral_glass_block(spectral, oracle_spectral):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1, glass_block=True)
    _device_equals_oracle(spectral, oracle_spectral, scene, spectral.PathIntegrator().render_job(sensor))


def test_iv_direct_integrator(native, oracle):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)
    _device_equals_oracle(native, oracle, scene, native.DirectIntegrator().render_job(sensor))


def test_v_camera_100_extents_away(native, oracle):
    from mitsuba2_amd import scenes
    distance = 100.0 * EXTENT / 800.0                            # the camera 100 extents in front of the box
    scene, sensor = _scaled_box(native, scenes, 1.0, distance=distance)
    _device_equals_oracle(native, oracle, scene, native.PathIntegrator().render_job(sensor))


@pytest.mark.parametrize("scale", [1e3, 1e-3])
def test_vi_scaled_scene(native, oracle, scale):
    from mitsuba2_amd import scenes
    scene, sensor = _scaled_box(native, scenes, scale)
    _device_equals_oracle(native, oracle, scene, native.PathIntegrator().render_job(sensor))


def test_vii_four_sample_chunk_jobs(native, oracle):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)

    def chunks(c):
        assert (c.job_chunk, c.job_chunks) == (4, 3), (c.job_chunk, c.job_chunks)      # 16 spp: 8 + 4 + 4

    _device_equals_oracle(native, oracle, scene, native.PathIntegrator().render_job(sensor),
                          options=(("MIW_JOB_CHUNK_FORCE", "1"), ("MIW_JOB_CHUNK", "4")), expect=chunks)
