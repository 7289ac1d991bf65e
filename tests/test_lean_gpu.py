"""The lean twins of the packet path kernels (device/resident_kernel.h: k_path_resident<..., Feat = FEAT_NONE>; csrc/kernel_pick.h: packet_features)
on the GPU. A lean kernel is the full kernel minus the routes of scene features the scene does not have — environment map, vertex normals on shapes or
on emitter faces, the moment pass — so the film must not move: every case renders 64 x 64 @ 16 spp through the oracle (which knows no such
thing), on the device as the library chooses, and on the device with MIW_LEAN=0 (the full kernel); the three films must be equal bit for bit and the
sample and segment counts equal. MIW_DEBUG=1 makes the library say on stderr, after each launch, which features the
instantiation it launched was compiled with — the mask the launch site recorded, not the mask chosen for the render: 0x0 only where a lean twin ran.

  the scenes that take the lean kernel
    i     the diffuse Cornell box, 32 triangles: 32-bit candidate masks (Tiny == 2, MATS_DIFFUSE). At this size the job fits four wavefronts per SIMD and
          takes the 128-register shard form; with MIW_PACKET_SHARD4=0 it is the headline's five-wavefront instantiation
    ii    the box with a flat-shaded level-0 icosphere for its short block, 42 triangles: 64-bit masks (Tiny == 1, MATS_DIFFUSE)
    iii   the glass-block box, 34 triangles, and the same without its short block, 24: both MATS_PLAIN kernels
    iv    scene i and the glass-block box under scalar_spectral
    v     scene i with 4-sample chunk jobs forced: pixels change lanes inside the launch
  the scenes that must NOT take it (the full kernel either way, still equal to the oracle)
    vi    scene i lit through its open front by an environment map
    vii   the box with a smooth-shaded icosphere (vertex normals on a shape)
    viii  the box with a second emitter whose mesh has vertex normals (an emitter's flag comes from its shape's, so this scene has both facts: the
          emitter fact alone cannot occur, and with only the all / none masks it cannot be told from vii)
    ix    scene i under the moment integrator, both passes
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 64, 16
FEAT_ALL, FEAT_NONE = 0xf, 0x0


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _features(capfd):
    """the feature masks of the packet path kernel instantiations LAUNCHED since the last call (the library's MIW_DEBUG line, printed after each launch
    with the mask its launch site recorded: 0x0 only where a lean twin was launched)"""
    err = capfd.readouterr().err
    return [int(m, 16) for m in re.findall(r"\[miwave\] packet path kernel launched: scene features 0x([0-9a-f]+) of 0xf compiled in", err)]


def _lean_full_oracle(api, orc, capfd, scene, job, want, options=(), expect=None, samples=W * HGT * SPP):
    o32, _, ost = orc.render(scene.desc(), job, threads=8)
    assert float(np.nanmax(o32[..., :3])) > 0 and o32[..., 4].min() > 0          # the reference side sees the scene
    d = api.Device(0)
    try:
        d.upload(scene.desc())
        d.set_option("MIW_DEBUG", "1")
        for k, v in options:
            d.set_option(k, v)
        films = {}
        for lean, feat in ((None, want), ("0", FEAT_ALL), ("1", want)):           # the default, the switch off, the switch on
            d.set_option("MIW_LEAN", lean)
            capfd.readouterr()
            g32, st = d.render(job)
            c = d.counters()
            assert st == 0 and c.plan == 2 and c.path_kernel == 0                 # k_path_resident: the packet kernel
            assert _features(capfd) == [feat], (lean, feat)
            if expect:
                expect(c)
            assert c.samples == ost.samples == samples and c.segments == ost.segments
            assert _same_bits(g32, o32), "MIW_LEAN=%s: %d of %d film words differ from the oracle's" % (lean, (g32.view(np.uint32) != o32.view(np.uint32)).sum(), g32.size)
            films[lean] = g32
        assert _same_bits(films[None], films["0"]) and _same_bits(films["1"], films["0"])
    finally:
        d.close()


def _flat_ball_box(api, scenes, normals):
    """the diffuse box, a level-0 icosphere in place of the short block: 32 - 10 + 20 = 42 triangles; flat-shaded, or smooth with exact vertex normals"""
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "short_block"]
    v, f, n = scenes.icosphere((185.0, 82.5, 169.0), 82.5, 0)
    meshes.append(api.Mesh("ball", v, f, normals=n if normals else None, bsdf=api.BSDF("diffuse", reflectance=scenes.WHITE)))
    return api.Scene(meshes).build(-1)


def _sensor(scenes):
    return scenes.cornell_sensor(W, HGT, SPP)


# ---- lean ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shard4", ["1", "0"])
def test_i_diffuse_cornell_box(native, oracle, capfd, shard4):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)
    assert scene.desc().contents.face_count == 32
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), FEAT_NONE, options=(("MIW_PACKET_SHARD4", shard4),))


def test_ii_flat_ball_42_triangles(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene = _flat_ball_box(native, scenes, normals=False)
    assert scene.desc().contents.face_count == 42
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(_sensor(scenes)), FEAT_NONE)


@pytest.mark.parametrize("short_block,triangles", [(True, 34), (False, 24)])
def test_iii_glass_block(native, oracle, capfd, short_block, triangles):
    from mitsuba2_amd import scenes
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True, glass_block=True) if short_block or m.name != "short_block"]
    scene = native.Scene(meshes).build(-1)
    assert scene.desc().contents.face_count == triangles
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(_sensor(scenes)), FEAT_NONE)


@pytest.mark.parametrize("glass_block", [False, True])
def test_iv_spectral(spectral, oracle_spectral, capfd, glass_block):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1, glass_block=glass_block)
    _lean_full_oracle(spectral, oracle_spectral, capfd, scene, spectral.PathIntegrator().render_job(sensor), FEAT_NONE)


def test_v_four_sample_chunk_jobs(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)

    def chunks(c):
        assert (c.job_chunk, c.job_chunks) == (4, 3), (c.job_chunk, c.job_chunks)      # 16 spp: 8 + 4 + 4

    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), FEAT_NONE,
                      options=(("MIW_JOB_CHUNK_FORCE", "1"), ("MIW_JOB_CHUNK", "4")), expect=chunks)


# ---- not lean ------------------------------------------------------------------------------------------------------------------------

def test_vi_environment_map_through_the_open_front(native, oracle, capfd):
    from mitsuba2_amd import scenes
    env = native.EnvMap(scenes.sky_envmap(64, 32), to_world=dict(origin=(0, 0, 0), target=(0.3, 0.1, -1.0), up=(0, 1, 0)))
    scene = native.Scene(scenes.cornell_box_meshes(diffuse_only=True), envmap=env).build(-1)
    assert scene.desc().contents.face_count == 32
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(_sensor(scenes)), FEAT_ALL)


def test_vii_smooth_shaded_shape(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene = _flat_ball_box(native, scenes, normals=True)
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(_sensor(scenes)), FEAT_ALL)


def test_viii_emitter_with_vertex_normals(native, oracle, capfd):
    from mitsuba2_amd import scenes
    import test_tri_frames_gpu as frames
    scene = native.Scene(frames.two_emitter_box_meshes(native, scenes)).build(-1)
    assert scene.desc().contents.face_count == 34
    _lean_full_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(_sensor(scenes)), FEAT_ALL)


@pytest.mark.parametrize("moment_pass", [1, 2])
def test_ix_moment_integrator(native, oracle, capfd, moment_pass):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(W, HGT, SPP, device=-1)
    job = native.MomentIntegrator(native.PathIntegrator()).render_job(sensor, moment_pass=moment_pass)
    _lean_full_oracle(native, oracle, capfd, scene, job, FEAT_ALL)
