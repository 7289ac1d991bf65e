"""The frame twins of the lean packet path kernels (device/resident_kernel.h: k_path_resident<..., FEAT_FRAME>; csrc/kernel_pick.h: frame_twin) on the GPU.

A frame twin is a lean kernel with the facts of a full frame's launch compiled in — chunk jobs from one queue, the 16-byte log, no tail priorities, the leaf
filter on — so it runs the statements the lean kernel ran for such a launch and the film must not move. Every case renders through the oracle (which knows no
such thing), on the device as the library chooses, and on the device with MIW_FRAME_TWIN=0; the three films must be equal bit for bit, `samples` and
`segments` equal to the oracle's, `samples`, `segments` and `shadow_rays` equal between the two device renders. MIW_DEBUG=1 makes the library say on stderr,
after each launch, which instantiation its launch site launched: the feature mask (0x0: a lean kernel) and, on a second line, whether it was a frame twin.

A small frame gets chunk jobs only when forced and would take the four-wavefront shard form, so the twin cases set MIW_JOB_CHUNK_FORCE=1, MIW_JOB_CHUNK=4 and
MIW_PACKET_SHARD4=0.

  the launches that take the twin
    i     the diffuse Cornell box, 64 x 64 @ 16 spp: the headline's kernel (Tiny == 2, MATS_DIFFUSE), chunks of 8 + 4 + 4 samples
    ii    the box at 8 x 8 @ 16 spp: one wavefront, so every chunk of a pixel is drawn at once and the parked-job path runs
    iii   the box at 64 x 64 @ 20 spp: halving chunks on a count that is no power of two (4 + 8 + 4 + 4)
    iv    the box with a flat-shaded icosphere, 42 triangles: 64-bit candidate masks (Tiny == 1)
    v     the glass-block box, 34 triangles, and the same without its short block, 24: both MATS_PLAIN kernels
    vi    the box and the glass-block box under scalar_spectral
  the launches that must NOT take it, and must still equal the oracle
    vii   the box without forced chunks (a job = a pixel)
    viii  the box uploaded with MI_BVH_NO_LEAF_FILTER
    ix    the box under a filter without class tables (lanczos: the 24-byte log)
    x     the box under the direct integrator
    xi    the box lit through its open front by an environment map: a scene that keeps the full kernel
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 64, 16
FEAT_ALL, FEAT_NONE = 0xf, 0x0
FORCED = (("MIW_JOB_CHUNK_FORCE", "1"), ("MIW_JOB_CHUNK", "4"), ("MIW_PACKET_SHARD4", "0"))
MI_BVH_NO_LEAF_FILTER = 0x20


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _launched(capfd):
    """(feature mask, frame twin) of every packet path kernel launched since the last call: the library's two MIW_DEBUG lines, printed after each launch"""
    err = capfd.readouterr().err
    feats = [int(m, 16) for m in re.findall(r"\[miwave\] packet path kernel launched: scene features 0x([0-9a-f]+) of 0xf compiled in", err)]
    twins = [m == "yes" for m in re.findall(r"\[miwave\] packet path kernel launched: frame twin (yes|no)\b", err)]
    assert len(feats) == len(twins), err
    return list(zip(feats, twins))


def _twin_lean_oracle(api, orc, capfd, scene, job, twin, feat=FEAT_NONE, options=FORCED, chunks=None, bvh_quality=0, record_bytes=16):
    """oracle, device as the library chooses (`twin`: whether that must be a frame twin), device with MIW_FRAME_TWIN=0"""
    o32, _, ost = orc.render(scene.desc(), job, threads=8)
    assert float(np.nanmax(o32[..., :3])) > 0 and o32[..., 4].min() > 0          # the reference side sees the scene
    d = api.Device(0)
    try:
        d.upload(scene.desc(), bvh_quality=bvh_quality)
        d.set_option("MIW_DEBUG", "1")
        for k, v in options:
            d.set_option(k, v)
        got = {}
        for switch, want in ((None, twin), ("0", False)):
            d.set_option("MIW_FRAME_TWIN", switch)
            capfd.readouterr()
            g32, st = d.render(job)
            c = d.counters()
            assert st == 0 and c.plan == 2 and c.path_kernel == 0                 # k_path_resident: the packet kernel
            assert _launched(capfd) == [(feat, want)], (switch, feat, want)
            if chunks is not None:
                assert (c.job_chunk, c.job_chunks if chunks[0] else 0) == chunks, (c.job_chunk, c.job_chunks)
            assert c.log_record_bytes == record_bytes
            assert (c.samples, c.segments) == (ost.samples, ost.segments)
            assert _same_bits(g32, o32), "MIW_FRAME_TWIN=%s: %d of %d film words differ from the oracle's" % (switch, (g32.view(np.uint32) != o32.view(np.uint32)).sum(), g32.size)
            got[switch] = (g32, c.samples, c.segments, c.shadow_rays)
        assert _same_bits(got[None][0], got["0"][0]) and got[None][1:] == got["0"][1:] and got[None][3] > 0
    finally:
        d.close()


def _box(scenes, w=W, h=HGT, spp=SPP, **kw):
    return scenes.cornell_box(w, h, spp, device=-1, **kw)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------

def test_i_diffuse_cornell_box(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    assert scene.desc().contents.face_count == 32
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), True, chunks=(4, 3))       # 8 + 4 + 4


def test_ii_one_wavefront_parks_its_jobs(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, 8, 8)
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), True, chunks=(4, 3))


def test_iii_sample_count_no_power_of_two(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, spp=20)
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), True, chunks=(4, 4))       # 4 + 8 + 4 + 4


def test_iv_flat_ball_42_triangles(native, oracle, capfd):
    from mitsuba2_amd import scenes
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "short_block"]
    v, f, _ = scenes.icosphere((185.0, 82.5, 169.0), 82.5, 0)
    meshes.append(native.Mesh("ball", v, f, bsdf=native.BSDF("diffuse", reflectance=scenes.WHITE)))
    scene = native.Scene(meshes).build(-1)
    assert scene.desc().contents.face_count == 42
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(scenes.cornell_sensor(W, HGT, SPP)), True, chunks=(4, 3))


@pytest.mark.parametrize("short_block,triangles", [(True, 34), (False, 24)])
def test_v_glass_block(native, oracle, capfd, short_block, triangles):
    from mitsuba2_amd import scenes
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True, glass_block=True) if short_block or m.name != "short_block"]
    scene = native.Scene(meshes).build(-1)
    assert scene.desc().contents.face_count == triangles
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(scenes.cornell_sensor(W, HGT, SPP)), True, chunks=(4, 3))


@pytest.mark.parametrize("glass_block", [False, True])
def test_vi_spectral(spectral, oracle_spectral, capfd, glass_block):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, glass_block=glass_block)
    _twin_lean_oracle(spectral, oracle_spectral, capfd, scene, spectral.PathIntegrator().render_job(sensor), True, chunks=(4, 3))


# ---- not the twin --------------------------------------------------------------------------------------------------------------------

def test_vii_without_forced_chunks(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), False, options=(("MIW_PACKET_SHARD4", "0"),), chunks=(0, 0))


def test_viii_leaf_filter_switched_off(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), False, chunks=(4, 3), bvh_quality=MI_BVH_NO_LEAF_FILTER)


def test_ix_filter_without_class_tables(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, rfilter="lanczos")
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), False, chunks=(4, 3), record_bytes=24)


def test_x_direct_integrator(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    _twin_lean_oracle(native, oracle, capfd, scene, native.DirectIntegrator().render_job(sensor), False, feat=FEAT_ALL, chunks=(4, 3))


def test_xi_environment_map_keeps_the_full_kernel(native, oracle, capfd):
    from mitsuba2_amd import scenes
    env = native.EnvMap(scenes.sky_envmap(64, 32), to_world=dict(origin=(0, 0, 0), target=(0.3, 0.1, -1.0), up=(0, 1, 0)))
    scene = native.Scene(scenes.cornell_box_meshes(diffuse_only=True), envmap=env).build(-1)
    _twin_lean_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(scenes.cornell_sensor(W, HGT, SPP)), False, feat=FEAT_ALL, chunks=(4, 3))
