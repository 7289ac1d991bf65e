"""The job pool of the frame twins on the GPU (device/resident_kernel.h: QueueWork<..., Frame>::refill / fetch_job; MIW_JOB_POOL).

With a pool a wavefront of a frame twin draws its chunk jobs 8 .. 32 ids at a time and reads their state words with the draw; which lane runs which job
changes, what a job computes does not. Every case renders through the oracle (which knows no queue), on the device with MIW_JOB_POOL = 8 and = 32, and on
the device with MIW_JOB_POOL = 0 (every job drawn on its own, as before the pool). The films must be equal bit for bit, `samples` and `segments` equal to the
oracle's, `samples`, `segments` and `shadow_rays` — now counted per wavefront in LDS — equal between the device renders, and the library's MIW_DEBUG line must
say that a frame twin ran with that pool. The switches are those of tests/test_frame_twin_gpu.py: MIW_JOB_CHUNK_FORCE=1, MIW_JOB_CHUNK=4, MIW_PACKET_SHARD4=0.

The cases are the smallest shapes at which the new code can go wrong:
    1  the box at 64 x 64 @ 16 spp: 4 096 slots in chunks of 8 + 4 + 4 on a device with far more lanes — every chunk of a pixel is drawn at once, so the prefetched
       words are not ready and the parked path and the direct load run
    2  the box at 8 x 8 @ 16 spp: one wavefront, job_total = 192, the last batch cut at job_total, batches astride a chunk boundary
    3  the box at 64 x 64 @ 20 spp: a count that is no power of two
    4  the 42-triangle box: 64-bit masks (Tiny == 1)
    5  the glass-block box: MATS_PLAIN
    6  the box under scalar_spectral
Each case runs once.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 64, 16
FORCED = (("MIW_JOB_CHUNK_FORCE", "1"), ("MIW_JOB_CHUNK", "4"), ("MIW_PACKET_SHARD4", "0"))
POOLS = ("8", "32", "0")


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _twin_pools(capfd):
    """the pool of every frame twin launched since the last call, from the library's MIW_DEBUG line"""
    err = capfd.readouterr().err
    assert "frame twin no" not in err, err[-2000:]
    return [int(m) for m in re.findall(r"\[miwave\] packet path kernel launched: frame twin yes \([^)]*\), job pool (\d+), smallest chunk 4\b", err)]


def _pools_and_oracle(api, orc, capfd, scene, job, chunks):
    o32, _, ost = orc.render(scene.desc(), job, threads=8)
    assert float(np.nanmax(o32[..., :3])) > 0 and o32[..., 4].min() > 0          # the reference side sees the scene
    d = api.Device(0)
    try:
        d.upload(scene.desc())
        d.set_option("MIW_DEBUG", "1")
        for k, v in FORCED:
            d.set_option(k, v)
        got = {}
        for pool in POOLS:
            d.set_option("MIW_JOB_POOL", pool)
            capfd.readouterr()
            g32, st = d.render(job)
            c = d.counters()
            assert st == 0 and c.plan == 2 and c.path_kernel == 0                 # k_path_resident: the packet kernel
            assert _twin_pools(capfd) == [int(pool)], pool
            assert (c.job_chunk, c.job_chunks) == chunks, (c.job_chunk, c.job_chunks)
            assert (c.samples, c.segments) == (ost.samples, ost.segments), (pool, c.samples, c.segments, ost.samples, ost.segments)
            assert _same_bits(g32, o32), "MIW_JOB_POOL=%s: %d of %d film words differ from the oracle's" % (pool, (g32.view(np.uint32) != o32.view(np.uint32)).sum(), g32.size)
            got[pool] = (g32, c.samples, c.segments, c.shadow_rays)
        for pool in POOLS[:-1]:
            assert _same_bits(got[pool][0], got["0"][0]) and got[pool][1:] == got["0"][1:], pool
        assert got["0"][3] > 0
    finally:
        d.close()


def _box(scenes, w=W, h=HGT, spp=SPP, **kw):
    return scenes.cornell_box(w, h, spp, device=-1, **kw)


def test_1_every_chunk_drawn_at_once(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    _pools_and_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), (4, 3))        # 8 + 4 + 4


def test_2_one_wavefront_last_batch_cut(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, 8, 8)
    _pools_and_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), (4, 3))        # job_total = 64 x 3 = 192


def test_3_sample_count_no_power_of_two(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes, spp=20)
    _pools_and_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(sensor), (4, 4))        # 4 + 8 + 4 + 4


def test_4_flat_ball_42_triangles(native, oracle, capfd):
    from mitsuba2_amd import scenes
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "short_block"]
    v, f, _ = scenes.icosphere((185.0, 82.5, 169.0), 82.5, 0)
    meshes.append(native.Mesh("ball", v, f, bsdf=native.BSDF("diffuse", reflectance=scenes.WHITE)))
    scene = native.Scene(meshes).build(-1)
    assert scene.desc().contents.face_count == 42
    _pools_and_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(scenes.cornell_sensor(W, HGT, SPP)), (4, 3))


def test_5_glass_block(native, oracle, capfd):
    from mitsuba2_amd import scenes
    scene = native.Scene(scenes.cornell_box_meshes(diffuse_only=True, glass_block=True)).build(-1)
    assert scene.desc().contents.face_count == 34
    _pools_and_oracle(native, oracle, capfd, scene, native.PathIntegrator().render_job(scenes.cornell_sensor(W, HGT, SPP)), (4, 3))


def test_6_spectral(spectral, oracle_spectral, capfd):
    from mitsuba2_amd import scenes
    scene, sensor = _box(scenes)
    _pools_and_oracle(spectral, oracle_spectral, capfd, scene, spectral.PathIntegrator().render_job(sensor), (4, 3))
