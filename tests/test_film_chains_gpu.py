"""The film replay in equal chains (device/film_kernels.h: k_film_chains; csrc/film_chains.h) on the GPU.

k_film_chains replays the block positions of a tile in chains of equal weight, one wavefront per (group of 64 tiles, chain), where k_film_lanes runs one
wavefront per (group, position). A position's additions are the same statements in the same order and positions own disjoint texels, so the film must not move.
Every case renders on the oracle, on the device as the library chooses (the chain kernel wherever k_film_lanes read the tile-interleaved log before: eight
records in flight per lane, compiled for two wavefronts per SIMD), with four records in flight (MIW_FILM_CHAINS_U=4: three wavefronts per SIMD) and with MIW_FILM_CHAINS=0
(k_film_lanes); the films are compared bit for bit. MIW_DEBUG=1 makes the library say on stderr which form ran and with how many chains.

  tiny blocks     the four cases of test_gpu_parity.py::test_film_replay_by_texel_blocks_on_tiny_blocks: blocks of 1, 2, 4 and 8 pixels, at least 448 tiles, a ragged
                  crop, a partial last group of 64 tiles (475 and 500 tiles; 576 and 1024 fill their groups), every filter reach: a tile has one to four positions per axis, and a chain holds many of them
  32-pixel tiles  150 x 83 cropped to 131 x 70 under MIW_FILM_LANES=1: 15 tiles (one partial group), 9 x 9 positions in 64 chains (interior, edge pairs, the corners),
                  the last row and column of tiles clipped; at 11 spp and at 1 spp, where a run ends inside the first trip of U records
"""
import re

import numpy as np
import pytest

from film_chains_ref import first_fit_decreasing, window_sizes

pytestmark = pytest.mark.gpu

def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _replays(capfd):
    """(kernel, chains or None, positions, records in flight or None) of every block-per-lane replay launched since the last call"""
    err = capfd.readouterr().err
    out = []
    for m in re.finditer(r"\[miwave\] film replay: (k_film_chains|k_film_lanes), (?:(\d+) chains of )?(\d+) positions per group of 64 tiles(?:, (\d+) records in flight per lane)?", err):
        out.append((m.group(1), int(m.group(2)) if m.group(2) else None, int(m.group(3)), int(m.group(4)) if m.group(4) else None))
    return out


def _expected_chains(tile, border, reach):
    """(chains, positions) of a tile's table, as csrc/film_chains.h states it (tests/test_film_chains_cpu.py checks the header against the same restatement)"""
    weight = window_sizes(tile, border, reach)
    return len(first_fit_decreasing(weight)), len(weight)


def _three_ways(api, orc, capfd, scene, job, options=()):
    o32, _, ost = orc.render(scene.desc(), job, threads=8, want_f64=False)
    assert float(np.nanmax(o32[..., :3])) > 0
    cfg = job.cfg
    reach = int(np.floor(cfg.filter_radius + 0.5))
    n_chains, n_pos = _expected_chains(cfg.block_size, cfg.filter_border, reach)
    d = api.Device(0)
    try:
        d.upload(scene.desc())
        d.set_option("MIW_DEBUG", "1")
        for k, v in options:
            d.set_option(k, v)
        films = {}
        for name, switches, want in (("chains", (), ("k_film_chains", n_chains, n_pos, 8)),
                                     ("chains of 4 records", (("MIW_FILM_CHAINS_U", "4"),), ("k_film_chains", n_chains, n_pos, 4)),
                                     ("lanes", (("MIW_FILM_CHAINS", "0"),), ("k_film_lanes", None, n_pos, None))):
            for k, v in switches:
                d.set_option(k, v)
            capfd.readouterr()
            film, st = d.render(job)
            c = d.counters()
            for k, _ in switches:
                d.set_option(k, None)
            assert st == 0 and (c.film_kernel, c.log_interleaved, c.samples) == (4, 1, ost.samples), name
            assert _replays(capfd) == [want], name
            assert _same_bits(film, o32), "%s: %d of %d film words differ from the oracle's" % (name, (film.view(np.uint32) != o32.view(np.uint32)).sum(), film.size)
            films[name] = film.copy()
        assert _same_bits(films["chains"], films["lanes"]) and _same_bits(films["chains of 4 records"], films["lanes"])
    finally:
        d.close()


@pytest.mark.parametrize("crop,n_threads,bs,rfilter", [((48, 48), 576, 2, "gaussian"), ((32, 32), 1024, 1, "tent"), ((100, 76), 450, 4, "mitchell"), ((197, 157), 480, 8, "box")])
def test_tiny_blocks(native, oracle, capfd, crop, n_threads, bs, rfilter):
    from mitsuba2_amd import scenes
    w, h = crop
    scene, _ = scenes.cornell_box(384, 216, 5, device=-1, seed=9)
    sensor = scenes.cornell_sensor(384, 216, 5, rfilter=rfilter, crop_offset_x=40, crop_offset_y=20, crop_width=w, crop_height=h)
    job = native.PathIntegrator().render_job(sensor, n_threads=n_threads)
    assert job.cfg.block_size == bs and job.cfg.block_count >= 448, (job.cfg.block_size, job.cfg.block_count)
    _three_ways(native, oracle, capfd, scene, job)


@pytest.mark.parametrize("spp", [11, 1])
@pytest.mark.parametrize("rfilter", ["gaussian", "tent", "box", "mitchell", "catmullrom"])
def test_32_pixel_tiles(native, oracle, capfd, rfilter, spp):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cornell_box(150, 83, spp, device=-1, seed=77, rfilter=rfilter, crop_offset_x=7, crop_offset_y=2, crop_width=131, crop_height=70)
    job = native.PathIntegrator().render_job(sensor)
    assert job.cfg.block_size == 32 and job.cfg.block_count == 15
    if job.cfg.filter_border == 2 and int(np.floor(job.cfg.filter_radius + 0.5)) == 2:
        assert _expected_chains(32, 2, 2) == (64, 81)                  # the headline's table: 49 interior positions, 14 pairs of edges, the four corners
    _three_ways(native, oracle, capfd, scene, job, options=(("MIW_FILM_LANES", "1"),))
