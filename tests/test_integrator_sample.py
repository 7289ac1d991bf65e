"""SamplingIntegrator::sample for caller-supplied rays (mi_sample) — the tier that needs no GPU.

* the reassembly harness (sample_harness.py) proves itself: with max_depth = 1 the path integrator returns emitter->eval(si) of the
  first hit and draws nothing, which the checker's scene queries give without any integrator; films reassembled from THAT must be
  the checker's own float64 films, bit for bit — scalar_rgb and scalar_spectral;
* the numpy PCG32 of the harness against the checker's;
* the boundary: mi_sample_cfg header <-> ctypes, the symbol in the header and in both libraries, the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sample_harness as H
from conftest import ROOT


def _box_job(api, scenes, which, w, h, spp, seed=0, **integ):
    kw = dict(device=-1, rfilter="box", seed=seed)
    if which == "cornell_box":
        scene, sensor = scenes.cornell_box(w, h, spp, **kw)
    elif which == "glass_block":
        scene, sensor = scenes.cornell_box(w, h, spp, diffuse_only=False, ball_level=1, glass_block=True, **kw)
    else:
        scene, sensor = getattr(scenes, which)(w, h, spp, **kw)
    return scene, sensor, api.PathIntegrator(**integ).render_job(sensor)


def test_numpy_pcg32_matches_the_checker(oracle):
    rng = np.random.default_rng(5)
    seeds = np.concatenate([np.array([0, 1, 42, 2 ** 64 - 1], np.uint64), rng.integers(0, 2 ** 63, 60, dtype=np.uint64)])
    for seq in (H.DEFAULT_STREAM, 54, 2 ** 64 - 1):
        state, inc = H.pcg32_seed(seeds, seq)
        su = state.copy(); sf = state.copy()
        got_u = np.zeros((len(seeds), 16), np.uint32); got_f = np.zeros((len(seeds), 16), np.float32)
        for k in range(16):
            got_u[:, k], su = H.pcg32_next_u32(su, inc)
            got_f[:, k], sf = H.pcg32_next_f32(sf, inc)
        assert np.array_equal(su, sf)
        for i, s in enumerate(seeds):
            wu = np.zeros(16, np.uint32); wf = np.zeros(16, np.float32)
            oracle.L.orc_pcg32_u32(int(s), seq, wu.ctypes.data_as(C.POINTER(C.c_uint32)), 16)
            oracle.L.orc_pcg32_f32(int(s), seq, wf.ctypes.data_as(C.POINTER(C.c_float)), 16)
            assert np.array_equal(got_u[i], wu) and np.array_equal(got_f[i].view(np.uint32), wf.view(np.uint32))
    # the public pcg32-demo vector: seed(42, 54)
    state, inc = H.pcg32_seed(np.array([42], np.uint64), 54)
    assert H.pcg32_next_u32(state, inc)[0][0] == 0xa15c02b7


@pytest.mark.parametrize("which", ["cornell_box", "open_box"])
def test_harness_reassembles_the_checkers_film_rgb(native, oracle, which):
    """The harness itself, without mi_sample and without a GPU (48 x 40: clipped edge blocks included). open_box: misses see the
    environment map."""
    from mitsuba2_amd import scenes
    scene, sensor, job = _box_job(native, scenes, which, 48, 40, 4, max_depth=1)
    _, want, _ = oracle.render(scene.desc(), job, threads=4, want_f64=True)
    films = [f.copy() for f in H.chain(oracle, job, H.first_hit_emission(oracle, scene.desc()), 4)]
    assert want[..., 4].min() == 4.0 and want[..., :3].max() > 0
    assert np.array_equal(films[-1].view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(films[-2], want)                  # (the last sample matters)


def test_harness_reassembles_the_checkers_film_spectral(spectral, oracle_spectral):
    from mitsuba2_amd import scenes
    scene, sensor, job = _box_job(spectral, scenes, "glass_block", 48, 40, 3, max_depth=1)
    _, want, _ = oracle_spectral.render(scene.desc(), job, threads=4, want_f64=True)
    films = [f.copy() for f in H.chain(oracle_spectral, job, H.first_hit_emission(oracle_spectral, scene.desc()), 3, spectral=True)]
    assert want[..., :3].max() > 0
    assert np.array_equal(films[-1].view(np.uint64), want.view(np.uint64))


def test_base_seed_keeps_every_sample_of_the_gpu_jobs_in_its_texel(native, oracle):
    """Where the reassembly's base seed is chosen (sample_harness.BASE_SEED): every job of test_integrator_sample_gpu.py, at spp + 1
    (a pixel's first spp samples are the same stream), rendered by the checker alone — weight channel == sample count in every texel."""
    from mitsuba2_amd import scenes
    for which in H.GPU_SCENES:
        scene, sensor = H.gpu_scene(scenes, which, H.GPU_SPP + 1)
        for kind, kw in H.GPU_INTEGRATORS:
            integ = native.PathIntegrator(**kw) if kind == "path" else native.DirectIntegrator(**kw)
            _, want, _ = oracle.render(scene.desc(), integ.render_job(sensor), threads=4, want_f64=True)
            assert H.every_sample_in_its_texel(want, H.GPU_SPP + 1), (which, kind, kw)


def test_base_seed_keeps_every_sample_of_the_spectral_gpu_job_in_its_texel(spectral, oracle_spectral):
    from mitsuba2_amd import scenes
    scene, sensor = H.gpu_scene(scenes, "glass_block", H.GPU_SPP + 1)
    _, want, _ = oracle_spectral.render(scene.desc(), spectral.PathIntegrator().render_job(sensor), threads=4, want_f64=True)
    assert H.every_sample_in_its_texel(want, H.GPU_SPP + 1)


def test_sample_cfg_mirror_matches_the_header(tmp_path):
    from mitsuba2_amd import _capi
    cls = _capi.mi_sample_cfg
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "miwave.h"', 'int main(void) {', '  printf("sizeof %zu\\n", sizeof(mi_sample_cfg));']
    lines += ['  printf("%s %%zu\\n", offsetof(mi_sample_cfg, %s));' % (f[0], f[0]) for f in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"; src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi")])
    out = subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(l.split() for l in out if l)
    assert int(got.pop("sizeof")) == C.sizeof(cls) == 32
    assert cls._fields_[0][0] == "struct_size" and cls.struct_size.offset == 0      # the size word comes first
    assert len(got) == len(cls._fields_) == 8
    for name, off in got.items():
        assert getattr(cls, name).offset == int(off), name


def test_mi_sample_is_declared_and_exported_by_both_libraries(native):
    from mitsuba2_amd import _capi
    header = open(os.path.join(ROOT, "include", "miwave.h")).read()
    assert re.search(r"mi_status\s+mi_sample\s*\(\s*mi_ctx\s*\*", header) and "mi_sample" in _capi.MI_SYMBOLS
    assert "moment" in header[header.index("SamplingIntegrator::sample(scene, sampler, ray)"):header.index("} mi_sample_cfg;")]
    for lib in ("libmiwave.so", "libmiwave_spectral.so"):
        assert C.CDLL(os.path.join(_capi.LIB_DIR, lib)).mi_sample
    for lib in ("libmiwave_host.so", "libmiwave_host_spectral.so"):
        L = C.CDLL(os.path.join(_capi.LIB_DIR, lib))
        assert L.mih_integrator_sample and L.mih_integrator_sample_batch and L.mih_sampler_get_state and L.mih_sampler_set_state


def test_refusals_that_need_no_device(native):
    """A bad job description is refused before anything else is looked at (MI_ERR_INVALID + text), the host class refuses a scene
    that is not on a device and the moment integrator; the sampler's state can be read and set."""
    from mitsuba2_amd import _capi, scenes
    L = native.device_lib()
    call = lambda cfg: L.mi_sample(None, C.byref(cfg), None, None, None, None, None, None, 0)
    cfg = native.sample_cfg()
    assert cfg.struct_size == 32 and call(cfg) == _capi.MI_ERR_INVALID          # (valid description, no context)
    cfg.struct_size = 28
    assert call(cfg) == _capi.MI_ERR_INVALID and b"struct_size 28" in L.mi_last_error(None)
    assert call(native.sample_cfg(integrator=7)) == _capi.MI_ERR_INVALID and b"unknown integrator 7" in L.mi_last_error(None)
    assert call(native.sample_cfg("direct", emitter_samples=0, bsdf_samples=0)) == _capi.MI_ERR_INVALID and b"at least 1 BSDF or emitter sample" in L.mi_last_error(None)
    assert call(native.sample_cfg(rr_depth=0)) == _capi.MI_ERR_INVALID and b"rr_depth" in L.mi_last_error(None)
    assert L.mi_sample(None, None, None, None, None, None, None, None, 0) == _capi.MI_ERR_INVALID

    scene, sensor = scenes.cornell_box(8, 8, 1, device=-1)
    sampler = native.Sampler(sample_count=1, seed=3)
    ray = [278, 273, -800, 0, 0, 1, 0, np.inf]
    for integ in (native.PathIntegrator(max_depth=4), native.DirectIntegrator(emitter_samples=2, bsdf_samples=0)):
        with pytest.raises(RuntimeError, match="not built on a device"):
            integ.sample(scene, sampler, ray)
        with pytest.raises(RuntimeError, match="not built on a device"):
            integ.sample_batch(scene, [ray[:3]], [ray[3:6]], [1])
    c = native.PathIntegrator(max_depth=4, rr_depth=2).sample_cfg()
    assert (c.struct_size, c.integrator, c.max_depth, c.rr_depth, c.on_device) == (32, 0, 4, 2, 0)
    c = native.DirectIntegrator(emitter_samples=2, bsdf_samples=0, hide_emitters=True).sample_cfg()
    assert (c.integrator, c.emitter_samples, c.bsdf_samples, c.hide_emitters) == (1, 2, 0, 1)
    moment = native.MomentIntegrator(native.PathIntegrator())
    with pytest.raises(RuntimeError, match="moment: sample\\(\\) returns AOVs"):
        moment.sample(scene, sampler, ray)
    with pytest.raises(RuntimeError, match="moment: sample\\(\\) returns AOVs"):
        moment.sample_batch(scene, [ray[:3]], [ray[3:6]], [1])

    # IndependentSampler: state() / set_state() are the stream behind next_1d()
    state, inc = H.pcg32_seed(np.array([3 + 0x853c49e6748fea9b], np.uint64))    # independent.cpp:62-63: seed(PCG32_DEFAULT_STATE) on top of the base seed
    assert sampler.state() == (int(state[0]), int(inc))
    want, after = H.pcg32_next_f32(state, inc)
    assert sampler.next_1d() == want[0] and sampler.state()[0] == int(after[0])
    sampler.set_state(int(state[0]), int(inc))
    assert sampler.next_1d() == want[0]
