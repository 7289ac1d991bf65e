"""k_sample_rays (mi_sample) against the independent float64 restatement of tests/f64_integrators.py, on the GPU.

The same jobs and the same restatement results as test_independent_integrators.py (computed once per job). Here Device.sample
returns L, `valid` and the sampler state per ray, so they are checked directly: L and valid under the rule of
f64_integrators.compare, and the state after the call EXACTLY — it must be the PCG32 state advanced by the number of draws the
restatement made, for every checked ray."""
import numpy as np
import pytest

import f64_integrators as F
import sample_harness as H
from test_independent_integrators import RTOL, report, restated, spectral_restated, xyz_of

pytestmark = pytest.mark.gpu


def _host(dev, cfg, ray, state, inc):
    o, d = np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6])
    return dev.sample(o, d, state, np.ascontiguousarray(ray[:, 6]), np.ascontiguousarray(ray[:, 7]), rng_inc=inc, cfg=cfg)


def _device(dev, cfg, ray, state, inc):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = t(state.view(np.int64))
    spec, valid = dev.sample_device([t(ray[:, k]) for k in range(8)], st, rng_inc=None if inc is None else t(inc.view(np.int64)), cfg=cfg)
    return spec.cpu().numpy(), valid.cpu().numpy() != 0, st.cpu().numpy().view(np.uint64)


def _check(name, res, n_samples, call, inc=None):
    for j in range(n_samples):
        spec, valid, after = call(res["ray"][j], res["state_before"][j].copy(), inc)
        checked, bad, dev = F.compare(spec, valid, res, j, RTOL, to_xyz=False)
        msg = report(name, res, checked, dev)
        print("sample %d: %s" % (j, msg))
        assert checked.mean() >= 1 - F.MAX_EXCLUDED and checked.sum() >= 0.95 * len(checked), msg
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            pytest.fail("%s\nsample %d: %d rays differ; first: pixel (%d, %d): device %s valid %s, restatement %s valid %s, margin %.3g (%s)"
                        % (msg, j, bad.sum(), res["px"][i], res["py"][i], spec[i], valid[i], res["L"][j, i], res["valid"][j, i], res["margin"][j, i], res["what"][j][i]))
        wrong = checked & (after != res["state_after"][j])
        assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count; first: ray %d, %d draws" % (
            msg, j, wrong.sum(), np.flatnonzero(wrong)[0], res["n_draws"][j, np.flatnonzero(wrong)[0]])


@pytest.mark.parametrize("name", list(F.JOBS))
def test_gpu_sample_against_float64_restatement(native, oracle, name):
    """both routes of test_integrator_sample_gpu.py — the scene's own (packet kernels for the small boxes) and the forced tree walk —
    each through host arrays and through arrays resident on the device"""
    from mitsuba2_amd import _capi
    scene, integ, job, res = restated(name, native, oracle)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            _check(name, res, F.JOB_SPP, lambda ray, st, inc: _host(dev, cfg, ray, st, inc))
            _check(name, res, F.JOB_SPP, lambda ray, st, inc: _device(dev, cfg, ray, st, inc))
    finally:
        dev.close()


def test_gpu_sample_with_a_callers_increment_against_float64_restatement(native, oracle):
    """a caller-supplied odd rng_inc per ray: other numbers, so another restatement run (one sample per pixel), same checks, on
    both routes"""
    from mitsuba2_amd import _capi, scenes
    name = "cornell-path-d3-rr2"
    which, kind, kw, seed = F.JOBS[name]
    scene, sensor = F.job_scene(scenes, which, 1, seed)
    integ = native.PathIntegrator(**kw)
    job = integ.render_job(sensor)
    inc = np.random.default_rng(17).integers(0, 2 ** 63, F.JOB_W * F.JOB_H, dtype=np.uint64) | np.uint64(1)
    res = F.restate_job(H, oracle, F.from_api_scene(scene), job, F.integrator_fn(kind, kw), 1, inc=inc)
    assert not np.array_equal(res["state_after"][0], restated(name, native, oracle)[3]["state_after"][0])     # (another stream)
    cfg = integ.sample_cfg()
    dev = native.Device(0)
    try:
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            _check(name + " (rng_inc)", res, 1, lambda ray, st, i: _host(dev, cfg, ray, st, i), inc)
            _check(name + " (rng_inc)", res, 1, lambda ray, st, i: _device(dev, cfg, ray, st, i), inc)
    finally:
        dev.close()


def test_gpu_sample_spectral_against_float64_restatement(spectral, oracle_spectral):
    """scalar_spectral: the glass-block Cornell box through spectral.Device.sample, both routes, host and device arrays. The
    restatement evaluates every colour per wavelength; both sides are compared after spectrum_to_xyz in float64; the state after
    every checked ray is exact."""
    import torch
    from mitsuba2_amd import _capi
    scene, integ, job, res, model = spectral_restated(spectral, oracle_spectral)
    cfg = integ.sample_cfg()
    dev = spectral.Device(0)

    def host(ray, st, wl):
        return dev.sample(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), st, np.ascontiguousarray(ray[:, 6]),
                          np.ascontiguousarray(ray[:, 7]), wavelengths=wl, cfg=cfg)

    def device(ray, st, wl):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        s_ = t(st.view(np.int64))
        spec, valid = dev.sample_device([t(ray[:, k]) for k in range(8)], s_, wavelengths=t(wl), cfg=cfg)
        return spec.cpu().numpy(), valid.cpu().numpy() != 0, s_.cpu().numpy().view(np.uint64)
    try:
        assert dev.L.mi_spectrum_channels() == 4
        for quality in (0, 1 | _capi.MI_BVH_FORCE_TREE):
            dev.upload(scene.desc(), quality)
            for call in (host, device):
                for j in range(F.JOB_SPP):
                    wl = np.ascontiguousarray(res["wl"][j])
                    spec, valid, after = call(res["ray"][j], res["state_before"][j].copy(), wl)
                    checked, bad, dv = F.compare(xyz_of(spec, wl, model.cie, False), valid, res, j, RTOL, to_xyz=False,
                                                 want=xyz_of(res["L"][j], wl, model.cie, False))
                    msg = report("glass-spectral-path", res, checked, dv)
                    print("sample %d: %s" % (j, msg))
                    assert checked.mean() >= 1 - F.MAX_EXCLUDED and checked.sum() >= 0.95 * len(checked), msg
                    assert not bad.any(), "%s\nsample %d: %d rays differ, first ray %d: device %s, restatement %s" % (
                        msg, j, bad.sum(), np.flatnonzero(bad)[0], spec[np.flatnonzero(bad)[0]], res["L"][j, np.flatnonzero(bad)[0]])
                    wrong = checked & (after != res["state_after"][j])
                    assert not wrong.any(), "%s\nsample %d: the sampler state of %d checked rays is not the state advanced by the restatement's draw count" % (msg, j, wrong.sum())
    finally:
        dev.close()
