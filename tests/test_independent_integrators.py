"""SamplingIntegrator::sample of `path` and `direct` against an independent float64 restatement — the tier that needs no GPU.

Every film this project produces is proven bit-identical to the CPU checker (oracle/miw_oracle.cpp), whose path loop is a hand
restatement of path.cpp / direct.cpp by the author of csrc/miw/path.h and direct.h: a shared misreading of how the leaves are
COMPOSED (which pdf enters which MIS weight, when eta enters the Russian-roulette probability, that a dead path still draws its
roulette number, the order and number of sampler draws, hide_emitters, direct's sample weights) would pass every device == checker
test. tests/f64_integrators.py states both integrators a second time, in float64 numpy, from the reference sources alone.

The checker exports no per-ray sample(); it exports float64 films, and a box-filter job puts every sample into its own texel
(sample_harness.py), so film(spp = k) - film(spp = k - 1) is sample k of every pixel, exactly (asserted: each difference
round-trips through float32). The restatement runs every pixel's own sampler; sample k starts from the state its own draw count
left after sample k - 1, so a wrong number of draws anywhere turns sample k into an unrelated one.

Samples on a decision threshold (f64_integrators.Margin) are excluded, at most MAX_EXCLUDED of a job."""
import numpy as np
import pytest

import f64_integrators as F
import sample_harness as H

# Measured: the largest relative deviation max(|checker - restatement| - atol, 0) / max(|checker|, |restatement|) over the checked
# samples of each job (float32 checker against float64 restatement; every test prints it, visible with -s) and the share of
# samples excluded by a margin:
#   cornell-path            2.44e-4  3.01 %     cornell-path-d3-rr2      1.38e-4  1.69 %     cornell-path-hide        2.44e-4  3.01 %
#   cornell-direct-1-1      3.34e-4  0.97 %     cornell-direct-1-1-hide  3.34e-4  0.97 %     cornell-direct-3-2       1.35e-4  1.75 %
#   cornell-direct-2-0      8.57e-5  0.93 %     cornell-direct-0-2       0        0.54 %     balls-path               4.11e-4  2.16 %
#   balls-path-rr1          3.27e-4  1.26 %     plugin-path              1.78e-4  2.01 %     plugin-direct-1-1        3.34e-4  0.52 %
#   open-path               2.26e-4  2.80 %     open-direct-1-1          3.34e-4  1.29 %     open-nolight-path        3.36e-4  3.99 %
#   open-nolight-direct-1-1 8.36e-5  1.75 %     glass-spectral-path      2.68e-4  2.16 %  (scalar_spectral, after spectrum_to_xyz)
# RTOL = four times the largest of them (4 x 4.11e-4 = 1.64e-3), rounded up to one significant digit. The checker is the yardstick:
# the device reproduces it bit for bit, so the same bound holds there; the headroom is for a compiler contracting differently
# where the GPU suite runs, nothing else.
RTOL = 2e-3

_cache = {}


def restated(name, native, oracle):
    """the restatement of job `name`, computed once per session (the GPU tier reads the same results)"""
    if name not in _cache:
        from mitsuba2_amd import scenes
        which, kind, kw, seed = F.JOBS[name]
        read = {k: v for k, v in kw.items() if not (kind == "path" and k == "hide_emitters")}     # path_sample reads no hide_emitters: one restatement serves both
        twin = [n for n in _cache if n in F.JOBS and F.JOBS[n][:2] == (which, kind) and F.JOBS[n][3] == seed and _cache[n][4] == read]
        scene, sensor = F.job_scene(scenes, which, F.JOB_SPP, seed)
        integ = (native.PathIntegrator if kind == "path" else native.DirectIntegrator)(**kw)
        job = integ.render_job(sensor)
        res = _cache[twin[0]][3] if twin else F.restate_job(H, oracle, F.from_api_scene(scene), job, F.integrator_fn(kind, kw), F.JOB_SPP)
        _cache[name] = (scene, integ, job, res, read)
    return _cache[name][:4]


def checker_samples(native, oracle, name):
    """-> [JOB_SPP, h, w, 5] float64: sample k of every pixel = the checker's film of spp = k + 1 minus its film of spp = k"""
    from mitsuba2_amd import scenes
    which, kind, kw, seed = F.JOBS[name]
    films = [np.zeros((F.JOB_H, F.JOB_W, 5))]
    for spp in range(1, F.JOB_SPP + 1):
        scene, sensor = F.job_scene(scenes, which, spp, seed)
        integ = (native.PathIntegrator if kind == "path" else native.DirectIntegrator)(**kw)
        _, f64, _ = oracle.render(scene.desc(), integ.render_job(sensor), threads=4, want_f64=True)
        assert H.every_sample_in_its_texel(f64, spp), "job %s: a sample left its texel, pick another base seed" % name
        films.append(f64)
    diff = np.stack([films[k + 1] - films[k] for k in range(F.JOB_SPP)])
    assert np.array_equal(diff.astype(np.float32).astype(np.float64), diff)      # exact: each difference is one float32 sample
    assert (diff[..., 4] == 1).all()
    return diff


def report(name, res, checked, dev):
    n = checked.size
    return "%s: %d of %d samples checked (%.2f %% excluded), largest deviation %.3g, stats %s" % (
        name, checked.sum(), n, 100.0 * (n - checked.sum()) / n, dev, res["stats"])


@pytest.mark.parametrize("name", list(F.JOBS))
def test_checker_sample_against_float64_restatement(native, oracle, name):
    scene, integ, job, res = restated(name, native, oracle)
    want = checker_samples(native, oracle, name)
    ty, tx = res["py"] - job.cfg.crop_y, res["px"] - job.cfg.crop_x
    checked_all, bad_all, dev_all = [], [], 0.0
    for j in range(F.JOB_SPP):
        got = want[j][ty, tx]
        checked, bad, dev = F.compare(got[:, :3], got[:, 3] != 0, res, j, RTOL, to_xyz=True)
        checked_all.append(checked); bad_all.append(bad); dev_all = max(dev_all, dev)
    checked, bad = np.stack(checked_all), np.stack(bad_all)
    msg = report(name, res, checked, dev_all)
    print(msg)
    st = res["stats"]
    assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
    assert checked.sum() >= 0.95 * F.JOB_W * F.JOB_H * F.JOB_SPP, msg
    assert st["hit"] > 1000 and st["miss"] > 20, msg                                      # both hit and miss occur
    if F.JOBS[name][0].startswith("open"):
        assert st.get("miss_after_bounce", 0) > 500, msg                                  # misses that see the environment mid-path (the env-miss DirectionSample)
    if F.JOBS[name][0] in ("balls", "open", "open-nolight"):
        assert st.get("reflect", 0) > 50 and st.get("refract", 0) > 200, msg              # both lobes of the dielectric
    if F.JOBS[name][0] == "plugin":
        assert st.get("plastic_specular", 0) > 50 and st.get("plastic_diffuse", 0) > 200, msg    # both lobes of the plastic
    if bad.any():
        j, i = np.argwhere(bad)[0]
        got = want[j][ty[i], tx[i]]
        pytest.fail("%s\n%d samples differ; first: sample %d pixel (%d, %d): checker XYZ %s valid %s, restatement %s valid %s, margin %.3g (%s), draws %d"
                    % (msg, bad.sum(), j, res["px"][i], res["py"][i], got[:3], got[3], res["L"][j, i] @ F.SRGB_TO_XYZ.T, res["valid"][j, i],
                       res["margin"][j, i], res["what"][j][i], res["n_draws"][j, i]))


def spectral_restated(spectral, oracle_spectral):
    """the restatement of the scalar_spectral job (glass-block Cornell box, `path`), once per session -> (scene, integ, job, res, model)"""
    if "spectral" not in _cache:
        from conftest import SRGB_COEFF
        from mitsuba2_amd import scenes
        from test_independent_leaves import _reference_tables
        which, kind, kw, seed = F.SPECTRAL_JOB
        cie, d65 = _reference_tables()
        model = F.SrgbModel(SRGB_COEFF, cie, d65)
        scene, sensor = F.job_scene(scenes, which, F.JOB_SPP, seed)
        integ = spectral.PathIntegrator(**kw)
        job = integ.render_job(sensor)
        res = F.restate_job(H, oracle_spectral, F.from_api_scene(scene), job, F.integrator_fn(kind, kw), F.JOB_SPP, model=model)
        _cache["spectral"] = (scene, integ, job, res, model)
    return _cache["spectral"]


def xyz_of(spec, wl, cie, weighted):
    """spectrum_to_xyz in float64 of [n, 4] spectra at their wavelengths; weighted: times the wavelength weights (the camera's ray_weight)"""
    spec, wl = np.asarray(spec, np.float64), np.asarray(wl, np.float64)
    return np.stack([F.spectrum_to_xyz(s * (F.sample_rgb_spectrum_weights(w) if weighted else 1.0), w, cie) for s, w in zip(spec, wl)])


def test_checker_sample_against_float64_restatement_spectral(spectral, oracle_spectral):
    """scalar_spectral: the glass-block Cornell box. The restatement evaluates every colour per wavelength (sRGB model, srgb_d65
    radiance) and the film sample is spectrum_to_xyz of the weighted spectrum, in float64."""
    from mitsuba2_amd import scenes
    scene, integ, job, res, model = spectral_restated(spectral, oracle_spectral)
    which, kind, kw, seed = F.SPECTRAL_JOB
    films = [np.zeros((F.JOB_H, F.JOB_W, 5))]
    for spp in range(1, F.JOB_SPP + 1):
        sc, sensor = F.job_scene(scenes, which, spp, seed)
        _, f64, _ = oracle_spectral.render(sc.desc(), spectral.PathIntegrator(**kw).render_job(sensor), threads=4, want_f64=True)
        assert H.every_sample_in_its_texel(f64, spp), "a sample left its texel, pick another base seed"
        films.append(f64)
    want = np.stack([films[k + 1] - films[k] for k in range(F.JOB_SPP)])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    ty, tx = res["py"] - job.cfg.crop_y, res["px"] - job.cfg.crop_x
    checked_all, bad_all, dev_all = [], [], 0.0
    for j in range(F.JOB_SPP):
        got = want[j][ty, tx]
        checked, bad, dev = F.compare(got[:, :3], got[:, 3] != 0, res, j, RTOL, to_xyz=False, want=xyz_of(res["L"][j], res["wl"][j], model.cie, True))
        checked_all.append(checked); bad_all.append(bad); dev_all = max(dev_all, dev)
    checked, bad = np.stack(checked_all), np.stack(bad_all)
    msg = report("glass-spectral-path", res, checked, dev_all)
    print(msg)
    st = res["stats"]
    assert checked.mean() >= 1 - F.MAX_EXCLUDED and checked.sum() >= 0.95 * checked.size, msg
    assert st["hit"] > 1000 and st["miss"] > 20 and st.get("reflect", 0) > 50 and st.get("refract", 0) > 200, msg
    assert not bad.any(), "%s\n%d samples differ, first (sample, pixel) %s" % (msg, bad.sum(), np.argwhere(bad)[0])
