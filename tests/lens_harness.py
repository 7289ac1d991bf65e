"""sample_harness.chain for a sensor with its own draw ledger (the general sensor route, mi_render_sensor).

render_sample draws, per camera sample (integrator.cpp:242-252): the jitter (next_2d), the aperture sample (next_2d, only where
sensor->needs_aperture_sample(): thinlens), the time (next_1d, only where shutter_open_time > 0), the wavelength sample (next_1d,
always). chain_lens replays exactly that on the numpy PCG32 of sample_harness; the camera rays come from `ray_fn` — the HOST
compile of the leaf (ThinLensCamera.sample_rays) —, `sample_fn` is the integrator under test as in sample_harness.chain, X Y Z are
formed with the checker's fused multiply-adds, and the film is summed in FLOAT32 in sample order: with the box filter of radius
0.5 ImageBlock::put adds a sample to exactly one texel with weight 1, the block's accumulator and the film are float32, and one
block covers a texel, so film[texel] = ((0 + aovs_0) + aovs_1) + ... in float32 (a sample ImageBlock::put rejects, imageblock.cpp:
85-109, is left out). Everything but the ledger is sample_harness's."""
import numpy as np

from sample_harness import (SCALAR_INC, pcg32_next_f32, pcg32_seed, pixels_and_seeds, sample_wavelengths, spectrum_to_xyz, srgb_to_xyz, _fp_sem)


def chain_lens(oracle, job, desc, ray_fn, sample_fn, n_samples, spectral=False):
    """desc: the sensor's mi_sensor_desc (type, shutter_open_time decide the ledger); ray_fn(position [n, 2], aperture [n, 2]) -> [n, 8]
    with the position already divided by the crop size; sample_fn as sample_harness.chain's. Yields after every sample j the float32
    film [crop_h, crop_w, 5] accumulated so far (a view: copy it to keep it)."""
    cfg = job.cfg
    assert cfg.filter_border == 0 and 0.5 <= cfg.filter_radius < 0.5002, "the reassembly holds for the box filter of radius 0.5"
    px, py, seed = pixels_and_seeds(job)
    n = len(px)
    state, inc = pcg32_seed(seed)
    assert inc == SCALAR_INC
    film = np.zeros((cfg.crop_h, cfg.crop_w, 5), np.float32)
    ty, tx = py - cfg.crop_y, px - cfg.crop_x
    crop_off = np.array([cfg.crop_x, cfg.crop_y], np.float32); crop_size = np.array([cfg.crop_w, cfg.crop_h], np.float32)
    for j in range(n_samples):
        jx, state = pcg32_next_f32(state)                          # integrator.cpp:242
        jy, state = pcg32_next_f32(state)
        aperture = np.full((n, 2), 0.5, np.float32)
        if desc.type == 1:                                         # :244-246, needs_aperture_sample()
            ax, state = pcg32_next_f32(state)
            ay, state = pcg32_next_f32(state)
            aperture = np.stack([ax, ay], 1)
        if desc.shutter_open_time > 0:                             # :248-250
            _, state = pcg32_next_f32(state)
        wsample, state = pcg32_next_f32(state)                     # :252
        pos = np.stack([px.astype(np.float32) + jx, py.astype(np.float32) + jy], 1)
        assert (jx != 0).all() and (jy != 0).all() and (pos[:, 0] > px).all() and (pos[:, 1] > py).all(), "a sample falls on its pixel's edge: pick another seed"
        adjusted = ((pos - crop_off) / crop_size).astype(np.float32)   # :254-256, float32 subtraction and division
        ray = np.asarray(ray_fn(adjusted, aperture), np.float32)
        wl = weight = None
        if spectral:
            wl, weight = sample_wavelengths(oracle, wsample)
        spec, valid, state = sample_fn(np.ascontiguousarray(ray[:, 0:3]), np.ascontiguousarray(ray[:, 3:6]), np.ascontiguousarray(ray[:, 6]),
                                       np.ascontiguousarray(ray[:, 7]), wl, state)
        spec = np.asarray(spec, np.float32); state = np.asarray(state, np.uint64)
        if spectral:
            zero = np.zeros(n, np.float32)
            weighted = np.stack([_fp_sem(oracle, weight[:, i], spec[:, i], zero)[0] for i in range(4)], 1)
            xyz = spectrum_to_xyz(oracle, weighted, wl)
        else:
            xyz = srgb_to_xyz(oracle, spec)
        aovs = np.concatenate([xyz, np.asarray(valid, bool).astype(np.float32)[:, None], np.ones((n, 1), np.float32)], 1).astype(np.float32)
        ok = (np.isfinite(aovs) & (aovs >= np.float32(-1e-5))).all(1)   # imageblock.cpp:85-109, warn_negative
        film[ty[ok], tx[ok]] += aovs[ok]                           # (every pixel once per sample: no repeated index)
        yield film
