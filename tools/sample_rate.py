"""Rays per second of mi_sample (SamplingIntegrator::sample for caller-supplied rays) beside the path kernel of mi_render.

    python tools/sample_rate.py [--scene c2|c3|both] [--spp 16] [--calls 5] [--render-lib DIR] [--out FILE]

For the C2 scene (diffuse Cornell box, packet route) and the C3 scene (material balls, 40 972 triangles, tree route): the camera
rays of the 1920 x 1080 frame at `spp` samples per pixel in pixel-major order (ray p * spp + j = sample j of pixel p, jittered
inside the pixel), device-resident (mi_sample_cfg::on_device = 1) — rays / s = n / median wall time of `calls` timed calls after
two warm-up calls, with the spread (min .. max) next to it; every call starts from the same sampler states. Next to it the
`ms_path` of mi_render for the same job (profile = 1, film_mode = 1: HIP events around the path kernel; C3 with
debug_path_kernel = MI_PATH_KERNEL_LOCKSTEP — mi_sample walks trees in lock step), median and spread of as many renders.
--render-lib DIR takes that number from the libmiwave.so in DIR (a build of another commit, e.g. the parent's) instead of the
in-tree one. mi_sample does the same path work minus the film log, plus ~60 B of I/O per ray. Last the host-pointer rate
(on_device = 0: the rays are staged through the context's chunk buffer), so that the cost of the copies is visible.
Line 1 of the output is the hash of the kernel sources (bench.kernel_src_sha16())."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def _render_lib(path):
    """mi_create / mi_scene_upload / mi_bvh_build / mi_render / mi_get_counters of the libmiwave.so in `path` (any commit's)"""
    from mitsuba2_amd import _capi
    L = C.CDLL(os.path.join(path, "libmiwave.so"))
    vp = C.c_void_p
    L.mi_create.argtypes = [C.c_int32, C.POINTER(vp)]; L.mi_destroy.argtypes = [vp]; L.mi_destroy.restype = None
    L.mi_scene_upload.argtypes = [vp, C.POINTER(_capi.mi_scene_desc)]; L.mi_bvh_build.argtypes = [vp, C.c_int32]
    L.mi_render.argtypes = [vp, C.POINTER(_capi.mi_render_cfg), vp]; L.mi_get_counters.argtypes = [vp, C.POINTER(_capi.mi_counters)]
    L.mi_last_error.argtypes = [vp]; L.mi_last_error.restype = C.c_char_p
    return L


def render_ms_path(L, desc, job, lockstep, calls, film):
    from mitsuba2_amd import _capi
    ctx = C.c_void_p()
    assert L.mi_create(0, C.byref(ctx)) == 0
    try:
        assert L.mi_scene_upload(ctx, desc) == 0 and L.mi_bvh_build(ctx, 0) == 0, L.mi_last_error(ctx)
        cfg = job.cfg
        cfg.film_on_device = 1; cfg.film_f64 = 0; cfg.film_mode = 1; cfg.profile = 1; cfg.samples_per_launch = int(cfg.spp)
        cfg.debug_path_kernel = 1 if lockstep else 0             # MI_PATH_KERNEL_LOCKSTEP
        ms = []
        for i in range(calls + 2):
            assert L.mi_render(ctx, C.byref(cfg), C.c_void_p(film.data_ptr())) == 0, L.mi_last_error(ctx)
            c = _capi.mi_counters(); L.mi_get_counters(ctx, C.byref(c))
            if i >= 2:
                ms.append(c.ms_path)
        return ms, c
    finally:
        L.mi_destroy(ctx)


def camera_rays(dev, job, spp, seed=1):
    """pixel-major camera rays of the frame -> eight float32 arrays (SoA) + one PCG32 state per ray"""
    rng = np.random.default_rng(seed)
    n = W * H * spp
    p = np.repeat(np.arange(W * H, dtype=np.int64), spp)
    pos = np.empty((n, 2), np.float32)
    pos[:, 0] = (p % W).astype(np.float32) + rng.random(n, dtype=np.float32)
    pos[:, 1] = (p // W).astype(np.float32) + rng.random(n, dtype=np.float32)
    ray = dev.eval(5, pos, cfg=job.cfg)                          # MI_EVAL_CAMERA_RAY: o.xyz d.xyz mint maxt
    state = rng.integers(0, 2 ** 63, n, dtype=np.int64)
    return [np.ascontiguousarray(ray[:, k]) for k in range(8)], state


def fmt(ms):
    return "median %.2f ms (min %.2f .. max %.2f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="both", choices=["c2", "c3", "both"])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--render-lib", default=None, help="directory of the libmiwave.so whose mi_render gives the yardstick (default: the in-tree build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mitsuba2_amd import api, scenes, _capi
    lines = ["# kernel sources sha256[:16] = %s (bench.kernel_src_sha16(): mitsuba2_amd/csrc/**/*.{h,hip})" % bench.kernel_src_sha16(),
             "# python tools/sample_rate.py --scene %s --spp %d --calls %d%s" % (args.scene, args.spp, args.calls, " --render-lib <a build of the parent commit>" if args.render_lib else ""),
             "# %d x %d x %d spp = %d camera rays, pixel-major; wall clock around mi_sample (it returns when the results are there); %s"
             % (W, H, args.spp, W * H * args.spp, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True); lines.append(s)
    for l in lines:
        print(l, flush=True)
    L_render = _render_lib(args.render_lib or _capi.LIB_DIR)
    film = torch.zeros(W * H * 5, dtype=torch.float32, device="cuda")
    for tag in (["c2", "c3"] if args.scene == "both" else [args.scene]):
        scene, sensor = scenes.cornell_box(W, H, args.spp, diffuse_only=(tag == "c2"), device=-1)
        job = api.PathIntegrator().render_job(sensor)
        ms, c = render_ms_path(L_render, scene.desc(), job, tag == "c3", args.calls, film)
        say("%s mi_render ms_path%s: %s; %.3f segments / sample; path_kernel %d, plan %d" %
            (tag, " (yardstick library)" if args.render_lib else "", fmt(ms), c.segments / max(c.samples, 1), c.path_kernel, c.plan))
        yard = statistics.median(ms)
        dev = api.Device(0)
        try:
            dev.upload(scene.desc())
            cols, state = camera_rays(dev, job, args.spp)
            n = len(state)
            cfg = api.sample_cfg("path")
            rays = [torch.from_numpy(a).cuda() for a in cols]
            st0 = torch.from_numpy(state).cuda()
            ms = []
            for i in range(args.calls + 2):
                st = st0.clone(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                spec, valid = dev.sample_device(rays, st, cfg=cfg)
                t1 = time.perf_counter()
                if i >= 2:
                    ms.append((t1 - t0) * 1e3)
            med = statistics.median(ms)
            say("%s mi_sample on_device=1: %s = %.1f Mrays/s; %.2f x the yardstick's ms_path; valid %.4f, mean radiance %.5f" %
                (tag, fmt(ms), n / med / 1e3, med / yard, float(valid.float().mean()), float(spec.mean())))
            del rays, st0, st, spec, valid
            torch.cuda.empty_cache()
            fp = lambda a: a.ctypes.data_as(_capi.c_float_p)
            vp = lambda a: C.c_void_p(a.ctypes.data)
            r = _capi.mi_rays_soa(*[fp(a) for a in cols])
            spec_h = np.zeros((n, 3), np.float32); valid_h = np.zeros(n, np.uint8)
            cfg.on_device = 0
            ms = []
            for i in range(args.host_calls + 1):
                st_h = state.copy()
                t0 = time.perf_counter()
                dev.check(dev.L.mi_sample(dev.ctx, C.byref(cfg), C.byref(r), None, vp(st_h), None, vp(spec_h), vp(valid_h), n))
                t1 = time.perf_counter()
                if i >= 1:
                    ms.append((t1 - t0) * 1e3)
            med = statistics.median(ms)
            say("%s mi_sample on_device=0 (pageable host arrays in and out): %s = %.1f Mrays/s; valid %.4f" % (tag, fmt(ms), n / med / 1e3, valid_h.mean()))
        finally:
            dev.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
