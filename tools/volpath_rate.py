"""Samples per second of the volpath integrator through mi_sample, beside mi_sample's `path` on the same scenes without media.

    python tools/volpath_rate.py [--scene fog-cornell|smoke-cube-gray|both] [--spp 2] [--calls 3] [--out FILE]

For the fog-cornell scene (the all-diffuse box inside a fog: a packet scene, every ray in a medium from its first segment) and
the smoke-cube-gray scene (a null-BSDF cube of smoke in the empty room; --tree forces the tree route) of scenes.volpath_scene:
the camera rays of the 1920 x 1080 frame at `spp` samples per pixel in pixel-major order, device-resident
(mi_sample_cfg::on_device = 1). Msamples / s = n / median wall time of `calls` timed calls after one warm-up call, with the spread
next to it; every call starts from the same sampler states. The comparison is mi_sample's `path` integrator (k_sample_rays) on the
same geometry with the media records taken away: what a sample costs without the media, the walks and the state machine.
mi_volpath_capped must answer 0. Line 1 of the output is the hash of the kernel sources (bench.kernel_src_sha16()).
In the style of tools/sample_rate.py, whose camera_rays it uses."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 1920, 1080


def fmt(ms):
    return "median %.2f ms (min %.2f .. max %.2f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def timed(dev, torch, rays, st0, cfg, calls):
    ms = []
    for i in range(calls + 1):
        st = st0.clone(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        spec, valid = dev.sample_device(rays, st, cfg=cfg)
        t1 = time.perf_counter()
        if i >= 1:
            ms.append((t1 - t0) * 1e3)
    return ms, float(valid.float().mean()), float(spec.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="both", choices=["fog-cornell", "smoke-cube-gray", "both"])
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--max-depth", type=int, default=-1)
    ap.add_argument("--tree", action="store_true", help="force the tree route (MI_BVH_FORCE_TREE)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()                                            # (before the library creates its context)
    import bench
    import sample_rate
    from mitsuba2_amd import api, scenes, _capi
    lines = ["# kernel sources sha256[:16] = %s (bench.kernel_src_sha16(): mitsuba2_amd/csrc/**/*.{h,hip})" % bench.kernel_src_sha16(),
             "# python tools/volpath_rate.py --scene %s --spp %d --calls %d --max-depth %d%s" % (args.scene, args.spp, args.calls, args.max_depth, " --tree" if args.tree else ""),
             "# %d x %d x %d spp = %d camera rays, pixel-major; wall clock around mi_sample (it returns when the results are there); %s"
             % (W, H, args.spp, W * H * args.spp, torch.cuda.get_device_name(0))]

    def say(s):
        print(s, flush=True); lines.append(s)
    for l in lines:
        print(l, flush=True)
    quality = (1 | _capi.MI_BVH_FORCE_TREE) if args.tree else 0
    for tag in (["fog-cornell", "smoke-cube-gray"] if args.scene == "both" else [args.scene]):
        scene = scenes.volpath_scene(tag)
        sensor = scenes.cornell_sensor(W, H, args.spp, sensor=dict(medium=scene.start_medium))
        scene.build(-1)
        bare = scenes.volpath_scene(tag)                         # the same geometry without media records
        for m in bare.shapes:
            m.set_media(None, None)
        bare = api.Scene(bare.shapes).build(-1)
        job = api.PathIntegrator().render_job(sensor)           # (the camera of the job: MI_EVAL_CAMERA_RAY reads a job mi_render would take)
        dev = api.Device(0)
        try:
            dev.upload(scene.desc(), quality)
            cols, state = sample_rate.camera_rays(dev, job, args.spp)
            n = len(state)
            rays = [torch.from_numpy(a).cuda() for a in cols]
            st0 = torch.from_numpy(state).cuda()
            ms, valid, mean = timed(dev, torch, rays, st0, api.sample_cfg("volpath", max_depth=args.max_depth), args.calls)
            med_v = statistics.median(ms)
            say("%s volpath (k_sample_volpath, %s route): %s = %.2f Msamples/s; valid %.4f, mean radiance %.5f, capped %d" %
                (tag, "tree" if args.tree else "scene's own", fmt(ms), n / med_v / 1e3, valid, mean, dev.volpath_capped()))
            dev.upload(bare.desc(), quality)
            ms, valid, mean = timed(dev, torch, rays, st0, api.sample_cfg("path", max_depth=args.max_depth), args.calls)
            med_p = statistics.median(ms)
            say("%s path without media (k_sample_rays): %s = %.2f Msamples/s; valid %.4f, mean radiance %.5f; volpath takes %.1f x as long" %
                (tag, fmt(ms), n / med_p / 1e3, valid, mean, med_v / med_p))
        finally:
            dev.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
