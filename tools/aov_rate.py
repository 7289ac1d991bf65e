"""Frame times of mi_render_aov (the aov integrator) beside mi_render's path frame of the same scene, from one process.

    python tools/aov_rate.py [--spp 64] [--nested-spp 16] [--calls 5] [--out FILE]

The C2 scene (diffuse Cornell box, packet route) at 1920 x 1080, device-resident films:
  1. aovs = depth, position, sh_normal, uv and no child at `spp` samples per pixel: wall time of the call, and with
     mi_render_cfg::profile its split into the sample launches (k_init_pixels + k_aov_samples: mi_counters::ms_path), k_aov_film
     (ms_film_blocks) and k_aov_film_merge (ms_film_merge);
  2. the same channels beside a nested path integrator at `nested_spp`;
  3. the yardstick: mi_render with the path integrator at both sample counts.
Every figure is the median of `calls` timed calls after one warm-up call, with min .. max beside it. Line 1 of the output is the
hash of the kernel sources (bench.kernel_src_sha16())."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
TYPES = ["depth", "position", "sh_normal", "uv"]


def fmt(ms):
    return "median %.2f ms (min %.2f .. max %.2f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--nested-spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mitsuba2_amd import api, scenes, _capi
    lines = ["# kernel sources sha256[:16] = %s (bench.kernel_src_sha16(): mitsuba2_amd/csrc/**/*.{h,hip})" % bench.kernel_src_sha16(),
             "# python tools/aov_rate.py --spp %d --nested-spp %d --calls %d" % (args.spp, args.nested_spp, args.calls),
             "# C2 (diffuse Cornell box) %d x %d, films on the device; wall clock around the call; %s" % (W, H, torch.cuda.get_device_name(0))]
    for l in lines:
        print(l, flush=True)

    def say(s):
        print(s, flush=True); lines.append(s)
    dev = api.Device(0)
    try:
        scene, _ = scenes.cornell_box(W, H, 1, device=-1)
        dev.upload(scene.desc())

        def timed(call, cfg):
            wall, parts = [], []
            for i in range(args.calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev.check(call())
                t1 = time.perf_counter()
                if i >= 1:
                    c = dev.counters()
                    wall.append((t1 - t0) * 1e3); parts.append((c.ms_path, c.ms_film_blocks, c.ms_film_merge))
            return wall, parts

        for spp, nested in ((args.spp, None), (args.nested_spp, "path")):
            sensor = scenes.cornell_sensor(W, H, spp)
            job = api.PathIntegrator().render_job(sensor)
            cfg = job.cfg
            cfg.film_on_device = 1; cfg.profile = 1; cfg.samples_per_launch = 0
            aov = api.aov_cfg(TYPES, nested)
            nch = dev.L.mi_aov_channel_count(C.byref(aov))
            film = torch.zeros(W * H * nch, dtype=torch.float32, device="cuda")
            wall, parts = timed(lambda: dev.L.mi_render_aov(dev.ctx, C.byref(cfg), C.byref(aov), C.c_void_p(film.data_ptr())), cfg)
            say("mi_render_aov %s, %s, %d spp, %d channels: %s" % (",".join(TYPES), "nested path" if nested else "no child", spp, nch, fmt(wall)))
            for k, what in enumerate(("sample launches (k_aov_samples%s)" % (" + k_sample_rays + k_aov_finish" if nested else ""), "k_aov_film", "k_aov_film_merge")):
                say("    %s: %s" % (what, fmt([p[k] for p in parts])))
            say("    W of the centre texel %.4f; mean depth / W %.3f" % (float(film.view(H, W, nch)[H // 2, W // 2, 4]), float((film.view(H, W, nch)[..., 5] / film.view(H, W, nch)[..., 4]).mean())))
            del film
            film5 = torch.zeros(W * H * 5, dtype=torch.float32, device="cuda")
            cfg.film_mode = 0
            wall, parts = timed(lambda: dev.L.mi_render(dev.ctx, C.byref(cfg), C.c_void_p(film5.data_ptr())), cfg)
            say("mi_render path, %d spp (the yardstick): %s; its path kernel %s" % (spp, fmt(wall), fmt([p[0] for p in parts])))
            del film5
            torch.cuda.empty_cache()
    finally:
        dev.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
