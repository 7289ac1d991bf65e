"""Sample rates of the general sensor route (mi_render_sensor) beside mi_render's frame of the same scene, from one process.

    python tools/lens_rate.py [--spp 64] [--calls 3] [--out FILE]

One Cornell frame (the diffuse box, packet route) at 1920 x 1080, `path`, device-resident films, Msamples/s of
  1. mi_render, the perspective camera (the resident kernel: the yardstick);
  2. mi_render_sensor, the same perspective camera through the route (the same film, word for word);
  3. mi_render_sensor, thinlens (aperture 8, focus 1000) on the same camera;
and for 2 and 3, with mi_render_cfg::profile, the split of the route's time into k_sensor_step (+ k_init_pixels: mi_counters::ms_init),
k_sample_rays (ms_path - ms_init), the film replay k_aov_film (ms_film_blocks) and k_aov_film_merge (ms_film_merge).
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


def fmt(ms):
    return "median %.2f ms (min %.2f .. max %.2f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mitsuba2_amd import api, scenes
    lines = ["# kernel sources sha256[:16] = %s (bench.kernel_src_sha16(): mitsuba2_amd/csrc/**/*.{h,hip})" % bench.kernel_src_sha16(),
             "# python tools/lens_rate.py --spp %d --calls %d" % (args.spp, args.calls),
             "# C2 (diffuse Cornell box) %d x %d @ %d spp, path, films on the device; wall clock around the call; %s" % (W, H, args.spp, torch.cuda.get_device_name(0))]
    for l in lines:
        print(l, flush=True)

    def say(s):
        print(s, flush=True); lines.append(s)
    msamples = W * H * args.spp / 1e6
    dev = api.Device(0)
    try:
        scene, pinhole = scenes.cornell_box(W, H, args.spp, device=-1)
        lens = scenes.cornell_sensor(W, H, args.spp, sensor=dict(type="thinlens", aperture_radius=8.0, focus_distance=1000.0))
        dev.upload(scene.desc())
        film = torch.zeros(W * H * 5, dtype=torch.float32, device="cuda")

        def timed(call):
            wall, parts = [], []
            for i in range(args.calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev.check(call())
                t1 = time.perf_counter()
                if i >= 1:
                    c = dev.counters()
                    wall.append((t1 - t0) * 1e3); parts.append((c.ms_init, c.ms_path - c.ms_init, c.ms_film_blocks, c.ms_film_merge))
            return wall, parts

        def job_of(sensor):
            job = api.PathIntegrator().render_job(sensor)
            job.cfg.film_on_device = 1; job.cfg.profile = 1
            return job

        job = job_of(pinhole)
        wall, _ = timed(lambda: dev.L.mi_render(dev.ctx, C.byref(job.cfg), C.c_void_p(film.data_ptr())))
        say("mi_render perspective: %.1f Msamples/s; %s" % (msamples / (statistics.median(wall) * 1e-3), fmt(wall)))
        for what, sensor in (("perspective", pinhole), ("thinlens", lens)):
            job, desc = job_of(sensor), sensor.desc()
            wall, parts = timed(lambda: dev.L.mi_render_sensor(dev.ctx, C.byref(job.cfg), C.byref(desc), C.c_void_p(film.data_ptr())))
            say("mi_render_sensor %s: %.1f Msamples/s; %s" % (what, msamples / (statistics.median(wall) * 1e-3), fmt(wall)))
            for k, name in enumerate(("k_init_pixels + k_sensor_step", "k_sample_rays", "k_aov_film", "k_aov_film_merge")):
                say("    %s: %s" % (name, fmt([p[k] for p in parts])))
    finally:
        dev.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
