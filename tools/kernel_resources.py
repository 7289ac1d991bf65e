"""Register / scratch / occupancy table of every gfx950 kernel in libmiwave (no GPU needed).

    python tools/kernel_resources.py [scalar_rgb|scalar_spectral] [filter-substring] [--split] [--mangled]

Compiles csrc/miwave.hip with -Rpass-analysis=kernel-resource-usage (same flags as mitsuba2_amd/build.py)
and prints one line per kernel: a quick check after touching a leaf header that the hot kernels still fit
their launch bounds without spilling.
  --split     the translation units mitsuba2_amd/build.py compiles (build.device_units) instead of miwave.hip alone, each row
              with the object its kernel lands in
  --mangled   rows named by the mangled symbol and sorted: two commits' tables can be diffed (same kernels, same numbers)"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mitsuba2_amd import build  # noqa: E402

REMARKS = "-Rpass-analysis=kernel-resource-usage"
KEYS = ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def parse(text):
    """(mangled name, the KEYS' values) of every kernel in a compile's remarks"""
    rows = []
    for blk in re.split(r"remark: Function Name: ", text)[1:]:
        rows.append((blk.split()[0],) + tuple(int(re.search(re.escape(k) + r": (\d+)", blk).group(1)) for k in KEYS))
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    split, mangled = "--split" in sys.argv, "--mangled" in sys.argv
    variant = args[0] if args else "scalar_rgb"
    flt = args[1] if len(args) > 1 else ""
    defs = build.VARIANTS[variant][1]
    rows = []                                                        # (object, mangled name, values...)
    with tempfile.TemporaryDirectory() as tmp:
        if split:
            flags = [f for f in build.HIP_FLAGS if f != "-shared"] + defs + ["-c", REMARKS]
            units = build.device_units(tmp)
            with ThreadPoolExecutor(max_workers=build._default_jobs()) as pool:
                texts = list(pool.map(lambda u: subprocess.run([build.HIPCC] + flags + u[1] + [u[0], "-o", u[2]], capture_output=True, text=True).stderr, units))
            for (_, _, obj), text in zip(units, texts):
                rows += [(os.path.basename(obj),) + r for r in parse(text)]
        else:
            cmd = [build.HIPCC] + build.HIP_FLAGS + defs + [os.path.join(build.PKG, "csrc", "miwave.hip"), "-o", os.path.join(tmp, "x.so"), REMARKS]
            rows = [("",) + r for r in parse(subprocess.run(cmd, capture_output=True, text=True).stderr)]
    if mangled:
        for r in sorted(rows, key=lambda r: (r[1], r[0])):
            if flt in r[1]:
                print(" ".join(str(x) for x in r[1:] + r[:1]).rstrip())
        print("# %d kernels" % len(rows))
        return
    print("%-64s %5s %5s %7s %7s %8s %4s %7s" % ("kernel", "VGPR", "AGPR", "v-spill", "s-spill", "scratch", "occ", "LDS") + ("  object" if split else ""))
    for r in rows:
        dem = subprocess.run(["c++filt", r[1]], capture_output=True, text=True).stdout.strip()
        dem = dem.split("(")[0].replace("void ", "")
        if flt in dem:
            print("%-64s %5d %5d %7d %7d %8d %4d %7d" % ((dem,) + r[2:]) + ("  " + r[0] if split else ""))


if __name__ == "__main__":
    main()
