"""Static instruction counts of one kernel in the assembly hipcc leaves with -S / -save-temps:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-flush-denormals-to-zero -S --cuda-device-only tools/probe_resident.hip -o probe.s
    python tools/valu_count.py probe.s _Z15k_path_residentILb1ELi2ELi1ELb0ELj0E

Prints vector-ALU (v_*), scalar, LDS (ds_*), scratch and global instructions, in the whole kernel and from the header of its first
loop that contains other loops onwards — in the render kernels that is the pixel loop (the staging loops in front of it are
innermost loops), followed only by the few instructions of the epilogue. The difference of two builds is what a change took out
of, or put into, the code a path segment runs through (profiles/r07_tri_frames.txt).

Two more lines (profiles/r08_packet_diet.txt): the pixel loop's register traffic — v_mov_b32, v_readlane_b32 / v_writelane_b32 (scalar
registers the compiler keeps in the lanes of a vector register), s_nop — and the kernel's registers and spill counts from its metadata."""
import re
import sys


def count(path, kernel):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel) and re.match(r"^\S+:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    kinds = (("valu", r"v_"), ("salu", r"s_"), ("lds", r"ds_"), ("scratch", r"scratch_"), ("global", r"global_|flat_|buffer_"))
    tot = {k: 0 for k, _ in kinds}
    loop = {k: 0 for k, _ in kinds}
    extra = {"v_sqrt_f32": 0, "v_rcp_f32": 0, "v_div_scale_f32": 0, "v_div_fmas_f32": 0, "v_div_fixup_f32": 0}
    moves = {"v_mov_b32": 0, "v_readlane_b32": 0, "v_writelane_b32": 0, "s_nop": 0}
    in_loop = False
    for l in lines[start:end]:
        m = re.match(r"^\.LBB\d+_\d+:\s*;?(.*)", l)
        if m:
            in_loop = in_loop or "=>This Loop Header: Depth=1" in m.group(1)
            continue
        t = l.strip()
        if not t or t.startswith((";", ".", "//")):
            continue
        op = t.split()[0]
        for k, pat in kinds:
            if re.match(pat, op):
                tot[k] += 1
                loop[k] += 1 if in_loop else 0
                break
        base = re.sub(r"_e(32|64)$", "", op)
        if base in extra:
            extra[base] += 1
        if base in moves and in_loop:
            moves[base] += 1
    return tot, loop, extra, moves


def resources(path, kernel):
    """registers and spill counts of the kernel from the metadata at the end of the file (amdhsa.kernels)"""
    text = open(path).read()
    # (a record's scalar fields follow its argument list in alphabetical order: .name ... .sgpr_count ... .vgpr_spill_count, one list item)
    block = next((rec for rec in re.split(r"\n\s+- \.", text[text.find("amdhsa.kernels"):]) if re.search(r"\.name:\s+%s" % re.escape(kernel), rec)), "")
    return {k: int(v) for k, v in re.findall(r"\.?(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count):\s+(\d+)", block)}


if __name__ == "__main__":
    tot, loop, extra, moves = count(sys.argv[1], sys.argv[2])
    print("kernel  ", " ".join("%s %d" % kv for kv in tot.items()))
    print("main loop", " ".join("%s %d" % kv for kv in loop.items()))
    print("        ", " ".join("%s %d" % kv for kv in extra.items()))
    print("main loop", " ".join("%s %d" % kv for kv in moves.items()))
    print("resources", " ".join("%s %d" % kv for kv in sorted(resources(sys.argv[1], sys.argv[2]).items())))
