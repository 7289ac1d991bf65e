"""The lists of path-kernel instantiations, read out of csrc/miwave.hip (shared by test_kernel_pick.py and test_instantiation_census.py).

miwave.hip names every instantiation of k_path_resident / k_path_phased / k_path_pooled / k_sample_rays it can launch in X-macro lists
(MIW_*_LIST) that a launch macro (MIW_*_LAUNCH) is applied to, plus a few literal launches in front of the tables. This module parses both:
`tuples()` / `tree_classes()` give the lists as test_kernel_pick.py compares them with the rules, `launchable()` gives every
instantiation as the text MIW_DEBUG prints for it ("NAME<ARG, ARG, ...>") — the template-id of the
launch inside each launch macro (MIW_LAUNCH_NAMED / hipLaunchKernelGGL) with the macro's parameters replaced by a list entry's arguments. No pytest imports.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba2_amd", "csrc")

ALL, DIFFUSE, PLAIN, TRIO, NESTED, LIGHTS = range(6)          # miw/path.h: MATS_*
MATS = dict(MATS_ALL=ALL, MATS_DIFFUSE=DIFFUSE, MATS_PLAIN=PLAIN, MATS_TRIO=TRIO, MATS_NESTED=NESTED, MATS_LIGHTS=LIGHTS)


def source():
    return open(os.path.join(CSRC, "miwave.hip")).read()


def body(src, name):
    """the replacement text of `#define name(X[, ...])`, continuation lines joined, comments removed"""
    m = re.search(r"#define %s\(X(?:, \.\.\.)?\)((?:.*\\\n)*.*)\n" % name, src)
    assert m, "no #define %s(X) in miwave.hip" % name
    return re.sub(r"/\*.*?\*/", "", m.group(1))


def tuples(src, name):
    """{(tiny, class, analytic, "INTEG_...")} of a list of X(Tiny, Mats, Analytic, Integ) entries"""
    return {(int(t), MATS[m], a == "true", i) for t, m, a, i in re.findall(r"X\((\d), (MATS_[A-Z]+), (true|false), (INTEG_[A-Z]+)\)", body(src, name))}


def tree_classes(src):
    """{(class, analytic)} of MIW_TREE_CLASSES"""
    return {(MATS[m], a == "true") for m, a in re.findall(r"X\((MATS_[A-Z]+), (true|false), __VA_ARGS__\)", body(src, "MIW_TREE_CLASSES"))}


# ---- every instantiation the source can launch, as MIW_DEBUG spells it ---------------------------------------------------------

def _entries(src, name, seen=()):
    """the argument lists of the X(...) entries of a list, lists that name other lists expanded: [["2", "MATS_DIFFUSE", ...], ...]"""
    assert name not in seen
    out = []
    for m in re.finditer(r"\b(X|MIW_[A-Z0-9_]+)\(([^()]*)\)", body(src, name)):
        head, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
        if head == "X":
            out.append(args)
        else:                                                  # MIW_PATH_TUPLES(X) / MIW_TREE_CLASSES(X, 4, 2, true): a list applied inside a list
            assert args[0] == "X", (name, m.group(0))
            for e in _entries(src, head, seen + (name,)):
                out.append([a for a in e if a != "__VA_ARGS__"] + (args[1:] if "__VA_ARGS__" in e else []))
    return out


def _launch_macro(src, name):
    """(parameter names, template-id) of a launch macro: the kernel its hipLaunchKernelGGL instantiates"""
    m = re.search(r"#define %s\(([^)]*)\)((?:.*\\\n)*.*)\n" % name, src)
    assert m, "no #define %s in miwave.hip" % name
    ids = re.findall(r"(?:hipLaunchKernelGGL\(|MIW_LAUNCH_NAMED\([a-z>-]+, )\((k_[a-z_]+<[^>]*>)\)", m.group(2))
    assert len(set(ids)) == 1, (name, ids)
    return [p.strip() for p in m.group(1).split(",")], ids[0]


def _apply(params, template, args):
    assert len(params) == len(args), (params, args)
    for p, a in zip(params, args):
        template = re.sub(r"\b%s\b" % re.escape(p), a, template)
    return template


def phase_spec():
    """device/phased_kernel.h: MIW_PHASE_SPEC, the Spec argument of every k_path_phased (MIW_DEBUG prints its value)"""
    m = re.search(r"#define MIW_PHASE_SPEC (\d)", open(os.path.join(CSRC, "device", "phased_kernel.h")).read())
    return "true" if int(m.group(1)) else "false"


def launchable(src=None):
    """{group: [instantiation, ...]} of everything mi_render and sample_launch can launch; the groups are the launch sites:
    resident, lean, frame, special (the literal launches in front of the packet table), atomic, phased, bvh2, pooled, sample"""
    src = src or source()
    out = {}
    for group, macro, lst in (("resident", "MIW_RESIDENT_LAUNCH", "MIW_RESIDENT_LIST"), ("lean", "MIW_LEAN_LAUNCH", "MIW_LEAN_LIST"),
                              ("frame", "MIW_FRAME_LAUNCH", "MIW_LEAN_LIST"), ("atomic", "MIW_ATOMIC_LAUNCH", "MIW_ATOMIC_LIST"),
                              ("phased", "MIW_PHASED_LAUNCH_", "MIW_PHASED_LIST"), ("pooled", "MIW_POOLED_LAUNCH", "MIW_POOLED_LIST"),
                              ("sample", "MIW_SAMPLE_LAUNCH", "MIW_SAMPLE_LIST")):
        params, template = _launch_macro(src, macro)
        out[group] = [_apply(params, template, e) for e in _entries(src, lst)]
    # the literal launches: the packet kernel's specials ...
    out["special"] = re.findall(r"MIW_PACKET_SPECIAL\((k_path_resident<[^>]*>)\);", src)
    # ... and the phase machine over the BVH2: MIW_PHASED_LAUNCH(M, A, W) launches MIW_PHASED_LAUNCH_(M, A, waves, W, false) for each wave count it names
    params, template = _launch_macro(src, "MIW_PHASED_LAUNCH_")
    m = re.search(r"#define MIW_PHASED_LAUNCH\(M, A, W\)(.*)\n", src)
    inner = re.findall(r"MIW_PHASED_LAUNCH_\(M, A, (\d), W, (true|false)\)", m.group(1))
    out["bvh2"] = []
    for call in re.findall(r"[^_A-Z]MIW_PHASED_LAUNCH\((MATS_[A-Z]+), (true|false), (\d)\);", src):
        out["bvh2"] += [_apply(params, template, [call[0], call[1], wv, call[2], pl]) for wv, pl in inner]
    spec = phase_spec()
    for g in ("phased", "bvh2"):
        out[g] = [k.replace("MIW_PHASE_SPEC != 0", spec) for k in out[g]]
    return out


def spectral_excluded(src=None):
    """the groups / instantiations the scalar_spectral build compiles a constant-false condition in front of: the pooled kernel
    (`#if MIW_SPECTRAL ... const bool pooled = false`), the four-wavefront shard form and the overlap's pair (`!MIW_SPECTRAL` in
    packet_shard4 and overlap). Asserts that the source still says so."""
    src = src or source()
    assert re.search(r"#if MIW_SPECTRAL\n\s*const bool pooled = false;", src)
    assert re.search(r"bool packet_shard4 = [^;]*!MIW_SPECTRAL[^;]*;", src)
    assert re.search(r"const bool overlap = [^;]*!MIW_SPECTRAL[^;]*;", src)
    L = launchable(src)
    return set(L["pooled"]) | set(L["special"])
