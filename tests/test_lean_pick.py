"""csrc/kernel_pick.h: which scene features a packet path kernel is compiled with (packet_features, packet_features_exist,
packet_features_kernel, packet_lean_class).

The packet kernels k_path_resident<true, tiny != 0, ..., INTEG_PATH> carry a mask of the scene features compiled into them (miw/scene.h:
FEAT_ENV, FEAT_SHAPE_NORMALS, FEAT_EMITTER_NORMALS, FEAT_MOMENT). Two masks exist as instantiations, all and none. A host program built
from the header prints the mask of every combination of the four facts, with the MIW_LEAN switch on and off:

  * the lean kernel (no feature) exactly when all four facts are false and the switch is on, every feature otherwise — the full kernel is
    correct for every scene, so a mask that is no instantiation falls back to it and is no error;
  * every mask the rule returns is one that exists, and the list of classes with a lean twin in miwave.hip (MIW_LEAN_LIST) is the one
    packet_lean_class names;
  * the rules the header had before are what they were: their picks for a handful of facts are printed before and after the calls of
    the new functions, and compared with the values tests/test_kernel_pick.py pins for them.
"""
import itertools
import re
import subprocess

import pytest

from conftest import ROOT

ALL, DIFFUSE, PLAIN, TRIO, NESTED, LIGHTS = range(6)          # miw/path.h: MATS_*
FEAT_ENV, FEAT_SHAPE_NORMALS, FEAT_EMITTER_NORMALS, FEAT_MOMENT, FEAT_ALL, FEAT_NONE = 1, 2, 4, 8, 15, 0

# (tiny, small, diffuse_only, trio, nested, textured, lights_on, no_rects, trio_on) -> path, sample path, direct, atomic, tree: the picks of the rules
# as tests/test_kernel_pick.py's parent_* chains give them
HANDFUL = {
    (1, 1, 1, 1, 0, 0, 0, 1, 1): ((2, DIFFUSE, 0), (2, DIFFUSE, 0), (1, PLAIN, 0), (1, ALL, 0), (0, TRIO, 0)),      # the Cornell box (C2)
    (1, 0, 1, 1, 0, 0, 0, 1, 1): ((1, DIFFUSE, 0), (1, DIFFUSE, 0), (1, PLAIN, 0), (1, ALL, 0), (0, TRIO, 0)),      # 33 - 64 diffuse triangles
    (1, 1, 0, 1, 0, 0, 0, 1, 1): ((2, PLAIN, 0), (2, PLAIN, 0), (1, PLAIN, 0), (1, ALL, 0), (0, TRIO, 0)),          # the glass-block box (C5's class)
    (0, 0, 0, 1, 0, 0, 0, 1, 1): ((0, PLAIN, 0), (0, TRIO, 0), (0, PLAIN, 1), (0, ALL, 1), (0, TRIO, 0)),           # a MATS_TRIO tree scene (C3 / C4)
    (0, 0, 0, 0, 1, 1, 1, 0, 1): ((0, LIGHTS, 1), (0, LIGHTS, 1), (0, LIGHTS, 1), (0, LIGHTS, 1), (0, LIGHTS, 1)),  # lights, rectangles
    (1, 0, 0, 0, 0, 1, 0, 1, 0): ((1, ALL, 0), (1, ALL, 0), (1, ALL, 0), (1, ALL, 0), (0, ALL, 1)),                 # a textured packet scene
}

MAIN = r"""
#include <stdio.h>
#include "mitsuba2_amd/csrc/kernel_pick.h"
using namespace miw_pick;
static void put(const Pick &p) { printf(" %d %d %d", p.tiny, p.mats, (int) p.analytic); }
static void rules(const char *tag) {
    static const int facts[][9] = { @FACTS@ };
    for (const auto &v : facts) {
        Facts f;
        f.tiny = v[0]; f.small = v[1]; f.diffuse_only = v[2]; f.trio = v[3]; f.nested = v[4]; f.textured = v[5]; f.lights_on = v[6]; f.no_rects = v[7]; f.trio_on = v[8];
        printf("%s", tag);
        for (int i = 0; i < 9; ++i) printf(" %d", v[i]);
        put(resident_path(f, false)); put(resident_path(f, true)); put(resident_direct(f)); put(resident_atomic(f)); put(tree_class(f));
        printf(" %d\n", (int) trio_kernel(f));
    }
}
int main() {
    rules("before");
    for (int b = 0; b < 16; ++b) {
        const unsigned needed = packet_features(b & 1, b & 2, b & 4, b & 8);
        printf("mask %d %u %d %u %u\n", b, needed, (int) packet_features_exist(needed), packet_features_kernel(needed, true), packet_features_kernel(needed, false));
    }
    for (unsigned m = 0; m < 16; ++m) printf("exists %u %d\n", m, (int) packet_features_exist(m));
    for (int t = 0; t < 3; ++t) for (int m = 0; m < 6; ++m) for (int a = 0; a < 2; ++a) { Pick p = { t, m, a != 0 }; printf("lean %d %d %d %d\n", t, m, a, (int) packet_lean_class(p)); }
    printf("bits %u %u %u %u %u %u\n", (unsigned) FEAT_ENV, (unsigned) FEAT_SHAPE_NORMALS, (unsigned) FEAT_EMITTER_NORMALS, (unsigned) FEAT_MOMENT, (unsigned) FEAT_ALL, (unsigned) FEAT_NONE);
    rules("after");
    return 0;
}
"""


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("lean_pick")
    facts = ", ".join("{ %s }" % ", ".join(str(x) for x in k) for k in HANDFUL)
    (d / "main.cpp").write_text(MAIN.replace("@FACTS@", facts))
    subprocess.check_call([build.CXX, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "picks")])
    rows = [l.split() for l in subprocess.run([str(d / "picks")], capture_output=True, text=True, check=True).stdout.splitlines()]
    return {tag: [[int(x) for x in r[1:]] for r in rows if r[0] == tag] for tag in ("before", "mask", "exists", "lean", "bits", "after")}


def test_lean_exactly_when_all_four_facts_are_false(out):
    assert out["bits"] == [[FEAT_ENV, FEAT_SHAPE_NORMALS, FEAT_EMITTER_NORMALS, FEAT_MOMENT, FEAT_ALL, FEAT_NONE]]
    assert len(out["mask"]) == 16
    for (b, needed, exists, kernel_on, kernel_off), facts in zip(out["mask"], itertools.product((0, 1), repeat=4)):
        env, shape_n, emit_n, moment = facts[::-1]                   # b counts with has_env as bit 0
        assert b == env | shape_n << 1 | emit_n << 2 | moment << 3
        assert needed == (FEAT_ENV * env | FEAT_SHAPE_NORMALS * shape_n | FEAT_EMITTER_NORMALS * emit_n | FEAT_MOMENT * moment), b
        assert kernel_on == (FEAT_NONE if not (env or shape_n or emit_n or moment) else FEAT_ALL), b
        assert kernel_off == FEAT_ALL, b                             # MIW_LEAN=0: the full kernel whatever the scene
        assert exists == int(needed in (FEAT_ALL, FEAT_NONE)), b


def test_every_mask_picked_is_an_instantiation(out):
    exists = {m for m, e in out["exists"] if e}
    assert exists == {FEAT_ALL, FEAT_NONE}                           # two per kernel, not sixteen
    for _, _, _, kernel_on, kernel_off in out["mask"]:
        assert kernel_on in exists and kernel_off in exists
    # ... and the classes with a lean twin are the ones miwave.hip instantiates and launches (MIW_LEAN_LIST), each also a tuple of the path list
    src = open(ROOT + "/mitsuba2_amd/csrc/miwave.hip").read()
    names = dict(MATS_ALL=ALL, MATS_DIFFUSE=DIFFUSE, MATS_PLAIN=PLAIN, MATS_TRIO=TRIO, MATS_NESTED=NESTED, MATS_LIGHTS=LIGHTS)
    body = re.search(r"#define MIW_LEAN_LIST\(X\)(.*)\n", src).group(1)
    listed = {(int(t), names[m]) for t, m in re.findall(r"X\((\d), (MATS_[A-Z]+)\)", body)}
    assert listed == {(2, DIFFUSE), (1, DIFFUSE), (2, PLAIN), (1, PLAIN)}
    assert {(t, m) for t, m, a, lean in out["lean"] if lean} == listed
    assert not any(lean and a for t, m, a, lean in out["lean"])      # packet scenes hold no analytic shapes
    path_body = re.sub(r"/\*.*?\*/", "", re.search(r"#define MIW_PATH_TUPLES\(X\)((?:.*\\\n)*.*)\n", src).group(1))
    path = {(int(t), names[m]) for t, m in re.findall(r"X\((\d), (MATS_[A-Z]+), false, INTEG_PATH\)", path_body)}
    assert listed <= path
    # the launches name FEAT_NONE and nothing between: the lean twins of the list, and the four-wavefront shard form of the headline
    assert len(re.findall(r"k_path_resident<true, T, M, false, INTEG_PATH, false, 0, FEAT_NONE>", src)) == 1
    assert len(re.findall(r"k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 4, FEAT_NONE>", src)) == 1


def test_the_rules_the_header_had_are_unchanged(out):
    assert out["before"] == out["after"] and len(out["before"]) == len(HANDFUL)
    for row, (facts, want) in zip(out["before"], HANDFUL.items()):
        assert tuple(row[:9]) == facts
        got = tuple(tuple(row[9 + 3 * i: 12 + 3 * i]) for i in range(5))
        assert got == want, (facts, got)
        f = dict(zip(("tiny", "small", "diffuse_only", "trio", "nested", "textured", "lights_on", "no_rects", "trio_on"), facts))
        assert row[24] == int(f["trio"] and f["trio_on"] and f["no_rects"] and not f["textured"])
