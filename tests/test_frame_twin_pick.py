"""csrc/kernel_pick.h: which launch takes the FRAME twin of a lean packet path kernel (frame_twin, LaunchFacts).

A frame twin, k_path_resident<true, tiny, class, false, INTEG_PATH, false, 0, FEAT_FRAME>, is a lean twin with the facts of a full frame's
launch compiled in: chunk jobs on, one queue, the 16-byte log, no tail priorities, the leaf filter on, no group counts. It is correct for that launch
only, so the rule must hold it back whenever one fact is otherwise. A host program built from the header prints the rule over every combination of

    the six launch facts x the MIW_FRAME_TWIN switch x direct x the feature mask (none, all, one between) x every (tiny, class, analytic)

and the test restates the rule: the twin exactly when the switch is on, the integrator is the path integrator, the mask is FEAT_NONE, the class is one of
MIW_LEAN_LIST (packet kernel, no analytic shapes, MATS_DIFFUSE or MATS_PLAIN) and all six facts are as compiled in.
"""
import re
import subprocess

import pytest

from conftest import ROOT

ALL, DIFFUSE, PLAIN, TRIO, NESTED, LIGHTS = range(6)          # miw/path.h: MATS_*
FEAT_ALL, FEAT_NONE = 15, 0
MASKS = (FEAT_NONE, FEAT_ALL, 2)
LEAN_LIST = {(2, DIFFUSE), (1, DIFFUSE), (2, PLAIN), (1, PLAIN)}
# the facts as the twin has them compiled in: job_chunks, log_rec16, one_queue, tail_prio, leaf_filter, group_counts
AS_COMPILED = (1, 1, 1, 0, 1, 0)

MAIN = r"""
#include <stdio.h>
#include "mitsuba2_amd/csrc/kernel_pick.h"
using namespace miw_pick;
int main() {
    static const unsigned masks[] = { @MASKS@ };
    for (int bits = 0; bits < 64; ++bits) for (int on = 0; on < 2; ++on) for (int direct = 0; direct < 2; ++direct) for (unsigned mask : masks)
        for (int t = 0; t < 3; ++t) for (int m = 0; m < 6; ++m) for (int a = 0; a < 2; ++a) {
            LaunchFacts l;
            l.job_chunks = bits & 1; l.log_rec16 = bits & 2; l.one_queue = bits & 4; l.tail_prio = bits & 8; l.leaf_filter = bits & 16; l.group_counts = bits & 32;
            const Pick p = { t, m, a != 0 };
            printf("%d %d %d %u %d %d %d %d\n", bits, on, direct, mask, t, m, a, (int) frame_twin(p, direct != 0, mask, l, on != 0));
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("frame_twin_pick")
    (d / "main.cpp").write_text(MAIN.replace("@MASKS@", ", ".join("%du" % m for m in MASKS)))
    subprocess.check_call([build.CXX, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "twin")])
    out = subprocess.run([str(d / "twin")], capture_output=True, text=True, check=True).stdout
    return [tuple(int(x) for x in l.split()) for l in out.splitlines()]


def _facts(bits):
    return tuple((bits >> i) & 1 for i in range(6))


def test_the_twin_exactly_when_every_fact_is_as_compiled_in(rows):
    assert len(rows) == 64 * 2 * 2 * len(MASKS) * 3 * 6 * 2
    taken = 0
    for bits, on, direct, mask, t, m, a, twin in rows:
        want = bool(on) and not direct and mask == FEAT_NONE and (t, m) in LEAN_LIST and not a and _facts(bits) == AS_COMPILED
        assert bool(twin) == want, (bits, on, direct, mask, t, m, a)
        taken += twin
    assert taken == len(LEAN_LIST)                                   # one combination per class of the list, nothing else


def test_one_fact_off_holds_the_twin_back(rows):
    by_key = {r[:7]: r[7] for r in rows}
    good = sum(v << i for i, v in enumerate(AS_COMPILED))
    for t, m in LEAN_LIST:
        assert by_key[(good, 1, 0, FEAT_NONE, t, m, 0)] == 1
        for i in range(6):                                           # each launch fact alone
            assert by_key[(good ^ (1 << i), 1, 0, FEAT_NONE, t, m, 0)] == 0, (t, m, i)
        assert by_key[(good, 0, 0, FEAT_NONE, t, m, 0)] == 0         # MIW_FRAME_TWIN=0
        assert by_key[(good, 1, 1, FEAT_NONE, t, m, 0)] == 0         # direct
        assert by_key[(good, 1, 0, FEAT_ALL, t, m, 0)] == 0          # the full kernel's launch (a scene feature, or MIW_LEAN=0)
        assert by_key[(good, 1, 0, 2, t, m, 0)] == 0
        assert by_key[(good, 1, 0, FEAT_NONE, t, m, 1)] == 0         # (no packet scene holds analytic shapes)


def test_classes_outside_the_lean_list_and_direct_never_take_it(rows):
    for bits, on, direct, mask, t, m, a, twin in rows:
        if (t, m) not in LEAN_LIST or a or direct:
            assert not twin, (bits, on, direct, mask, t, m, a)


def test_the_launch_site_follows_the_rule():
    src = open(ROOT + "/mitsuba2_amd/csrc/miwave.hip").read()
    # one launch of the twins, expanded from the list of the lean twins and in front of their launch; the rule's answer is the only thing it asks
    assert len(re.findall(r"k_path_resident<true, T, M, false, INTEG_PATH, false, 0, FEAT_FRAME>", src)) == 1
    assert src.index("MIW_LEAN_LIST(MIW_FRAME_LAUNCH)") < src.index("MIW_LEAN_LIST(MIW_LEAN_LAUNCH)")
    assert re.search(r"#define MIW_FRAME_LAUNCH\(T, M\) if \(frame && MIW_PICKED\(T, M, false\)\)", src)
    assert len(re.findall(r"miw_pick::frame_twin\(", src)) == 1 and '!ropt.off("MIW_FRAME_TWIN")' in src
    # the Groups pair, the four-wavefront shard form, the direct kernels and the float64-atomics film name no twin
    assert len(re.findall(r"k_path_resident<[^<>]*FEAT_FRAME>\)", src)) == 1
    assert src.count('"MIW_FRAME_TWIN"') == 2                   # the options table and the launch
