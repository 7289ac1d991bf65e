"""csrc/kernel_pick.h: which instantiation of the path kernels a scene gets, checked against the if-chains it replaced.

mi_render picked the template arguments of k_path_resident / k_path_phased / k_path_pooled in nine if-chains and sample_launch restated
two of them for k_sample_rays; kernel_pick.h states the rules once. A wrong branch is silent (MATS_ALL where MATS_PLAIN was meant renders
the same film, slower), so the rules are pinned here: a host program built from the header prints the pick of every rule for EVERY
combination of the nine fact bits, and each is compared with the old chain, transcribed below branch by branch, in the old order, from
miwave.hip as it was before the header existed (`parent_*`: one function per chain). That covers the combinations no scene has
(lights_on without nested): the order of a chain decides what happens there, and it must not move.
"""
import itertools
import subprocess

import pytest

from conftest import ROOT

ALL, DIFFUSE, PLAIN, TRIO, NESTED, LIGHTS = range(6)          # miw/path.h: MATS_*
BITS = ("tiny", "small", "diffuse_only", "trio", "nested", "textured", "lights_on", "no_rects", "trio_on")

MAIN = r"""
#include <stdio.h>
#include "mitsuba2_amd/csrc/kernel_pick.h"
using namespace miw_pick;
static void put(const Pick &p) { printf(" %d %d %d", p.tiny, p.mats, (int) p.analytic); }
int main() {
    for (int b = 0; b < 512; ++b) {
        Facts f;
        f.tiny = b & 1; f.small = b & 2; f.diffuse_only = b & 4; f.trio = b & 8; f.nested = b & 16; f.textured = b & 32;
        f.lights_on = b & 64; f.no_rects = b & 128; f.trio_on = b & 256;
        printf("%d", b);
        put(resident_path(f, false)); put(resident_path(f, true)); put(resident_direct(f)); put(resident_atomic(f)); put(tree_class(f));
        printf(" %d\n", (int) trio_kernel(f));
    }
    return 0;
}
"""


class F:
    """the facts as the old chains named them"""
    def __init__(self, b):
        for i, name in enumerate(BITS):
            setattr(self, name, bool(b >> i & 1))
        self.rects_empty = self.no_rects
        self.trio_kernel = self.trio and self.trio_on and self.rects_empty and not self.textured    # (spelled three times in the parent, the same way)


# ---- the parent commit's chains, literally -----------------------------------------------------------------------------------
def parent_path(f):
    """mi_render, lock-step / packet route (MIW_PATH_LAUNCH and the spelled-out launches), after the overlap / shard special cases"""
    if f.tiny and f.diffuse_only and f.small: return (2, DIFFUSE, False)
    elif f.tiny and f.diffuse_only: return (1, DIFFUSE, False)
    elif f.tiny and f.lights_on: return (1, LIGHTS, False)
    elif f.tiny and f.nested: return (1, NESTED, False)
    elif f.lights_on: return (0, LIGHTS, True)
    elif f.nested: return (0, NESTED, True)
    elif f.tiny and f.textured: return (1, ALL, False)
    elif not f.tiny and f.textured: return (0, ALL, True)
    elif f.tiny and f.small: return (2, PLAIN, False)
    elif f.tiny: return (1, PLAIN, False)
    elif f.rects_empty: return (0, PLAIN, False)
    else: return (0, PLAIN, True)


def parent_direct(f):
    """mi_render, MIW_DIRECT_LAUNCH"""
    if f.tiny and f.lights_on: return (1, LIGHTS, False)
    elif f.tiny and f.nested: return (1, NESTED, False)
    elif f.lights_on: return (0, LIGHTS, True)
    elif f.nested: return (0, NESTED, True)
    elif f.tiny and f.textured: return (1, ALL, False)
    elif f.tiny: return (1, PLAIN, False)
    elif f.textured: return (0, ALL, True)
    else: return (0, PLAIN, True)


def parent_atomic(f, direct):
    """mi_render, film_mode == 2: k_path_resident<false, Tiny, Mats = MATS_ALL, Analytic = (Tiny == 0), Integ>; returns (tiny, mats, analytic, direct)"""
    if f.lights_on and direct and f.tiny: return (1, LIGHTS, False, True)
    elif f.nested and direct and f.tiny: return (1, NESTED, False, True)
    elif f.lights_on and direct: return (0, LIGHTS, True, True)
    elif f.nested and direct: return (0, NESTED, True, True)
    elif f.lights_on and f.tiny: return (1, LIGHTS, False, False)      # <false, 1, MATS_LIGHTS>: Analytic = (1 == 0)
    elif f.nested and f.tiny: return (1, NESTED, False, False)
    elif f.lights_on: return (0, LIGHTS, True, False)                  # <false, 0, MATS_LIGHTS>: Analytic = (0 == 0)
    elif f.nested: return (0, NESTED, True, False)
    elif direct and f.tiny: return (1, ALL, False, True)
    elif direct: return (0, ALL, True, True)
    elif f.tiny: return (1, ALL, False, False)                         # <false, 1>
    else: return (0, ALL, True, False)                                 # <false, 0>


def parent_phased8_placed(f):
    if f.lights_on: return (LIGHTS, True, 4, 2, True)
    elif f.nested: return (NESTED, True, 4, 2, True)
    elif f.textured: return (ALL, True, 4, 2, True)
    elif f.trio_kernel: return (TRIO, False, 4, 2, True)
    elif f.rects_empty: return (PLAIN, False, 4, 2, True)
    else: return (PLAIN, True, 4, 2, True)


def parent_phased8(f):
    if f.lights_on: return (LIGHTS, True, 4, 2, False)
    elif f.nested: return (NESTED, True, 4, 2, False)
    elif f.textured: return (ALL, True, 4, 2, False)
    elif f.trio_kernel: return (TRIO, False, 4, 2, False)
    elif f.rects_empty: return (PLAIN, False, 4, 2, False)
    else: return (PLAIN, True, 4, 2, False)


def parent_phased4_placed(f):
    if f.lights_on: return (LIGHTS, True, 4, 1, True)
    elif f.nested: return (NESTED, True, 4, 1, True)
    elif f.textured: return (ALL, True, 4, 1, True)
    elif f.trio_kernel: return (TRIO, False, 4, 1, True)
    elif f.rects_empty: return (PLAIN, False, 4, 1, True)
    else: return (PLAIN, True, 4, 1, True)


def parent_phased4(f, ph_waves):
    """(behind the `!c->view.nodes4` special case, which stays in front of the table); MIW_PHASED_LAUNCH: four or three wavefronts per SIMD"""
    if f.lights_on: return (LIGHTS, True, ph_waves, 1, False)
    elif f.nested: return (NESTED, True, ph_waves, 1, False)
    elif f.textured: return (ALL, True, ph_waves, 1, False)
    elif f.trio_kernel: return (TRIO, False, ph_waves, 1, False)
    elif f.rects_empty: return (PLAIN, False, ph_waves, 1, False)
    else: return (PLAIN, True, ph_waves, 1, False)


def parent_pooled(f, pool_pp):
    """MIW_POOLED_LAUNCH: (mats, analytic, wavefronts, pixels per lane), or the refusal"""
    if f.lights_on: return "refused: emitters"
    elif f.nested: return "refused: nested"
    elif f.textured: return (ALL, True, 12, 1)
    elif f.trio_kernel: return (TRIO, False, 8, 2) if pool_pp == 2 else (TRIO, False, 12, 1)
    elif f.rects_empty: return (PLAIN, False, 12, 1)
    else: return (PLAIN, True, 12, 1)


def parent_sample_direct(f):
    if f.tiny and f.lights_on: return (1, LIGHTS, False)
    elif f.tiny and f.nested: return (1, NESTED, False)
    elif f.lights_on: return (0, LIGHTS, True)
    elif f.nested: return (0, NESTED, True)
    elif f.tiny and f.textured: return (1, ALL, False)
    elif f.tiny: return (1, PLAIN, False)
    elif f.textured: return (0, ALL, True)
    else: return (0, PLAIN, True)


def parent_sample_path(f):
    if f.tiny and f.diffuse_only and f.small: return (2, DIFFUSE, False)
    elif f.tiny and f.diffuse_only: return (1, DIFFUSE, False)
    elif f.tiny and f.lights_on: return (1, LIGHTS, False)
    elif f.tiny and f.nested: return (1, NESTED, False)
    elif f.lights_on: return (0, LIGHTS, True)
    elif f.nested: return (0, NESTED, True)
    elif f.tiny and f.textured: return (1, ALL, False)
    elif f.textured: return (0, ALL, True)
    elif f.tiny and f.small: return (2, PLAIN, False)
    elif f.tiny: return (1, PLAIN, False)
    elif f.trio_kernel: return (0, TRIO, False)
    elif f.rects_empty: return (0, PLAIN, False)
    else: return (0, PLAIN, True)


# ---- the header's picks ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def picks(tmp_path_factory):
    from mitsuba2_amd import build
    d = tmp_path_factory.mktemp("kernel_pick")
    (d / "main.cpp").write_text(MAIN)
    subprocess.check_call([build.CXX, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "picks")])
    out = subprocess.run([str(d / "picks")], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        v = [int(x) for x in line.split()]
        t = lambda i: (v[i], v[i + 1], bool(v[i + 2]))
        rows[v[0]] = dict(path=t(1), sample_path=t(4), direct=t(7), atomic=t(10), tree=t(13), trio_kernel=bool(v[16]))
    assert sorted(rows) == list(range(512))
    return rows


def test_every_rule_is_the_parent_chain_over_all_512_fact_combinations(picks):
    for b in range(512):
        f, p = F(b), picks[b]
        assert p["trio_kernel"] == f.trio_kernel, b
        assert p["path"] == parent_path(f), (b, "path")
        assert p["direct"] == parent_direct(f), (b, "direct")
        assert p["sample_path"] == parent_sample_path(f), (b, "sample path")
        assert p["direct"] == parent_sample_direct(f), (b, "sample direct")
        for direct in (False, True):                                   # one rule for both integrators: the integrator is the launch's, not the pick's
            assert p["atomic"] + (direct,) == parent_atomic(f, direct), (b, "atomic", direct)
        # the phase machine: the rule gives the class, the launch adds (waves, wide, placed) as it finds them
        assert p["tree"][0] == 0
        m, a = p["tree"][1], p["tree"][2]
        assert (m, a, 4, 2, True) == parent_phased8_placed(f), (b, "phased8 placed")
        assert (m, a, 4, 2, False) == parent_phased8(f), (b, "phased8")
        assert (m, a, 4, 1, True) == parent_phased4_placed(f), (b, "phased4 placed")
        for w in (4, 3):
            assert (m, a, w, 1, False) == parent_phased4(f, w), (b, "phased4", w)
        # the pooled kernel: refusals in front, then the same class; the 8 x 2 shape only survives for the MATS_TRIO class (mi_render resets it otherwise)
        for pp in (1, 2):
            pool_pp = pp if f.trio_kernel else 1
            want = parent_pooled(f, pool_pp)
            if isinstance(want, str):
                assert m == (LIGHTS if f.lights_on else NESTED), (b, "pooled refusal")
            else:
                assert (m, a, 8 if pool_pp == 2 else 12, pool_pp) == want, (b, "pooled", pp)


def test_render_and_sample_agree_except_for_the_trio_tree_kernel(picks):
    """sample_launch promises "the instantiation mi_render would pick for this scene": the same rule, but for the one MATS_TRIO line"""
    differ = 0
    for b in range(512):
        f, p = F(b), picks[b]
        if p["path"] != p["sample_path"]:
            differ += 1
            assert p["sample_path"] == (0, TRIO, False) and f.trio_kernel and not f.tiny, b
            assert p["path"] == (0, PLAIN, False), b                   # (trio_kernel: no analytic rectangles)
        else:
            assert not (f.trio_kernel and not f.tiny and not f.lights_on and not f.nested), b
    assert differ > 0


def test_every_pick_is_in_its_list():
    """the lists of instantiations (miwave.hip: MIW_*_LIST) hold every tuple a rule can return: a pick outside is MI_ERR_STATE at run time"""
    import kernel_lists as K                                      # (the list parser, shared with test_instantiation_census.py)
    src = K.source()
    path, direct, atomic = K.tuples(src, "MIW_PATH_TUPLES"), K.tuples(src, "MIW_DIRECT_TUPLES"), K.tuples(src, "MIW_ATOMIC_LIST")
    assert len(path) == 12 and len(direct) == 8 and len(atomic) == 12
    tree = K.tree_classes(src)
    assert len(tree) == 6
    for b in range(512):
        f = F(b)
        assert parent_path(f) + ("INTEG_PATH",) in path and parent_direct(f) + ("INTEG_DIRECT",) in direct
        assert parent_sample_path(f) + ("INTEG_PATH",) in path | {(0, TRIO, False, "INTEG_PATH")}
        for d in (False, True):
            assert parent_atomic(f, d)[:3] + ("INTEG_DIRECT" if d else "INTEG_PATH",) in atomic
        assert parent_phased8(f)[:2] in tree
