"""The case table of the instantiation census (tests/instantiation_cases.py) is complete, and its scenes are what it says: the CPU tier.

csrc/miwave.hip can launch about a hundred separately compiled instantiations of the four path kernels per variant. The GPU tier
(test_instantiation_census_gpu.py) runs one case per instantiation; here, without a GPU:

  - the set of instantiations the SOURCE can launch (tests/kernel_lists.py: the MIW_*_LIST X-macros applied to their launch macros, the literal
    launches in front of the tables) equals the key set of the case table, for scalar_rgb and for scalar_spectral. A tuple added to a list without a
    case, or a case for a tuple that is gone, fails here with the tuple's name;
  - every scene of the table builds, and has the triangle count and the facts (mi_scene_upload's, restated in instantiation_cases.scene_facts)
    its entry claims; for every case the rule of kernel_pick.h that decides its (tiny, class, analytic) — evaluated by the host enumerator
    test_kernel_pick.py builds from the header — returns the case's tuple for those facts;
  - an entry marked `unreachable` is returned by NO rule over all 512 fact combinations (a mark the rules contradict fails);
  - the CPU checker renders every job of the table the GPU tier compares with it: a non-black film with weight in every texel, and for the
    k_sample_rays jobs (box filter) weight == spp in every texel at spp and spp + 1 — every sample stays in its own texel, the condition of the
    reassembly, which fixes the sampler seed in the table.
"""
import re

import numpy as np
import pytest

import instantiation_cases as IC
import kernel_lists as K
import sample_harness as H
from test_kernel_pick import BITS, picks                      # noqa: F401  (the fixture: kernel_pick.h's rules over all 512 fact combinations)

TEMPLATES = ("k_path_resident<true", "k_path_resident<false", "k_path_phased", "k_path_pooled", "k_sample_rays")


def _tuple_of(case):
    """(tiny, class, analytic) the case's key names, as the rule of its launch site returns it"""
    a = IC._args(case.key)
    if case.key.startswith("k_path_resident"):
        return int(a[1]), K.MATS[a[2]], a[3] == "true"
    if case.key.startswith("k_sample_rays"):
        return int(a[0]), K.MATS[a[1]], a[2] == "true"
    return 0, K.MATS[a[0]], a[1] == "true"                      # k_path_phased / k_path_pooled: the tree class


@pytest.mark.parametrize("variant", IC.VARIANTS)
def test_the_case_table_is_the_set_of_instantiations_the_source_can_launch(variant):
    src = K.source()
    groups = K.launchable(src)
    excluded = K.spectral_excluded(src) if variant == "scalar_spectral" else set()
    source_keys = {k for g in groups.values() for k in g} - excluded
    assert sum(len(g) for g in groups.values()) == len({k for g in groups.values() for k in g}), "an instantiation is listed twice"
    table = IC.cases(variant)
    for t in TEMPLATES:
        print("%s: %s...>: %d instantiations" % (variant, t, sum(k.startswith(t) for k in source_keys)))
    print("%s: %d instantiations in all; by launch site: %s" % (variant, len(source_keys), {g: len(set(v) - excluded) for g, v in groups.items()}))
    missing, gone = sorted(source_keys - set(table)), sorted(set(table) - source_keys)
    assert not missing, "%s: instantiations of miwave.hip without a case in tests/instantiation_cases.py: %s" % (variant, missing)
    assert not gone, "%s: cases of tests/instantiation_cases.py for instantiations miwave.hip cannot launch: %s" % (variant, gone)
    for key, case in table.items():
        assert key in groups[case.group], (key, case.group)
    # the cases only the other variant has are exactly the ones this variant's build compiles a constant-false condition in front of, and they say why
    everything = IC.cases(variant, everything=True)
    for key, case in everything.items():
        if variant not in case.variants:
            assert key in excluded and case.why_not, key
    assert {k for k in everything if k not in table} == (excluded if variant == "scalar_spectral" else set())


def test_a_list_entry_more_or_less_is_noticed():
    """the completeness test above would fail on an edited source: one X(...) deleted from a list, and one added, change launchable()"""
    src = K.source()
    before = {k for g in K.launchable(src).values() for k in g}
    less = src.replace("X(MATS_TRIO, false, 8, 2) ", "", 1)
    more = src.replace("X(MATS_TRIO, false, 8, 2) ", "X(MATS_TRIO, false, 8, 2) X(MATS_ALL, true, 8, 2) ", 1)
    assert less != src and more != src
    assert before - {k for g in K.launchable(less).values() for k in g} == {"k_path_pooled<MATS_TRIO, false, 8, 2>"}
    assert {k for g in K.launchable(more).values() for k in g} - before == {"k_path_pooled<MATS_ALL, true, 8, 2>"}


def _bits(facts, tiny, small, trio_on):
    f = dict(facts, tiny=tiny, small=small, trio_on=trio_on)
    return sum(int(bool(f[name])) << i for i, name in enumerate(BITS))


@pytest.fixture(scope="module")
def built(native):
    from mitsuba2_amd import scenes
    return {name: IC.build_scene(name, native, scenes) for name in IC.SCENES}


def test_every_scene_has_the_facts_its_cases_need(native, built, picks):
    for name, (_, tris, facts) in IC.SCENES.items():
        got_tris, got = IC.scene_facts(built[name].desc())
        assert (got_tris, got) == (tris, facts), (name, got_tris, got)
    for variant in IC.VARIANTS:
        for key, case in IC.cases(variant).items():
            if case.unreachable:
                continue
            _, tris, facts = IC.SCENES[case.scene]
            tiny = case.tiny(tris, facts["no_rects"])
            pick = picks[_bits(facts, tiny, tris <= 32, case.trio_on())][case.rule]
            assert pick == _tuple_of(case), "%s: for the facts of scene %s the rule %s gives %s" % (key, case.scene, case.rule, pick)
            if case.rule == "tree":                               # the phase machine needs a stack walk: past MIW_BRUTE_MAX_TRIS triangles (mi_bvh_build)
                assert tris > 64 and not case.quality
            elif not tiny:                                        # the lock-step tree kernels: a tree that fits LDS (forced, or analytic shapes), at most 64 triangles
                assert tris <= 64
            w, h, spp = case.film
            if case.kind == "placed":                             # mi_render: place needs n_lanes >= 64 * n_simd / 2 (256 CUs) and every sample in one launch of >= 128
                assert w * h >= 64 * 256 * 4 // 2 and spp >= 128 and case.render["samples_per_launch"] >= spp and (w, h, spp) == (IC.PLACED_W, IC.PLACED_H, IC.PLACED_SPP)


def test_an_unreachable_mark_is_not_contradicted_by_the_rules(picks):
    marked = 0
    for variant in IC.VARIANTS:
        for key, case in IC.cases(variant, everything=True).items():
            if not case.unreachable:
                continue
            marked += 1
            assert re.search(r"kernel_pick\.h|mi_render|sample_launch", case.unreachable), "%s: the reason names the lines that exclude it" % key
            for b in range(512):
                assert picks[b][case.rule] != _tuple_of(case), "%s is marked unreachable, but the rule %s returns it for the facts %#x" % (key, case.rule, b)
    print("%d instantiations marked unreachable" % marked)


@pytest.mark.parametrize("variant", IC.VARIANTS)
def test_the_checker_sees_every_job(request, native, variant):
    from mitsuba2_amd import scenes
    api = native
    if variant == "scalar_spectral":
        api = request.getfixturevalue("spectral")
        orc = request.getfixturevalue("oracle_spectral")
    else:
        orc = request.getfixturevalue("oracle")
    seen, scene_of = set(), {}
    for key, case in IC.cases(variant).items():
        if case.reference != "oracle" or case.unreachable:
            continue                                              # (placed: the same scene as the class's small case; MATS_LIGHTS: the checker renders no shapeless emitter)
        for extra in (0, 1) if case.kind == "sample" else (0,):
            k = IC.job_key(case, variant, extra)
            if k in seen:
                continue
            seen.add(k)
            if case.scene not in scene_of:
                scene_of[case.scene] = IC.build_scene(case.scene, api, scenes)
            job = IC.integrator(api, case).render_job(IC.sensor(scenes, case, variant, extra), n_threads=case.n_threads)
            o32, o64, st = orc.render(scene_of[case.scene].desc(), job, threads=8, want_f64=True)
            w, h, spp = case.film
            assert o32.shape == (h, w, 5) and st.samples == w * h * (spp + extra)
            assert float(np.nanmax(o32[..., :3])) > 0 and o32[..., 4].min() > 0, (key, "a black film, or a texel without weight")
            if case.kind == "sample":
                assert H.every_sample_in_its_texel(o64, spp + extra), "%s: a sample leaves its texel at spp %d: pick another SAMPLE_SEED" % (key, spp + extra)
    print("%s: %d checker renders" % (variant, len(seen)))
