"""One case per instantiation of the path kernels: the smallest scene, upload flags, options and debug fields that make the library launch it.

csrc/miwave.hip compiles about a hundred instantiations of k_path_resident / k_path_phased / k_path_pooled / k_sample_rays per variant
(the MIW_*_LIST X-macros and a few literal launches; tests/kernel_lists.py reads them out of the source). `cases(variant)` maps each, keyed
by the text MIW_DEBUG prints for it, to a Case. test_instantiation_census.py proves on the CPU that the key set
IS the set the source can launch and that every scene has the facts its tuple needs; test_instantiation_census_gpu.py runs every case on the GPU.

Adding a tuple to a list in miwave.hip = adding a line here (or the CPU test fails, naming the tuple). Plain module: no pytest imports.

How a tuple is selected (kernel_pick.h; mi_scene_upload and mi_bvh_build set the facts):
  class      MATS_DIFFUSE   diffuse only                                      the Cornell box, the flat-shaded ball box
             MATS_PLAIN     no texture coordinates, nothing nested            the glass-block boxes (packets), plugin_box / rect_box (tree), MIW_TRIO=0
             MATS_TRIO      diffuse + dielectric + roughconductor, triangles  the glass-block box, the material balls
             MATS_ALL       texture coordinates                               the box with a panel that has them ("uv")
             MATS_NESTED    mask / blendbsdf / null / thindielectric          cutout_box
             MATS_LIGHTS    a point light                                     lit_box
  Tiny       2 / 1          up to 32 / up to 64 triangles and no analytic shape
             0              MI_BVH_FORCE_TREE (a tree that fits LDS: the lock-step kernel), analytic shapes, or more than 64 triangles
                            (a stack walk: the phase machine; a level-1 icosphere of 80 triangles is the smallest ball that gets there)
"""
import numpy as np

VARIANTS = ("scalar_rgb", "scalar_spectral")
MI_BVH_FORCE_TREE = 0x10
LOCKSTEP, PHASED, POOLED = 1, 2, 3                              # include/miwave.h: MI_PATH_KERNEL_*

W, H, SPP = 64, 64, 8                                           # every case, unless its tuple needs more
FRAME_SPP = 16                                                  # the frame twins: the recipe of test_frame_twin_gpu.py (forced chunks of 8 + 4 + 4 samples)
PLACED_W, PLACED_H, PLACED_SPP = 256, 128, 128                  # n_lanes >= 64 * n_simd / 2 (256 CUs) and spp >= 128 in one launch: the smallest film that is placed
OVERLAP_THREADS = 1024                                          # render_job(n_threads=): 2 x 2-pixel blocks, 1024 tiles >= 448: the tile-interleaved log the overlap needs
# k_sample_rays: the reassembly of sample_harness.chain (box filter; every sample must stay in its own texel — a property of the job, so the
# seed is chosen here, on the CPU: test_instantiation_census.py asserts the checker's weight channel is the sample count in every texel)
SAMPLE_W, SAMPLE_H, SAMPLE_SPP = 48, 32, 3
LIGHTS_FILM = (32, 32, 8)                                       # the MATS_LIGHTS films, reassembled from mi_sample results: box filter, LIGHTS_SEED (the chain asserts its condition)
LIGHTS_SAMPLE_FILM = (32, 24, 2)                                # ... and k_sample_rays<MATS_LIGHTS>: f64_lights.JOB_W x JOB_H at JOB_SPP, the restated job
LIGHTS_SEED = 50000                                             # f64_lights.SEED
SAMPLE_SEED = {"scalar_rgb": 50000, "scalar_spectral": 50000}


class Case:
    def __init__(self, key, group, scene, rule, integrator="path", quality=0, options=(), build_options=(), render=None, film=(W, H, SPP),
                 n_threads=1, kind="log", expect=None, variants=VARIANTS, unreachable=None, why_not=None, reference=None):
        self.key = key                      # the instantiation, as MIW_DEBUG prints it
        self.group = group                  # the launch site (kernel_lists.launchable)
        self.scene = scene                  # a name of SCENES
        self.rule = rule                    # the rule of kernel_pick.h that decides (tiny, class, analytic): path | sample_path | direct | atomic | tree
        self.integrator = integrator        # path | direct
        self.quality = quality              # mi_bvh_build flags
        self.options = tuple(options)       # (name, value) of mi_set_option, set after the upload
        self.build_options = tuple(build_options)   # ... set before it (MIW_BVH4 is read by mi_bvh_build)
        self.render = dict(render or {})    # Device.render keywords: film_mode, f64, path_kernel, tree_width, samples_per_launch
        self.film = film                    # (width, height, spp)
        self.n_threads = n_threads          # render_job(n_threads=): the block size
        self.kind = kind                    # log | atomic | placed | sample: how the GPU tier checks it
        self.expect = dict(expect or {})    # mi_counters fields after the render
        self.variants = tuple(variants)     # the variants whose library can launch it
        self.why_not = why_not              # ... and why the others cannot
        # what the GPU tier compares with. oracle: the CPU checker's film of the same job. The checker cannot render a shapeless emitter, so the MATS_LIGHTS
        # cases have none: their films are compared with the film reassembled from the device's own mi_sample results (chain: sample_harness.chain, the method
        # of test_lights_gpu.py; box filter) and their k_sample_rays with the float64 restatement of tests/f64_lights.py (f64). unplaced: the same context's
        # render with MIW_PLACE=0 (the checker needs some 20 s for the placed job; the unplaced kernel of the class is pinned by its own case at the small size)
        self.reference = reference or ("unplaced" if kind == "placed" else "oracle")
        if "MATS_LIGHTS" in key and kind != "placed":
            self.reference = "f64" if kind == "sample" else "chain"
            self.film = LIGHTS_SAMPLE_FILM if kind == "sample" else LIGHTS_FILM
        self.unreachable = unreachable      # None, or why no scene / option / debug field reaches it (names the lines that exclude it)

    def trio_on(self):
        return dict(self.options).get("MIW_TRIO") != "0"

    def tiny(self, tris, no_rects):
        return tris <= 64 and no_rects and not (self.quality & MI_BVH_FORCE_TREE)

    def pytest_id(self):
        return self.key.replace("MATS_", "").replace("INTEG_", "").replace("FEAT_", "").replace(", ", "-").replace("<", "[").replace(">", "]")


# ---- scenes: name -> (builder(api, scenes) -> scene description built with device = -1, triangles, the facts mi_scene_upload derives) ----------
BALL = ((185.0, 82.5, 169.0), 82.5)


def _facts(diffuse_only=False, trio=False, nested=False, textured=False, lights_on=False, no_rects=True):
    return dict(diffuse_only=diffuse_only, trio=trio, nested=nested, textured=textured, lights_on=lights_on, no_rects=no_rects)


def _uv_panel(api):
    """one diffuse quad WITH texture coordinates: the fact that selects MATS_ALL (mi_scene_upload: textured = !tri_uv_in.empty())"""
    v = np.array([(60, 0, 330), (150, 0, 460), (150, 220, 460), (60, 220, 330)], np.float32)
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    return api.Mesh("uv_panel", v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32), bsdf=api.BSDF("diffuse", reflectance=(0.2, 0.3, 0.8)), texcoords=uv)


def _flat_ball(api, scenes):
    meshes = [m for m in scenes.cornell_box_meshes(diffuse_only=True) if m.name != "short_block"]
    v, f, _ = scenes.icosphere(BALL[0], BALL[1], 0)
    return meshes + [api.Mesh("ball", v, f, bsdf=api.BSDF("diffuse", reflectance=scenes.WHITE))]


def _glass(scenes, short_block):
    return [m for m in scenes.cornell_box_meshes(diffuse_only=True, glass_block=True) if short_block or m.name != "short_block"]


def _rect_ball(api, scenes):
    """rect_box (analytic walls and light) with a flat-shaded diffuse level-1 icosphere on the short block: past 64 triangles"""
    v, f, _ = scenes.icosphere((185.0, 225.0, 169.0), 60.0, 1)
    return scenes.rect_box_meshes() + [api.Mesh("ball", v, f, bsdf=api.BSDF("diffuse", reflectance=scenes.WHITE))]


SCENES = {
    "cornell32": (lambda api, scenes: api.Scene(scenes.cornell_box_meshes(diffuse_only=True)).build(-1), 32, _facts(diffuse_only=True, trio=True)),
    "flatball42": (lambda api, scenes: api.Scene(_flat_ball(api, scenes)).build(-1), 42, _facts(diffuse_only=True, trio=True)),
    "glass24": (lambda api, scenes: api.Scene(_glass(scenes, False)).build(-1), 24, _facts(trio=True)),
    "glass34": (lambda api, scenes: api.Scene(_glass(scenes, True)).build(-1), 34, _facts(trio=True)),
    "plugin26": (lambda api, scenes: api.Scene(scenes.plugin_box_meshes()).build(-1), 26, _facts()),
    "uv34": (lambda api, scenes: api.Scene(scenes.cornell_box_meshes(diffuse_only=True) + [_uv_panel(api)]).build(-1), 34, _facts(textured=True, trio=True)),
    "cutout24": (lambda api, scenes: scenes.cutout_box(W, H, SPP, device=-1)[0], 24, _facts(nested=True, textured=True)),
    # (without the null rectangle in front of the camera: behind it the direct integrator, whose one bounce the Null lobe is, sees emitters only)
    "cutout22": (lambda api, scenes: scenes.cutout_box(W, H, SPP, device=-1, proxy=False)[0], 22, _facts(nested=True, textured=True)),
    "lit30": (lambda api, scenes: scenes.lit_box("point", W, H, SPP, device=-1)[0], 30, _facts(nested=True, textured=True, lights_on=True)),
    # rect_box: 6 analytic rectangles (two bounding triangles each) + the two blocks' 20 triangles
    "rect34": (lambda api, scenes: api.Scene(scenes.rect_box_meshes()).build(-1), 34, _facts(trio=True, no_rects=False)),
    # past 64 triangles: the stack walk
    "balls172": (lambda api, scenes: api.Scene(scenes.cornell_box_meshes(False, 1)).build(-1), 172, _facts(trio=True)),
    "uvballs174": (lambda api, scenes: api.Scene(scenes.cornell_box_meshes(False, 1) + [_uv_panel(api)]).build(-1), 174, _facts(textured=True, trio=True)),
    "cutoutball104": (lambda api, scenes: scenes.cutout_box(W, H, SPP, device=-1, ball_level=1)[0], 104, _facts(nested=True, textured=True)),
    "litballs170": (lambda api, scenes: scenes.lit_box("point", W, H, SPP, device=-1, diffuse_only=False, ball_level=1)[0], 170, _facts(nested=True, textured=True, lights_on=True)),
    "rectball114": (lambda api, scenes: api.Scene(_rect_ball(api, scenes)).build(-1), 114, _facts(trio=True, no_rects=False)),
}


def scene_facts(desc):
    """the facts mi_scene_upload (csrc/miwave.hip) derives from a scene description, restated: (triangles on the device, facts as _facts)"""
    d = desc.contents
    bsdfs = [d.bsdfs[i] for i in range(d.bsdf_count)]
    shapes = [d.shapes[i] for i in range(d.shape_count)]
    uv = any(s.flags & 8 for s in shapes)                                           # MI_SHAPE_HAS_TEXCOORDS
    bitmap = any(t.type == 5 for b in bsdfs for t in b.tex)                         # TEX_BITMAP
    twosided = any(b.flags & 0x100 for b in bsdfs)                                  # MI_BSDF_FLAG_TWOSIDED
    types = {b.type for b in bsdfs}                                                 # miw/bsdf.h: BSDF_TYPE_*
    lights_on = d.light_count != 0
    nested = any(7 <= t <= 10 for t in types)                                       # thindielectric, null, mask, blendbsdf
    f = _facts(diffuse_only=types <= {0} and not twosided and not uv and not bitmap, trio=types <= {0, 1, 2},
               nested=nested, textured=uv or bitmap or 6 in types or nested, lights_on=lights_on,
               no_rects=d.rectangle_count + d.sphere_count == 0)
    if lights_on:                                                                   # -> the MATS_LIGHTS kernels
        f.update(nested=True, textured=True, diffuse_only=False, trio=False)
    return d.face_count + d.rectangle_count + d.sphere_count, f


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
_FORCED = (("MIW_JOB_CHUNK_FORCE", "1"), ("MIW_JOB_CHUNK", "4"), ("MIW_PACKET_SHARD4", "0"))
_NO_SPECTRAL = dict(variants=("scalar_rgb",))


def _packet_scene(mats, tiny, integ="INTEG_PATH"):
    if mats == "MATS_NESTED" and integ == "INTEG_DIRECT":
        return "cutout22"
    return {"MATS_DIFFUSE": {2: "cornell32", 1: "flatball42"}, "MATS_PLAIN": {2: "glass24", 1: "glass34"},
            "MATS_LIGHTS": {1: "lit30"}, "MATS_NESTED": {1: "cutout24"}, "MATS_ALL": {1: "uv34"}}[mats][tiny]


def _resident_scene(tiny, mats, analytic, integ, sample):
    """(scene, quality, options) that make a rule return (tiny, mats, analytic) for the sample-log film's kernels / k_sample_rays"""
    if tiny:
        return _packet_scene(mats, tiny, integ), 0
    if mats in ("MATS_LIGHTS", "MATS_NESTED", "MATS_ALL"):
        return _packet_scene(mats, 1, integ), MI_BVH_FORCE_TREE
    if mats == "MATS_TRIO":
        return "glass34", MI_BVH_FORCE_TREE
    if integ == "INTEG_DIRECT":
        return "glass34", MI_BVH_FORCE_TREE             # (the direct integrator's tree kernels all have the analytic shapes compiled in)
    if analytic:
        return "rect34", 0
    # MATS_PLAIN without analytic shapes: mi_render has no MATS_TRIO lock-step kernel, so the trio scene gets it; mi_sample has one, so a scene outside the trio
    return ("plugin26" if sample else "glass34"), MI_BVH_FORCE_TREE


_TREE_SCENE = {("MATS_LIGHTS", "true"): ("litballs170", ()), ("MATS_NESTED", "true"): ("cutoutball104", ()), ("MATS_ALL", "true"): ("uvballs174", ()),
               ("MATS_TRIO", "false"): ("balls172", ()), ("MATS_PLAIN", "false"): ("balls172", (("MIW_TRIO", "0"),)), ("MATS_PLAIN", "true"): ("rectball114", ())}


def _args(key):
    return [a.strip() for a in key[key.index("<") + 1:-1].split(",")]


def _all_cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    MATS_ = ("MATS_DIFFUSE", "MATS_LIGHTS", "MATS_NESTED", "MATS_ALL", "MATS_PLAIN")

    def tuples(path_only_extra=()):
        for integ, mats_list in (("INTEG_PATH", MATS_), ("INTEG_DIRECT", MATS_[1:])):
            for mats in mats_list:
                if integ == "INTEG_PATH" and mats in ("MATS_DIFFUSE", "MATS_PLAIN"):
                    shapes = [(2, "false"), (1, "false")] + ([(0, "false"), (0, "true")] if mats == "MATS_PLAIN" else [])
                else:
                    shapes = [(1, "false"), (0, "true")]
                for tiny, analytic in shapes:
                    yield tiny, mats, analytic, integ
        for t in path_only_extra:
            yield t

    # k_path_resident<true, ...>: the sample-log film. The packet kernels of MATS_DIFFUSE / MATS_PLAIN have lean twins in front of the table (MIW_LEAN=0 keeps
    # the full kernel) and the 32-triangle diffuse box takes the four-wavefront shard form at this size (MIW_PACKET_SHARD4=0 keeps the table's)
    for tiny, mats, analytic, integ in tuples():
        scene, quality = _resident_scene(tiny, mats, analytic == "true", integ, False)
        opts = ()
        if integ == "INTEG_PATH" and tiny and mats in ("MATS_DIFFUSE", "MATS_PLAIN"):
            opts = (("MIW_LEAN", "0"),) + ((("MIW_PACKET_SHARD4", "0"),) if (tiny, mats) == (2, "MATS_DIFFUSE") else ())
        add("k_path_resident<true, %d, %s, %s, %s>" % (tiny, mats, analytic, integ), "resident", scene, "direct" if integ == "INTEG_DIRECT" else "path",
            integrator="direct" if integ == "INTEG_DIRECT" else "path", quality=quality, options=opts, render=dict(film_mode=1), expect=dict(path_kernel=0))
    # ... their lean twins (a scene with no environment map, no vertex normals, not the moment pass) and frame twins (+ the launch facts of
    # kernel_pick.h: frame_twin — chunk jobs forced at this size)
    for tiny, mats in ((2, "MATS_DIFFUSE"), (1, "MATS_DIFFUSE"), (2, "MATS_PLAIN"), (1, "MATS_PLAIN")):
        add("k_path_resident<true, %d, %s, false, INTEG_PATH, false, 0, FEAT_NONE>" % (tiny, mats), "lean", _packet_scene(mats, tiny), "path",
            options=(("MIW_PACKET_SHARD4", "0"),), render=dict(film_mode=1), expect=dict(path_kernel=0))
        add("k_path_resident<true, %d, %s, false, INTEG_PATH, false, 0, FEAT_FRAME>" % (tiny, mats), "frame", _packet_scene(mats, tiny), "path",
            options=_FORCED, film=(W, H, FRAME_SPP), render=dict(film_mode=1), expect=dict(path_kernel=0, job_chunk=4, job_chunks=3))
    # ... and the launches spelled out in front of the table: the overlap's Groups = true pair (the replay beside the render, opt-in), the four-wavefront
    # shard form of the 32-triangle diffuse box with and without scene features
    why = "compiled false under MIW_SPECTRAL (mi_render: packet_shard4 and overlap test !MIW_SPECTRAL)"
    for tiny, scene in ((2, "cornell32"), (1, "flatball42")):
        add("k_path_resident<true, %d, MATS_DIFFUSE, false, INTEG_PATH, true>" % tiny, "special", scene, "path", options=(("MIW_FILM_OVERLAP", "1"),),
            n_threads=OVERLAP_THREADS, render=dict(film_mode=1), expect=dict(path_kernel=0, film_overlapped=1), why_not=why, **_NO_SPECTRAL)
    add("k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 4, FEAT_NONE>", "special", "cornell32", "path", render=dict(film_mode=1),
        expect=dict(path_kernel=0), why_not=why, **_NO_SPECTRAL)
    add("k_path_resident<true, 2, MATS_DIFFUSE, false, INTEG_PATH, false, 4>", "special", "cornell32", "path", options=(("MIW_LEAN", "0"),), render=dict(film_mode=1),
        expect=dict(path_kernel=0), why_not=why, **_NO_SPECTRAL)

    # k_path_resident<false, ...>: the float64-atomics film, three classes (MATS_ALL serves every scene without lights or nested records)
    for integ in ("INTEG_PATH", "INTEG_DIRECT"):
        for mats in ("MATS_LIGHTS", "MATS_NESTED", "MATS_ALL"):
            for tiny, analytic in ((1, "false"), (0, "true")):
                add("k_path_resident<false, %d, %s, %s, %s>" % (tiny, mats, analytic, integ), "atomic", _packet_scene(mats, 1, integ), "atomic",
                    integrator="direct" if integ == "INTEG_DIRECT" else "path", quality=0 if tiny else MI_BVH_FORCE_TREE, kind="atomic",
                    render=dict(film_mode=2, f64=True), expect=dict(path_kernel=0, film_mode=2))

    # k_path_phased: six tree classes x {8-wide placed, 8-wide, 4-wide placed, 4-wide, 4-wide at three wavefronts per SIMD}
    spec = "true"
    for (mats, analytic), (scene, opts) in _TREE_SCENE.items():
        for waves, wide, placed in ((4, 2, True), (4, 2, False), (4, 1, True), (4, 1, False), (3, 1, False)):
            o = opts + ((("MIW_PHASED_WAVES", "3"),) if waves == 3 else ())
            render = dict(film_mode=1, path_kernel=PHASED, tree_width=8 if wide == 2 else 4)
            expect = dict(path_kernel=1, tree_width=8 if wide == 2 else 4, pooled=0, placed=int(placed), n_path=2 if placed else 1)
            if placed:
                render["samples_per_launch"] = PLACED_SPP
            add("k_path_phased<%s, %s, %s, %d, %d, %s>" % (mats, analytic, spec, waves, wide, "true" if placed else "false"), "phased", scene, "tree",
                options=o, render=render, expect=expect, kind="placed" if placed else "log", film=(PLACED_W, PLACED_H, PLACED_SPP) if placed else (W, H, SPP))
    # ... and over the BVH2 (MIW_BVH4=0 when the tree is built: the MATS_TRIO class only), at four and at three wavefronts per SIMD
    for waves in (4, 3):
        add("k_path_phased<MATS_TRIO, false, %s, %d, 0, false>" % (spec, waves), "bvh2", "balls172", "tree", build_options=(("MIW_BVH4", "0"),),
            options=(("MIW_PHASED_WAVES", "3"),) if waves == 3 else (), render=dict(film_mode=1), expect=dict(path_kernel=3, tree_width=2, pooled=0))

    # k_path_pooled (mi_render_cfg::debug_path_kernel = MI_PATH_KERNEL_POOLED): 12 wavefronts x 1 pixel per lane, and 8 x 2 for the MATS_TRIO class
    why = "compiled false under MIW_SPECTRAL (mi_render: `const bool pooled = false`)"
    for (mats, analytic), (scene, opts) in _TREE_SCENE.items():
        if mats in ("MATS_LIGHTS", "MATS_NESTED"):
            continue                                            # (the pooled kernel refuses them: no instantiation)
        for nw, pp in ((12, 1), (8, 2)) if mats == "MATS_TRIO" else ((12, 1),):
            add("k_path_pooled<%s, %s, %d, %d>" % (mats, analytic, nw, pp), "pooled", scene, "tree", options=opts + ((("MIW_POOL_SHAPE", "8x2"),) if pp == 2 else ()),
                render=dict(film_mode=1, path_kernel=POOLED), expect=dict(path_kernel=1, tree_width=8, pooled=1, pool_waves=nw), why_not=why, **_NO_SPECTRAL)

    # k_sample_rays: the tuples of the sample-log film + the MATS_TRIO tree kernel mi_render leaves to its phase machine
    for tiny, mats, analytic, integ in tuples([(0, "MATS_TRIO", "false", "INTEG_PATH")]):
        scene, quality = _resident_scene(tiny, mats, analytic == "true", integ, True)
        add("k_sample_rays<%d, %s, %s, %s>" % (tiny, mats, analytic, integ), "sample", scene, "direct" if integ == "INTEG_DIRECT" else "sample_path",
            integrator="direct" if integ == "INTEG_DIRECT" else "path", quality=quality, kind="sample", film=(SAMPLE_W, SAMPLE_H, SAMPLE_SPP))
    return out


_CASES = _all_cases()


def cases(variant="scalar_rgb", everything=False):
    """{key: Case} of the instantiations the library of `variant` can launch (everything: also those it compiles a constant-false condition in front of)"""
    keys = [c.key for c in _CASES]
    assert len(keys) == len(set(keys)), "a key twice in the case table"
    return {c.key: c for c in _CASES if everything or variant in c.variants}


def build_scene(name, api, scenes):
    return SCENES[name][0](api, scenes)


def integrator(api, case):
    return api.DirectIntegrator() if case.integrator == "direct" else api.PathIntegrator()


def sensor(scenes, case, variant="scalar_rgb", extra_spp=0):
    w, h, spp = case.film
    if case.reference in ("chain", "f64"):
        return scenes.cornell_sensor(w, h, spp + extra_spp, seed=LIGHTS_SEED, rfilter="box")
    if case.kind == "sample":
        return scenes.cornell_sensor(w, h, spp + extra_spp, seed=SAMPLE_SEED[variant], rfilter="box")
    return scenes.cornell_sensor(w, h, spp)


def job_key(case, variant="scalar_rgb", extra_spp=0):
    """cases with the same job_key render the same job of the same scene: one oracle render serves them all"""
    return (variant, case.scene, case.integrator, case.film, case.n_threads, case.kind == "sample", case.reference, extra_spp)
