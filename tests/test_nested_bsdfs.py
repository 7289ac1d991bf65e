"""The mask / blendbsdf wrappers and the null / thindielectric leaves on the CPU: known answers through the host classes and
through the checker's BSDF query (oracle.eval op 3: [record, wi, sample1, sample2, wo] -> [wo, pdf, eta, sampled_type, weight,
eval, pdf]), the record table Scene::build flattens them into, the XML front-end, and the CPU wavefront emulator against the
scalar checker on scenes.cutout_box."""
import numpy as np
import pytest

NULL, DIFFUSE, GLOSSY, DELTA_R = 0x1, 0x2, 0x8, 0x20
INV_PI = np.float32(1 / np.pi)


def _one_shape_scene(native, bsdf):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return native.Scene([native.Mesh("t", v, np.array([[0, 1, 2]], np.uint32), bsdf=bsdf)]).build(-1)


def _query(oracle, scene, wi, s1, s2=(0.3, 0.6), wo=(0, 0, 1), record=0):
    q = np.zeros((1, 10), np.float32)
    q[0, 0] = record; q[0, 1:4] = wi; q[0, 4] = s1; q[0, 5:7] = s2; q[0, 7:10] = wo
    o = oracle.eval(3, q, scene.desc())[0]
    return dict(wo=o[0:3], pdf=o[3], eta=o[4], type=int(o[5:6].view(np.uint32)[0]), weight=o[6:9], eval=o[9:12], eval_pdf=o[12])


def test_blend_known_answers(native, oracle):
    """src/bsdfs/tests/test_blendbsdf.py: weight 0.2 between reflectance 0 and reflectance 1 evaluates to 0.2 / pi at normal
    incidence; the flags are the union of the children's (test01)."""
    black, white = native.BSDF("diffuse", reflectance=(0, 0, 0)), native.BSDF("diffuse", reflectance=(1, 1, 1))
    blend = native.BlendBSDF(black, white, weight=0.2)
    e, p = blend.eval_pdf([0, 0, 1], [0, 0, 1])
    assert np.allclose(e, 0.2 / np.pi, rtol=1e-6) and np.isclose(p, 1 / np.pi, rtol=1e-6)
    r = _query(oracle, _one_shape_scene(native, blend), [0, 0, 1], 0.5)
    assert np.array_equal(r["eval"], e) and r["eval_pdf"] == p
    rough = native.BSDF("roughconductor", alpha=0.2)
    assert native.BlendBSDF(black, rough, weight=0.5).flags() == DIFFUSE | GLOSSY
    assert native.BlendBSDF(rough, native.BSDF("conductor"), weight=0.5).flags() == GLOSSY | DELTA_R
    # sample1 > weight takes child 0 with (sample1 - weight) / (1 - weight), sample1 <= weight child 1 with sample1 / weight
    pl = native.BSDF("plastic")
    b2 = native.BlendBSDF(pl, white, weight=0.25)
    wi = np.array([0.3, 0.2, 0.9], np.float32); wi /= np.linalg.norm(wi)
    got = b2.sample(wi, 0.5, (0.3, 0.6)); want = pl.sample(wi, (np.float32(0.5) - np.float32(0.25)) / (np.float32(1) - np.float32(0.25)), (0.3, 0.6))
    assert all(np.array_equal(got[k], want[k]) for k in got)
    got = b2.sample(wi, 0.25, (0.3, 0.6)); want = white.sample(wi, 1.0, (0.3, 0.6))
    assert all(np.array_equal(got[k], want[k]) for k in got)


def test_thindielectric_and_null_known_answers(native, oracle):
    td = native.BSDF("thindielectric")                           # bk7 / air
    assert td.record().type == 7 and td.flags() == DELTA_R | NULL
    eta = np.float32(1.5046) / np.float32(1.000277)
    r = ((eta - 1) / (eta + 1)) ** 2
    rp = 2 * r / (1 + r)                                         # r' = r + trt + tr^3t + ...
    scene = _one_shape_scene(native, td)
    for wi in ([0, 0, 1], [0, 0, -1]):
        lo = _query(oracle, scene, wi, np.float32(rp) * np.float32(0.99))
        hi = _query(oracle, scene, wi, np.float32(rp) * np.float32(1.01))
        assert lo["type"] == DELTA_R and np.isclose(lo["pdf"], rp, rtol=1e-5) and np.array_equal(lo["wo"], np.float32([0, 0, wi[2]]))
        assert hi["type"] == NULL and np.isclose(hi["pdf"], 1 - rp, rtol=1e-5) and np.array_equal(hi["wo"], -np.float32(wi))
        assert lo["eta"] == 1 and hi["eta"] == 1 and np.array_equal(lo["weight"], [1, 1, 1]) and np.array_equal(hi["weight"], [1, 1, 1])
        assert not lo["eval"].any() and lo["eval_pdf"] == 0
    tinted = native.BSDF("thindielectric", specular_reflectance=(0.5, 0.6, 0.7), specular_transmittance=(0.9, 0.8, 0.7))
    assert np.array_equal(tinted.sample([0, 0, 1], 0.0, (0, 0))["weight"], np.float32([0.5, 0.6, 0.7]))
    assert np.array_equal(tinted.sample([0, 0, 1], 0.9, (0, 0))["weight"], np.float32([0.9, 0.8, 0.7]))
    nl = native.BSDF("null")
    assert nl.record().type == 8 and nl.flags() == NULL
    wi = np.float32([0.6, 0.0, -0.8])
    s = _query(oracle, _one_shape_scene(native, nl), wi, 0.7)
    assert np.array_equal(s["wo"], -wi) and s["pdf"] == 1 and s["eta"] == 1 and s["type"] == NULL and np.array_equal(s["weight"], [1, 1, 1])
    assert not s["eval"].any() and s["eval_pdf"] == 0


def test_mask_known_answers(native, oracle):
    nested = native.BSDF("plastic")
    mask = native.Mask(nested, opacity=0.3)
    assert mask.record().type == 9 and mask.flags() == nested.flags() | NULL
    assert native.Mask(nested).record().params[0] == 0.5          # mask.cpp:70
    scene = _one_shape_scene(native, mask)
    wi = np.array([0.3, -0.2, 0.9], np.float32); wi /= np.linalg.norm(wi)
    through = _query(oracle, scene, wi, 0.3)                     # sample1 < opacity fails: the null lobe
    assert through["type"] == NULL and np.array_equal(through["wo"], -wi) and through["pdf"] == np.float32(1) - np.float32(0.3)
    assert np.array_equal(through["weight"], [1, 1, 1]) and through["eta"] == 1
    for s1 in (0.01, 0.2, 0.29):                                 # the nested sampler sees sample1 / opacity, its result is taken as it is
        got = _query(oracle, scene, wi, s1)
        want = nested.sample(wi, np.float32(s1) / np.float32(0.3), (0.3, 0.6))
        assert np.array_equal(got["wo"], want["wo"]) and got["pdf"] == want["pdf"] and got["type"] == want["sampled_type"]
        assert np.array_equal(got["weight"], want["weight"])
    wo = np.array([-0.1, 0.4, 0.9], np.float32); wo /= np.linalg.norm(wo)
    e, p = nested.eval_pdf(wi, wo)
    got = _query(oracle, scene, wi, 0.5, wo=wo)
    assert np.array_equal(got["eval"], e * np.float32(0.3)) and got["eval_pdf"] == p * np.float32(0.3)
    he, hp = mask.eval_pdf(wi, wo)
    assert np.array_equal(he, got["eval"]) and hp == got["eval_pdf"]


def test_host_helpers_refuse_bitmap_driven_wrappers(native):
    """BSDF.sample / eval / pdf of the host classes carry no texture coordinates: a bitmap opacity / weight is an error there, not the bitmap's index"""
    from mitsuba2_amd import scenes
    a, b = native.BSDF("diffuse"), native.BSDF("conductor")
    tex = lambda: native.BitmapTexture(scenes.cutout_weight(), filter_type="nearest", wrap_mode="clamp")
    for bsdf, what in ((native.Mask(a, opacity=tex()), "opacity of a mask"), (native.BlendBSDF(a, b, weight=tex()), "weight of a blendbsdf"),
                       (native.Mask(native.BlendBSDF(a, b, weight=tex()), opacity=0.5), "weight of a blendbsdf")):
        for call in (lambda: bsdf.sample([0, 0, 1], 0.5, (0.3, 0.6)), lambda: bsdf.eval_pdf([0, 0, 1], [0, 0, 1])):
            with pytest.raises(RuntimeError, match=what):
                call()


def test_record_table_of_the_longest_chain(native):
    plastic, mirror = native.BSDF("plastic"), native.BSDF("conductor")
    chain = native.Mask(native.BlendBSDF(native.TwoSided(plastic), mirror, weight=0.6), opacity=0.7)
    scene = _one_shape_scene(native, chain)
    d = scene.desc().contents
    types = [d.bsdfs[i].type for i in range(d.bsdf_count)]
    assert types == [9, 10, 4, 3]                                # mask, blendbsdf, plastic (twosided, its own back side), conductor
    assert d.bsdfs[0].back == 1 and d.bsdfs[1].back == 2 and d.bsdfs[1].params[3] == 3.0
    assert d.bsdfs[2].flags & 0x100 and d.bsdfs[2].back == 2
    assert d.bsdfs[0].params[0] == np.float32(0.7) and d.bsdfs[1].params[0] == np.float32(0.6)
    assert d.shapes[0].bsdf == 0


def test_twosided_blend_is_rewritten_and_other_nesting_is_refused(native):
    a, b = native.BSDF("diffuse", reflectance=(0.2, 0.3, 0.4)), native.BSDF("roughconductor", alpha=0.3)
    ts = native.TwoSided(native.BlendBSDF(a, b, weight=0.4))
    scene = _one_shape_scene(native, ts)
    d = scene.desc().contents
    assert [d.bsdfs[i].type for i in range(d.bsdf_count)] == [10, 0, 2]
    assert all(d.bsdfs[i].flags & 0x100 and d.bsdfs[i].back == i for i in (1, 2)) and not d.bsdfs[0].flags & 0x100
    # mirroring commutes with the selection and with the weighted sums: the rewritten record answers for the back side like the front
    wi, wo = np.float32([0.3, 0.2, 0.93]), np.float32([-0.4, 0.1, 0.91])
    flip = np.float32([1, 1, -1])
    e0, p0 = ts.eval_pdf(wi, wo); e1, p1 = ts.eval_pdf(wi * flip, wo * flip)
    assert np.array_equal(e0, e1) and p0 == p1 and p0 > 0
    s0, s1 = ts.sample(wi, 0.7, (0.2, 0.9)), ts.sample(wi * flip, 0.7, (0.2, 0.9))
    assert np.array_equal(s0["wo"], s1["wo"] * flip) and s0["pdf"] == s1["pdf"] and np.array_equal(s0["weight"], s1["weight"])
    with pytest.raises(RuntimeError, match="twosided"):
        native.TwoSided(native.Mask(a, opacity=0.5))
    with pytest.raises(RuntimeError, match="transmission component"):
        native.TwoSided(native.BSDF("thindielectric"))
    with pytest.raises(RuntimeError, match="transmission component"):
        native.TwoSided(native.BSDF("null"))
    with pytest.raises(RuntimeError, match="nested in a blendbsdf"):
        native.BlendBSDF(native.BlendBSDF(a, b, weight=0.5), a, weight=0.5)
    with pytest.raises(RuntimeError, match="nested in a blendbsdf"):
        native.BlendBSDF(native.Mask(a), a, weight=0.5)
    with pytest.raises(RuntimeError, match="BlendBSDF: Two child BSDFs must be specified!"):
        native.BlendBSDF(a, weight=0.5)
    with pytest.raises(RuntimeError, match="Cannot specify more than two child BSDFs"):
        native.BlendBSDF(a, b, a, weight=0.5)
    with pytest.raises(RuntimeError, match="weight"):
        native.BlendBSDF(a, b)


XML = """<scene version="2.0.0">
  <sensor type="perspective"><float name="fov" value="45"/>
    <transform name="to_world"><lookat origin="0, -3, 2" target="0, 0, 0" up="0, 0, 1"/></transform>
    <film type="hdrfilm"><integer name="width" value="24"/><integer name="height" value="16"/></film>
    <sampler type="independent"><integer name="sample_count" value="3"/></sampler></sensor>
  <bsdf type="diffuse" id="paint"><rgb name="reflectance" value="0.7, 0.2, 0.2"/></bsdf>
  <shape type="rectangle"><bsdf type="mask"><float name="opacity" value="0.4"/>
    <bsdf type="blendbsdf"><spectrum name="weight" value="0.3"/><ref id="paint"/><bsdf type="conductor"/></bsdf></bsdf></shape>
  <shape type="rectangle"><transform name="to_world"><translate x="0" y="0" z="0.5"/></transform><bsdf type="thindielectric"><string name="int_ior" value="water"/></bsdf></shape>
  <shape type="rectangle"><transform name="to_world"><translate x="0" y="0" z="0.8"/></transform><bsdf type="null"/></shape>
  %s
  <shape type="sphere"><point name="center" x="0" y="0" z="1.5"/><float name="radius" value="0.3"/>
    <emitter type="area"><rgb name="radiance" value="30, 30, 30"/></emitter></shape>
</scene>"""


def test_xml_round_trip_and_error_texts(native, oracle):
    scene, sensor, integ = native.load_string(XML % "")
    scene.build(-1)
    d = scene.desc().contents
    types = [d.bsdfs[i].type for i in range(d.bsdf_count)]
    assert types[:6] == [9, 10, 0, 3, 7, 8]
    assert d.bsdfs[0].params[0] == np.float32(0.4) and d.bsdfs[1].params[0] == np.float32(0.3) and d.bsdfs[1].back == 2 and d.bsdfs[1].params[3] == 3.0
    assert d.bsdfs[4].params[0] == np.float32(1.3330) / np.float32(1.000277)
    job = integ.render_job(sensor)
    o32, _, st = oracle.render(scene.desc(), job, threads=2)
    job.cfg.plan = 2
    e64, e32, est = oracle.emu_render(scene.desc(), job)
    assert np.array_equal(e32, o32) and est[1] == st.segments and o32[..., 1].max() > 0
    one = '<shape type="rectangle"><bsdf type="blendbsdf"><float name="weight" value="0.5"/><ref id="paint"/></bsdf></shape>'
    with pytest.raises(RuntimeError, match="BlendBSDF: Two child BSDFs must be specified!"):
        native.load_string(XML % one)
    three = '<shape type="rectangle"><bsdf type="blendbsdf"><float name="weight" value="0.5"/><ref id="paint"/><ref id="paint"/><bsdf type="null"/></bsdf></shape>'
    with pytest.raises(RuntimeError, match="Cannot specify more than two child BSDFs"):
        native.load_string(XML % three)


def test_emulator_equals_checker_on_the_cutout_box(native, oracle):
    from mitsuba2_amd import scenes
    scene, sensor = scenes.cutout_box(48, 40, 6, device=-1)
    d = scene.desc().contents
    assert {d.bsdfs[i].type for i in range(d.bsdf_count)} >= {7, 8, 9, 10} and d.bitmap_count == 2
    # (behind the null rectangle the direct integrator's one bounce is the Null lobe: its wrappers are looked at without the proxy as well)
    for integ, proxy in ((native.PathIntegrator(), True), (native.DirectIntegrator(emitter_samples=2, bsdf_samples=2), True),
                         (native.DirectIntegrator(emitter_samples=2, bsdf_samples=2), False)):
        if not proxy:
            scene, sensor = scenes.cutout_box(48, 40, 6, device=-1, proxy=False)
        job = integ.render_job(sensor)
        o32, _, st = oracle.render(scene.desc(), job, threads=4)
        job.cfg.plan = 2
        e64, e32, est = oracle.emu_render(scene.desc(), job)
        assert est[1] == st.segments and np.array_equal(e32, o32)
        assert np.isfinite(o32).all() and o32[..., 1].max() > 0
        if job.cfg.integrator == 0 or not proxy:
            plain, _ = scenes.cutout_box(48, 40, 6, device=-1, wrappers=False, proxy=proxy)
            p32, _, _ = oracle.render(plain.desc(), integ.render_job(sensor), threads=4)
            assert not np.array_equal(p32, o32)                  # the wrappers are seen


def test_furnace_reflectance_one_children_lose_no_energy(native, oracle):
    """White children under mask, blendbsdf and thindielectric: E[weight] of BSDF::sample is 1 in every channel (the null lobe
    and both children carry weight 1; the cosine-sampled diffuse lobe has weight = reflectance)."""
    white = native.BSDF("diffuse", reflectance=(1, 1, 1))
    rng = np.random.default_rng(5)
    n = 20000
    for bsdf in (native.Mask(white, opacity=0.35), native.BlendBSDF(white, native.TwoSided(white), weight=0.6),
                 native.Mask(native.BlendBSDF(white, white, weight=0.25), opacity=0.8), native.BSDF("thindielectric")):
        scene = _one_shape_scene(native, bsdf)
        q = np.zeros((n, 10), np.float32); q[:, 1:4] = np.float32([0.3, 0.2, 0.93]); q[:, 4:7] = rng.random((n, 3)); q[:, 7:10] = (0, 0, 1)
        out = oracle.eval(3, q, scene.desc())
        assert np.array_equal(out[:, 6:9], np.ones((n, 3), np.float32))


def _close(a, b, rtol, atol=1e-7):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= atol + rtol * np.maximum(np.abs(a), np.abs(b)))


# what test_independent_leaves.py asks of the wrapped leaves: (eval / pdf rtol, atol), (sampled density rtol, atol), (weight rtol, atol);
# the sampled direction 3e-6 absolute for all of them
TOL_DIFFUSE = ((2e-6, 1e-7), (1e-5, 2e-6), (1e-6, 1e-7))          # :98-103
TOL_PLASTIC = ((3e-5, 1e-8), (3e-5, 2e-6), (1e-4, 1e-7))          # :327-343
TOL_DIELECTRIC = ((0, 0), (2e-5, 1e-7), (2e-6, 1e-7))             # :87 (eval = pdf = 0 exactly)
# cosine hemisphere: z = sqrt(1 - x^2 - y^2), and the argument carries three float32 roundings of numbers <= 1, so z is off by up to
# 3 * 2^-24 / (2 z): below this height the 3e-6 bound on the direction is not a statement about the code. Such samples go to the
# Margin, and count as excluded.
B_HORIZON = 3 * 2.0 ** -24 / (2 * 3e-6)


def test_float64_restatement_of_the_four_plugins(native, oracle):
    """4096 random inputs per record against tests/f64_nested_bsdfs.py under the tolerances test_independent_leaves.py uses for the
    wrapped leaves (TOL_* above; a wrapper adds at most four float32 roundings, 2.4e-7 relative, to its leaf). Inputs within B_LOBE
    of a discrete decision, on the concentric map's seam, at grazing incidence or sampled within B_HORIZON of the horizon are left
    out, and counted. The last case is twosided(blendbsdf(a, b)) as the host layer rewrites it, against the form as written:
    F.TwoSided(N.BlendBSDF(a, b)) with distinguishable children and a weight other than one half, wi on both sides.
    Measured: largest deviation 1.78e-6 (absolute, directions) / 5.4e-5 (relative, over values above 1e-6: inside its absolute
    bound); excluded share 0.31 %."""
    import f64_integrators as F
    import f64_nested_bsdfs as N
    refl, refl2 = (0.2, 0.7, 0.3), (0.7, 0.25, 0.1)
    tint_r, tint_t = (0.5, 0.6, 0.7), (0.9, 0.8, 0.7)
    d, d2 = native.BSDF("diffuse", reflectance=refl), native.BSDF("diffuse", reflectance=refl2)
    pl = lambda: native.BSDF("plastic", diffuse_reflectance=refl)
    cases = [
        (native.BSDF("null"), N.Null(), TOL_DIELECTRIC),
        (native.BSDF("thindielectric", specular_reflectance=tint_r, specular_transmittance=tint_t),
         N.ThinDielectric(specular_reflectance=tint_r, specular_transmittance=tint_t), TOL_DIELECTRIC),
        (native.Mask(native.TwoSided(d), opacity=0.3), N.Mask(F.TwoSided(F.Diffuse(refl)), 0.3), TOL_DIFFUSE),
        (native.BlendBSDF(d, d2, weight=0.3), N.BlendBSDF(F.Diffuse(refl), F.Diffuse(refl2), 0.3), TOL_DIFFUSE),
        (native.Mask(native.BlendBSDF(pl(), d2, weight=0.6), opacity=0.7),
         N.Mask(N.BlendBSDF(F.Plastic(diffuse_reflectance=refl), F.Diffuse(refl2), 0.6), 0.7), TOL_PLASTIC),
        (native.TwoSided(native.BlendBSDF(d, d2, weight=0.3)), F.TwoSided(N.BlendBSDF(F.Diffuse(refl), F.Diffuse(refl2), 0.3)), TOL_DIFFUSE),
        (native.TwoSided(native.BlendBSDF(pl(), d2, weight=0.7)), F.TwoSided(N.BlendBSDF(F.Plastic(diffuse_reflectance=refl), F.Diffuse(refl2), 0.7)), TOL_PLASTIC),
    ]
    rng = np.random.default_rng(23)
    n = 4096
    worst_abs = worst_rel = 0.0
    excluded = total = 0
    for bsdf, ref, ((e_r, e_a), (p_r, p_a), (w_r, w_a)) in cases:
        scene = _one_shape_scene(native, bsdf)
        q = np.zeros((n, 10), np.float32)
        for c0 in (1, 7):
            w = rng.normal(size=(n, 3)); w /= np.linalg.norm(w, axis=1, keepdims=True)
            q[:, c0:c0 + 3] = w
        q[:, 4:7] = rng.random((n, 3))
        out = oracle.eval(3, q, scene.desc())
        for xi, o in zip(q.astype(np.float64), out):
            total += 1
            wi, s1, u2, wo = xi[1:4], xi[4], xi[5:7], xi[7:10]
            M = F.Margin()
            s_wo, s_pdf, s_eta, s_delta, s_w = ref.sample(wi, s1, u2, M)
            ev, pd = ref.eval(wi, wo, M), ref.pdf(wi, wo, M)
            if not s_delta and s_pdf != 0:
                M.add(s_wo[2], B_HORIZON, "sampled direction at the horizon")
            if M.value < 1:
                excluded += 1
                continue
            what = (type(ref).__name__, wi, wo, s1, u2, o, ev, pd, s_wo, s_pdf, s_w)
            assert _close(o[9:12], ev, e_r, e_a) and _close(o[12], pd, e_r, e_a), what
            assert _close(o[0:3], s_wo, 0, 3e-6) and _close(o[3], s_pdf, p_r, p_a) and o[4] == s_eta, what
            assert _close(o[6:9], s_w, w_r, w_a), what
            worst_abs = max(worst_abs, np.abs(o[0:3] - s_wo).max())
            for a, b in ((o[9:12], ev), (o[12:13], [pd]), (o[3:4], [s_pdf]), (o[6:9], s_w)):
                a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
                nz = np.abs(b) > 1e-6
                if nz.any():
                    worst_rel = max(worst_rel, (np.abs(a - b)[nz] / np.abs(b)[nz]).max())
    print("f64 restatement: largest deviation %.3g (absolute, directions) / %.3g (relative, values); excluded share %.2f %%"
          % (worst_abs, worst_rel, 100.0 * excluded / total))
    assert excluded <= F.MAX_EXCLUDED * total, (excluded, total)


# ---------------------------------------------------------------- the integrators over the wrappers, against the float64 restatement
NESTED_JOBS = {   # name -> (integrator, its arguments, the null rectangle in front of the camera)
    "cutout-path": ("path", dict(), True),
    "cutout-direct-2-2": ("direct", dict(emitter_samples=2, bsdf_samples=2), True),
    # behind the null rectangle the direct integrator's one bounce is the Null lobe; without it its first hit is a wrapper
    "cutout-direct-2-2-open": ("direct", dict(emitter_samples=2, bsdf_samples=2), False),
}
NESTED_SPP, NESTED_SEED = 2, 50000


def _nested_job_scene(spp, proxy):
    """scenes.cutout_box at 64 x 48 with the box filter, the light hung f64_integrators.LIGHT_DROP lower (job_scene there says why:
    shadow rays leaving the ceiling at a grazing angle; the jobs move, not the cap on exclusions)"""
    import f64_integrators as F
    from mitsuba2_amd import api, scenes
    meshes = scenes.cutout_box_meshes(proxy=proxy)
    for i, m in enumerate(meshes):
        if m.name == "light":
            meshes[i] = api.Mesh("light", m.vertices - np.array([0, F.LIGHT_DROP, 0], np.float32), m.faces, emitter=api.AreaLight(scenes.LIGHT_RADIANCE))
    return api.Scene(meshes).build(-1), scenes.cornell_sensor(F.JOB_W, F.JOB_H, spp, seed=NESTED_SEED, rfilter="box")


@pytest.mark.parametrize("name", list(NESTED_JOBS))
def test_integrators_over_the_wrappers_against_float64_restatement(native, oracle, name):
    """SamplingIntegrator::sample of path / direct on scenes.cutout_box, 64 x 48 at 2 spp, by the method of
    test_independent_integrators.py: sample k of every pixel is the checker's float64 film of spp = k + 1 minus that of spp = k,
    compared with f64_integrators.path_sample / direct_sample over f64_nested_bsdfs.Scene under that file's RTOL and
    f64_integrators.MAX_EXCLUDED. Measured (largest deviation, excluded share): cutout-path 2.06e-4, 2.20 %;
    cutout-direct-2-2 0, 0.10 %; cutout-direct-2-2-open 1.94e-4, 1.16 %."""
    import f64_integrators as F
    import f64_nested_bsdfs as N
    import sample_harness as H
    from test_independent_integrators import RTOL, report
    kind, kw, proxy = NESTED_JOBS[name]
    make = lambda: (native.PathIntegrator if kind == "path" else native.DirectIntegrator)(**kw)
    films = [np.zeros((F.JOB_H, F.JOB_W, 5))]
    for spp in range(1, NESTED_SPP + 1):
        scene, sensor = _nested_job_scene(spp, proxy)
        _, f64, _ = oracle.render(scene.desc(), make().render_job(sensor), threads=4, want_f64=True)
        assert H.every_sample_in_its_texel(f64, spp), "job %s: a sample left its texel, pick another base seed" % name
        films.append(f64)
    want = np.stack([films[k + 1] - films[k] for k in range(NESTED_SPP)])
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    job = make().render_job(sensor)
    res = F.restate_job(H, oracle, N.Scene(scene.shapes), job, F.integrator_fn(kind, kw), NESTED_SPP)
    ty, tx = res["py"] - job.cfg.crop_y, res["px"] - job.cfg.crop_x
    checked_all, bad_all, dev_all = [], [], 0.0
    for j in range(NESTED_SPP):
        got = want[j][ty, tx]
        checked, bad, dev = F.compare(got[:, :3], got[:, 3] != 0, res, j, RTOL, to_xyz=True)
        checked_all.append(checked); bad_all.append(bad); dev_all = max(dev_all, dev)
    checked, bad = np.stack(checked_all), np.stack(bad_all)
    msg = report(name, res, checked, dev_all)
    print(msg)
    assert checked.mean() >= 1 - F.MAX_EXCLUDED, msg
    assert res["stats"]["hit"] > 1000, msg
    if bad.any():
        j, i = np.argwhere(bad)[0]
        got = want[j][ty[i], tx[i]]
        pytest.fail("%s\n%d samples differ; first: sample %d pixel (%d, %d): checker XYZ %s valid %s, restatement %s valid %s, margin %.3g (%s), draws %d"
                    % (msg, bad.sum(), j, res["px"][i], res["py"][i], got[:3], got[3], res["L"][j, i] @ F.SRGB_TO_XYZ.T, res["valid"][j, i],
                       res["margin"][j, i], res["what"][j][i], res["n_draws"][j, i]))
