"""Independent restatements of the float leaves the oracle SHARES with the product.

oracle/miw_oracle.cpp has its own control flow (path loop, scene queries, splat, spiral) but includes the product's leaf
headers (csrc/miw/{bsdf,scene,shape,warp,...}.h): a transcription slip inside one of them would pass every device-vs-oracle
test by construction. This file closes that gap for the leaves that carry the arithmetic of BASELINE configs 2 - 4: each
function below is written a SECOND time, in float64 numpy, straight from the reference source it cites — sharing no code with
csrc/ — and compared with what the oracle's leaf entry points return for random inputs. Float64 against the float32 of the
headers: agreement to ~1e-5 relative wherever the function is well-conditioned (the tolerance of each check is next to it;
samples that sit on a branch boundary of the float32 evaluation — lobe choice, quadrant choice, CDF bin — are excluded by an
explicit margin, never by the comparison's outcome).
"""
import math

import numpy as np
import pytest

from f64_integrators import (PI, Microfacet, cosine_hemisphere, dielectric_sample, disk_concentric, fresnel, fresnel_conductor,  # noqa: F401
                             fresnel_diffuse_reflectance, hier2d_build, hier2d_sample, roughconductor, roughdielectric)


def _bsdf_inputs(rng, n, upper=True):
    wi = rng.normal(size=(n, 3)); wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo = rng.normal(size=(n, 3)); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    if upper:
        wi[:, 2] = np.abs(wi[:, 2]); wo[:, 2] = np.abs(wo[:, 2])
    x = np.zeros((n, 10), np.float32)
    x[:, 1:4] = wi; x[:, 4:7] = rng.random((n, 3)); x[:, 7:10] = wo
    return x


def _one_bsdf_scene(native, bsdf):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return native.Scene([native.Mesh("t", v, np.array([[0, 1, 2]], np.uint32), bsdf=bsdf)]).build(-1)


def _close(a, b, rtol, atol=1e-7):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= atol + rtol * np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("kw", [
    dict(distribution="ggx", alpha=0.1),                                   # BASELINE config 3's metal
    dict(distribution="ggx", alpha=0.35, sample_visible=False),
    dict(distribution="ggx", alpha_u=0.4, alpha_v=0.12),
    dict(distribution="ggx", alpha_u=0.15, alpha_v=0.3, sample_visible=False),
    dict(distribution="beckmann", alpha=0.3, sample_visible=False),
    dict(distribution="beckmann", alpha_u=0.2, alpha_v=0.45, sample_visible=False),
])
def test_roughconductor_against_float64_restatement(native, oracle, kw):
    """sample / eval / pdf of roughconductor.cpp + microfacet.h + fresnel_conductor, every distribution branch the configs
    can reach except Beckmann's visible-normal inversion (Newton iterations on erf: pinned by the reference's own sample table,
    test_oracle_kat.py, and by chi-square)."""
    eta, k = np.array([0.2, 0.92, 1.1]), np.array([3.9, 2.45, 2.14])
    scene = _one_bsdf_scene(native, native.BSDF("roughconductor", eta=tuple(eta), k=tuple(k), **kw))
    x = _bsdf_inputs(np.random.default_rng(11), 600)
    up = np.array([[0.3, 0.2, 0.93]]) / np.linalg.norm([0.3, 0.2, 0.93])
    x[:, 1:4] = np.where(x[:, 3:4] < 0.05, up.astype(np.float32), x[:, 1:4])                       # keep wi off the horizon
    out = oracle.eval(3, x, scene.desc())
    au, av = kw.get("alpha_u", kw.get("alpha")), kw.get("alpha_v", kw.get("alpha"))
    d = Microfacet(kw["distribution"], au, av, kw.get("sample_visible", True))
    checked = 0
    for xi, o in zip(x.astype(np.float64), out):
        wi, u2, wo = xi[1:4], xi[5:7], xi[7:10]
        if min(u2[0], 1 - u2[0], abs(abs(2 * u2[0] - 1) - abs(2 * u2[1] - 1))) < 1e-3 or abs(abs(u2[1] - 0.5) - 0.25) < 1e-3:
            continue                                             # the concentric map's quadrant seam / tan()'s poles
        (s_wo, s_pdf, s_w), ev, pd = roughconductor(d, eta, k, wi, u2, wo)
        assert _close(o[9:12], ev, 2e-4, 1e-6) and _close(o[12], pd, 2e-4, 1e-6), (kw, wi, wo, o[9:13], ev, pd)
        if s_pdf > 1e-3 and s_wo[2] > 1e-3:                      # well-conditioned samples: direction, density, weight
            assert _close(o[0:3], s_wo, 0, 2e-4) and _close(o[3], s_pdf, 1e-3) and _close(o[6:9], s_w, 5e-4, 1e-6), (kw, wi, u2, o[:9], s_wo, s_pdf, s_w)
            assert o[4] == 1.0
            checked += 1
    assert checked > 300


def test_dielectric_and_diffuse_against_float64_restatement(native, oracle):
    """dielectric.cpp:201-310 with fresnel.h:34-70 / :275-294 (config 3's bk7 glass, from both sides) and diffuse.cpp:78-135."""
    eta = 1.5046 / 1.000277
    scene = _one_bsdf_scene(native, native.BSDF("dielectric", int_ior=1.5046, ext_ior=1.000277))
    x = _bsdf_inputs(np.random.default_rng(3), 800, upper=False)
    out = oracle.eval(3, x, scene.desc())
    n_t = 0
    for xi, o in zip(x.astype(np.float64), out):
        wi = xi[1:4]
        wo, pdf, bs_eta, w, r = dielectric_sample(eta, wi, xi[4])
        if abs(xi[4] - r) < 1e-4:
            continue                                             # lobe choice on the float32 knife edge
        assert _close(o[0:3], wo, 0, 3e-6) and _close(o[3], pdf, 2e-5) and _close(o[4], bs_eta, 2e-6) and _close(o[6:9], [w] * 3, 2e-6), (wi, xi[4], o[:9])
        assert not o[9:13].any()                                 # eval = pdf = 0 (delta lobes), dielectric.cpp:312-320
        n_t += bs_eta != 1.0
    assert n_t > 200
    refl = np.array([0.63, 0.065, 0.05])
    scene = _one_bsdf_scene(native, native.BSDF("diffuse", reflectance=tuple(refl)))
    x = _bsdf_inputs(np.random.default_rng(4), 600, upper=False)
    out = oracle.eval(3, x, scene.desc())
    for xi, o in zip(x.astype(np.float64), out):
        wi, wo = xi[1:4], xi[7:10]
        both = wi[2] > 0 and wo[2] > 0
        assert _close(o[9:12], refl / PI * wo[2] if both else np.zeros(3), 2e-6)          # eval, :104-119
        assert _close(o[12], wo[2] / PI if both else 0.0, 2e-6)                           # pdf, :121-135
        u2 = xi[5:7]
        if wi[2] > 0 and abs(abs(2 * u2[0] - 1) - abs(2 * u2[1] - 1)) > 1e-3:
            s = cosine_hemisphere(u2)
            assert _close(o[0:3], s, 0, 3e-6) and _close(o[3], s[2] / PI, 1e-5, 2e-6) and _close(o[6:9], refl, 1e-6)   # sample, :78-102 (z = sqrt(1 - r^2) cancels near the horizon)


def test_area_light_sampling_against_float64_restatement(native, oracle):
    """Scene::sample_emitter_direction (scene.cpp:164-200, one emitter) -> AreaLight::sample_direction (area.cpp:121-166)
    -> Shape::sample_direction (shape.cpp:292-309) -> Mesh::sample_position (mesh.cpp:352-397: face by area through
    DiscreteDistribution::sample_reuse, distr_1d.h:193-203, then square_to_uniform_triangle, warp.h:153-156), and
    pdf_direction (area.cpp:168-187, shape.cpp:311-323) on a three-face emitter with unequal areas."""
    v = np.array([[0, 2, 0], [1, 2, 0], [1, 2, 1], [0, 2, 1], [3, 2, 0.5], [0.5, 2, 3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [2, 4, 5]], np.uint32)          # normals point down (-y)
    radiance = (17.0, 12.0, 4.0)
    light = native.Mesh("light", v, f, emitter=native.AreaLight(radiance))
    floor = native.Mesh("floor", np.array([[-5, 0, -5], [5, 0, -5], [5, 0, 5], [-5, 0, 5]], np.float32),
                        np.array([[0, 2, 1], [0, 3, 2]], np.uint32), bsdf=native.BSDF("diffuse", reflectance=(0.5, 0.5, 0.5)))
    scene = native.Scene([floor, light]).build(-1)
    rng = np.random.default_rng(8)
    n = 500
    ref = np.concatenate([rng.uniform(-3, 3, (n, 1)), rng.uniform(-1, 3.5, (n, 1)), rng.uniform(-3, 3, (n, 1)), rng.random((n, 2))], 1).astype(np.float32)
    out = oracle.eval(6, ref, scene.desc())
    P = v.astype(np.float64)
    areas = np.array([0.5 * np.linalg.norm(np.cross(P[b] - P[a], P[c] - P[a])) for a, b, c in f])
    cdf = np.cumsum(areas) / areas.sum()
    checked = 0
    for r, o in zip(ref.astype(np.float64), out):
        p_ref, u = r[0:3], r[3:5]
        face = int(np.searchsorted(cdf, u[1], side="left")) if u[1] > 0 else 0          # first index with cdf >= value
        face = min(face, 2)
        lo = cdf[face - 1] if face else 0.0
        if min(abs(u[1] - cdf[face]), abs(u[1] - lo)) < 1e-5:
            continue                                              # CDF bin edge
        u1 = (u[1] - lo) / (areas[face] / areas.sum())            # sample_reuse
        t = math.sqrt(max(0.0, 1 - u[0]))
        b = (1 - t, t * u1)                                       # square_to_uniform_triangle
        a_, b_, c_ = f[face]
        p = P[a_] + (P[b_] - P[a_]) * b[0] + (P[c_] - P[a_]) * b[1]
        nrm = np.cross(P[b_] - P[a_], P[c_] - P[a_]); nrm /= np.linalg.norm(nrm)
        d = p - p_ref
        dist2 = d @ d
        dist = math.sqrt(dist2)
        d /= dist
        dp = abs(d @ nrm)
        pdf = (1 / areas.sum()) * (dist2 / dp if dp != 0 else 0.0)
        active = d @ nrm < 0 and pdf != 0
        if dp < 1e-3:
            continue                                              # grazing: pdf ill-conditioned
        assert _close(o[0:3], d, 0, 3e-6) and _close(o[3], dist, 3e-6) and _close(o[4], pdf, 1e-4) and _close(o[5:8], p, 0, 3e-6) and _close(o[8:11], nrm, 0, 1e-6), (r, o)
        assert _close(o[11:14], np.array(radiance) / pdf if active else np.zeros(3), 1e-4, 1e-9)
        checked += 1
    assert checked > 400


def test_surface_interaction_against_float64_restatement(native, oracle):
    """Mesh::compute_surface_interaction (mesh.cpp:449-545) with vertex normals and texture coordinates (position from the
    barycentrics, dp_du from the uv Jacobian), the Gram-Schmidt shading frame of interaction.h:153-156 and wi = to_local(-d)
    (interaction.h:591), through the Scene::ray_intersect surface (mi_ray_intersect's checker). A second mesh without
    texture coordinates takes the other branch: dp_du from coordinate_system(n), vector.h:116-136."""
    rng = np.random.default_rng(21)
    v = np.array([[0, 0, 0], [2, 0, 0.3], [0.2, 1.5, 0.1], [2.1, 1.7, -0.2]], np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.uint32)
    nrm = np.array([[0.1, -0.1, 1], [0.3, 0.0, 1], [-0.2, 0.2, 1], [0.0, 0.3, 1]], np.float64)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = np.array([[0, 0], [1, 0.1], [0.1, 0.9], [1.2, 1.1]], np.float32)
    mesh = native.Mesh("m", v, f, normals=nrm.astype(np.float32), texcoords=uv, bsdf=native.BSDF("diffuse", reflectance=(0.5, 0.5, 0.5)))
    scene = native.Scene([mesh]).build(-1)
    n = 300
    o = np.concatenate([rng.uniform(0.2, 1.8, (n, 1)), rng.uniform(0.2, 1.3, (n, 1)), rng.uniform(1.0, 3.0, (n, 1))], 1).astype(np.float32)
    d = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), -np.ones((n, 1))], 1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    si = oracle.ray_intersect(scene.desc(), o, d, 1e-4, np.inf)
    P, N, UV = v.astype(np.float64), nrm.astype(np.float32).astype(np.float64), uv.astype(np.float64)
    checked = 0
    for i in range(n):
        if not np.isfinite(si["t"][i]):
            continue
        oo, dd = o[i].astype(np.float64), d[i].astype(np.float64)
        best = None
        for face, (a, b, c) in enumerate(f):                     # mesh.h:194-226
            e1, e2 = P[b] - P[a], P[c] - P[a]
            pv = np.cross(dd, e2)
            det = e1 @ pv
            tv = oo - P[a]
            uu = (tv @ pv) / det
            qv = np.cross(tv, e1)
            vv = (dd @ qv) / det
            t = (e2 @ qv) / det
            if uu >= 0 and vv >= 0 and uu + vv <= 1 and t >= 1e-4 and (best is None or t < best[0]):
                best = (t, uu, vv, face)
        assert best is not None
        t, b1, b2, face = best
        if min(b1, b2, 1 - b1 - b2) < 1e-4:
            continue                                              # on the shared edge: either face is a valid answer
        a, b, c = f[face]
        b0 = 1 - b1 - b2
        p = P[a] * b0 + P[b] * b1 + P[c] * b2
        dp0, dp1 = P[b] - P[a], P[c] - P[a]
        ng = np.cross(dp0, dp1); ng /= np.linalg.norm(ng)
        tex = UV[a] * b0 + UV[b] * b1 + UV[c] * b2
        ns = N[a] * b0 + N[b] * b1 + N[c] * b2; ns /= np.linalg.norm(ns)
        duv0, duv1 = UV[b] - UV[a], UV[c] - UV[a]                # dp_du from the texture coordinates, mesh.cpp:498-510
        det = duv0[0] * duv1[1] - duv0[1] * duv1[0]
        assert det != 0
        dp_du = (duv1[1] * dp0 - duv0[1] * dp1) / det
        s_ = dp_du - ns * (ns @ dp_du); s_ /= np.linalg.norm(s_)  # initialize_sh_frame, interaction.h:153-156
        t_ = np.cross(ns, s_)
        wi = np.array([-dd @ s_, -dd @ t_, -dd @ ns])
        assert face == si["prim_index"][i] and si["shape_index"][i] == 0
        assert _close(si["t"][i], t, 2e-6) and _close(si["p"][i], p, 0, 2e-6) and _close(si["n"][i], ng, 0, 1e-6)
        assert _close(si["uv"][i], tex, 0, 1e-6) and _close(si["sh_n"][i], ns, 0, 1e-6)
        assert _close(si["sh_s"][i], s_, 0, 2e-6) and _close(si["sh_t"][i], t_, 0, 2e-6) and _close(si["wi"][i], wi, 0, 3e-6)
        checked += 1
    assert checked > 200

    # no texture coordinates, no vertex normals: uv = barycentrics, frame from coordinate_system(face normal)
    scene = native.Scene([native.Mesh("m", v, f, bsdf=native.BSDF("diffuse", reflectance=(0.5, 0.5, 0.5)))]).build(-1)
    si = oracle.ray_intersect(scene.desc(), o, d, 1e-4, np.inf)
    checked = 0
    for i in range(n):
        if not np.isfinite(si["t"][i]):
            continue
        a, b, c = f[si["prim_index"][i]]
        ng = np.cross(P[b] - P[a], P[c] - P[a]); ng /= np.linalg.norm(ng)
        sgn = math.copysign(1.0, ng[2])                           # vector.h:116-136
        aa = -1 / (sgn + ng[2]); bb = ng[0] * ng[1] * aa
        ms = (lambda x, y: x if y >= 0 else -x)                  # enoki::mulsign: x times the sign of y
        dp_du = np.array([ms(ng[0] * ng[0] * aa, ng[2]) + 1, ms(bb, ng[2]), -ms(ng[0], ng[2])])
        s_ = dp_du - ng * (ng @ dp_du); s_ /= np.linalg.norm(s_)
        dd = d[i].astype(np.float64)
        assert _close(si["sh_n"][i], ng, 0, 1e-6) and _close(si["sh_s"][i], s_, 0, 2e-6) and _close(si["sh_t"][i], np.cross(ng, s_), 0, 2e-6)
        assert _close(si["wi"][i], [-dd @ s_, -dd @ np.cross(ng, s_), -dd @ ng], 0, 3e-6)
        bary = si["uv"][i].astype(np.float64)
        assert _close(si["p"][i], P[a] * (1 - bary.sum()) + P[b] * bary[0] + P[c] * bary[1], 0, 2e-6)
        checked += 1
    assert checked > 200


def test_environment_map_against_float64_restatement(native, oracle):
    """EnvironmentMapEmitter (envmap.cpp): eval (:134-147, lat-long coordinates + the bilinear lookup of eval_spectrum
    :269-320), pdf_direction (:192-208) with the density Hierarchical2D normalises in its constructor (distr_2d.h:372-440:
    patch averages of luminance * sin(theta), summed in double) and sample_direction (:157-190) — whose warp is checked here
    through what it must satisfy: the direction it returns carries exactly the density pdf_direction assigns to it, the value
    is eval / pdf, the point lies two bounding-sphere radii away (set_scene, :127-131). The warp's own mapping is pinned by
    the reference's spot values and a chi-square test (tests/test_oracle_kat.py)."""
    from mitsuba2_amd import scenes
    Wd, Hd = 48, 24
    img = scenes.sky_envmap(Wd, Hd).astype(np.float64)
    scale = 1.7
    org, tgt, up = np.array([0.0, 0, 0]), np.array([0.3, 0.1, 1.0]), np.array([0.0, 1, 0])
    fwd = (tgt - org) / np.linalg.norm(tgt - org)                                  # Transform::look_at, transform.h:241-258
    left = np.cross(up, fwd); left /= np.linalg.norm(left)
    R = np.stack([left, np.cross(fwd, left), fwd], 1)                              # columns: to_world's rotation
    env = native.EnvMap(img.astype(np.float32), scale=scale, to_world=dict(origin=tuple(org), target=tuple(tgt), up=tuple(up)))
    v = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2], [0, 3, 0]], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2], [0, 1, 4]], np.uint32)
    scene = native.Scene([native.Mesh("m", v, f, bsdf=native.BSDF("diffuse", reflectance=(0.5, 0.5, 0.5)))], envmap=env).build(-1)
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    eps = 2.0 ** -24 * 1500
    radius = max(eps, np.linalg.norm(0.5 * (lo + hi) - hi) * (1 + eps))             # bbox.h:329-332, envmap.cpp:127-131

    lum = img[..., 0] * 0.212671 + img[..., 1] * 0.715160 + img[..., 2] * 0.072169    # mitsuba::luminance, spectrum.h
    lum = lum.astype(np.float32).astype(np.float64)
    sin_t = np.sin(np.arange(Hd) / (Hd - 1) * PI)
    dens = lum * sin_t[:, None]
    avg = 0.25 * (dens[:-1, :-1] + dens[:-1, 1:] + dens[1:, :-1] + dens[1:, 1:])
    dens = dens * ((Wd - 1) * (Hd - 1) / avg.sum())

    def bilinear(table, uv):
        x, y = uv[0] * (Wd - 1), uv[1] * (Hd - 1)
        px, py = min(int(x), Wd - 2), min(int(y), Hd - 2)
        w1x, w1y = x - px, y - py
        return ((1 - w1y) * ((1 - w1x) * table[py, px] + w1x * table[py, px + 1]) +
                w1y * ((1 - w1x) * table[py + 1, px] + w1x * table[py + 1, px + 1]))

    def to_uv(d_world):
        dl = R.T @ d_world
        uv = np.array([math.atan2(dl[0], -dl[2]) / (2 * PI), math.acos(max(-1.0, min(1.0, dl[1]))) / PI])
        return uv - np.floor(uv), dl

    rng = np.random.default_rng(31)
    n = 400
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.concatenate([d, rng.uniform(-1, 1, (n, 3)), rng.random((n, 2))], 1).astype(np.float32)
    out = oracle.eval(9, x, scene.desc())
    checked = 0
    for xi, o in zip(x.astype(np.float64), out.astype(np.float64)):
        uv, dl = to_uv(xi[0:3])
        if min(uv[0], 1 - uv[0]) < 1e-3 or abs(dl[1]) > 0.999:
            continue                                              # the atan2 seam / the poles (inv_sin_theta ill-conditioned)
        inv_sin = 1 / math.sqrt(max(dl[0] ** 2 + dl[2] ** 2, (2.0 ** -24) ** 2))
        assert _close(o[0:3], bilinear(img, uv) * scale, 3e-4, 1e-5), (xi[:3], uv, o[:3])            # eval
        assert _close(o[3], bilinear(dens, uv) * inv_sin / (2 * PI * PI), 3e-4, 1e-7)                # pdf_direction
        sd, dist, pdf, spec = o[4:7], o[7], o[8], o[9:12]                                             # sample_direction
        assert abs(np.linalg.norm(sd) - 1) < 1e-5 and _close(dist, 2 * radius, 1e-6)
        suv, sdl = to_uv(sd / np.linalg.norm(sd))
        if min(suv[0], 1 - suv[0]) < 1e-3 or abs(sdl[1]) > 0.999 or pdf <= 0:
            continue
        s_inv_sin = 1 / math.sqrt(max(sdl[0] ** 2 + sdl[2] ** 2, (2.0 ** -24) ** 2))
        assert _close(pdf, bilinear(dens, suv) * s_inv_sin / (2 * PI * PI), 2e-3, 1e-7), (xi[6:8], suv, pdf)
        assert _close(spec * pdf, bilinear(img, suv) * scale, 2e-3, 1e-5)
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("nonlinear", [False, True])
def test_plastic_and_conductor_against_float64_restatement(native, oracle, nonlinear):
    """plastic.cpp:161-290 (lobe choice by the Fresnel-weighted sampling weights of parameters_changed, :161-176; the diffuse
    lobe's 1 / (1 - fdr_int * rho) with and without `nonlinear`) and the smooth conductor (conductor.cpp:216-262)."""
    rho = np.array([0.55, 0.3, 0.12])
    int_ior, ext_ior = 1.49, 1.000277
    eta = int_ior / ext_ior
    scene = _one_bsdf_scene(native, native.BSDF("plastic", diffuse_reflectance=tuple(rho), int_ior=int_ior, ext_ior=ext_ior, nonlinear=nonlinear))
    x = _bsdf_inputs(np.random.default_rng(13), 700, upper=False)
    out = oracle.eval(3, x, scene.desc())
    fdr_int = fresnel_diffuse_reflectance(1 / eta)
    ssw = 1.0 / (rho.mean() + 1.0)                               # specular sampling weight, s_mean = 1
    inv_eta_2 = 1 / (eta * eta)
    n_spec = n_diff = 0
    for xi, o in zip(x.astype(np.float64), out.astype(np.float64)):
        wi, s1, u2, wo = xi[1:4], xi[4], xi[5:7], xi[7:10]
        f_i = fresnel(wi[2], eta)[0]
        ps, pd_ = f_i * ssw, (1 - f_i) * (1 - ssw)
        ps = ps / (ps + pd_)
        diff = rho / (1 - (rho * fdr_int if nonlinear else fdr_int))
        if wi[2] > 0 and wo[2] > 0:
            f_o = fresnel(wo[2], eta)[0]
            assert _close(o[9:12], diff * wo[2] / PI * inv_eta_2 * (1 - f_i) * (1 - f_o), 3e-5, 1e-8)       # eval
            assert _close(o[12], wo[2] / PI * (1 - ps), 3e-5, 1e-8)                                            # pdf
        else:
            assert not o[9:13].any()
        if wi[2] <= 0:
            assert not o[6:9].any()
            continue
        if abs(s1 - ps) < 1e-4:
            continue
        if s1 < ps:
            assert _close(o[0:3], [-wi[0], -wi[1], wi[2]], 0, 1e-7) and _close(o[3], ps, 3e-5) and _close(o[6:9], [f_i / ps] * 3, 3e-5)
            n_spec += 1
        elif abs(abs(2 * u2[0] - 1) - abs(2 * u2[1] - 1)) > 1e-3:
            s = cosine_hemisphere(u2)
            f_o = fresnel(s[2], eta)[0]
            assert _close(o[0:3], s, 0, 3e-6) and _close(o[3], (1 - ps) * s[2] / PI, 3e-5, 2e-6)
            assert _close(o[6:9], diff * inv_eta_2 * (1 - f_i) * (1 - f_o) / (1 - ps), 1e-4, 1e-7)
            n_diff += 1
    assert n_spec > 10 and n_diff > 150
    if nonlinear:
        return
    eta_c, k_c = np.array([0.2, 0.92, 1.1]), np.array([3.9, 2.45, 2.14])
    scene = _one_bsdf_scene(native, native.BSDF("conductor", eta=tuple(eta_c), k=tuple(k_c)))
    x = _bsdf_inputs(np.random.default_rng(14), 300, upper=False)
    out = oracle.eval(3, x, scene.desc())
    for xi, o in zip(x.astype(np.float64), out.astype(np.float64)):
        wi = xi[1:4]
        assert not o[9:13].any()                                 # a delta lobe: eval = pdf = 0
        if wi[2] > 0:
            assert _close(o[0:3], [-wi[0], -wi[1], wi[2]], 0, 1e-7) and o[3] == 1.0 and o[4] == 1.0
            assert _close(o[6:9], fresnel_conductor(wi[2], eta_c, k_c), 3e-5)
        else:
            assert not o[6:9].any()


@pytest.mark.parametrize("kw", [
    dict(distribution="ggx", alpha=0.2),
    dict(distribution="ggx", alpha_u=0.1, alpha_v=0.35, sample_visible=False),
    dict(distribution="beckmann", alpha=0.3, sample_visible=False),
])
def test_roughdielectric_against_float64_restatement(native, oracle, kw):
    """roughdielectric.cpp: reflection and transmission lobes from both sides, the half-vector Jacobians, Walter's roughness
    scaling for plain sampling, the solid-angle compression factor (Beckmann's visible-normal inversion excepted, as above)."""
    int_ior, ext_ior = 1.5046, 1.000277
    eta = int_ior / ext_ior
    scene = _one_bsdf_scene(native, native.BSDF("roughdielectric", int_ior=int_ior, ext_ior=ext_ior, **kw))
    x = _bsdf_inputs(np.random.default_rng(23), 900, upper=False)
    x[np.abs(x[:, 3]) < 0.05, 3] = 0.3                           # keep wi off the horizon (pdfs blow up there)
    x[:, 1:4] /= np.linalg.norm(x[:, 1:4], axis=1, keepdims=True)
    out = oracle.eval(3, x, scene.desc())
    au, av = kw.get("alpha_u", kw.get("alpha")), kw.get("alpha_v", kw.get("alpha"))
    vis = kw.get("sample_visible", True)
    n_r = n_t = n_ev = 0
    for xi, o in zip(x.astype(np.float64), out.astype(np.float64)):
        wi, s1, u2, wo = xi[1:4], xi[4], xi[5:7], xi[7:10]
        if min(u2[0], 1 - u2[0], abs(abs(2 * u2[0] - 1) - abs(2 * u2[1] - 1))) < 1e-3 or abs(abs(u2[1] - 0.5) - 0.25) < 1e-3:
            continue
        smp, ev, pd = roughdielectric(kw["distribution"], au, av, vis, eta, wi, s1, u2, wo)
        if abs(wo[2]) > 0.02:
            assert _close(o[9], ev, 5e-4, 1e-6) and _close(o[12], pd, 5e-4, 1e-6), (kw, wi, wo, o[9:13], ev, pd)
            n_ev += ev > 0
        if smp is None:
            continue
        s_wo, s_pdf, s_eta, s_w, F = smp
        if abs(s1 - F) < 1e-3 or s_pdf < 1e-3 or abs(s_wo[2]) < 1e-2 or s_w == 0:
            continue
        assert _close(o[0:3], s_wo, 0, 3e-4) and _close(o[3], s_pdf, 2e-3) and _close(o[4], s_eta, 1e-6) and _close(o[6:9], [s_w] * 3, 1e-3, 1e-6), (kw, wi, s1, u2, o[:9], smp)
        n_r += s_eta == 1.0; n_t += s_eta != 1.0
    assert n_r > 30 and n_t > 200 and n_ev > 300


# sha256 of the 95 x 3 CIE 1931 values followed by the 95 D65 values, as little-endian float64: the digest of the reference's
# tables (src/libcore/spectrum.cpp:110-186, src/spectra/d65.cpp:12-25), which csrc/miw/cie_data.h was checked to hold value for value
CIE_D65_SHA256 = "34cf5367aab345b19c5d40931a6bef2ba193f31f21916d101009c3ae350632e3"


def _reference_tables():
    """CIE 1931 (95 samples x 3, 360 - 830 nm) and D65 (95 samples), parsed from the text of csrc/miw/cie_data.h (not compiled in) and
    pinned to the reference's own values by CIE_D65_SHA256: a table edited or regenerated wrongly fails here, before any sum below."""
    import hashlib
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mitsuba2_amd", "csrc", "miw", "cie_data.h")).read()
    num = r"[-+]?\d*\.?\d+(?:[eE][-+]?\d+)?"

    def table(name):
        head = "#define %s \\" % name
        body = txt[txt.index(head) + len(head):]
        body = body[:body.index("\n\n")] if "\n\n" in body else body
        return np.array([float(x) for x in re.findall(num, re.sub(r"(?<=\d)f", "", body.replace("(float)", "")))])
    cie, d65 = table("MIW_CIE1931_TABLE").reshape(3, 95), table("MIW_D65_TABLE")
    assert cie.shape == (3, 95) and d65.shape == (95,)
    assert hashlib.sha256(np.concatenate([cie.ravel(), d65]).astype("<f8").tobytes()).hexdigest() == CIE_D65_SHA256
    return cie, d65


def test_spectral_leaves_against_float64_restatement(native, oracle_spectral):
    """scalar_spectral (config 5): sample_shifted (math.h:419-442) + sample_rgb_spectrum (spectrum.h:271-285), srgb_model_eval
    (srgb.h:9-23), the srgb_d65 emitter spectrum = the upsampled colour times the D65 table (srgb_d65.cpp:56-62, d65.cpp:50-66,
    `regular`'s linear interpolation distr_1d.h:378-392) and spectrum_to_xyz over the CIE 1931 table (spectrum.h:147-217) —
    with both tables pinned to the reference's values by digest (_reference_tables)."""
    cie, d65 = _reference_tables()

    def lerp_table(tab, lam):
        t = (lam - 360.0) * (94 / 470.0)
        i = int(min(max(int(t), 0), 93))
        return (1 - (t - i)) * tab[i] + (t - i) * tab[i + 1] if 360.0 <= lam <= 830.0 else 0.0

    rng = np.random.default_rng(41)
    n = 300
    x = np.zeros((n, 5), np.float32)
    x[:, 0] = rng.random(n)
    x[:, 1] = rng.normal(0, 2e-5, n); x[:, 2] = rng.normal(0, 2e-2, n); x[:, 3] = rng.normal(0, 3.0, n)   # sigmoid-polynomial coefficients
    x[:, 4] = rng.uniform(0.2, 30.0, n) / 10568.0                                                          # D65Spectrum::m_scale (d65.cpp:54-55: scale / 10568; the host folds it into the record)
    out = oracle_spectral.eval(11, x).astype(np.float64)
    for xi, o in zip(x.astype(np.float64), out):
        u, c0, c1, c2, scale = xi
        for k in range(4):
            s = u + k / 4.0
            if s > 1:
                s -= 1
            if min(s, 1 - s) < 1e-3:
                continue                                          # atanh's argument near its poles
            lam = 538.0 - math.atanh(0.8569106254698279 - 1.8275019724092267 * s) * 138.88888888888889
            wgt = 253.82 * math.cosh(0.0072 * (lam - 538.0)) ** 2
            assert _close(o[k], lam, 3e-6) and _close(o[4 + k], wgt, 3e-5), (u, k, o[k], lam)
            lam32 = o[k]                                          # evaluate the spectra at the wavelength the float32 code drew
            v = (c0 * lam32 + c1) * lam32 + c2
            srgb = max(0.0, 0.5 * v / math.sqrt(v * v + 1) + 0.5)
            assert _close(o[8 + k], srgb, 2e-4, 2e-6), (c0, c1, c2, lam32, o[8 + k], srgb)
            # (the sigmoid cancels badly for very negative v: the D65 factor is checked on the float32 colour the line above accepted)
            assert _close(o[12 + k], o[8 + k] * lerp_table(d65, lam32) * scale, 2e-5, 1e-12)
        lam4, w4, sd4 = o[0:4], o[4:8], o[12:16]
        xyz = [np.mean([lerp_table(cie[c], lam4[k]) * w4[k] * sd4[k] for k in range(4)]) for c in range(3)]
        assert _close(o[16:19], xyz, 2e-5, 1e-12)


@pytest.mark.parametrize("shape", [(5, 7), (2, 2), (9, 4), (17, 33)])
def test_hierarchical2d_sample_against_float64_restatement(oracle, shape):
    """The warp the environment map is sampled with: the MIP hierarchy of patch averages (zero-padded to even sizes) and the
    top-down row / column selection of Hierarchical2D::sample, then the bilinear patch — odd and even sizes, the 1-patch case."""
    import ctypes as C
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    data = (rng.random(shape) * 10 + 0.05).astype(np.float32)
    levels, npatch = hier2d_build(data.astype(np.float64))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    checked = 0
    for u in rng.random((300, 2)):
        xy = np.array(u, np.float32); out = np.zeros(3, np.float32)
        assert oracle.L.orc_hier2d(fp(data), shape[1], shape[0], 0, fp(xy), fp(out)) == 0
        x, y, pdf = hier2d_sample(levels, npatch, xy.astype(np.float64))
        # a sample within float32 rounding of a row / column boundary may legitimately fall on the other side
        if abs(x * npatch[0] - round(x * npatch[0])) < 2e-3 or abs(y * npatch[1] - round(y * npatch[1])) < 2e-3:
            continue
        assert _close(out[0:2], [x, y], 0, 3e-5) and _close(out[2], pdf, 3e-4), (shape, u, out, (x, y, pdf))
        checked += 1
    assert checked > 200
