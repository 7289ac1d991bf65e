"""Float64 restatements of the reference, shared by the independent test tiers.

Everything here is written straight from the reference source it cites by file and line, in plain Python and numpy, and shares no
code with mitsuba2_amd/csrc/, oracle/ or the mih_* / mi_* entry points:

* the leaves (warps, Fresnel terms, the microfacet distribution, the BSDF plugins, Hierarchical2D) that
  test_independent_leaves.py compares with the checker's leaf entry points;
* a Scene read from the Python mesh objects of mitsuba2_amd/scenes.py, with brute-force scene queries;
* PathIntegrator::sample (path.cpp:100-227) and DirectIntegrator::sample (direct.cpp:105-198) on top of both:
  path_sample / direct_sample, which also count the sampler draws they make and report how far the path stayed from every
  discrete decision's threshold (Margin), so that a float32 evaluation of the same path can be compared with a tolerance.

No pytest fixture and no conftest is imported here."""
import math

import numpy as np

PI = math.pi


# ---------------------------------------------------------------- warp.h
def disk_concentric(u):
    """core/warp.h:54-90"""
    x, y = 2.0 * u[0] - 1.0, 2.0 * u[1] - 1.0
    if x == 0 and y == 0:
        return 0.0, 0.0
    if abs(x) < abs(y):
        r, phi = y, 0.5 * PI - 0.25 * PI * x / y
    else:
        r, phi = x, 0.25 * PI * y / x
    return r * math.cos(phi), r * math.sin(phi)


def cosine_hemisphere(u):
    """core/warp.h:325-334"""
    px, py = disk_concentric(u)
    return np.array([px, py, math.sqrt(max(0.0, 1.0 - px * px - py * py))])


# ---------------------------------------------------------------- fresnel.h
def fresnel(cos_i, eta):
    """render/fresnel.h:34-70 -> r, cos_theta_t, eta_it, eta_ti"""
    outside = cos_i >= 0
    eta_it, eta_ti = (eta, 1 / eta) if outside else (1 / eta, eta)
    cos_t_sqr = 1 - (1 - cos_i * cos_i) * eta_ti * eta_ti
    ci, ct = abs(cos_i), math.sqrt(max(0.0, cos_t_sqr))
    if eta == 1:
        r = 0.0
    elif ci == 0:
        r = 1.0
    else:
        a_s = (ci - eta_it * ct) / (ci + eta_it * ct)
        a_p = (ct - eta_it * ci) / (ct + eta_it * ci)
        r = 0.5 * (a_s * a_s + a_p * a_p)
    return r, (-ct if cos_i >= 0 else ct), eta_it, eta_ti          # mulsign_neg(cos_theta_t_abs, cos_theta_i)


def fresnel_conductor(cos_i, eta, k):
    """render/fresnel.h:92-116 (per channel)"""
    c2 = cos_i * cos_i
    s2 = 1 - c2
    s4 = s2 * s2
    t1 = eta * eta - k * k - s2
    a2pb2 = np.sqrt(np.maximum(0, t1 * t1 + 4 * k * k * eta * eta))
    a = np.sqrt(np.maximum(0, 0.5 * (a2pb2 + t1)))
    term1, term2 = a2pb2 + c2, 2 * cos_i * a
    rs = (term1 - term2) / (term1 + term2)
    term3, term4 = a2pb2 * c2 + s4, term2 * s2
    rp = rs * (term3 - term4) / (term3 + term4)
    return 0.5 * (rs + rp)


# ---------------------------------------------------------------- microfacet.h
class Microfacet:
    def __init__(self, kind, au, av, visible):
        self.kind, self.visible = kind, visible
        self.au, self.av = max(au, 1e-4), max(av, 1e-4)          # configure(), microfacet.h:415-418

    def eval(self, m):                                           # :184-202
        c = m[2]
        c2 = c * c
        if self.kind == "beckmann":
            res = math.exp(-((m[0] / self.au) ** 2 + (m[1] / self.av) ** 2) / c2) / (PI * self.au * self.av * c2 * c2)
        else:
            res = 1 / (PI * self.au * self.av * ((m[0] / self.au) ** 2 + (m[1] / self.av) ** 2 + m[2] ** 2) ** 2)
        return res if res * c > 1e-20 else 0.0

    def g1(self, v, m):                                          # :331-355
        xy = (self.au * v[0]) ** 2 + (self.av * v[1]) ** 2
        if xy == 0:
            res = 1.0
        else:
            t2 = xy / (v[2] * v[2])
            if self.kind == "beckmann":
                a = 1 / math.sqrt(t2)
                res = 1.0 if a >= 1.6 else (3.535 * a + 2.181 * a * a) / (1 + 2.276 * a + 2.577 * a * a)
            else:
                res = 2 / (1 + math.sqrt(1 + t2))
        return 0.0 if np.dot(v, m) * v[2] <= 0 else res

    def G(self, wi, wo, m):
        return self.g1(wi, m) * self.g1(wo, m)

    def pdf(self, wi, m):                                        # :214-223
        if self.visible:
            return self.eval(m) * self.g1(wi, m) * abs(np.dot(wi, m)) / wi[2]
        return self.eval(m) * m[2]

    def sample_visible_11_ggx(self, cos_i, u):                   # :395-411
        px, py = disk_concentric(u)
        s = 0.5 * (1 + cos_i)
        py = (1 - s) * math.sqrt(max(0.0, 1 - px * px)) + s * py
        z = math.sqrt(max(0.0, 1 - px * px - py * py))
        sin_i = math.sqrt(max(0.0, 1 - cos_i * cos_i))
        norm = 1 / (sin_i * py + cos_i * z)
        return (cos_i * py - sin_i * z) * norm, px * norm

    def sample(self, wi, u):                                     # :234-316 (GGX; Beckmann's visible branch is table-tested)
        if not self.visible:
            if self.au == self.av:
                sin_phi, cos_phi = math.sin(2 * PI * u[1]), math.cos(2 * PI * u[1])
                a2 = self.au * self.au
            else:
                tmp = self.av / self.au * math.tan(2 * PI * u[1])
                cos_phi = 1 / math.sqrt(tmp * tmp + 1)
                cos_phi = math.copysign(cos_phi, abs(u[1] - 0.5) - 0.25)
                sin_phi = cos_phi * tmp
                a2 = 1 / ((cos_phi / self.au) ** 2 + (sin_phi / self.av) ** 2)
            if self.kind == "beckmann":
                cos_t = 1 / math.sqrt(1 - a2 * math.log(1 - u[0]))
                pdf = (1 - u[0]) / (PI * self.au * self.av * max(cos_t ** 3, 1e-20))
            else:
                tan2 = a2 * u[0] / (1 - u[0])
                cos_t = 1 / math.sqrt(1 + tan2)
                pdf = 1 / (PI * self.au * self.av * max(cos_t ** 3, 1e-20) * (1 + tan2 / a2) ** 2)
            sin_t = math.sqrt(1 - cos_t * cos_t)
            return np.array([cos_phi * sin_t, sin_phi * sin_t, cos_t]), pdf
        wp = np.array([self.au * wi[0], self.av * wi[1], wi[2]])
        wp /= np.linalg.norm(wp)
        sin_t = math.sqrt(max(0.0, 1 - wp[2] * wp[2]))                          # Frame::sincos_phi, frame.h
        sin_phi, cos_phi = (wp[1] / sin_t, wp[0] / sin_t) if sin_t > 1e-12 else (0.0, 1.0)
        sx, sy = self.sample_visible_11_ggx(wp[2], u)
        sx, sy = (cos_phi * sx - sin_phi * sy) * self.au, (sin_phi * sx + cos_phi * sy) * self.av
        m = np.array([-sx, -sy, 1.0])
        m /= np.linalg.norm(m)
        return m, self.eval(m) * self.g1(wi, m) * abs(np.dot(wi, m)) / wi[2]


# ---------------------------------------------------------------- bsdfs
def roughconductor(d, eta, k, wi, u2, wo_eval):
    """roughconductor.cpp:196-275 (sample), :277-345 (eval), :347-382 (pdf) -> (wo, pdf, weight[3]), eval[3], pdf"""
    zero = np.zeros(3)
    smp = (zero, 0.0, zero)
    if wi[2] > 0:
        m, pdf = d.sample(wi, u2)
        wo = 2 * np.dot(wi, m) * m - wi
        if pdf != 0 and wo[2] > 0:
            w = d.g1(wo, m) if d.visible else d.G(wi, wo, m) * np.dot(wi, m) / (wi[2] * m[2])
            smp = (wo, pdf / (4 * np.dot(wo, m)), fresnel_conductor(np.dot(wi, m), eta, k) * w)
        else:
            smp = (wo, pdf / (4 * np.dot(wo, m)) if np.dot(wo, m) != 0 else 0.0, zero)
    ev, pd = zero, 0.0
    if wi[2] > 0 and wo_eval[2] > 0:
        h = wo_eval + wi
        h /= np.linalg.norm(h)
        D = d.eval(h)
        if D != 0:
            ev = fresnel_conductor(np.dot(wi, h), eta, k) * D * d.G(wi, wo_eval, h) / (4 * wi[2])
        if np.dot(wi, h) > 0 and np.dot(wo_eval, h) > 0:
            pd = D * d.g1(wi, h) / (4 * wi[2]) if d.visible else d.pdf(wi, h) / (4 * np.dot(wo_eval, h))
    return smp, ev, pd


def dielectric_sample(eta, wi, s1):
    """dielectric.cpp:201-310, unpolarised, both lobes enabled, TransportMode::Radiance -> wo, pdf, eta, weight"""
    r, cos_t, eta_it, eta_ti = fresnel(wi[2], eta)
    if s1 <= r:
        return np.array([-wi[0], -wi[1], wi[2]]), r, 1.0, 1.0, r
    return np.array([-eta_ti * wi[0], -eta_ti * wi[1], cos_t]), 1 - r, eta_it, eta_ti * eta_ti, r

def fresnel_diffuse_reflectance(eta):
    """render/fresnel.h:327-362"""
    if eta < 1:
        return -1.4399 * eta * eta + 0.7099 * eta + 0.6681 + 0.0636 / eta
    i = 1 / eta
    return 0.919317 - 3.4793 * i + 6.75335 * i ** 2 - 7.80989 * i ** 3 + 4.98554 * i ** 4 - 1.36881 * i ** 5

def roughdielectric(kind, au, av, visible, eta, wi, s1, u2, wo_eval):
    """roughdielectric.cpp:203-310 (sample), :312-390 (eval), :392-447 (pdf); TransportMode::Radiance, both lobes enabled"""
    ms = lambda v, s: v if s >= 0 else -v                         # enoki::mulsign on vectors / scalars
    d = Microfacet(kind, au, av, visible)
    ci = wi[2]
    out_s = None
    if ci != 0:
        sd = Microfacet(kind, au, av, visible)
        if not visible:
            k = 1.2 - 0.2 * math.sqrt(abs(ci))
            sd.au, sd.av = sd.au * k, sd.av * k                  # scale_alpha, microfacet.h:173-176
        m, pdf = sd.sample(ms(wi, ci), u2)
        if pdf != 0:
            F, cos_t, eta_it, eta_ti = fresnel(float(np.dot(wi, m)), eta)
            if s1 <= F:
                wo = 2 * np.dot(wi, m) * m - wi
                pdf *= F; bs_eta = 1.0; w = 1.0
                dwh = 1 / (4 * np.dot(wo, m))
            else:
                wo = m * (np.dot(wi, m) * eta_ti + cos_t) - wi * eta_ti
                pdf *= 1 - F; bs_eta = eta_it; w = eta_ti * eta_ti
                dwh = (bs_eta ** 2 * np.dot(wo, m)) / (np.dot(wi, m) + bs_eta * np.dot(wo, m)) ** 2
            w *= d.g1(wo, m) if visible else d.G(wi, wo, m) * np.dot(wi, m) / (ci * m[2])
            out_s = (wo, pdf * abs(dwh), bs_eta, w, F)
    ev = pd = 0.0
    co = wo_eval[2]
    if ci != 0:
        refl = ci * co > 0
        e, inv_e = (eta, 1 / eta) if ci > 0 else (1 / eta, eta)
        m = wi + wo_eval * (1.0 if refl else e)
        m /= np.linalg.norm(m)
        m = ms(m, m[2])
        D = d.eval(m)
        F = fresnel(float(np.dot(wi, m)), eta)[0]
        G = d.G(wi, wo_eval, m)
        if refl:
            ev = F * D * G / (4 * abs(ci))
        else:
            ev = abs((inv_e ** 2 * (1 - F) * D * G * e * e * np.dot(wi, m) * np.dot(wo_eval, m)) /
                     (ci * (np.dot(wi, m) + e * np.dot(wo_eval, m)) ** 2))
        if np.dot(wi, m) * ci > 0 and np.dot(wo_eval, m) * co > 0:
            dwh = 1 / (4 * np.dot(wo_eval, m)) if refl else (e * e * np.dot(wo_eval, m)) / (np.dot(wi, m) + e * np.dot(wo_eval, m)) ** 2
            sd = Microfacet(kind, au, av, visible)
            if not visible:
                k = 1.2 - 0.2 * math.sqrt(abs(ci))
                sd.au, sd.av = sd.au * k, sd.av * k
            pd = sd.pdf(ms(wi, ci), m) * (F if refl else 1 - F) * abs(dwh)
    return out_s, ev, pd

def hier2d_build(data):
    """Hierarchical2D<Float, 0> constructor, distr_2d.h:372-462 -> levels[0] = normalised data, levels[1..] = MIP hierarchy"""
    h, w = data.shape
    ny, nx = h - 1, w - 1
    avg = 0.25 * (data[:-1, :-1] + data[:-1, 1:] + data[1:, :-1] + data[1:, 1:])
    scale = nx * ny / avg.sum()
    levels = [data * scale]

    def pad(a):
        return np.pad(a, ((0, a.shape[0] & 1), (0, a.shape[1] & 1)))
    cur = pad(avg * scale)
    levels.append(cur)
    max_level = int(math.ceil(math.log2(max(nx, ny)))) if max(nx, ny) > 1 else 0
    for _ in range(2, max_level + 2):
        nxt = cur[0::2, 0::2] + cur[0::2, 1::2] + cur[1::2, 0::2] + cur[1::2, 1::2]
        cur = pad(nxt) if max(nxt.shape) > 1 else nxt
        levels.append(cur)
    return levels, (nx, ny)


def hier2d_sample(levels, npatch, u):
    """Hierarchical2D::sample, distr_2d.h:473-556 + warp::square_to_bilinear / interval_to_linear, warp.h:359-407"""
    sx, sy = min(max(u[0], 0.0), 1.0), min(max(u[1], 0.0), 1.0)
    ox = oy = 0
    for l in range(len(levels) - 2, 0, -1):
        lv = levels[l]
        ox, oy = ox * 2, oy * 2
        # the four entries the reference fetches are consecutive in ITS storage (2 x 2 blocks, Level::index); here by coordinates
        v00, v10, v01, v11 = lv[oy, ox], lv[oy, ox + 1], lv[oy + 1, ox], lv[oy + 1, ox + 1]
        sx, sy = min(max(sx, 0.0), 1.0), min(max(sy, 0.0), 1.0)
        r0, r1 = v00 + v10, v01 + v11
        sy *= r0 + r1
        m = sy > r0
        if m:
            oy += 1; sy -= r0
        sy /= r1 if m else r0
        c0, c1 = (v01, v11) if m else (v00, v10)
        sx *= c0 + c1
        m = sx > c0
        if m:
            sx -= c0; ox += 1
        sx /= c1 if m else c0
    d = levels[0]
    v00, v10, v01, v11 = d[oy, ox], d[oy, ox + 1], d[oy + 1, ox], d[oy + 1, ox + 1]

    def i2l(v0, v1, s):
        if abs(v0 - v1) > 1e-4 * (v0 + v1):
            return (v0 - math.sqrt(max(0.0, v0 * v0 + (v1 * v1 - v0 * v0) * s))) / (v0 - v1)
        return s
    r0, r1 = v00 + v10, v01 + v11
    sy = i2l(r0, r1, sy)
    c0, c1 = v00 + (v01 - v00) * sy, v10 + (v11 - v10) * sy
    sx = i2l(c0, c1, sx)
    return (ox + sx) / npatch[0], (oy + sy) / npatch[1], c0 + (c1 - c0) * sx



# ================================================================ scalar_spectral leaves
def sample_rgb_spectrum_wavelengths(u):
    """sample_shifted (math.h:419-442) + sample_rgb_spectrum (spectrum.h:271-285) -> the four wavelengths of wavelength sample u"""
    out = []
    for k in range(4):
        s = u + k / 4.0
        if s > 1:
            s -= 1
        out.append(538.0 - math.atanh(0.8569106254698279 - 1.8275019724092267 * s) * 138.88888888888889)
    return np.array(out)


def sample_rgb_spectrum_weights(wl):
    """... and the weight 1 / pdf of each wavelength, spectrum.h:271-285"""
    return 253.82 * np.cosh(0.0072 * (np.asarray(wl, np.float64) - 538.0)) ** 2


def srgb_model_eval(coeff, wl):
    """srgb.h:9-23"""
    wl = np.asarray(wl, np.float64)
    if math.isinf(coeff[2]):
        return np.full(len(wl), 0.5 * math.copysign(1.0, coeff[2]) + 0.5)
    v = (coeff[0] * wl + coeff[1]) * wl + coeff[2]
    return np.maximum(0.0, 0.5 * v / np.sqrt(v * v + 1) + 0.5)


def lerp_regular(tab, lam, lo=360.0, hi=830.0):
    """`regular` spectrum, distr_1d.h:378-392: linear interpolation of equally spaced samples, zero outside"""
    n = len(tab)
    t = (lam - lo) * ((n - 1) / (hi - lo))
    i = int(min(max(int(t), 0), n - 2))
    return (1 - (t - i)) * tab[i] + (t - i) * tab[i + 1] if lo <= lam <= hi else 0.0


def spectrum_to_xyz(value, wl, cie):
    """spectrum.h:147-217: the mean over the wavelengths of CIE 1931 (95 samples x 3) times the spectrum"""
    return np.array([np.mean([lerp_regular(cie[c], wl[k]) * value[k] for k in range(len(wl))]) for c in range(3)])


class SrgbModel:
    """srgb_model_fetch, srgb.cpp:14-42 over rgb2spec_load / rgb2spec_fetch (ext/rgb2spec/rgb2spec.c:12-119): the coefficient file
    ("SPEC", res, res scale values, 3 x res^3 x 3 coefficients), trilinear in (x, y) and in the non-uniform scale axis. Also carries
    the CIE 1931 and D65 tables the caller read (test_independent_leaves._reference_tables)."""

    def __init__(self, path, cie, d65):
        raw = open(path, "rb").read()
        assert raw[:4] == b"SPEC"
        self.res = int(np.frombuffer(raw, "<u4", 1, 4)[0])
        self.scale = np.frombuffer(raw, "<f4", self.res, 8).astype(np.float64)
        self.data = np.frombuffer(raw, "<f4", 9 * self.res ** 3, 8 + 4 * self.res).astype(np.float64).reshape(3, self.res, self.res, self.res, 3)
        self.cie, self.d65 = cie, d65

    def fetch(self, rgb):
        rgb = np.asarray(rgb, np.float64)
        if not rgb.any():
            return np.array([0.0, 0.0, -math.inf])
        if (rgb == 1).all():
            return np.array([0.0, 0.0, math.inf])
        rgb = np.clip(rgb, 0.0, 1.0)
        i = 0
        for j in (1, 2):
            if rgb[j] >= rgb[i]:
                i = j
        res = self.res
        z = rgb[i]
        sc = (res - 1) / z
        x, y = rgb[(i + 1) % 3] * sc, rgb[(i + 2) % 3] * sc
        xi, yi = min(int(x), res - 2), min(int(y), res - 2)
        zi = min(max(int(np.searchsorted(self.scale, z, side="right")) - 1, 0), res - 2)      # the last interval whose left end is <= z
        x1, y1, z1 = x - xi, y - yi, (z - self.scale[zi]) / (self.scale[zi + 1] - self.scale[zi])
        d = self.data[i]
        lx = lambda a, b: d[a, b, xi] * (1 - x1) + d[a, b, xi + 1] * x1
        ly = lambda a: lx(a, yi) * (1 - y1) + lx(a, yi + 1) * y1
        return (ly(zi) * (1 - z1) + ly(zi + 1) * z1).astype(np.float32).astype(np.float64)       # (the reference keeps float coefficients)


# ================================================================ margins
# A float32 and a float64 evaluation of one path agree closely unless a discrete decision sits on its threshold. Every decision
# the restatement takes reports its distance from the threshold, divided by the bound below which the float32 evaluation may
# decide otherwise: Margin.value is the smallest such ratio over the path, and a sample with value < 1 is not comparable. The
# bounds are fixed here, from the precision of the formats; nothing in this module sees what the code under test answered.
B_LOBE = 1e-4            # lobe choice against Fresnel / the sampling weight, Russian roulette: |u - p|
B_CDF = 1e-5             # emitter and face CDF bin: distance to the bin edge
B_SEAM = 1e-3            # concentric map: quadrant seam, u0 near 0 / 1 (as in test_independent_leaves.py)
B_BARY = 1e-4            # hit triangle: the smallest barycentric of the accepted hit and of rejected triangles in the segment
B_T = 1e-4               # t against mint / maxt, relative
B_TIE = 1e-5             # two accepted hits at the same distance, relative
B_T_ABS = 3 * 2.0 ** -23  # ... and absolute, in units of the coordinates' magnitude. The hit point p = p0 b0 + p1 b1 + p2 b2 with
#                          b0 = 1 - b1 - b2 is rounded five times in float32, so it lies up to about 3 ulp of its largest coordinate
#                          off the triangle's plane. A ray leaving p at the angle theta to that plane meets the plane again at
#                          t = offset / |cos theta|: for a grazing ray that t reaches mint, and the float32 evaluation re-hits the
#                          surface it leaves. Excluded: |t - mint| (or maxt) below B_T_ABS * (max|o| + |t|) / |cos theta|, for every
#                          triangle the ray would pass through.
B_TIR = 1e-4             # total internal reflection: |cos^2 theta_t|
B_GRAZE = 1e-3           # |cos theta| where a pdf divides by it, or where a side test reads its sign


class Margin:
    def __init__(self):
        self.value, self.what = math.inf, None
        self.scale = 0.0                                         # the largest single term the path added to its radiance (the comparison's atol is scaled by it)

    def add(self, distance, bound, what):
        r = abs(distance) / bound
        if r < self.value:
            self.value, self.what = r, what


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _normalize(v):
    return v / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


_CHANNELS = [3]           # the width of a Spectrum: 3 (scalar_rgb) or 4 wavelengths (scalar_spectral, Scene.set_wavelengths)


def _zspec():
    return np.zeros(_CHANNELS[0])


def _ospec():
    return np.ones(_CHANNELS[0])


def coordinate_system_s(n):
    """the first vector of coordinate_system(n), core/vector.h:116-136 (enoki::sign / mulsign read the sign BIT: -0.0 is negative)"""
    sgn = math.copysign(1.0, n[2])
    a = -1.0 / (sgn + n[2])
    b = n[0] * n[1] * a
    return np.array([math.copysign(1.0, n[2]) * (n[0] * n[0] * a) + 1.0, math.copysign(1.0, n[2]) * b, -math.copysign(1.0, n[2]) * n[0]])


RAY_EPSILON = float(np.float32(2.0 ** -24) * np.float32(1500))            # math.h:36-37, the float32 constants
SHADOW_EPSILON = float(np.float32(RAY_EPSILON) * np.float32(10))          # math.h:38


# ================================================================ BSDF plugins behind one interface
# sample(wi, s1, s2, M) -> (wo, pdf, eta, delta, weight[3]);  eval(wi, wo, M) -> f * cos[3];  pdf(wi, wo, M);  smooth = has a
# non-delta lobe (BSDFFlags::Smooth, bsdf.h)
def _seam(u2, M, poles=False):
    M.add(abs(abs(2 * u2[0] - 1) - abs(2 * u2[1] - 1)), B_SEAM, "concentric seam")
    if poles:
        M.add(min(u2[0], 1 - u2[0]), B_SEAM, "u0 edge")


class Diffuse:
    """diffuse.cpp:78-135"""
    smooth = True

    def __init__(self, reflectance=(0.5, 0.5, 0.5)):
        self.rgb = self.r = np.array(reflectance, np.float32).astype(np.float64)
        self.black = not self.r.any()

    def set_wavelengths(self, wl, model):
        """scalar_spectral: the colour is a `srgb` spectrum (srgb.cpp of src/spectra): srgb_model_fetch once, srgb_model_eval per ray"""
        if not hasattr(self, "coeff"):
            self.coeff = model.fetch(self.rgb)
        self.r = srgb_model_eval(self.coeff, wl)

    def sample(self, wi, s1, s2, M):
        M.add(wi[2], B_GRAZE, "diffuse side")
        if not wi[2] > 0:
            return np.zeros(3), 0.0, 0.0, False, _zspec()
        _seam(s2, M)
        wo = cosine_hemisphere(s2)
        pdf = wo[2] / PI
        return wo, pdf, 1.0, False, (self.r if pdf > 0 else _zspec())

    def eval(self, wi, wo, M):
        M.add(wi[2], B_GRAZE, "diffuse side"); M.add(wo[2], B_GRAZE, "diffuse side")
        return self.r / PI * wo[2] if wi[2] > 0 and wo[2] > 0 else _zspec()

    def pdf(self, wi, wo, M):
        return wo[2] / PI if wi[2] > 0 and wo[2] > 0 else 0.0


class RoughConductor:
    """roughconductor.cpp:196-382 over microfacet.h (the leaf restatement roughconductor above)"""
    smooth = True

    def __init__(self, distribution="beckmann", alpha=0.1, alpha_u=None, alpha_v=None, sample_visible=True, eta=(0, 0, 0), k=(1, 1, 1)):
        f32 = lambda x: float(np.float32(x))
        self.d = Microfacet(distribution, f32(alpha if alpha_u is None else alpha_u), f32(alpha if alpha_v is None else alpha_v), sample_visible)
        self.eta, self.k = np.array(eta, np.float32).astype(np.float64), np.array(k, np.float32).astype(np.float64)

    def sample(self, wi, s1, s2, M):
        M.add(wi[2], B_GRAZE, "conductor side")
        if not wi[2] > 0:
            return np.zeros(3), 0.0, 0.0, False, _zspec()
        _seam(s2, M, poles=True)
        up = np.array([0.0, 0.0, 1.0])
        (wo, pdf, w), _, _ = roughconductor(self.d, self.eta, self.k, wi, s2, up)
        M.add(wo[2], B_GRAZE, "conductor wo side")
        return wo, pdf, 1.0, False, w

    def eval(self, wi, wo, M):
        M.add(wi[2], B_GRAZE, "conductor side"); M.add(wo[2], B_GRAZE, "conductor side")
        return _roughconductor_eval(self.d, self.eta, self.k, wi, wo)[0]

    def pdf(self, wi, wo, M):
        return _roughconductor_eval(self.d, self.eta, self.k, wi, wo)[1]


def _roughconductor_eval(d, eta, k, wi, wo):
    """the eval / pdf half of the leaf restatement `roughconductor` (its sample half needs wi above the surface and two numbers)"""
    zero = np.zeros(3)
    ev, pd = zero, 0.0
    if wi[2] > 0 and wo[2] > 0:
        h = _normalize(wo + wi)
        D = d.eval(h)
        if D != 0:
            ev = fresnel_conductor(np.dot(wi, h), eta, k) * D * d.G(wi, wo, h) / (4 * wi[2])
        if np.dot(wi, h) > 0 and np.dot(wo, h) > 0:
            pd = D * d.g1(wi, h) / (4 * wi[2]) if d.visible else d.pdf(wi, h) / (4 * np.dot(wo, h))
    return ev, pd


class Dielectric:
    """dielectric.cpp:201-320 (the leaf restatement dielectric_sample above): two delta lobes, eval = pdf = 0"""
    smooth = False

    def __init__(self, int_ior=1.5046, ext_ior=1.000277):
        self.eta = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))       # m_eta is a float32 member

    def sample(self, wi, s1, s2, M):
        wo, pdf, bs_eta, w, r = dielectric_sample(self.eta, wi, s1)
        eta_ti = 1 / self.eta if wi[2] >= 0 else self.eta
        M.add(1 - (1 - wi[2] * wi[2]) * eta_ti * eta_ti, B_TIR, "total internal reflection")
        M.add(s1 - r, B_LOBE, "dielectric lobe")
        self.last_reflected = bs_eta == 1.0 and pdf == r
        return wo, pdf, bs_eta, True, _ospec() * w

    def eval(self, wi, wo, M):
        return _zspec()

    def pdf(self, wi, wo, M):
        return 0.0


class Conductor:
    """conductor.cpp:216-262: one delta reflection lobe, weight = specular_reflectance * fresnel_conductor(cos theta_i)"""
    smooth = False

    def __init__(self, eta=(0, 0, 0), k=(1, 1, 1), specular_reflectance=(1, 1, 1)):
        f = lambda x: np.array(x, np.float32).astype(np.float64)
        self.eta, self.k, self.sr = f(eta), f(k), f(specular_reflectance)

    def sample(self, wi, s1, s2, M):
        M.add(wi[2], B_GRAZE, "conductor side")
        if not wi[2] > 0:
            return np.zeros(3), 0.0, 0.0, True, _zspec()
        return np.array([-wi[0], -wi[1], wi[2]]), 1.0, 1.0, True, self.sr * fresnel_conductor(wi[2], self.eta, self.k)

    def eval(self, wi, wo, M):
        return _zspec()

    def pdf(self, wi, wo, M):
        return 0.0


class Plastic:
    """plastic.cpp:161-290: a delta reflection lobe and a diffuse lobe under it, chosen by the Fresnel-weighted sampling weights"""
    smooth = True

    def __init__(self, diffuse_reflectance=(0.5, 0.5, 0.5), specular_reflectance=(1, 1, 1), int_ior=1.49, ext_ior=1.000277, nonlinear=False):
        f = lambda x: np.array(x, np.float32).astype(np.float64)
        self.rho, self.spec, self.nonlinear = f(diffuse_reflectance), f(specular_reflectance), nonlinear
        self.eta = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))
        self.inv_eta_2 = 1 / (self.eta * self.eta)
        self.fdr_int = fresnel_diffuse_reflectance(1 / self.eta)
        d_mean, s_mean = self.rho.mean(), self.spec.mean()                   # parameters_changed, :161-176
        self.ssw = s_mean / (d_mean + s_mean)

    def _ps(self, f_i):
        ps, pd = f_i * self.ssw, (1 - f_i) * (1 - self.ssw)
        return ps / (ps + pd)

    def _diff(self):
        return self.rho / (1 - (self.rho * self.fdr_int if self.nonlinear else self.fdr_int))

    def sample(self, wi, s1, s2, M):
        M.add(wi[2], B_GRAZE, "plastic side")
        if not wi[2] > 0:
            return np.zeros(3), 0.0, 0.0, False, _zspec()
        f_i = fresnel(wi[2], self.eta)[0]
        ps = self._ps(f_i)
        M.add(s1 - ps, B_LOBE, "plastic lobe")
        if s1 < ps:
            return np.array([-wi[0], -wi[1], wi[2]]), ps, 1.0, True, self.spec * (f_i / ps)
        _seam(s2, M)
        wo = cosine_hemisphere(s2)
        f_o = fresnel(wo[2], self.eta)[0]
        return wo, (1 - ps) * wo[2] / PI, 1.0, False, self._diff() * (self.inv_eta_2 * (1 - f_i) * (1 - f_o) / (1 - ps))

    def eval(self, wi, wo, M):
        M.add(wi[2], B_GRAZE, "plastic side"); M.add(wo[2], B_GRAZE, "plastic side")
        if not (wi[2] > 0 and wo[2] > 0):
            return _zspec()
        f_i, f_o = fresnel(wi[2], self.eta)[0], fresnel(wo[2], self.eta)[0]
        return self._diff() * (wo[2] / PI * self.inv_eta_2 * (1 - f_i) * (1 - f_o))

    def pdf(self, wi, wo, M):
        if not (wi[2] > 0 and wo[2] > 0):
            return 0.0
        return wo[2] / PI * (1 - self._ps(fresnel(wi[2], self.eta)[0]))


class TwoSided:
    """twosided.cpp:96-180: seen from behind, the back BSDF is asked with the z components of wi and wo mirrored"""

    def __init__(self, front, back=None):
        self.f, self.b = front, back if back is not None else front
        self.smooth = self.f.smooth or self.b.smooth

    @staticmethod
    def _flip(v):
        return np.array([v[0], v[1], -v[2]])

    def sample(self, wi, s1, s2, M):
        M.add(wi[2], B_GRAZE, "twosided side")
        if wi[2] > 0:
            return self.f.sample(wi, s1, s2, M)
        if wi[2] < 0:
            wo, pdf, eta, delta, w = self.b.sample(self._flip(wi), s1, s2, M)
            return self._flip(wo), pdf, eta, delta, w
        return np.zeros(3), 0.0, 0.0, False, _zspec()

    def eval(self, wi, wo, M):
        M.add(wi[2], B_GRAZE, "twosided side")
        return self.f.eval(wi, wo, M) if wi[2] > 0 else self.b.eval(self._flip(wi), self._flip(wo), M) if wi[2] < 0 else _zspec()

    def pdf(self, wi, wo, M):
        return self.f.pdf(wi, wo, M) if wi[2] > 0 else self.b.pdf(self._flip(wi), self._flip(wo), M) if wi[2] < 0 else 0.0


def make_bsdf(obj, is_emitter):
    """an api.BSDF object (its plugin name and constructor arguments) -> the restatement; None: the default of shape.cpp:75-81"""
    if obj is None:
        return Diffuse((0, 0, 0) if is_emitter else (0.5, 0.5, 0.5))
    from mitsuba2_amd import api
    if isinstance(obj, api.TwoSided):                            # (keeps its nested BSDF objects)
        return TwoSided(make_bsdf(obj._front, False), None if obj._back is None else make_bsdf(obj._back, False))
    kw = dict(obj.params)
    return {"diffuse": Diffuse, "roughconductor": RoughConductor, "dielectric": Dielectric, "conductor": Conductor, "plastic": Plastic}[obj.plugin](**kw)


# ================================================================ emitters
class AreaEmitter:
    """area.cpp:63-71 / :121-187 on a triangle mesh: shape.cpp:292-323, mesh.cpp:352-397, distr_1d.h:144-203, warp.h:153-156"""

    def __init__(self, radiance, P, faces):
        self.rgb = self.radiance = np.array(radiance, np.float32).astype(np.float64)
        self.P, self.faces = P, faces
        e0, e1 = P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]]
        self.areas = 0.5 * np.linalg.norm(np.cross(e0, e1), axis=1)
        self.cdf = np.cumsum(self.areas) / self.areas.sum()
        self.inv_area = 1 / self.areas.sum()

    def set_wavelengths(self, wl, model):
        """scalar_spectral: the radiance is a `srgb_d65` spectrum, srgb_d65.cpp:27-62: the colour scaled so that its largest
        component is 0.5, upsampled, times the D65 table scaled by that factor / 10568 (d65.cpp:44-64, float32 table values)"""
        if not hasattr(self, "coeff"):
            f32 = np.float32
            scale = f32(self.rgb.max()) * f32(2)
            color = np.array(self.rgb, f32) / scale if scale != 0 else np.array(self.rgb, f32)
            self.coeff = model.fetch(color.astype(np.float64))
            m_scale = f32(f32(1) * scale) * (f32(1) / f32(10568))
            self.d65 = (model.d65.astype(f32) * m_scale).astype(np.float64)
        self.radiance = np.array([lerp_regular(self.d65, x) for x in wl]) * srgb_model_eval(self.coeff, wl)

    def eval(self, wi_local):
        return self.radiance if wi_local[2] > 0 else _zspec()

    def sample_direction(self, ref_p, u, M):
        """-> d, dist, pdf, radiance / pdf (zero where the light faces away), n"""
        nf = len(self.faces)
        face = min(int(np.searchsorted(self.cdf, u[1], side="left")) if u[1] > 0 else 0, nf - 1)
        lo = self.cdf[face - 1] if face else 0.0
        if nf > 1:
            if face < nf - 1:
                M.add(u[1] - self.cdf[face], B_CDF, "face cdf")
            if face:
                M.add(u[1] - lo, B_CDF, "face cdf")
        u1 = (u[1] - lo) / (self.areas[face] * self.inv_area)
        t = math.sqrt(max(0.0, 1 - u[0]))
        b0, b1 = 1 - t, t * u1
        a, b, c = self.faces[face]
        e0, e1 = self.P[b] - self.P[a], self.P[c] - self.P[a]
        p = self.P[a] + e0 * b0 + e1 * b1
        n = _normalize(_cross(e0, e1))
        d = p - ref_p
        dist2 = float(d @ d)
        dist = math.sqrt(dist2)
        d = d / dist
        dp = abs(float(d @ n))
        M.add(dp, B_GRAZE, "light grazing")
        pdf = self.inv_area * (dist2 / dp if dp != 0 else 0.0)
        active = float(d @ n) < 0 and pdf != 0
        return d, dist, pdf, (self.radiance / pdf if active else _zspec()), n

    def pdf_direction(self, d, dist, n, M):
        dp = float(d @ n)
        M.add(dp, B_GRAZE, "light grazing")
        if not dp < 0:
            return 0.0
        return self.inv_area * (dist * dist / abs(dp) if dp != 0 else 0.0)


class Hit:
    """SurfaceInteraction3f of a closest-hit query; valid = False: a miss (wi = -d in world coordinates, interaction.h:591)"""
    valid = False


class Scene:
    """The scene of mitsuba2_amd/scenes.py read from its Python objects: vertices, faces, vertex normals, the BSDF objects' plugin
    names and arguments, the area lights' radiance, the environment map's pixels — as float64 numpy arrays of the float32 inputs."""

    def __init__(self, meshes, envmap=None, envmap_after=None):
        self.meshes = list(meshes)
        P0, E1, E2, mesh_of, face_of = [], [], [], [], []
        self.bsdfs, self.mesh_emitter, self.normals, self.P, self.F = [], [], [], [], []
        self.emitters = []                                       # scene order, scene.cpp:38-60
        pos = len(self.meshes) if envmap_after is None else envmap_after
        self.env = None
        for i, m in enumerate(self.meshes):
            if envmap is not None and i == pos:
                self.env = make_envmap(envmap); self.env.index = len(self.emitters); self.emitters.append(self.env)
            P = m.vertices.astype(np.float64); F = m.faces.astype(np.int64)
            self.P.append(P); self.F.append(F)
            P0.append(P[F[:, 0]]); E1.append(P[F[:, 1]] - P[F[:, 0]]); E2.append(P[F[:, 2]] - P[F[:, 0]])
            mesh_of += [i] * len(F); face_of += list(range(len(F)))
            self.normals.append(None if m.normals is None else m.normals.astype(np.float64))
            self.bsdfs.append(make_bsdf(m.bsdf, m.emitter is not None))
            if m.emitter is not None:
                self.mesh_emitter.append(len(self.emitters)); self.emitters.append(AreaEmitter(m.emitter.radiance, P, F))
            else:
                self.mesh_emitter.append(-1)
        if envmap is not None and self.env is None:
            self.env = make_envmap(envmap); self.env.index = len(self.emitters); self.emitters.append(self.env)
        self.P0, self.E1, self.E2 = np.concatenate(P0), np.concatenate(E1), np.concatenate(E2)
        self.mesh_of, self.face_of = np.array(mesh_of), np.array(face_of)
        self.n_len = np.linalg.norm(np.cross(self.E1, self.E2), axis=1)
        if self.env is not None:
            allp = np.concatenate(self.P)
            self.env.set_scene(allp.min(0), allp.max(0))
        self.n_hit = self.n_miss = 0

    def set_wavelengths(self, wl, model):
        """scalar_spectral: every colour of the scene evaluated at the ray's four wavelengths"""
        _CHANNELS[0] = len(wl)
        for x in self.bsdfs + self.emitters:
            if hasattr(x, "set_wavelengths"):
                x.set_wavelengths(wl, model)

    # ---- mesh.h:194-226 over every triangle
    def _all_triangles(self, o, d):
        E1, E2 = self.E1, self.E2
        pv = np.stack([d[1] * E2[:, 2] - d[2] * E2[:, 1], d[2] * E2[:, 0] - d[0] * E2[:, 2], d[0] * E2[:, 1] - d[1] * E2[:, 0]], 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            det = (E1 * pv).sum(1)
            self._cos = np.abs(det) / self.n_len                 # |cos| between the ray and every triangle's plane
            inv_det = 1.0 / det
            tv = o - self.P0
            u = (tv * pv).sum(1) * inv_det
            qv = np.stack([tv[:, 1] * E1[:, 2] - tv[:, 2] * E1[:, 1], tv[:, 2] * E1[:, 0] - tv[:, 0] * E1[:, 2], tv[:, 0] * E1[:, 1] - tv[:, 1] * E1[:, 0]], 1)
            v = (qv @ d) * inv_det
            t = (E2 * qv).sum(1) * inv_det
        return t, u, v

    def _query(self, o, d, mint, maxt, M, any_hit):
        t, u, v = self._all_triangles(o, d)
        w = 1.0 - u - v
        with np.errstate(invalid="ignore"):
            edge = np.minimum(np.minimum(u, v), w)
            hit = (edge >= 0) & (t >= mint) & (t <= maxt)
            idx = np.flatnonzero(hit)
            best = -1
            if len(idx):
                best = int(idx[np.argmin(t[idx])])
            # the margins: any triangle whose plane is crossed within the part of the segment that decides the answer
            limit = maxt if (any_hit or best < 0) else t[best]
            inside = edge > -B_BARY                              # t against mint / maxt with the absolute error of a float32 t
            if inside.any():
                t_err = B_T_ABS * (np.abs(o).max() + np.abs(t[inside])) / self._cos[inside]
                M.add((np.abs(t[inside] - mint) / t_err).min(), 1.0, "t at mint (grazing)")
                if math.isfinite(maxt):
                    M.add((np.abs(t[inside] - maxt) / t_err).min(), 1.0, "t at maxt (grazing)")
            cand = (t >= mint * (1 - B_T)) & (t <= limit * (1 + B_T))
            if cand.any():
                M.add(np.abs(edge[cand]).min(), B_BARY, "triangle edge")
                near = cand & (edge > -B_BARY)
                if near.any():
                    M.add(np.abs(t[near] / mint - 1).min(), B_T, "t at mint")
                    if math.isfinite(maxt):
                        M.add(np.abs(t[near] / maxt - 1).min(), B_T, "t at maxt")
                    if not any_hit and best >= 0 and near.sum() > 1:
                        others = t[near & (np.arange(len(t)) != best)]
                        M.add(np.abs(others / t[best] - 1).min(), B_TIE, "two hits at one distance")
        return best, t, u, v

    def ray_test(self, o, d, mint, maxt, M):
        return self._query(o, d, mint, maxt, M, True)[0] >= 0

    def ray_intersect(self, o, d, mint, maxt, M):
        """Scene::ray_intersect: closest hit, then Mesh::compute_surface_interaction (mesh.cpp:449-545) and the shading frame
        (interaction.h:153-156, :591)"""
        best, t, u, v = self._query(o, d, mint, maxt, M, False)
        si = Hit()
        si.d = d
        if best < 0:
            self.n_miss += 1
            si.wi = -d
            return si
        self.n_hit += 1
        m, f = int(self.mesh_of[best]), int(self.face_of[best])
        b1, b2 = float(u[best]), float(v[best])
        b0 = 1.0 - b1 - b2
        P = self.P[m]; ia, ib, ic = self.F[m][f]
        dp0, dp1 = P[ib] - P[ia], P[ic] - P[ia]
        si.valid, si.t, si.mesh = True, float(t[best]), m
        si.p = P[ia] * b0 + P[ib] * b1 + P[ic] * b2
        si.n = _normalize(_cross(dp0, dp1))
        N = self.normals[m]
        si.sh_n = si.n if N is None else _normalize(N[ia] * b0 + N[ib] * b1 + N[ic] * b2)
        dp_du = coordinate_system_s(si.n)
        si.sh_s = _normalize(dp_du - si.sh_n * float(si.sh_n @ dp_du))
        si.sh_t = _cross(si.sh_n, si.sh_s)
        si.wi = si.to_local(-d)
        return si

    def emitter_of(self, si):
        """si.emitter(scene), interaction.h:169-178: the hit shape's area light, or the environment for a miss"""
        if si.valid:
            e = self.mesh_emitter[si.mesh]
            return self.emitters[e] if e >= 0 else None
        return self.env

    def emitter_eval(self, emitter, si):
        return emitter.eval(si.wi) if si.valid else emitter.eval_direction(si.d)

    # ---- scene.cpp:164-231
    def sample_emitter_direction(self, si, u, M):
        """-> d, pdf, delta, value (visibility tested: zero when occluded), with the shadow ray of scene.cpp:203-206"""
        n = len(self.emitters)
        if n == 0:
            return np.zeros(3), 0.0, False, _zspec()
        u = [u[0], u[1]]
        if n == 1:
            em, sel = self.emitters[0], 1.0
        else:
            sel = 1.0 / n
            x = u[0] * n
            index = min(int(x), n - 1)
            M.add(x - round(x), B_CDF * n, "emitter choice")
            u[0] = (u[0] - index * sel) * n
            em = self.emitters[index]
        d, dist, pdf, val, _ = em.sample_direction(si.p, u, M)
        pdf *= sel
        val = val / sel
        if pdf != 0:
            mint = RAY_EPSILON * (1 + np.abs(si.p).max())
            if self.ray_test(si.p, d, mint, dist * (1 - SHADOW_EPSILON), M):
                val = _zspec()
        return d, pdf, False, val

    def pdf_emitter_direction(self, emitter, d, dist, n, M):
        p = emitter.pdf_direction(d, dist, n, M)
        return p if len(self.emitters) == 1 else p * (1.0 / len(self.emitters))


def _to_local(self, v):
    return np.array([float(v @ self.sh_s), float(v @ self.sh_t), float(v @ self.sh_n)])


def _to_world(self, v):
    return self.sh_s * v[0] + self.sh_t * v[1] + self.sh_n * v[2]


def _spawn(self, d):
    """spawn_ray, interaction.h:58-61 -> (o, d, mint, maxt)"""
    return self.p, d, (1 + np.abs(self.p).max()) * RAY_EPSILON, math.inf


Hit.to_local, Hit.to_world, Hit.spawn_ray = _to_local, _to_world, _spawn


def from_api_scene(api_scene):
    return Scene(api_scene.shapes, api_scene.envmap, api_scene.envmap_after)


def make_envmap(obj):
    return EnvMap(obj.rgba[..., :3], **obj.params)


# ================================================================ the integrators
def mis_weight(pdf_a, pdf_b):
    """path.cpp:223-227, direct.cpp:210-214"""
    a, b = pdf_a * pdf_a, pdf_b * pdf_b
    return a / (a + b) if a > 0 else 0.0


class _Acc:
    """the radiance sum of one path and the largest single term added to it"""

    def __init__(self):
        self.L, self.biggest = _zspec(), 0.0

    def add(self, c):
        self.L = self.L + c
        self.biggest = max(self.biggest, float(np.abs(c).max()))


def _hit_emitter_pdf(scene, si_prev, si_new, emitter, delta, M):
    """path.cpp:194-204 / direct.cpp:185-189: DirectionSample3f(si_new, si_prev), records.h:168-174, then pdf_emitter_direction"""
    if delta:
        return 0.0
    if si_new.valid:
        d = si_new.p - si_prev.p
        dist = math.sqrt(float(d @ d))
        return scene.pdf_emitter_direction(emitter, d / dist, dist, si_new.sh_n, M)
    return scene.pdf_emitter_direction(emitter, -si_new.wi, 0.0, np.zeros(3), M)


def _count_lobe(stats, bsdf, eta, delta):
    """which lobe a BSDF sample took: the dielectric's two (reflect / refract), the plastic's two (specular / diffuse)"""
    key = None
    if isinstance(bsdf, Dielectric):
        key = "reflect" if eta == 1.0 else "refract"
    elif isinstance(bsdf, Plastic):
        key = "plastic_specular" if delta else "plastic_diffuse"
    if key:
        stats[key] = stats.get(key, 0) + 1


def path_sample(scene, ray, rng, max_depth=-1, rr_depth=5, hide_emitters=False, stats=None):
    """PathIntegrator::sample, path.cpp:100-211 -> (L[3], valid, n_draws, margin). `hide_emitters` is accepted and, as in the
    reference (path.cpp never reads m_hide_emitters), changes nothing. stats: optional dict the function adds counts to."""
    M, acc = Margin(), _Acc()
    n0 = rng.count
    o, d, mint, maxt = ray
    eta, emission_weight, tp = 1.0, 1.0, _ospec()                              # :111-116
    si = scene.ray_intersect(o, d, mint, maxt, M)                                # :120
    valid_ray = si.valid
    emitter = scene.emitter_of(si)
    depth = 1
    active = True
    while True:
        if emitter is not None:                                                  # :128-129
            acc.add(emission_weight * tp * scene.emitter_eval(emitter, si))
        active = active and si.valid                                             # :131
        if depth > rr_depth:                                                     # :137-141, drawn whether or not the path lives
            q = min(tp.max() * eta * eta, 0.95)
            u = rng.next_1d()
            if active:
                M.add(u - q, B_LOBE, "russian roulette")
            active = active and u < q
            tp = tp * (1.0 / q)
        if (depth & 0xffffffff) >= (max_depth & 0xffffffff) or not active:      # :147-149 (the comparison is unsigned)
            break
        bsdf = scene.bsdfs[si.mesh]
        if bsdf.smooth:                                                          # :155-172
            # (a black surface — the default BSDF of an emitter's shape — multiplies whatever is sampled by an exact zero: the
            # decisions taken on the way cannot move the result, so their margins are not the path's)
            ed, epdf, edelta, eval_ = scene.sample_emitter_direction(si, rng.next_2d(), Margin() if getattr(bsdf, "black", False) else M)
            if epdf != 0:
                wo = si.to_local(ed)
                bsdf_val, bsdf_pdf = bsdf.eval(si.wi, wo, M), bsdf.pdf(si.wi, wo, M)
                mis = 1.0 if edelta else mis_weight(epdf, bsdf_pdf)
                acc.add(mis * tp * bsdf_val * eval_)
        s1 = rng.next_1d()                                                       # :177-178, in the order written
        s2 = rng.next_2d()
        wo, bpdf, beta, bdelta, bweight = bsdf.sample(si.wi, s1, s2, M)
        tp = tp * bweight                                                        # :181-184
        if not (tp != 0).any():
            break
        eta *= beta                                                              # :186
        if stats is not None:
            _count_lobe(stats, bsdf, beta, bdelta)
        si_next = scene.ray_intersect(*si.spawn_ray(si.to_world(wo)), M)         # :189-190
        if stats is not None and not si_next.valid:
            stats["miss_after_bounce"] = stats.get("miss_after_bounce", 0) + 1
        emitter = scene.emitter_of(si_next)                                      # :194-205
        if emitter is not None:
            emission_weight = mis_weight(bpdf, _hit_emitter_pdf(scene, si, si_next, emitter, bdelta, M))
        si = si_next
        depth += 1
    if stats is not None:
        stats["depth_max"] = max(stats.get("depth_max", 0), depth)
    M.scale = acc.biggest
    return acc.L, valid_ray, rng.count - n0, M


def direct_sample(scene, ray, rng, emitter_samples=1, bsdf_samples=1, hide_emitters=False, stats=None):
    """DirectIntegrator::sample, direct.cpp:105-198 with the constants of :98-102 -> (L[3], valid, n_draws, margin)"""
    M, acc = Margin(), _Acc()
    n0 = rng.count
    total = emitter_samples + bsdf_samples
    f32 = lambda x: float(np.float32(x))
    with np.errstate(divide="ignore"):
        weight_bsdf, weight_lum = f32(np.float32(1) / np.float32(bsdf_samples)), f32(np.float32(1) / np.float32(emitter_samples))
    frac_bsdf, frac_lum = f32(np.float32(bsdf_samples) / np.float32(total)), f32(np.float32(emitter_samples) / np.float32(total))
    o, d, mint, maxt = ray
    si = scene.ray_intersect(o, d, mint, maxt, M)                                # :113
    valid_ray = si.valid
    if not hide_emitters:                                                        # :119-123
        emitter = scene.emitter_of(si)
        if emitter is not None:
            acc.add(scene.emitter_eval(emitter, si))
    if not si.valid:                                                             # :125-127
        M.scale = acc.biggest
        return acc.L, valid_ray, rng.count - n0, M
    bsdf = scene.bsdfs[si.mesh]
    if bsdf.smooth:                                                              # :133-160
        for _ in range(emitter_samples):
            ed, epdf, edelta, eval_ = scene.sample_emitter_direction(si, rng.next_2d(), Margin() if getattr(bsdf, "black", False) else M)
            if epdf == 0:
                continue
            wo = si.to_local(ed)
            bsdf_val, bsdf_pdf = bsdf.eval(si.wi, wo, M), bsdf.pdf(si.wi, wo, M)
            mis = 1.0 if edelta else mis_weight(epdf * frac_lum, bsdf_pdf * frac_bsdf) * weight_lum
            acc.add(mis * bsdf_val * eval_)
    for _ in range(bsdf_samples):                                                # :164-196
        s1 = rng.next_1d()
        s2 = rng.next_2d()
        wo, bpdf, beta, bdelta, bweight = bsdf.sample(si.wi, s1, s2, M)
        if not (bweight != 0).any():
            continue
        if stats is not None:
            _count_lobe(stats, bsdf, beta, bdelta)
        si_b = scene.ray_intersect(*si.spawn_ray(si.to_world(wo)), M)
        if stats is not None and not si_b.valid:
            stats["miss_after_bounce"] = stats.get("miss_after_bounce", 0) + 1
        emitter = scene.emitter_of(si_b)
        if emitter is None:
            continue
        emitter_val = scene.emitter_eval(emitter, si_b)
        emitter_pdf = _hit_emitter_pdf(scene, si, si_b, emitter, bdelta, M)
        acc.add(bweight * emitter_val * (mis_weight(bpdf * frac_bsdf, emitter_pdf * frac_lum) * weight_bsdf))
    M.scale = acc.biggest
    return acc.L, valid_ray, rng.count - n0, M


# ================================================================ the environment map
B_ENV_SEAM = 1e-3        # the atan2 seam of the lat-long map (u within this of 0 / 1), as in test_independent_leaves.py
B_ENV_POLE = 1e-3        # 1 - |cos theta| at the poles, where inv_sin_theta is ill-conditioned
B_ENV_PATCH = 2e-3       # a warped sample this close (in patches) to a row / column boundary of Hierarchical2D


def look_at_rotation(origin, target, up):
    """the rotation of Transform::look_at, transform.h:241-258 (columns: left, up, forward)"""
    org, tgt, up = (np.array(x, np.float32).astype(np.float64) for x in (origin, target, up))
    fwd = _normalize(tgt - org)
    left = _normalize(_cross(up, fwd))
    return np.stack([left, _cross(fwd, left), fwd], 1)


class EnvMap:
    """EnvironmentMapEmitter, envmap.cpp:69-208, scalar_rgb: eval (:134-147 + the bilinear lookup :269-320), sample_direction
    (:157-190: Hierarchical2D warp, then theta / phi to a direction), pdf_direction (:192-208), set_scene (:128-132)"""

    def __init__(self, rgb, scale=1.0, to_world=None):
        self.img = np.asarray(rgb, np.float32).astype(np.float64)
        self.H, self.W = self.img.shape[:2]
        self.scale = float(np.float32(scale))
        self.R = np.eye(3) if to_world is None else look_at_rotation(to_world["origin"], to_world["target"], to_world.get("up", (0, 1, 0)))
        img = self.img
        lum = img[..., 0] * 0.212671 + img[..., 1] * 0.715160 + img[..., 2] * 0.072169        # mitsuba::luminance, spectrum.h
        lum = lum.astype(np.float32).astype(np.float64)
        sin_t = np.sin(np.arange(self.H) / (self.H - 1) * PI)
        self.levels, self.npatch = hier2d_build(lum * sin_t[:, None])
        self.dens = self.levels[0]
        self.radius = 1.0

    def set_scene(self, lo, hi):
        """bbox.h:329-332 + envmap.cpp:128-132"""
        self.radius = max(RAY_EPSILON, float(np.linalg.norm(0.5 * (lo + hi) - hi)) * (1 + RAY_EPSILON))

    def bilinear(self, table, uv):
        x, y = uv[0] * (self.W - 1), uv[1] * (self.H - 1)
        px, py = min(int(x), self.W - 2), min(int(y), self.H - 2)
        w1x, w1y = x - px, y - py
        return ((1 - w1y) * ((1 - w1x) * table[py, px] + w1x * table[py, px + 1]) +
                w1y * ((1 - w1x) * table[py + 1, px] + w1x * table[py + 1, px + 1]))

    def to_uv(self, d_world):
        dl = self.R.T @ d_world
        uv = np.array([math.atan2(dl[0], -dl[2]) / (2 * PI), math.acos(max(-1.0, min(1.0, dl[1]))) / PI])
        return uv - np.floor(uv), dl

    def _margins(self, uv, dl, M):
        M.add(min(uv[0], 1 - uv[0]), B_ENV_SEAM, "envmap seam")
        M.add(1 - abs(dl[1]), B_ENV_POLE, "envmap pole")

    def eval_direction(self, d_world, M=None):
        uv, dl = self.to_uv(d_world)
        if M is not None:
            self._margins(uv, dl, M)
        return self.bilinear(self.img, uv) * self.scale

    def pdf_direction(self, d, dist, n, M):
        uv, dl = self.to_uv(d)
        self._margins(uv, dl, M)
        inv_sin = 1 / math.sqrt(max(dl[0] ** 2 + dl[2] ** 2, (2.0 ** -24) ** 2))
        return self.bilinear(self.dens, uv) * inv_sin / (2 * PI * PI)

    def sample_direction(self, ref_p, u, M):
        x, y, pdf = hier2d_sample(self.levels, self.npatch, u)
        M.add(x * self.npatch[0] - round(x * self.npatch[0]), B_ENV_PATCH, "envmap patch column")
        M.add(y * self.npatch[1] - round(y * self.npatch[1]), B_ENV_PATCH, "envmap patch row")
        theta, phi = y * PI, x * 2 * PI
        dl = np.array([math.sin(theta) * math.sin(phi), math.cos(theta), -math.sin(theta) * math.cos(phi)])
        self._margins((x, y), dl, M)
        inv_sin = 1 / math.sqrt(max(dl[0] ** 2 + dl[2] ** 2, (2.0 ** -24) ** 2))
        d = self.R @ dl
        dist = 2 * self.radius
        dpdf = pdf * inv_sin / (2 * PI * PI) if pdf > 0 else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            val = self.bilinear(self.img, (x, y)) * self.scale / dpdf
        return d, dist, dpdf, val, -d


# ================================================================ jobs shared by the CPU and the GPU tier
JOB_W, JOB_H, JOB_SPP = 64, 48, 3
MAX_EXCLUDED = 0.05      # a condition of the jobs, not a measurement: at most this share of a job's samples may sit on a margin
ATOL_SCALE = 1e-6        # atol = ATOL_SCALE * the largest single term of the path: a float32 sum of about ten terms carries an
#                          absolute rounding error of a few float32 epsilons (6e-8) of its largest term, whatever the sum's size
SRGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float32).astype(np.float64)

# name -> (scene, integrator, its arguments, base seed). The seed is chosen per job so that every sample of the job stays in its
# own texel (sample_harness.every_sample_in_its_texel), which the CPU tier asserts.
JOBS = {
    "cornell-path":            ("cornell", "path", dict(), 50000),
    "cornell-path-d3-rr2":     ("cornell", "path", dict(max_depth=3, rr_depth=2), 50000),
    "cornell-path-hide":       ("cornell", "path", dict(hide_emitters=True), 50000),     # path.cpp never reads the flag: same as cornell-path
    "cornell-direct-1-1":      ("cornell", "direct", dict(emitter_samples=1, bsdf_samples=1), 50000),
    "cornell-direct-1-1-hide": ("cornell", "direct", dict(emitter_samples=1, bsdf_samples=1, hide_emitters=True), 50000),   # direct.cpp:119
    "cornell-direct-3-2":      ("cornell", "direct", dict(emitter_samples=3, bsdf_samples=2), 50000),
    "cornell-direct-2-0":      ("cornell", "direct", dict(emitter_samples=2, bsdf_samples=0), 50000),
    "cornell-direct-0-2":      ("cornell", "direct", dict(emitter_samples=0, bsdf_samples=2), 50000),
    "balls-path":              ("balls", "path", dict(), 50000),
    "balls-path-rr1":          ("balls", "path", dict(rr_depth=1), 50000),
    "plugin-path":             ("plugin", "path", dict(), 50000),
    "plugin-direct-1-1":       ("plugin", "direct", dict(emitter_samples=1, bsdf_samples=1), 50000),
    "open-path":               ("open", "path", dict(), 50000),
    "open-direct-1-1":         ("open", "direct", dict(emitter_samples=1, bsdf_samples=1), 50000),
    "open-nolight-path":       ("open-nolight", "path", dict(), 50000),
    "open-nolight-direct-1-1": ("open-nolight", "direct", dict(emitter_samples=1, bsdf_samples=1), 50000),
}


SPECTRAL_JOB = ("glass", "path", dict(), 50000)              # scalar_spectral: the glass-block Cornell box
LIGHT_DROP = 40.0        # see job_scene


def job_scene(scenes, which, spp, seed):
    """-> (api scene: description only, sensor) with the box filter: the boxes of scenes.py with the light hung LIGHT_DROP lower.
    As scenes.py places it, 0.8 under the ceiling, every shadow ray from the ceiling leaves at |cos| of 2e-3 to 4e-3, where a
    float32 evaluation can re-hit the ceiling beyond mint (Margin: "t at mint (grazing)") — a quarter of all paths would sit on that
    margin. The jobs change, not the cap on exclusions; arithmetic and materials are those of the configurations."""
    from mitsuba2_amd import api
    env = None
    if which == "cornell":
        meshes = scenes.cornell_box_meshes(diffuse_only=True)
    elif which == "balls":
        meshes = scenes.cornell_box_meshes(diffuse_only=False, ball_level=1)
    elif which == "glass":                                       # config C5's geometry: the tall block a closed dielectric solid
        meshes = scenes.cornell_box_meshes(diffuse_only=True, glass_block=True)
    elif which == "plugin":
        meshes = scenes.plugin_box_meshes()
    elif which in ("open", "open-nolight"):                      # scenes.open_box: no ceiling, the synthetic sky around the box
        meshes = [m for m in scenes.cornell_box_meshes(False, 1) if m.name != "ceiling" and (which == "open" or m.name != "light")]
        env = api.EnvMap(scenes.sky_envmap(64, 32), scale=1.0, to_world=dict(origin=(0, 0, 0), target=(0.3, 0.1, 1.0), up=(0, 1, 0)))
        ref, _ = scenes.open_box(JOB_W, JOB_H, spp, device=-1, with_area_light=(which == "open"), rfilter="box")     # (rebuilt by hand only to move the light: keep it tied to scenes.open_box)
        assert [m.name for m in ref.shapes] == [m.name for m in meshes] and np.array_equal(ref.envmap.rgba, env.rgba)
        assert ref.envmap.params == env.params and ref.envmap_after is None
    else:
        raise KeyError(which)
    for i, m in enumerate(meshes):
        if m.name == "light":
            v = m.vertices - np.array([0, LIGHT_DROP, 0], np.float32)
            meshes[i] = api.Mesh("light", v, m.faces, emitter=api.AreaLight(scenes.LIGHT_RADIANCE))
    return api.Scene(meshes, envmap=env).build(-1), scenes.cornell_sensor(JOB_W, JOB_H, spp, seed=seed, rfilter="box")


class DrawBank:
    """The sampler streams of all pixels of a job, drawn column by column with the numpy PCG32 of sample_harness.py (whose float
    conversion is exact): value(i, k) is draw k of stream i, state(i, k) the state after k draws."""

    def __init__(self, H, state, inc):
        self.H, self.inc = H, inc
        self.states, self.values = [np.asarray(state, np.uint64)], []

    def _extend(self, k):
        while len(self.values) <= k:
            v, s = self.H.pcg32_next_f32(self.states[-1], self.inc)
            self.values.append(v.astype(np.float64)); self.states.append(s)

    def column(self, k):
        self._extend(int(np.max(k)))
        k = np.broadcast_to(k, self.states[0].shape)
        return np.array([self.values[kk][i] for i, kk in enumerate(k)])

    def value(self, i, k):
        self._extend(k)
        return float(self.values[k][i])

    def state(self, i, k):
        self._extend(k)
        return self.states[k][i]


class Rng:
    """one stream of a DrawBank from draw `start` on; counts what it hands out"""

    def __init__(self, bank, i, start):
        self.bank, self.i, self.start, self.count = bank, i, start, 0

    def next_1d(self):
        v = self.bank.value(self.i, self.start + self.count)
        self.count += 1
        return v

    def next_2d(self):
        a = self.next_1d()
        return (a, self.next_1d())


def integrator_fn(kind, kw):
    fn = path_sample if kind == "path" else direct_sample
    return lambda scene, ray, rng, stats: fn(scene, ray, rng, stats=stats, **kw)


def restate_job(H, oracle, scene64, job, fn, n_samples, inc=None, model=None):
    """Runs the restatement over every pixel of `job` for n_samples camera samples, each pixel on its own sampler (seeded as the
    renderer seeds it; `inc`: another odd increment for every stream), sample k from the state its own draw count left after
    sample k - 1. The camera ray is the checker's (MI_EVAL_CAMERA_RAY): it is an input of sample(), not part of it.
    model (an SrgbModel): scalar_spectral — the third number of every camera sample gives the ray's four wavelengths
    (sample_rgb_spectrum_wavelengths, rounded to the float32 the device is handed), the scene's colours are evaluated at them.
    -> dict of arrays [n_samples, n_pixels(, channels)]: rays, L, valid, margin, scale, n_draws, state_before, state_after; px, py; stats"""
    px, py, seed = H.pixels_and_seeds(job)
    n = len(px)
    state, inc0 = H.pcg32_seed(seed)
    bank = DrawBank(H, state, inc0 if inc is None else inc)
    pos = np.zeros(n, np.int64)
    nch = 3 if model is None else 4
    _CHANNELS[0] = nch
    out = dict(px=px, py=py, stats={}, ray=np.zeros((n_samples, n, 8), np.float32), L=np.zeros((n_samples, n, nch)), wl=np.zeros((n_samples, n, 4), np.float32), valid=np.zeros((n_samples, n), bool),
               margin=np.zeros((n_samples, n)), scale=np.zeros((n_samples, n)), n_draws=np.zeros((n_samples, n), np.int64),
               state_before=np.zeros((n_samples, n), np.uint64), state_after=np.zeros((n_samples, n), np.uint64), what=[])
    scene64.n_hit = scene64.n_miss = 0
    for j in range(n_samples):
        jx, jy = bank.column(pos), bank.column(pos + 1)         # integrator.cpp:242-252: jitter, then the wavelength sample
        if model is not None:
            out["wl"][j] = np.stack([sample_rgb_spectrum_wavelengths(u) for u in bank.column(pos + 2)]).astype(np.float32)
        pos += 3
        film_pos = np.stack([px.astype(np.float32) + jx.astype(np.float32), py.astype(np.float32) + jy.astype(np.float32)], 1)
        ray = oracle.eval(5, film_pos, cfg=job.cfg)
        out["ray"][j] = ray[:, :8]
        what = []
        for i in range(n):
            r = ray[i].astype(np.float64)
            rng = Rng(bank, i, int(pos[i]))
            if model is not None:
                scene64.set_wavelengths(out["wl"][j, i].astype(np.float64), model)
            out["state_before"][j, i] = bank.state(i, int(pos[i]))
            L, valid, nd, M = fn(scene64, (r[0:3], r[3:6], float(r[6]), float(r[7])), rng, out["stats"])
            assert nd == rng.count
            pos[i] += nd
            out["L"][j, i], out["valid"][j, i], out["n_draws"][j, i], out["margin"][j, i], out["scale"][j, i] = L, valid, nd, M.value, M.scale
            out["state_after"][j, i] = bank.state(i, int(pos[i]))
            what.append(M.what)
        out["what"].append(what)
    out["stats"]["hit"], out["stats"]["miss"] = scene64.n_hit, scene64.n_miss
    _CHANNELS[0] = 3
    return out


def compare(got, got_valid, res, j, rtol, to_xyz, want=None):
    """The rule of the comparison for sample j of every pixel: among the samples whose margin is at least 1, `valid` is equal and
    every channel satisfies |got - want| <= atol + rtol * max(|got|, |want|), atol = ATOL_SCALE * the path's largest single term.
    -> (checked mask, bad mask, the largest relative deviation max(|got - want| - atol, 0) / max(|got|, |want|) among the checked:
    what rtol has to cover, whatever rtol is)"""
    if want is None:                                             # (spectral: the caller converts both sides, spectrum_to_xyz)
        want = res["L"][j] @ SRGB_TO_XYZ.T if to_xyz else res["L"][j]
    got = np.asarray(got, np.float64)
    checked = res["margin"][j] >= 1.0
    mag = np.maximum(np.abs(got), np.abs(want))
    atol = ATOL_SCALE * res["scale"][j][:, None]
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = np.where(err > atol, (err - atol) / mag, 0.0).max(1)
    bad = checked & ((err > atol + rtol * mag).any(1) | (np.asarray(got_valid, bool) != res["valid"][j]))
    return checked, bad, float(dev[checked].max()) if checked.any() else 0.0
