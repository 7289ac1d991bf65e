"""Float64 restatement of the null, thindielectric, mask and blendbsdf plugins, written from the reference's sources
(src/bsdfs/null.cpp:44-71, thindielectric.cpp:101-160, mask.cpp:93-156, blendbsdf.cpp:83-160; full BSDFContext, scalar
semantics), behind the interface of tests/f64_integrators.py:

    sample(wi, s1, s2, M) -> (wo, pdf, eta, delta, weight);  eval(wi, wo, M) -> f * cos;  pdf(wi, wo, M);  smooth

so that path_sample / direct_sample accept them beside the leaves there. Every discrete decision — sample1 against the opacity, the
weight or the reflectance r' — is reported to the Margin with the bound B_LOBE.

Opacity and weight are a constant or a nearest-filtered one-channel bitmap (bitmap.cpp:458-473, eval_1 :285-302). The interface of
f64_integrators.py carries no uv, so a wrapper is asked through `at(uv)`, a copy bound to the hit's texture coordinates; Scene below
is f64_integrators.Scene with the texture coordinates of mesh.cpp:489-511 (uv and the dp_du the shading frame starts from) whose
`bsdfs[si.mesh]` hands out the bound copy."""
import copy
import math

import numpy as np

import f64_integrators as F
from f64_integrators import B_LOBE, fresnel, _zspec, _ospec

B_TEXEL = 1e-4           # nearest-filtered bitmap: distance of uv * resolution to a texel boundary, in texels (uv is a float32 sum of three products)


class Constant:
    def __init__(self, value):
        self.value = min(max(float(np.float32(value)), 0.0), 1.0)

    def eval_1(self, uv, M):
        return self.value


class NearestBitmap:
    """bitmap.cpp:458-473 with wrap_mode clamp (:386-389), identity to_uv, one channel; the wrappers clamp the value to [0, 1]"""

    def __init__(self, pixels):
        self.a = np.asarray(pixels, np.float32).astype(np.float64).reshape(pixels.shape[0], pixels.shape[1])

    def eval_1(self, uv, M):
        h, w = self.a.shape
        x, y = uv[0] * w, uv[1] * h
        for v, n in ((x, w), (y, h)):
            if -0.5 < v < n + 0.5:                               # (clamped outside: no boundary there)
                M.add(v - round(v), B_TEXEL, "texel boundary")
        xi, yi = min(max(math.floor(x), 0), w - 1), min(max(math.floor(y), 0), h - 1)
        return min(max(float(self.a[yi, xi]), 0.0), 1.0)


def _texture(v):
    return v if hasattr(v, "eval_1") else Constant(v)


class _Wrapper:
    uv = None

    def at(self, uv):
        c = copy.copy(self)
        c.uv = uv
        c.children = [k.at(uv) if hasattr(k, "at") else k for k in self.children]
        return c


class Null:
    """null.cpp:44-71"""
    smooth = False

    def sample(self, wi, s1, s2, M):
        return -np.asarray(wi, np.float64), 1.0, 1.0, True, _ospec()

    def eval(self, wi, wo, M):
        return _zspec()

    def pdf(self, wi, wo, M):
        return 0.0


class ThinDielectric:
    """thindielectric.cpp:101-160"""
    smooth = False

    def __init__(self, int_ior=1.5046, ext_ior=1.000277, specular_reflectance=(1, 1, 1), specular_transmittance=(1, 1, 1)):
        self.eta = float(np.float32(int_ior)) / float(np.float32(ext_ior))
        self.sr = np.array(specular_reflectance, np.float32).astype(np.float64)
        self.st = np.array(specular_transmittance, np.float32).astype(np.float64)

    def reflectance(self, wi):
        r = fresnel(abs(wi[2]), self.eta)[0]
        return r * 2.0 / (1.0 + r)                               # r' = r + trt + tr^3t + ..

    def sample(self, wi, s1, s2, M):
        r = self.reflectance(wi)
        M.add(s1 - r, B_LOBE, "thindielectric lobe")
        if s1 <= r:
            return np.array([-wi[0], -wi[1], wi[2]]), r, 1.0, True, self.sr
        return -np.asarray(wi, np.float64), 1.0 - r, 1.0, True, self.st

    def eval(self, wi, wo, M):
        return _zspec()

    def pdf(self, wi, wo, M):
        return 0.0


class Mask(_Wrapper):
    """mask.cpp:93-156"""

    def __init__(self, nested, opacity=0.5):
        self.children, self.tex = [nested], _texture(opacity)
        self.smooth = nested.smooth

    def sample(self, wi, s1, s2, M):
        opacity = self.tex.eval_1(self.uv, M)
        M.add(s1 - opacity, B_LOBE, "mask lobe")
        if s1 < opacity:
            return self.children[0].sample(wi, s1 / opacity, s2, M)
        return -np.asarray(wi, np.float64), 1.0 - opacity, 1.0, True, _ospec()

    def eval(self, wi, wo, M):
        return self.children[0].eval(wi, wo, M) * self.tex.eval_1(self.uv, M)

    def pdf(self, wi, wo, M):
        return self.children[0].pdf(wi, wo, M) * self.tex.eval_1(self.uv, M)


class BlendBSDF(_Wrapper):
    """blendbsdf.cpp:83-160"""

    def __init__(self, bsdf0, bsdf1, weight):
        self.children, self.tex = [bsdf0, bsdf1], _texture(weight)
        self.smooth = bsdf0.smooth or bsdf1.smooth

    def sample(self, wi, s1, s2, M):
        w = self.tex.eval_1(self.uv, M)
        M.add(s1 - w, B_LOBE, "blendbsdf child")
        if s1 > w:
            return self.children[0].sample(wi, (s1 - w) / (1 - w), s2, M)
        return self.children[1].sample(wi, s1 / w, s2, M)

    def eval(self, wi, wo, M):
        w = self.tex.eval_1(self.uv, M)
        return self.children[0].eval(wi, wo, M) * (1 - w) + self.children[1].eval(wi, wo, M) * w

    def pdf(self, wi, wo, M):
        w = self.tex.eval_1(self.uv, M)
        return self.children[0].pdf(wi, wo, M) * (1 - w) + self.children[1].pdf(wi, wo, M) * w


def make_bsdf(obj, is_emitter):
    """f64_integrators.make_bsdf plus the four plugins: an api object (plugin name, constructor arguments, nested objects) -> the restatement"""
    from mitsuba2_amd import api

    def tex(v):
        if isinstance(v, api.BitmapTexture):
            assert v.params.get("filter_type") == "nearest" and v.params.get("wrap_mode") == "clamp" and v._pixels.shape[2] == 1
            return NearestBitmap(v._pixels)
        return Constant(v)
    if isinstance(obj, api.Mask):
        return Mask(make_bsdf(obj._children[0], False), tex(obj.params.get("opacity", 0.5)))
    if isinstance(obj, api.BlendBSDF):
        return BlendBSDF(make_bsdf(obj._children[0], False), make_bsdf(obj._children[1], False), tex(obj.params["weight"]))
    if isinstance(obj, api.TwoSided):
        return F.TwoSided(make_bsdf(obj._front, False), None if obj._back is None else make_bsdf(obj._back, False))
    if obj is not None and obj.plugin == "null":
        return Null()
    if obj is not None and obj.plugin == "thindielectric":
        return ThinDielectric(**dict(obj.params))
    return F.make_bsdf(obj, is_emitter)


class _Mesh(int):
    """Hit.mesh: the mesh index, carrying the hit's texture coordinates to Scene.bsdfs"""
    uv = None


class _Bsdfs(list):
    def __getitem__(self, i):
        b = list.__getitem__(self, int(i))
        return b.at(i.uv) if hasattr(b, "at") else b


class _Plain:
    """what f64_integrators.Scene reads of a mesh, without its BSDF (the default one stands in until make_bsdf above replaces it)"""

    def __init__(self, m):
        self.vertices, self.faces, self.normals, self.emitter, self.bsdf = m.vertices, m.faces, m.normals, m.emitter, None


class Scene(F.Scene):
    """f64_integrators.Scene + vertex texture coordinates (mesh.cpp:489-511) + the BSDFs of make_bsdf"""

    def __init__(self, meshes):
        F.Scene.__init__(self, [_Plain(m) for m in meshes])
        self.bsdfs = _Bsdfs(make_bsdf(m.bsdf, m.emitter is not None) for m in meshes)
        self.uvs = [None if m.texcoords is None else m.texcoords.astype(np.float64) for m in meshes]

    def ray_intersect(self, o, d, mint, maxt, M):
        best, t, u, v = self._query(o, d, mint, maxt, M, False)
        si = F.Hit()
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
        si.valid, si.t, si.mesh = True, float(t[best]), _Mesh(m)
        si.p = P[ia] * b0 + P[ib] * b1 + P[ic] * b2
        si.n = F._normalize(F._cross(dp0, dp1))
        dp_du = F.coordinate_system_s(si.n)                      # :491
        si.mesh.uv = np.array([b1, b2])                          # :490
        T = self.uvs[m]
        if T is not None:                                        # :492-511
            si.mesh.uv = T[ia] * b0 + T[ib] * b1 + T[ic] * b2
            duv0, duv1 = T[ib] - T[ia], T[ic] - T[ia]
            det = duv0[0] * duv1[1] - duv0[1] * duv1[0]
            if det != 0:
                dp_du = (duv1[1] * dp0 - duv0[1] * dp1) * (1.0 / det)
        N = self.normals[m]
        si.sh_n = si.n if N is None else F._normalize(N[ia] * b0 + N[ib] * b1 + N[ic] * b2)
        si.sh_s = F._normalize(dp_du - si.sh_n * float(si.sh_n @ dp_du))      # interaction.h:153-156
        si.sh_t = F._cross(si.sh_n, si.sh_s)
        si.wi = si.to_local(-d)
        return si
