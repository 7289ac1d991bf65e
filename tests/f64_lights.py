"""Float64 restatements of the emitters without a shape — point.cpp, spot.cpp, directional.cpp, constant.cpp — written from the
reference sources alone, and the scene of f64_integrators.py extended by them: Scene.sample_emitter_direction hands the sampled
emitter's `delta` flag to path_sample / direct_sample, whose MIS weight is `1 if delta else mis_weight(...)` (path.cpp:170,
direct.cpp:156). f64_integrators.py is imported, not edited.

A light is described by the Python object of mitsuba2_amd/api.py (plugin name + the keyword arguments it was made with), never by
anything the library computed from them."""
import math

import numpy as np

import f64_integrators as F

INV_FOUR_PI = 1.0 / (4.0 * math.pi)
B_SPOT = 1e-4            # spot: cos(theta) against the cosines of beam_width and cutoff_angle (the falloff's two branch points)


def _f32(x):
    return float(np.float32(x))


def _look_at(origin, target, up):
    """Transform4f::look_at, transform.h:241-269 -> 4x4 (columns left, new_up, dir, origin)"""
    o, t, u = (np.array(v, np.float32).astype(np.float64) for v in (origin, target, up))
    d = F._normalize(t - o)
    left = F._normalize(F._cross(F._normalize(u), d))
    new_up = F._cross(d, left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, new_up, d, o
    return m


def _to_world(params):
    tw = params.get("to_world")
    if tw is None:
        return np.eye(4)
    if isinstance(tw, dict):
        return _look_at(tw["origin"], tw["target"], tw.get("up", (0, 1, 0)))
    return np.asarray(tw, np.float64)


class _Light:
    delta = True

    def __init__(self, value):
        self.rgb = self.radiance = np.array(value, np.float32).astype(np.float64)

    def set_wavelengths(self, wl, model):
        F.AreaEmitter.set_wavelengths(self, wl, model)           # the same srgb_d65 spectrum as an area light's radiance

    def set_scene(self, lo, hi):                                 # directional.cpp / constant.cpp set_scene: bbox().bounding_sphere()
        c = (lo + hi) * 0.5
        self.bsphere_radius = max(F.RAY_EPSILON, float(np.linalg.norm(c - hi)) * (1 + F.RAY_EPSILON))

    def eval(self, wi_local):                                    # point.cpp:106, spot.cpp:170, directional.cpp:75
        return F._zspec()

    def eval_direction(self, d):
        return F._zspec()

    def pdf_direction(self, d, dist, n, M):
        return 0.0


class Point(_Light):
    """point.cpp:75-104"""

    def __init__(self, position=None, intensity=(1, 1, 1), to_world=None):
        super().__init__(intensity)
        self.p = np.array(position, np.float32).astype(np.float64) if position is not None else _to_world(dict(to_world=to_world))[:3, 3]

    def sample_direction(self, ref_p, u, M):
        d = self.p - ref_p
        dist = math.sqrt(float(d @ d))
        inv = 1.0 / dist
        return d * inv, dist, 1.0, self.radiance * (inv * inv), np.zeros(3)


class Spot(_Light):
    """spot.cpp:74-168"""

    def __init__(self, to_world=None, intensity=(1, 1, 1), cutoff_angle=20.0, beam_width=None):
        super().__init__(intensity)
        self.m = _to_world(dict(to_world=to_world))
        self.p = self.m[:3, 3]
        beam_width = cutoff_angle * 3.0 / 4.0 if beam_width is None else beam_width
        self.cutoff, self.beam = math.radians(_f32(cutoff_angle)), math.radians(_f32(beam_width))
        self.inv_transition = 1.0 / (self.cutoff - self.beam)

    def falloff(self, local_d, M):
        c = float(F._normalize(local_d)[2])
        M.add(c - math.cos(self.beam), B_SPOT, "spot beam edge")
        M.add(c - math.cos(self.cutoff), B_SPOT, "spot cutoff edge")
        if c <= math.cos(self.cutoff):
            return F._zspec()
        if c >= math.cos(self.beam):
            return self.radiance
        return self.radiance * ((self.cutoff - math.acos(c)) * self.inv_transition)

    def sample_direction(self, ref_p, u, M):
        d = self.p - ref_p
        dist = math.sqrt(float(d @ d))
        inv = 1.0 / dist
        d = d * inv
        local = np.linalg.inv(self.m[:3, :3]) @ (-d)
        return d, dist, 1.0, self.falloff(local, M) * (inv * inv), np.zeros(3)


class Directional(_Light):
    """directional.cpp:49-137"""

    def __init__(self, direction=None, irradiance=(1, 1, 1), to_world=None):
        super().__init__(irradiance)
        if direction is not None:
            self.d = F._normalize(np.array(direction, np.float32).astype(np.float64))
        else:
            self.d = _to_world(dict(to_world=to_world))[:3, 2]

    def sample_direction(self, ref_p, u, M):
        return -self.d, 2.0 * self.bsphere_radius, 1.0, self.radiance, self.d


class Constant(_Light):
    """constant.cpp:42-121: an environment emitter"""
    delta = False

    def __init__(self, radiance=(1, 1, 1)):
        super().__init__(radiance)

    def eval_direction(self, d):
        return self.radiance

    def sample_direction(self, ref_p, u, M):
        z = 1.0 - 2.0 * u[1]                                     # warp.h:255-260
        r = math.sqrt(max(0.0, 1.0 - z * z))
        phi = 2.0 * math.pi * u[0]
        d = np.array([r * math.cos(phi), r * math.sin(phi), z])
        return d, 2.0 * self.bsphere_radius, INV_FOUR_PI, self.radiance / INV_FOUR_PI, -d

    def pdf_direction(self, d, dist, n, M):
        return INV_FOUR_PI


_PLUGINS = dict(point=Point, spot=Spot, directional=Directional, constant=Constant)


def make_light(obj):
    """the restatement of an api light object (obj.plugin, obj.params)"""
    return _PLUGINS[obj.plugin](**obj.params)


class Scene(F.Scene):
    """f64_integrators.Scene plus the scene's light children, in the emitter order of scene.cpp:38-60"""

    def __init__(self, meshes, envmap=None, envmap_after=None, lights=()):
        super().__init__(meshes, envmap, envmap_after)
        n = len(self.meshes)
        # the emitter list again, with the lights where they were declared: `area_before[i]` emitters precede the children at place i
        base = list(self.emitters)
        area = [e for e in base if e is not self.env]
        env_pos = None if self.env is None else (n if envmap_after is None else min(envmap_after, n))
        emitters, k = [], 0
        self.lights = []
        for i in range(n + 1):
            if env_pos == i:
                emitters.append(self.env)
            for obj, after in lights:
                if (n if after is None else min(after, n)) == i:
                    l = make_light(obj); self.lights.append(l); emitters.append(l)
            if i < n and self.mesh_emitter[i] >= 0:
                self.mesh_emitter[i] = len(emitters); emitters.append(area[k]); k += 1
        self.emitters = emitters
        if self.env is not None:
            self.env.index = emitters.index(self.env)
        allp = np.concatenate(self.P)
        for l in self.lights:
            l.set_scene(allp.min(0), allp.max(0))
            if isinstance(l, Constant):
                assert self.env is None, "one environment emitter per scene"
                self.env = l                                     # what a miss sees (scene.h:248-249)

    def sample_emitter_direction(self, si, u, M):
        """scene.cpp:164-214 as in the base class, returning the sampled emitter's delta flag"""
        n = len(self.emitters)
        if n == 0:
            return np.zeros(3), 0.0, False, F._zspec()
        u = [u[0], u[1]]
        if n == 1:
            em, sel = self.emitters[0], 1.0
        else:
            sel = 1.0 / n
            x = u[0] * n
            index = min(int(x), n - 1)
            M.add(x - round(x), F.B_CDF * n, "emitter choice")
            u[0] = (u[0] - index * sel) * n
            em = self.emitters[index]
        d, dist, pdf, val, _ = em.sample_direction(si.p, u, M)
        pdf *= sel
        val = val / sel
        if pdf != 0:
            mint = F.RAY_EPSILON * (1 + np.abs(si.p).max())
            if self.ray_test(si.p, d, mint, dist * (1 - F.SHADOW_EPSILON), M):
                val = F._zspec()
        return d, pdf, bool(getattr(em, "delta", False)), val


def from_api_scene(api_scene):
    return Scene(api_scene.shapes, api_scene.envmap, api_scene.envmap_after, api_scene.lights)


# ---- the jobs: scenes.lit_box(kind) and scenes.mixed_light_box with the box filter, description only ----
JOB_W, JOB_H, JOB_SPP = 32, 24, 2
JOBS = {
    "point-path":            ("point", "path", dict()),
    "point-path-d3-rr2":     ("point", "path", dict(max_depth=3, rr_depth=2)),
    "spot-path":             ("spot", "path", dict()),
    "directional-path":      ("directional", "path", dict()),
    "constant-path":         ("constant", "path", dict()),
    "point-direct-1-1":      ("point", "direct", dict(emitter_samples=1, bsdf_samples=1)),
    "spot-direct-2-0":       ("spot", "direct", dict(emitter_samples=2, bsdf_samples=0)),
    "directional-direct-1-1": ("directional", "direct", dict(emitter_samples=1, bsdf_samples=1)),
    "constant-direct-1-1":   ("constant", "direct", dict(emitter_samples=1, bsdf_samples=1)),
    "constant-direct-1-1-hide": ("constant", "direct", dict(emitter_samples=1, bsdf_samples=1, hide_emitters=True)),
    "mixed-path":            ("mixed", "path", dict()),
    "mixed-path-d3-rr2":     ("mixed", "path", dict(max_depth=3, rr_depth=2)),
    "mixed-direct-1-1":      ("mixed", "direct", dict(emitter_samples=1, bsdf_samples=1)),
    "mixed-direct-2-0-hide": ("mixed", "direct", dict(emitter_samples=2, bsdf_samples=0, hide_emitters=True)),
}
SEED = 50000


def job_scene(scenes, which, spp, variant_kw=None):
    kw = dict(device=-1, rfilter="box", seed=SEED)
    kw.update(variant_kw or {})
    if which == "mixed":
        return scenes.mixed_light_box(JOB_W, JOB_H, spp, **kw)
    return scenes.lit_box(which, JOB_W, JOB_H, spp, **kw)
