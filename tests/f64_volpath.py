"""Float64 restatement of the volpath integrator over homogeneous media, written straight from the reference's sources:
VolumetricPathIntegrator::sample / sample_emitter / evaluate_direct_light (src/integrators/volpath.cpp:60-257, :261-367, :370-465),
Medium::sample_interaction / eval_tr_and_pdf (src/librender/medium.cpp:36-89), HomogeneousMedium (src/media/homogeneous.cpp:21-54),
the isotropic and hg phase functions (src/phase/isotropic.cpp:30-45, hg.cpp:51-81), BSDF::eval_null_transmission
(src/librender/bsdf.cpp:11, null.cpp:69, mask.cpp:158-161, thindielectric.cpp:162-176) and the medium a surface hands a ray to
(interaction.h:178-200, shape.h:341-348).

It stands on tests/f64_integrators.py (Scene queries, BSDFs, emitters, Rng, Margin, restate_job, compare) and
tests/f64_nested_bsdfs.py (null, mask, thindielectric) and shares no code with mitsuba2_amd/csrc/.

Scalar semantics of the sampler: a next_1d / next_2d call that is reached draws, whatever its mask (the convention of
f64_integrators.path_sample's Russian roulette). Every discrete decision the media add reports to the Margin:

    channel choice                u * 3 against 1 and 2                          B_CDF * 3 (as the emitter choice)
    sampled_t against maxt        free flight against the ray's end              B_T, relative
    sampled_t against si.t        ... against the surface ahead                  B_T, relative
    sampled_t / si.t against the remaining distance of an emitter walk           B_T, relative
    remaining_dist > 0                                                           B_T, relative to the emitter's distance
    dot(d, n) in target_medium    which side of the boundary the ray leaves on   B_GRAZE
    |g| against Epsilon           the hg sampling branch                         Epsilon (a property of the medium, not of a path)
    the sign of d.z               Frame3f(ray.d) of the hg sample                B_FRAME
    offset from an area emitter's plane (a conditioning term, not a decision)     B_OFFSET, see below

The hit, CDF and lobe margins of f64_integrators.py apply as they stand."""
import math

import numpy as np

import f64_integrators as F
import f64_nested_bsdfs as N
from f64_integrators import B_CDF, B_GRAZE, B_LOBE, B_T, PI, SHADOW_EPSILON, Margin, mis_weight

EPSILON = 2.0 ** -24     # math::Epsilon<float>
B_FRAME = 1e-6           # |d.z| below which float32 and float64 may pick the other branch of coordinate_system's sign(n.z)
B_OFFSET = 1e-3          # a reference point this close to an area emitter's plane, relative to the magnitude of its coordinates. The emitter's
#                          solid-angle density divides by |cos| = offset / dist, and a float32 hit point lies about 1e-6 of its coordinates'
#                          magnitude off the float64 one (its barycentrics come out of the ray-triangle test with an absolute error of a few
#                          float32 epsilons and multiply edges as long as the room): the quotient is then off by 1e-6 / B_OFFSET = 1e-3
#                          relative, half of RTOL. f64_integrators.B_GRAZE bounds |cos| alone, which is the same condition only for a
#                          reference point a unit distance away; the fog jobs sample the light from walls hundreds of units away.
#                          Measured once, for the sample that led to the term (fog-cornell-hide, sample 1, pixel (10, 18): the light
#                          sampled from the wall point (0, 507.63, 254.77), 0.37 under the light's plane, |cos| 1.24e-3): this
#                          restatement gives L = 4.70928e-5, the device 4.71881e-5 (2.02e-3 apart); with the float32 hit points of the
#                          CPU checker fed into this restatement in place of its own it gives 4.718806e-5, the device's value to 2e-7.
#                          What the term ALONE excludes of a job's 9216 samples: fog-cornell 56 (0.61 %), fog-panes 43 (0.47 %),
#                          smoke-cube-gray 98 (1.06 %), milk-block 87 (0.94 %), bubble-cube 58 (0.63 %), cornell-nomedia 54 (0.59 %).
INF = math.inf


# ================================================================ phase functions
class Isotropic:
    def eval(self, ray_d, wo):
        return 1.0 / (4 * PI)

    def sample(self, ray_d, u, M):
        z = 1.0 - 2.0 * u[1]                                     # warp.h: square_to_uniform_sphere
        r = math.sqrt(max(0.0, 1.0 - z * z))
        phi = 2 * PI * u[0]
        return np.array([r * math.cos(phi), r * math.sin(phi), z]), 1.0 / (4 * PI)


class HG:
    def __init__(self, g=0.8):
        self.g = float(np.float32(g))

    def eval_hg(self, cos_theta):                                # hg.cpp:51-54
        g = self.g
        temp = 1.0 + g * g + 2.0 * g * cos_theta
        return (1.0 / (4 * PI)) * (1 - g * g) / (temp * math.sqrt(temp))

    def eval(self, ray_d, wo):                                   # :77-81, mi.wi = -ray.d
        return self.eval_hg(float(wo @ -ray_d))

    def sample(self, ray_d, u, M):                               # :56-75
        g = self.g
        M.add(abs(g) - EPSILON, EPSILON, "|g| at Epsilon")
        if abs(g) < EPSILON:
            cos_theta = 1 - 2 * u[0]
        else:
            sqr_term = (1 - g * g) / (1 - g + 2 * g * u[0])
            cos_theta = (1 + g * g - sqr_term * sqr_term) / (2 * g)
        sin_theta = math.sqrt(max(0.0, 1.0 - cos_theta * cos_theta))
        phi = 2 * PI * u[1]
        M.add(ray_d[2], B_FRAME, "hg frame sign")
        s, t = coordinate_system(ray_d)                          # Frame3f(ray.d), medium.cpp:42
        wo = s * (sin_theta * math.cos(phi)) + t * (sin_theta * math.sin(phi)) + ray_d * cos_theta
        return wo, self.eval_hg(-cos_theta)


def coordinate_system(n):
    """core/vector.h:116-136 -> (s, t)"""
    sgn = math.copysign(1.0, n[2])
    a = -1.0 / (sgn + n[2])
    b = n[0] * n[1] * a
    return (np.array([sgn * (n[0] * n[0] * a) + 1.0, sgn * b, -sgn * n[0]]), np.array([b, sgn + n[1] * n[1] * a, -n[1]]))


def make_phase(obj):
    if obj is None or obj.plugin == "isotropic":
        return Isotropic()
    return HG(**obj.params)


# ================================================================ the medium
class MI:
    pass


class Medium:
    """HomogeneousMedium: sigma_t * scale is formed in float32, as the record the device is handed holds it"""

    def __init__(self, obj):
        p = obj.params
        self.sigma_t = (np.array(p["sigma_t"], np.float32) * np.float32(p["scale"])).astype(np.float64)
        self.albedo = np.array(p["albedo"], np.float32).astype(np.float64)
        self.spectral, self.sample_emitters = bool(p["has_spectral_extinction"]), bool(p["sample_emitters"])
        self.phase = make_phase(obj.phase)

    def sample_interaction(self, o, d, mint, maxt, u, channel, M):
        """medium.cpp:36-75 with intersect_aabb = (true, 0, inf)"""
        mi = MI()
        mi.mint = max(mint, 0.0)
        m = self.sigma_t[channel]
        mi.ts = mi.mint + (-math.log1p(-u) / m)
        if math.isfinite(maxt):
            M.add(mi.ts / maxt - 1, B_T, "free flight at maxt")
        mi.t = mi.ts if mi.ts <= maxt else INF
        mi.p = o + d * mi.ts
        mi.sigma_t = mi.comb = self.sigma_t
        mi.sigma_s = self.sigma_t * self.albedo
        return mi

    @staticmethod
    def eval_tr_and_pdf(mi, si_t):
        """medium.cpp:80-89"""
        t = min(mi.t, si_t) - mi.mint
        tr = np.exp(-t * mi.comb)
        return tr, (tr if si_t < mi.t else tr * mi.comb)


def _tr_weight(tr, pdf, channel):
    return tr / pdf[channel] if pdf[channel] > 0 else np.zeros(3)


# ================================================================ surfaces between media
def null_transmission(bsdf, si, M):
    """BSDF::eval_null_transmission of the restated plugins"""
    if isinstance(bsdf, N.Null):
        return np.ones(3)
    if isinstance(bsdf, N.Mask):
        return 1 - bsdf.tex.eval_1(bsdf.uv, M) * (1 - null_transmission(bsdf.children[0], si, M))
    if isinstance(bsdf, N.ThinDielectric):
        return (1 - bsdf.reflectance(si.wi)) * bsdf.st
    return np.zeros(3)


class Media:
    """the media of an api scene: per mesh (interior, exterior), and the medium rays start in"""

    def __init__(self, api_scene):
        made = {}

        def get(obj):
            if obj is None:
                return None
            if id(obj) not in made:
                made[id(obj)] = Medium(obj)
            return made[id(obj)]
        self.start = get(api_scene.start_medium)
        self.of_mesh = [(get(m.interior), get(m.exterior)) for m in api_scene.shapes]

    def is_transition(self, si):
        a, b = self.of_mesh[int(si.mesh)]
        return a is not None or b is not None

    def target(self, si, d, M):
        """interaction.h:186-200: the exterior where dot(d, n) > 0 with the geometric normal"""
        c = float(d @ si.n)
        M.add(c, B_GRAZE, "medium side")
        return self.of_mesh[int(si.mesh)][1 if c > 0 else 0]


PANES = {}               # how often a shadow walk asked a mask / a thindielectric for its null transmission (the jobs' conditions read it)


def _count_pane(bsdf):
    for cls, key in ((N.Mask, "mask"), (N.ThinDielectric, "thindielectric")):
        if isinstance(bsdf, cls):
            PANES[key] = PANES.get(key, 0) + 1


def _si_t(si):
    return si.t if si.valid else INF


def _no_hit():
    si = F.Hit()
    si.t = INF
    return si


def _scene_sample_emitter(scene, ref_p, u, M):
    """Scene::sample_emitter_direction with test_visibility = false, scene.cpp:164-200 -> d, dist, pdf, delta, value"""
    n = len(scene.emitters)
    if n == 0:
        return np.zeros(3), 0.0, 0.0, False, np.zeros(3)
    u = [u[0], u[1]]
    if n == 1:
        em, sel = scene.emitters[0], 1.0
    else:
        sel = 1.0 / n
        x = u[0] * n
        index = min(int(x), n - 1)
        M.add(x - round(x), B_CDF * n, "emitter choice")
        u[0] = (u[0] - index * sel) * n
        em = scene.emitters[index]
    d, dist, pdf, val, n_l = em.sample_direction(ref_p, u, M)
    if isinstance(em, F.AreaEmitter) and pdf != 0:
        M.add(abs(float(d @ n_l)) * dist / max(1.0, np.abs(ref_p).max()), B_OFFSET, "offset from the light's plane")
    return d, dist, pdf * sel, False, val / sel


# ================================================================ the integrator
def sample_emitter(scene, media, ref_p, is_medium, medium, channel, rng, M):
    """volpath.cpp:261-367 -> (transmittance * emitter_val, ds.d, ds.pdf, ds.delta)"""
    d, dist, pdf, delta, emitter_val = _scene_sample_emitter(scene, ref_p, rng.next_2d(), M)      # :267
    if pdf == 0:                                                                                # :268-273
        return np.zeros(3), d, 0.0, delta
    T = np.ones(3)
    o = ref_p
    mint = 0.0 if is_medium else (1 + np.abs(ref_p).max()) * F.RAY_EPSILON                      # :275-276
    total_dist = 0.0
    si = _no_hit()
    needs = True
    active = True
    while active:
        remaining = dist * (1.0 - SHADOW_EPSILON) - total_dist                                  # :283
        maxt = remaining
        M.add(remaining / dist, B_T, "remaining distance at 0")
        if not remaining > 0:                                                                   # :285-287
            break
        escaped, active_medium = False, medium is not None
        active_surface = not active_medium
        if active_medium:
            mi = medium.sample_interaction(o, d, mint, maxt, rng.next_1d(), channel, M)         # :294
            if mi.t != INF:
                maxt = min(mi.t, remaining)                                                     # :295
            if needs:
                si = scene.ray_intersect(o, d, mint, maxt, M)                                   # :296-298
            if si.valid:
                M.add(mi.ts / si.t - 1, B_T, "free flight at the surface")
            if _si_t(si) < mi.t:                                                                # :300
                mi.t = INF
            needs = False
            if medium.spectral:                                                                 # :305-311
                t = min(remaining, min(mi.t, _si_t(si))) - mi.mint
                tr = np.exp(-t * mi.comb)
                ff = tr if (_si_t(si) < mi.t or mi.t > remaining) else tr * mi.comb
                T = T * _tr_weight(tr, ff, channel)
            if mi.t > remaining and mi.t != INF:                                                # :314
                total_dist = dist
            if mi.t > remaining:                                                                # :315
                mi.t = INF
            escaped = mi.t == INF
            active_medium = not escaped
            if active_medium:                                                                   # :322-333, sigma_n = 0
                total_dist += mi.t
                o, mint = mi.p, 0.0
                if si.valid:
                    si.t = si.t - mi.t
                T = T * 0.0
        if active_surface and needs:                                                            # :337-340
            si = scene.ray_intersect(o, d, mint, maxt, M)
            needs = False
        active_surface = active_surface or escaped                                              # :341
        if active_surface:
            total_dist += _si_t(si)                                                             # :342
        active_surface = active_surface and si.valid and not active_medium                     # :344
        if active_surface:
            _count_pane(scene.bsdfs[si.mesh])
            T = T * null_transmission(scene.bsdfs[si.mesh], si, M)                              # :346-349
            o, mint = si.p, (1 + np.abs(si.p).max()) * F.RAY_EPSILON                            # :353
            needs = True
        active = active and (active_medium or active_surface) and bool(T.any())                 # :358
        if active_surface and media.is_transition(si):                                          # :361-364
            medium = media.target(si, d, M)
    return T * emitter_val, d, pdf, delta


def evaluate_direct_light(scene, media, si_ref, medium, ray, si_ray, channel, rng, M):
    """volpath.cpp:370-465 -> (transmittance * emitter_val, emitter_pdf)"""
    o, d, mint, maxt = ray
    emitter_val, emitter_pdf = np.zeros(3), 0.0
    needs = False
    T = np.ones(3)
    si = si_ray
    active = True
    while active:
        escaped, active_medium = False, medium is not None
        active_surface = not active_medium
        if active_medium:
            mi = medium.sample_interaction(o, d, mint, maxt, rng.next_1d(), channel, M)         # :391
            if mi.t != INF:
                maxt = mi.t
            if needs:
                si = scene.ray_intersect(o, d, mint, maxt, M)
            if si.valid:
                M.add(mi.ts / si.t - 1, B_T, "free flight at the surface")
            if _si_t(si) < mi.t:                                                                # :397
                mi.t = INF
            if medium.spectral:                                                                 # :401-405
                tr, pdf = Medium.eval_tr_and_pdf(mi, _si_t(si))
                T = T * _tr_weight(tr, pdf, channel)
            needs = False
            escaped = mi.t == INF
            active_medium = not escaped
            if active_medium:                                                                   # :411-420, sigma_n = 0
                o, mint = mi.p, 0.0
                if si.valid:
                    si.t = si.t - mi.t
                T = T * 0.0
        if active_surface and needs:                                                            # :424-426
            si = scene.ray_intersect(o, d, mint, maxt, M)
            needs = False
        active_surface = active_surface or escaped
        emitter = scene.emitter_of(si) if active_surface else None                              # :430-440
        if emitter is not None:
            emitter_val = scene.emitter_eval(emitter, si)
            emitter_pdf = F._hit_emitter_pdf(scene, si_ref, si, emitter, False, M)
            if si.valid and isinstance(emitter, F.AreaEmitter):
                M.add(abs(float((si.p - si_ref.p) @ si.sh_n)) / max(1.0, np.abs(si_ref.p).max()), B_OFFSET, "offset from the light's plane")
            active = active_surface = active_medium = False
        active_surface = active_surface and si.valid and not active_medium                     # :442
        if active_surface:
            T = T * null_transmission(scene.bsdfs[si.mesh], si, M)
            o, mint, maxt = si.p, (1 + np.abs(si.p).max()) * F.RAY_EPSILON, INF                 # :452
            needs = True
        active = active and (active_medium or active_surface) and bool(T.any())                 # :456
        if active_surface and media.is_transition(si):
            medium = media.target(si, d, M)
    return T * emitter_val, emitter_pdf


def _is_null_lobe(bsdf, wi, wo, delta):
    """BSDFFlags::Null of the sampled lobe: the pass-through of null, mask and thindielectric (wo = -wi exactly)"""
    return delta and isinstance(bsdf, (N.Null, N.Mask, N.ThinDielectric)) and np.array_equal(wo, -np.asarray(wi, np.float64))


def volpath_sample(scene, media, ray, rng, max_depth=-1, rr_depth=5, hide_emitters=False, stats=None):
    """VolumetricPathIntegrator::sample, volpath.cpp:60-257 -> (L[3], valid, n_draws, margin)"""
    M, acc = Margin(), F._Acc()
    n0 = rng.count
    o, d, mint, maxt = ray
    tp, eta = np.ones(3), 1.0
    medium = media.start
    specular_chain = not hide_emitters                                                          # :60
    depth, valid_ray = 0, False
    x = rng.next_1d() * 3                                                                       # :66
    channel = min(int(x), 2)
    channel_margin = x - round(x)
    si = _no_hit()
    needs = True
    active = True
    md, rd = max_depth & 0xffffffff, rr_depth & 0xffffffff
    st = stats if stats is not None else {}

    def count(key):
        st[key] = st.get(key, 0) + 1
    while True:
        active = active and bool(tp.any())                                                      # :79
        q = min(tp.max() * eta * eta, 0.95)
        perform_rr = depth > rd
        u = rng.next_1d()                                                                       # :82, every bounce
        if perform_rr and active:
            M.add(u - q, B_LOBE, "russian roulette")
        active = active and (u < q or not perform_rr)
        if perform_rr:
            tp = tp * (1.0 / q)
        if not active or depth >= md:                                                           # :85-87
            break
        act_ms, escaped, active_medium = False, False, medium is not None
        active_surface = not active_medium
        if active_medium:
            M.add(channel_margin, B_CDF * 3, "channel choice")
            mi = medium.sample_interaction(o, d, mint, maxt, rng.next_1d(), channel, M)         # :105
            if mi.t != INF:
                maxt = mi.t                                                                     # :106
            if needs:
                si = scene.ray_intersect(o, d, mint, maxt, M)                                   # :107-109
            needs = False
            if si.valid:
                M.add(mi.ts / si.t - 1, B_T, "free flight at the surface")
            if _si_t(si) < mi.t:                                                                # :112
                mi.t = INF
            if medium.spectral:                                                                 # :113-117
                tr, pdf = Medium.eval_tr_and_pdf(mi, _si_t(si))
                tp = tp * _tr_weight(tr, pdf, channel)
            escaped = mi.t == INF                                                               # :119-120
            active_medium = not escaped
            rng.next_1d()                                                                       # :123: sigma_n = 0, never a null event
            act_ms = active_medium
            if act_ms:
                depth += 1                                                                      # :133
        active = active and depth < md                                                          # :137
        act_ms = act_ms and active
        if act_ms:
            count("medium_scatter")
            if medium.spectral:                                                                 # :147-151
                tp = tp * (mi.sigma_s * mi.comb[channel] / mi.sigma_t[channel])
            else:
                tp = tp * (mi.sigma_s / mi.sigma_t)
            valid_ray = True                                                                    # :158-160
            specular_chain = not medium.sample_emitters
            if medium.sample_emitters:                                                          # :162-167
                emitted, ed, epdf, _ = sample_emitter(scene, media, mi.p, True, medium, channel, rng, M)
                if epdf != 0:
                    acc.add(tp * medium.phase.eval(d, ed) * emitted)
            wo, _ = medium.phase.sample(d, rng.next_2d(), M)                                    # :171-175
            o, d, mint, maxt = mi.p, wo, 0.0, INF
            needs = True
        active_surface = active_surface or escaped                                              # :179
        if not active:
            active_surface = False
        if active_surface and needs:                                                            # :180-182
            si = scene.ray_intersect(o, d, mint, maxt, M)
        if active_surface:                                                                      # :186-191
            emitter = scene.emitter_of(si)
            if specular_chain and emitter is not None:
                acc.add(tp * scene.emitter_eval(emitter, si))
        active_surface = active_surface and si.valid                                            # :193
        if active_surface:
            bsdf = scene.bsdfs[si.mesh]
            if bsdf.smooth and ((depth + 1) & 0xffffffff) < md:                                 # :198-212
                emitted, ed, epdf, edelta = sample_emitter(scene, media, si.p, False, medium, channel, rng, M)
                if epdf != 0:
                    wo = si.to_local(ed)
                    bsdf_val, bsdf_pdf = bsdf.eval(si.wi, wo, M), bsdf.pdf(si.wi, wo, M)
                    acc.add(tp * bsdf_val * mis_weight(epdf, 0.0 if edelta else bsdf_pdf) * emitted)
            s1 = rng.next_1d()                                                                  # :215-216
            s2 = rng.next_2d()
            wo, bpdf, beta, bdelta, bweight = bsdf.sample(si.wi, s1, s2, M)
            tp = tp * bweight                                                                   # :219-220
            eta *= beta
            new_d = si.to_world(wo)
            new_ray = si.spawn_ray(new_d)                                                       # :222-224
            needs = True
            failed = bpdf == 0 and not np.any(bweight)                                          # (sampled_type = 0)
            is_null = (not failed) and _is_null_lobe(bsdf, si.wi, wo, bdelta)
            if is_null:
                count("null_pass")
            sampled_delta, sampled_smooth = (not failed) and bdelta, (not failed) and not bdelta
            if not is_null:                                                                     # :226-231
                depth += 1
                valid_ray = True
                if sampled_delta:
                    specular_chain = True
            if sampled_smooth:
                specular_chain = False
            add_emitter = (not sampled_delta) and bool(tp.any()) and depth < md                 # :233-234
            si_new = si
            if add_emitter:                                                                     # :238-247
                si_new = scene.ray_intersect(*new_ray, M)
                needs = False
                emitted, emitter_pdf = evaluate_direct_light(scene, media, si, medium, new_ray, _copy_hit(si_new), channel, rng, M)
                if emitter_pdf != 0:
                    acc.add(mis_weight(bpdf, emitter_pdf) * tp * emitted)
            if media.is_transition(si):                                                         # :249-250
                medium = media.target(si, new_d, M)
                count("transition_in" if medium is not None else "transition_out")
            si = si_new                                                                         # :252
            o, d, mint, maxt = new_ray
        active = active and (active_surface or active_medium)                                   # :254
    M.scale = acc.biggest
    return acc.L, valid_ray, rng.count - n0, M


def _copy_hit(si):
    """evaluate_direct_light changes its copy of the hit (si.t -= mi.t), sample() keeps its own"""
    c = F.Hit()
    c.__dict__.update(si.__dict__)
    return c


def integrator_fn(media, kw):
    return lambda scene, ray, rng, stats: volpath_sample(scene, media, ray, rng, stats=stats, **kw)


# ================================================================ jobs shared by the CPU and the GPU tier
# name -> (scene, integrator arguments, base seed): 64 x 48, 3 camera samples, the Cornell sensor, box filter — f64_integrators.JOB_*
JOBS = {
    "fog-cornell":       ("fog-cornell", dict(), 50000),
    "fog-cornell-hide":  ("fog-cornell", dict(hide_emitters=True), 50000),
    "smoke-cube-gray":   ("smoke-cube-gray", dict(max_depth=-1, rr_depth=2), 50000),
    "milk-block":        ("milk-block", dict(max_depth=6), 50000),
    "bubble-cube":       ("bubble-cube", dict(max_depth=8), 50000),
    "fog-panes":         ("fog-panes", dict(max_depth=6), 50000),              # null transmission of mask and thindielectric in the walks
    "cornell-nomedia":   ("cornell-nomedia", dict(max_depth=3, rr_depth=2), 50000),     # no media at all: the surface half of sample() alone
}


def job_scene(scenes, which, spp, seed):
    """-> (api scene: description only, sensor); scenes.volpath_scene names the builders"""
    scene = scenes.volpath_scene(which, light_drop=F.LIGHT_DROP)
    return scene.build(-1), scenes.cornell_sensor(F.JOB_W, F.JOB_H, spp, seed=seed, rfilter="box", sensor=dict(medium=scene.start_medium))
