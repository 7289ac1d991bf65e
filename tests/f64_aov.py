"""float64 numpy restatement of what the aov integrator reads off a surface interaction (src/integrators/aov.cpp:166-219):
t, p, uv, n, sh_frame.n and the partials dp_du, dp_dv of a mesh triangle (src/librender/mesh.cpp:484-545), a rectangle
(src/shapes/rectangle.cpp:86-90, 196-203) and a sphere (src/shapes/sphere.cpp:356-397). Written from those lines, independent of
csrc/miw/aov.h; vectorised over hits. duv_dx / duv_dy are zero (include/mitsuba/render/interaction.h:593 clears them, and only
si.bsdf(ray) -> compute_uv_partials would fill them, which aov.cpp never calls)."""
import numpy as np

TYPES = ["depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "duv_dx", "duv_dy"]
CHANNELS = dict(depth=1, position=3, uv=2, geo_normal=3, sh_normal=3, dp_du=3, dp_dv=3, duv_dx=2, duv_dy=2)
SUFFIX = {1: [""], 2: [".U", ".V"], 3: [".X", ".Y", ".Z"]}


def aov_names(spec, children=()):
    """aov.cpp:83-150 for a list of (name, type) pairs and child names"""
    names = []
    for name, typ in spec:
        names += [name + s for s in SUFFIX[CHANNELS[typ]]]
    for c in children:
        names += [c + s for s in (".R", ".G", ".B", ".A")]
    return names


def _norm(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def coordinate_system(n, sign=None):
    """include/mitsuba/core/vector.h: coordinate_system (Duff et al.). The construction BRANCHES on the sign of n.z and is discontinuous
    there; `sign` overrides the branch (see triangle())"""
    sign = np.copysign(1.0, n[..., 2]) if sign is None else sign
    a = -1.0 / (sign + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    s = np.stack([n[..., 0] * n[..., 0] * a * sign + 1.0, b * sign, -sign * n[..., 0]], -1)
    t = np.stack([b, n[..., 1] * n[..., 1] * a + sign, -n[..., 1]], -1)
    return s, t


def triangle(p0, p1, p2, b1, b2, t, tc=None, vn=None):
    """mesh.cpp:484-545. p*: [n, 3]; b1, b2, t: [n]; tc: [n, 6] texture coordinates of the face or None; vn: [n, 9] or None"""
    p0, p1, p2 = (np.asarray(x, np.float64) for x in (p0, p1, p2))
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    b0 = 1.0 - b1 - b2
    dp0, dp1 = p1 - p0, p2 - p0
    p = p0 * b0[:, None] + p1 * b1[:, None] + p2 * b2[:, None]
    n = _norm(np.cross(dp0, dp1))
    uv = np.stack([b1, b2], -1)
    # The branch of coordinate_system() is the reference's own float32 decision: for a face whose normal lies in the xy plane up to
    # rounding (the equator faces of an icosphere) the sign of n.z IS rounding, and a float64 normal may take the other branch — a
    # different, equally valid tangent pair. So the sign is taken from the float32 cross product the scalar_rgb reference forms,
    # fmsub(dp0.x, dp1.y, dp0.y * dp1.x) of the float32 edges (exact here: the product of two float32 is exact in float64, and a
    # correctly rounded difference keeps its sign); everything else stays float64.
    e0, e1 = (p1.astype(np.float32) - p0.astype(np.float32)), (p2.astype(np.float32) - p0.astype(np.float32))
    z32 = e0[:, 0].astype(np.float64) * e1[:, 1].astype(np.float64) - (e0[:, 1] * e1[:, 0]).astype(np.float64)
    dp_du, dp_dv = coordinate_system(n, np.where(z32 < 0, -1.0, 1.0))
    if tc is not None:
        tc = np.asarray(tc, np.float64)
        uv0, uv1, uv2 = tc[:, 0:2], tc[:, 2:4], tc[:, 4:6]
        uv = uv0 * b0[:, None] + uv1 * b1[:, None] + uv2 * b2[:, None]
        duv0, duv1 = uv1 - uv0, uv2 - uv0
        det = duv0[:, 0] * duv1[:, 1] - duv0[:, 1] * duv1[:, 0]
        ok = det != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            du = (dp0 * duv1[:, 1:2] - dp1 * duv0[:, 1:2]) * inv[:, None]
            dv = (-dp0 * duv1[:, 0:1] + dp1 * duv0[:, 0:1]) * inv[:, None]
        dp_du = np.where(ok[:, None], du, dp_du)
        dp_dv = np.where(ok[:, None], dv, dp_dv)
    sh_n = n
    if vn is not None:
        vn = np.asarray(vn, np.float64)
        sh_n = _norm(vn[:, 0:3] * b0[:, None] + vn[:, 3:6] * b1[:, None] + vn[:, 6:9] * b2[:, None])
    return dict(t=np.asarray(t, np.float64), p=p, uv=uv, n=n, sh_n=sh_n, dp_du=dp_du, dp_dv=dp_dv)


def _xf_vec(m, v):
    """column-major 4x4 times a direction"""
    M = np.asarray(m, np.float64).reshape(4, 4).T
    return np.asarray(v, np.float64) @ M[:3, :3].T


def _xf_point(m, v):
    M = np.asarray(m, np.float64).reshape(4, 4).T
    return np.asarray(v, np.float64) @ M[:3, :3].T + M[:3, 3]


def rectangle(to_world, o, d):
    """rectangle.cpp:86-90, 139-158, 196-203 for rays (o, d) [n, 3] that hit it"""
    to_object = np.linalg.inv(np.asarray(to_world, np.float64).reshape(4, 4).T).T.reshape(-1)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ol, dl = _xf_point(to_object, o), _xf_vec(to_object, d)
    t = -ol[:, 2] / dl[:, 2]
    local = ol + dl * t[:, None]
    dp_du, dp_dv = _xf_vec(to_world, [2.0, 0, 0]), _xf_vec(to_world, [0, 2.0, 0])
    # m_to_world * Normal3f(0, 0, 1): normals transform by the inverse transpose
    M = np.asarray(to_world, np.float64).reshape(4, 4).T
    n = _norm(np.linalg.inv(M[:3, :3]).T @ np.array([0, 0, 1.0]))
    k = len(o)
    return dict(t=t, p=o + d * t[:, None], uv=np.stack([local[:, 0] * .5 + .5, local[:, 1] * .5 + .5], -1), n=np.tile(n, (k, 1)), sh_n=np.tile(n, (k, 1)),
                dp_du=np.tile(dp_du, (k, 1)), dp_dv=np.tile(dp_dv, (k, 1)))


def sphere(to_world, center, radius, flip, o, d, t):
    """sphere.cpp:356-397 for rays (o, d) and their hit distances t"""
    to_object = np.linalg.inv(np.asarray(to_world, np.float64).reshape(4, 4).T).T.reshape(-1)
    o, d, t = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(t, np.float64)
    center = np.asarray(center, np.float64)
    n = _norm(o + d * t[:, None] - center)
    p = n * radius + center
    local = _xf_point(to_object, p)
    rd = np.sqrt(local[:, 0] ** 2 + local[:, 1] ** 2)
    theta = np.arccos(np.clip(local[:, 2] / np.linalg.norm(local, axis=1), -1, 1))       # unit_angle_z of the (radius-scaled) local point's direction
    phi = np.arctan2(local[:, 1], local[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    uv = np.stack([phi / (2 * np.pi), theta / np.pi], -1)
    dp_du = np.stack([-local[:, 1], local[:, 0], np.zeros_like(rd)], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_phi, sin_phi = local[:, 0] / rd, local[:, 1] / rd
    dp_dv = np.stack([local[:, 2] * cos_phi, local[:, 2] * sin_phi, -rd], -1)
    dp_dv = np.where((rd == 0)[:, None], np.array([1.0, 0, 0]), dp_dv)
    dp_du = _xf_vec(to_world, dp_du) * (2 * np.pi)
    dp_dv = _xf_vec(to_world, dp_dv) * np.pi
    if flip:
        n = -n
    return dict(t=t, p=p, uv=uv, n=n, sh_n=n, dp_du=dp_du, dp_dv=dp_dv)


def fill(si, types, valid=True):
    """aov.cpp:166-219: [n, channels] in the order of `types`; all zero for an invalid interaction (:167)"""
    key = dict(depth="t", position="p", uv="uv", geo_normal="n", sh_normal="sh_n", dp_du="dp_du", dp_dv="dp_dv")
    k = len(si["t"])
    cols = []
    for typ in types:
        if typ in ("duv_dx", "duv_dy"):
            cols.append(np.zeros((k, 2)))
        else:
            v = np.asarray(si[key[typ]], np.float64)
            cols.append(v[:, None] if v.ndim == 1 else v)
    out = np.concatenate(cols, 1) if cols else np.zeros((k, 0))
    return out if valid else np.zeros_like(out)


def scene_arrays(desc):
    """numpy views of a mi_scene_desc: vertices, faces, texture coordinates, shape records, analytic records by shape index"""
    V = np.ctypeslib.as_array(desc.vertex_positions, shape=(desc.vertex_count * 3,)).reshape(-1, 3).copy()
    F = np.ctypeslib.as_array(desc.faces, shape=(desc.face_count * 3,)).reshape(-1, 3).copy()
    T = np.ctypeslib.as_array(desc.vertex_texcoords, shape=(desc.vertex_count * 2,)).reshape(-1, 2).copy() if desc.vertex_texcoords else None
    flags = np.array([desc.shapes[i].flags for i in range(desc.shape_count)], np.uint32)
    rects = {desc.rectangles[i].shape: np.array(desc.rectangles[i].to_world[:], np.float32) for i in range(desc.rectangle_count)}
    spheres = {desc.spheres[i].shape: (np.array(desc.spheres[i].to_world[:], np.float32), np.array(desc.spheres[i].center[:], np.float32),
                                       float(desc.spheres[i].radius), bool(desc.spheres[i].flip_normals)) for i in range(desc.sphere_count)}
    return dict(V=V, F=F, T=T, flags=flags, rects=rects, spheres=spheres)


def partials_at(arr, si, o, d):
    """dp_du, dp_dv [n, 3] (float64) of the hits of a mi_ray_intersect result `si` (structured array, _capi.SI_DTYPE) for the rays
    (o, d); rows of misses are zero"""
    n = len(si)
    du, dv = np.zeros((n, 3)), np.zeros((n, 3))
    hit = np.isfinite(si["t"])
    shape = si["shape_index"].astype(np.int64)
    for s in np.unique(shape[hit]):
        m = hit & (shape == s)
        fl = int(arr["flags"][s])
        if fl & 2:
            r = rectangle(arr["rects"][s], o[m], d[m])
        elif fl & 4:
            tw, c, rad, flip = arr["spheres"][s]
            r = sphere(tw, c, rad, flip, o[m], d[m], si["t"][m])
        else:
            f = arr["F"][si["prim_index"][m]]
            tc = None
            if fl & 8:
                tc = np.concatenate([arr["T"][f[:, 0]], arr["T"][f[:, 1]], arr["T"][f[:, 2]]], 1)
            z = np.zeros(m.sum())
            r = triangle(arr["V"][f[:, 0]], arr["V"][f[:, 1]], arr["V"][f[:, 2]], z, z, z, tc=tc)
        du[m], dv[m] = r["dp_du"], r["dp_dv"]
    return du, dv
