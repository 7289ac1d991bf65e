"""The aov integrator (src/integrators/aov.cpp) without a GPU: channel grammar and aov_names(), the XML front-end, the leaf
arithmetic of csrc/miw/aov.h on the host build against the float64 restatement tests/f64_aov.py, the portable N-channel film
replay of csrc/miw/film_gather_n.h against the five-channel one, Film development with AOV channels, the C ABI record, and the
register / scratch budgets of the kernels (device/aov_kernel.h) from the compiler's remarks for gfx950."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import f64_aov as F
from test_independent_integrators import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. grammar and aov_names()
@pytest.mark.parametrize("typ", F.TYPES)
def test_every_type_names_its_channels(native, typ):
    integ = native.AOVIntegrator(aovs="c:%s" % typ)
    assert integ.aov_names() == F.aov_names([("c", typ)])
    cfg = integ.aov_cfg()
    assert cfg.struct_size == C.sizeof(type(cfg)) and cfg.n_types == 1 and cfg.types[0] == F.TYPES.index(typ) and cfg.nested == 0
    assert native.device_lib().mi_aov_channel_count(C.byref(cfg)) == 5 + F.CHANNELS[typ]


def test_mixed_lists_delimiters_and_a_child(native):
    spec = [("dd", "depth"), ("nn", "sh_normal"), ("pp", "position"), ("tex", "uv"), ("g", "geo_normal"), ("a", "dp_du"), ("b", "dp_dv"), ("x", "duv_dx"), ("y", "duv_dy")]
    for sep in (",", " ", ", ", " ,  "):
        integ = native.AOVIntegrator(aovs=sep.join("%s:%s" % s for s in spec))
        assert integ.aov_names() == F.aov_names(spec)
    integ = native.AOVIntegrator(aovs="dd:depth,nn:sh_normal", nested=native.PathIntegrator(max_depth=4), name="img")
    assert integ.aov_names() == ["dd", "nn.X", "nn.Y", "nn.Z", "img.R", "img.G", "img.B", "img.A"]
    cfg = integ.aov_cfg()
    assert (cfg.n_types, cfg.nested, cfg.child.integrator, cfg.child.max_depth, cfg.child.rr_depth) == (2, 1, 0, 4, 5)
    assert native.device_lib().mi_aov_channel_count(C.byref(cfg)) == 5 + 4 + 4
    direct = native.AOVIntegrator(aovs="", nested=native.DirectIntegrator(emitter_samples=2, bsdf_samples=0), name="d")
    assert direct.aov_names() == ["d.R", "d.G", "d.B", "d.A"]
    cfg = direct.aov_cfg()
    assert (cfg.n_types, cfg.nested, cfg.child.integrator, cfg.child.emitter_samples, cfg.child.bsdf_samples) == (0, 2, 1, 2, 0)


def test_grammar_refusals(native):
    with pytest.raises(RuntimeError, match='Invalid AOV type "colour"'):
        native.AOVIntegrator(aovs="c:colour")
    with pytest.raises(RuntimeError, match="require <name>:<type> pair"):
        native.AOVIntegrator(aovs="depth")
    with pytest.raises(RuntimeError, match="more than one nested integrator"):
        native.AOVIntegrator(aovs="d:depth", nested=[("a", native.PathIntegrator()), ("b", native.DirectIntegrator())])
    with pytest.raises(RuntimeError, match="nested moment or aov"):
        native.AOVIntegrator(aovs="d:depth", nested=native.AOVIntegrator(aovs="e:depth"))
    with pytest.raises(RuntimeError, match="more than 32"):
        native.AOVIntegrator(aovs=",".join("c%d:depth" % i for i in range(33)))
    # duplicate channels, also against R, G, B: Film::prepare (hdrfilm.cpp:190-199)
    film = native.Film(width=4, height=3)
    for names in (["d", "d"], ["R"], ["n.X", "n.Y", "n.X"]):
        with pytest.raises(RuntimeError, match="duplicate channel name"):
            film.set_channels(["X", "Y", "Z", "A", "W"] + names)
    film.set_channels(["X", "Y", "Z", "A", "W", "d", "n.X"])
    # the C ABI's own refusals need no context
    L = native.device_lib()
    cfg = native.aov_cfg(["depth"])
    assert L.mi_aov_channel_count(C.byref(cfg)) == 6
    cfg.types[0] = 9
    assert L.mi_aov_channel_count(C.byref(cfg)) == 0
    cfg = native.aov_cfg(["depth"]); cfg.n_types = 33
    assert L.mi_aov_channel_count(C.byref(cfg)) == 0
    cfg = native.aov_cfg(["depth"]); cfg.struct_size += 4
    assert L.mi_aov_channel_count(C.byref(cfg)) == 0
    job = native.PathIntegrator().render_job(native.Sensor(native.Film(width=8, height=8), native.Sampler(sample_count=1)))
    assert L.mi_render_aov(None, C.byref(job.cfg), C.byref(cfg), None) == -1


# ---------------------------------------------------------------- 2. XML
XML = """<scene version="2.0.0">
  <integrator type="aov">
    <string name="aovs" value="dd:depth, nn:sh_normal"/>
    <integrator type="path" name="img"><integer name="max_depth" value="3"/></integrator>
  </integrator>
  <sensor type="perspective"><film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="8"/></film></sensor>
</scene>"""


def test_xml_round_trip(native):
    scene, sensor, integ = native.load_string(XML)
    assert integ.aov_names() == ["dd", "nn.X", "nn.Y", "nn.Z", "img.R", "img.G", "img.B", "img.A"]
    cfg = native.AOVIntegrator.aov_cfg(integ)
    assert (cfg.n_types, cfg.types[0], cfg.types[1], cfg.nested, cfg.child.max_depth) == (2, 0, 4, 1, 3)
    _, _, bare = native.load_string(XML.replace('<integrator type="path" name="img"><integer name="max_depth" value="3"/></integrator>', ""))
    assert bare.aov_names() == ["dd", "nn.X", "nn.Y", "nn.Z"]
    with pytest.raises(RuntimeError, match="more than one nested integrator"):
        native.load_string(XML.replace("</integrator>\n  </integrator>", '</integrator><integrator type="direct" name="b"/>\n  </integrator>'))
    with pytest.raises(RuntimeError, match="Invalid AOV type"):
        native.load_string(XML.replace("nn:sh_normal", "nn:normal"))


# ---------------------------------------------------------------- 3. aov_fill and the partials on the host build
def _host_fill(native, shape, geom, has_tc, ray, hit, valid, types):
    t = (C.c_uint8 * len(types))(*[F.TYPES.index(x) for x in types])
    n = sum(F.CHANNELS[x] for x in types)
    out, pt = np.full(n, np.nan, np.float32), np.zeros(6, np.float32)
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    g, r, h = (np.ascontiguousarray(a, np.float32) for a in (geom, ray, hit))
    got = native.host_lib().mih_aov_fill(shape, fp(g), int(has_tc), fp(r), fp(h), int(valid), t, len(types),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), pt.ctypes.data_as(C.POINTER(C.c_float)))
    assert got == n, native._err()
    return out, pt


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64).reshape(-1)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max() / scale
    print("%s: max |got - want| / max |want| = %.3g" % (what, err))
    assert err <= RTOL, (what, got, want)


def _matrix(rng, uniform):
    a, b, c = rng.uniform(-3, 3, 3)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    s = np.diag([1.7, 1.7, 1.7] if uniform else [0.6, 2.3, 1.0])
    M = np.eye(4); M[:3, :3] = rx @ ry @ rz @ s; M[:3, 3] = rng.uniform(-2, 2, 3)
    return M.astype(np.float32)


def _inverse(M):
    return np.linalg.inv(M.astype(np.float64)).T.reshape(-1).astype(np.float32)       # column-major


@pytest.mark.parametrize("case", ["triangle", "triangle_uv", "triangle_uv_degenerate", "rectangle", "sphere", "sphere_flipped"])
def test_aov_fill_against_float64(native, case):
    rng = np.random.default_rng(sum(map(ord, case)))
    types = F.TYPES
    for trial in range(8):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        if case.startswith("triangle"):
            P = rng.uniform(-2, 2, (3, 3)).astype(np.float32)
            tc = None
            if case != "triangle":
                tc = rng.uniform(0, 1, 6).astype(np.float32)
                if case.endswith("degenerate"):
                    tc[4:6] = tc[0:2] + 2 * (tc[2:4] - tc[0:2])          # the three uv points on a line (exact in float32 for these): det == 0
                    tc = np.round(tc * 64).astype(np.float32) / 64
                    tc[4:6] = tc[0:2] + 2 * (tc[2:4] - tc[0:2])
                    assert (tc[2] - tc[0]) * (tc[5] - tc[1]) - (tc[3] - tc[1]) * (tc[4] - tc[0]) == 0
            b1, b2 = rng.uniform(0, .5, 2)
            t = rng.uniform(.5, 4)
            hit = [t, b1, b2]
            want = F.triangle(P[0:1], P[1:2], P[2:3], [b1], [b2], [t], tc=None if tc is None else tc[None])
            geom = np.concatenate([P.reshape(-1)] + ([] if tc is None else [tc]))
            got, pt = _host_fill(native, 0, geom, tc is not None, np.concatenate([np.zeros(3), d]), hit, True, types)
        elif case == "rectangle":
            M = _matrix(rng, uniform=False)
            local = np.append(rng.uniform(-.9, .9, 2), 0)
            target = M[:3, :3].astype(np.float64) @ local + M[:3, 3]
            o = target - d * rng.uniform(1, 3)
            want = F.rectangle(M.T.reshape(-1), o[None].astype(np.float32), d[None].astype(np.float32))
            got, pt = _host_fill(native, 1, np.concatenate([M.T.reshape(-1), _inverse(M)]), False, np.concatenate([o, d]), [0, 0, 0], True, types)
        else:
            M = _matrix(rng, uniform=True)
            center, radius, flip = M[:3, 3], 1.7, case.endswith("flipped")
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            t = rng.uniform(1, 3)
            o = (center + radius * n - d * t).astype(np.float32)
            want = F.sphere(M.T.reshape(-1), center, radius, flip, o[None], d[None].astype(np.float32), [t])
            geom = np.concatenate([M.T.reshape(-1), _inverse(M), center, [radius, float(flip)]])
            got, pt = _host_fill(native, 2, geom, False, np.concatenate([o, d]), [t, 0, 0], True, types)
        full = F.fill(want, types)
        k = 0
        for typ in types:
            c = F.CHANNELS[typ]
            if typ in ("duv_dx", "duv_dy"):
                assert (got[k:k + c].view(np.uint32) == 0).all()          # exactly +0
            else:
                _close(got[k:k + c], full[0, k:k + c], "%s %s" % (case, typ))
            k += c
        _close(pt[:3], want["dp_du"], case + " dp_du"); _close(pt[3:], want["dp_dv"], case + " dp_dv")
        if case == "triangle_uv_degenerate":                              # mesh.cpp:506: the coordinate_system() tangents stay
            plain = F.triangle(P[0:1], P[1:2], P[2:3], [b1], [b2], [t])
            _close(pt[:3], plain["dp_du"], "degenerate uv keeps dp_du"); _close(pt[3:], plain["dp_dv"], "degenerate uv keeps dp_dv")
        # an invalid interaction: exactly zero in every channel
        if case.startswith("triangle"):
            inv, _ = _host_fill(native, 0, geom, tc is not None, np.concatenate([np.zeros(3), d]), hit, False, types)
            assert (inv.view(np.uint32) << 1 == 0).all() and len(inv) == 22


# ---------------------------------------------------------------- 4. the portable N-channel replay
def test_n_channel_replay_equals_the_five_channel_replay(native):
    W, H, SPP = 70, 45, 3
    sensor = native.Sensor(native.Film(width=W, height=H), native.Sampler(sample_count=SPP, seed=7), fov=40.0)
    job = native.PathIntegrator(block_size=32).render_job(sensor)
    cfg = job.cfg
    assert (cfg.block_size, cfg.filter_border) == (32, 2) and cfg.filter_radius == 2.0
    nbx, nby = 3, 2
    lanes = nbx * nby * 1024
    rng = np.random.default_rng(3)
    q = np.arange(1024)
    x = (q & 1) | ((q >> 1) & 2) | ((q >> 2) & 4) | ((q >> 3) & 8) | ((q >> 4) & 16)
    y = ((q >> 1) & 1) | ((q >> 2) & 2) | ((q >> 3) & 4) | ((q >> 4) & 8) | ((q >> 5) & 16)
    pos = np.zeros((lanes, SPP, 2), np.float32)
    for b in range(nbx * nby):
        px, py = (b % nbx) * 32 + x, (b // nbx) * 32 + y
        pos[b * 1024:(b + 1) * 1024, :, 0] = px[:, None] + rng.random((1024, SPP), np.float32)
        pos[b * 1024:(b + 1) * 1024, :, 1] = py[:, None] + rng.random((1024, SPP), np.float32)
    val = rng.uniform(-1, 3, (lanes, SPP, 4)).astype(np.float32)
    pos[rng.random((lanes, SPP)) < .02, 0] = np.nan                      # rejected samples
    film5, filmn = np.zeros((H, W, 5), np.float32), np.zeros((H, W, 5), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert native.host_lib().mih_film_replay_pair(C.byref(cfg), fp(pos), fp(val), fp(film5), fp(filmn)) == 0, native._err()
    assert np.abs(film5).sum() > 0 and (film5[..., 4] > 0).all()
    assert np.array_equal(film5.view(np.uint32), filmn.view(np.uint32))


# ---------------------------------------------------------------- 5. develop
def test_develop_with_aov_channels(native, tmp_path):
    film = native.Film(width=4, height=3, component_format="float32")
    rng = np.random.default_rng(5)
    data = rng.uniform(.1, 2, (3, 4, 7)).astype(np.float32)
    data[0, 0, 4] = 0                                                    # a texel without weight develops to 0
    film.set_channels(["X", "Y", "Z", "A", "W", "dd", "nn.X"], data)
    assert np.array_equal(film.data((3, 4, 7)), data)
    names, img = film.bitmap()
    assert names == ["R", "G", "B", "A", "dd", "nn.X"] and img.shape == (3, 4, 6)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(data[..., 4] != 0, np.float32(1) / data[..., 4], np.float32(0)).astype(np.float32)
    for k, src in ((3, 3), (4, 5), (5, 6)):
        assert np.array_equal(img[..., k], data[..., src] * inv)        # A and the AOV channels: divided by W, W dropped
    M = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
    want = (data[..., :3].astype(np.float64) * inv[..., None]) @ M.T
    assert np.allclose(img[..., :3], want, rtol=1e-5, atol=1e-6)
    assert np.allclose(film.develop(), img[..., :3], rtol=0, atol=0)    # the RGB view of the same film
    path = film.develop_to(tmp_path / "aov.exr")
    raw = open(path, "rb").read()
    for nm in names:
        assert nm.encode() + b"\0" in raw[:600]
    pfm = native.Film(width=4, height=3, file_format="pfm")
    pfm.set_channels(["X", "Y", "Z", "A", "W", "dd"], np.ones((3, 4, 6), np.float32))
    with pytest.raises(RuntimeError, match="cannot be written as PFM"):
        pfm.develop_to(tmp_path / "aov.pfm")


# ---------------------------------------------------------------- C ABI layout
def test_mi_aov_cfg_layout(native, tmp_path):
    from mitsuba2_amd import _capi
    T = _capi.mi_aov_cfg
    assert C.sizeof(T) == 76 and C.sizeof(_capi.mi_sample_cfg) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("struct_size", 0), ("n_types", 4), ("types", 8), ("nested", 40), ("child", 44)]
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx:                                                              # ... and the compiler's view of include/miwave.h
        src = tmp_path / "layout.cpp"
        src.write_text('#include <cstdio>\n#include <cstddef>\n#include "%s"\nint main() { printf("%%zu %%zu %%zu %%zu %%zu %%zu %%d", sizeof(mi_aov_cfg), '
                       'offsetof(mi_aov_cfg, n_types), offsetof(mi_aov_cfg, types), offsetof(mi_aov_cfg, nested), offsetof(mi_aov_cfg, child), '
                       'sizeof(mi_sample_cfg), MI_AOV_MAX_TYPES); }\n' % os.path.join(ROOT, "include", "miwave.h"))
        exe = tmp_path / "layout"
        subprocess.run([cxx, str(src), "-o", str(exe)], check=True)
        assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["76", "4", "8", "40", "44", "32", "32"]
    assert [_capi.MI_AOV[t] for t in F.TYPES] == list(range(9)) and _capi.MI_AOV_CHANNELS == F.CHANNELS
    for sym in ("mi_render_aov", "mi_aov_channel_count"):
        assert sym in _capi.MI_SYMBOLS and hasattr(native.device_lib(), sym)


# ---------------------------------------------------------------- 6. register and scratch budgets
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-gpu-flush-denormals-to-zero", "-c", "-Rpass-analysis=kernel-resource-usage"]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("defs", [[], ["-DMIW_SPECTRAL=1"]], ids=["scalar_rgb", "scalar_spectral"])
def test_aov_kernel_budgets(tmp_path, defs):
    """What the compiler reports for csrc/miwave_aov.hip, the unit mitsuba2_amd/build.py compiles, pinned as upper bounds. k_aov_samples
    carries no scratch in any instantiation: the packet route fits 128 registers (four wavefronts per SIMD), the tree routes 168 (three,
    MIW_TREE_WAVES) — the classes k_sample_rays is compiled for."""
    out = subprocess.run([HIPCC] + FLAGS + defs + [os.path.join(ROOT, "mitsuba2_amd", "csrc", "miwave_aov.hip"), "-o", str(tmp_path / "aov.o")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = blk.split()[0]
        m = re.match(r"_Z13k_aov_samplesILi(\d)ELb([01])EE", name)
        key = ("samples", int(m.group(1)), int(m.group(2))) if m else ("finish",) if name.startswith("_Z12k_aov_finish") else \
            ("merge",) if name.startswith("_Z16k_aov_film_merge") else ("film",) if name.startswith("_Z10k_aov_film") else None
        if key:
            val = lambda k: int(re.search(re.escape(k) + r": (\d+)", blk).group(1))
            res[key] = dict(vgprs=val("VGPRs"), scratch=val("ScratchSize [bytes/lane]"), spilled=val("VGPRs Spill"), waves=val("Occupancy [waves/SIMD]"))
    print(res)
    small = [("film",), ("merge",)] + ([] if defs else [("finish",)])
    assert sorted(res) == sorted([("samples", 1, 0), ("samples", 0, 0), ("samples", 0, 1)] + small), sorted(res)
    for key, r in res.items():
        assert r["scratch"] == 0 and r["spilled"] == 0, (key, r)
    assert res[("samples", 1, 0)]["waves"] == 4 and res[("samples", 1, 0)]["vgprs"] <= PIN_PACKET
    for key in (("samples", 0, 0), ("samples", 0, 1)):
        assert res[key]["waves"] == 3 and res[key]["vgprs"] <= PIN_TREE, (key, res[key])
    for key in small:
        assert res[key]["waves"] == 8 and res[key]["vgprs"] <= PIN_SMALL, (key, res[key])


# what hipcc reports for this source, both variants alike: k_aov_samples<packets> 101 VGPRs, <tree> 140, <tree, analytic> 141; k_aov_finish 18,
# k_aov_film 32, k_aov_film_merge 26 — pinned as upper bounds
PIN_PACKET, PIN_TREE, PIN_SMALL = 101, 141, 32
