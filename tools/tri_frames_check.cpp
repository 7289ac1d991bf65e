// Per-triangle shading frames (miw/shape.h: TriFrame) against the per-hit code they replace — tests/test_tri_frames_cpu.py builds and
// runs this program (host flags of mitsuba2_amd/build.py; once more with -fsanitize=address,undefined).
//
// Three routes per hit, every field of SurfaceInteraction compared by bit pattern (a NaN equals a NaN of any payload):
//   legacy   the statements of compute_surface_interaction as they stood before the split, frozen below;
//   classic  compute_surface_interaction(p0, p1, p2, vn, tc, t, b1, b2, ray_d, si) — tri_frame + the per-hit half;
//   table    tri_frame() of every triangle stored in an array first (what the packet kernels do in LDS), then the per-hit half alone.
// The same for mesh_sample_position: legacy / classic / FaceNormalTable over face_normal() records.
// Prints "mismatches 0" and returns 0 when all agree.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include "../mitsuba2_amd/csrc/miw/shape.h"

using namespace miw;

// ---- the code before the split, verbatim -----------------------------------------------------------------------------
static void legacy_compute_surface_interaction(V3 p0, V3 p1, V3 p2, const float *vn, const float *tc,
                                               float t, float b1, float b2, V3 ray_d, SurfaceInteraction &si) {
    float b0 = 1.f - b1 - b2;
    V3 dp0 = p1 - p0, dp1 = p2 - p0;
    si.t = t;
    si.p = p0 * b0 + p1 * b1 + p2 * b2;
    si.n = normalize(cross(dp0, dp1));
    si.uv = v2(b1, b2);
    V3 dp_du, dp_dv;
    coordinate_system(si.n, dp_du, dp_dv);
    if (tc) {
        const V2 uv0 = v2(tc[0], tc[1]), uv1 = v2(tc[2], tc[3]), uv2 = v2(tc[4], tc[5]);
        si.uv = v2(uv0.x * b0 + uv1.x * b1 + uv2.x * b2, uv0.y * b0 + uv1.y * b1 + uv2.y * b2);
        const V2 duv0 = v2(uv1.x - uv0.x, uv1.y - uv0.y), duv1 = v2(uv2.x - uv0.x, uv2.y - uv0.y);
        const float det = fmsub(duv0.x, duv1.y, duv0.y * duv1.x), inv_det = rcp(det);
        if (det != 0.f) {
            dp_du = fmsub3(dp0, duv1.y, dp1 * duv0.y) * inv_det;
            dp_dv = fnmadd3(dp0, duv1.x, dp1 * duv0.x) * inv_det;
        }
    }
    if (vn) {
        V3 n0 = ld3(vn), n1 = ld3(vn + 3), n2 = ld3(vn + 6);
        si.sh.n = normalize(n0 * b0 + n1 * b1 + n2 * b2);
    } else {
        si.sh.n = si.n;
    }
    si.sh.s = normalize(fnmadd3(si.sh.n, dot(si.sh.n, dp_du), dp_du));
    si.sh.t = cross(si.sh.n, si.sh.s);
    si.wi = to_local(si.sh, -ray_d);
}
static PositionSample legacy_mesh_sample_position(const MeshSampler &m, V2 sample) {
    uint32_t idx = distr_sample(m, sample.y);
    float pmf = m.pmf[idx] * m.normalization,
          cdf = idx > 0 ? m.cdf[idx - 1] * m.normalization : 0.f;
    sample.y = (sample.y - cdf) / pmf;
    const float *f = m.tri + 9 * (size_t) idx;
    V3 p0 = ld3(f), p1 = ld3(f + 3), p2 = ld3(f + 6);
    V3 e0 = p1 - p0, e1 = p2 - p0;
    V2 b = square_to_uniform_triangle(sample);
    PositionSample ps;
    ps.p = p0 + e0 * b.x + e1 * b.y;
    ps.pdf = m.normalization;
    ps.uv = b;
    if (m.vnorm) {
        const float *vn = m.vnorm + 9 * (size_t) idx;
        V3 n0 = ld3(vn), n1 = ld3(vn + 3), n2 = ld3(vn + 6);
        ps.n = normalize(n0 * (1.f - b.x - b.y) + n1 * b.x + n2 * b.y);
    } else {
        ps.n = normalize(cross(e0, e1));
    }
    return ps;
}

// ---- comparison -------------------------------------------------------------------------------------------------
static bool same_bits(float a, float b) {
    if (a != a && b != b) return true;                      // NaN == NaN, whatever the payload
    return f2u(a) == f2u(b);
}
static void si_words(const SurfaceInteraction &s, float out[21]) {
    const float w[21] = { s.t, s.p.x, s.p.y, s.p.z, s.n.x, s.n.y, s.n.z, s.sh.s.x, s.sh.s.y, s.sh.s.z, s.sh.t.x, s.sh.t.y, s.sh.t.z,
                          s.sh.n.x, s.sh.n.y, s.sh.n.z, s.wi.x, s.wi.y, s.wi.z, s.uv.x, s.uv.y };
    memcpy(out, w, sizeof w);
}
static int si_diff(const SurfaceInteraction &a, const SurfaceInteraction &b) {
    float x[21], y[21];
    si_words(a, x); si_words(b, y);
    int bad = 0;
    for (int i = 0; i < 21; ++i) bad += same_bits(x[i], y[i]) ? 0 : 1;
    return bad + (a.shape != b.shape) + (a.prim != b.prim);
}
static int ps_diff(const PositionSample &a, const PositionSample &b) {
    const float x[9] = { a.p.x, a.p.y, a.p.z, a.n.x, a.n.y, a.n.z, a.uv.x, a.uv.y, a.pdf };
    const float y[9] = { b.p.x, b.p.y, b.p.z, b.n.x, b.n.y, b.n.z, b.uv.x, b.uv.y, b.pdf };
    int bad = 0;
    for (int i = 0; i < 9; ++i) bad += same_bits(x[i], y[i]) ? 0 : 1;
    return bad;
}

// ---- inputs -----------------------------------------------------------------------------------------------------
struct Rng {                                                 // splitmix64: seeded, the same everywhere
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    float uni() { return (float) (next() >> 40) * (1.f / 16777216.f); }                  // [0, 1)
    float sym(float r) { return (uni() * 2.f - 1.f) * r; }
};
struct Case { float p[9]; float vn[9]; float tc[6]; bool has_vn, has_tc; };
struct HitIn { float t, b1, b2; V3 d; };

static Case make_case(const float p[9], const float *vn, const float *tc) {
    Case c; memcpy(c.p, p, sizeof c.p);
    c.has_vn = vn != nullptr; c.has_tc = tc != nullptr;
    for (int i = 0; i < 9; ++i) c.vn[i] = vn ? vn[i] : 0.f;
    for (int i = 0; i < 6; ++i) c.tc[i] = tc ? tc[i] : 0.f;
    return c;
}

static long run_cases(const std::vector<Case> &cases, const std::vector<HitIn> &hits, size_t hits_per_case, long &checked) {
    // the table first, as the kernels build it: one record per triangle, from what the per-hit call would pass
    std::vector<TriFrame> frames(cases.size());
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case &c = cases[i];
        frames[i] = tri_frame(ld3(c.p), ld3(c.p + 3), ld3(c.p + 6), c.has_tc ? c.tc : nullptr);
    }
    long bad = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case &c = cases[i];
        const V3 p0 = ld3(c.p), p1 = ld3(c.p + 3), p2 = ld3(c.p + 6);
        const float *vn = c.has_vn ? c.vn : nullptr, *tc = c.has_tc ? c.tc : nullptr;
        for (size_t k = 0; k < hits_per_case; ++k) {
            const HitIn &h = hits[(i * hits_per_case + k) % hits.size()];
            SurfaceInteraction a, b, t;
            memset(&a, 0, sizeof a); memset(&b, 0, sizeof b); memset(&t, 0, sizeof t);
            legacy_compute_surface_interaction(p0, p1, p2, vn, tc, h.t, h.b1, h.b2, h.d, a);
            compute_surface_interaction(p0, p1, p2, vn, tc, h.t, h.b1, h.b2, h.d, b);
            compute_surface_interaction(p0, p1, p2, vn, tc, frames[i], h.t, h.b1, h.b2, h.d, t);
            const int d1 = si_diff(a, b), d2 = si_diff(a, t);
            if ((d1 || d2) && bad < 8) fprintf(stderr, "case %zu hit %zu (vn %d tc %d): classic differs in %d words, table in %d\n", i, k, (int) c.has_vn, (int) c.has_tc, d1, d2);
            bad += (d1 != 0) + (d2 != 0);
            checked += 2;
        }
        if (!tc && !vn) {                                    // the three-argument classic form (no texture coordinates)
            const HitIn &h = hits[i % hits.size()];
            SurfaceInteraction a, b;
            memset(&a, 0, sizeof a); memset(&b, 0, sizeof b);
            legacy_compute_surface_interaction(p0, p1, p2, nullptr, nullptr, h.t, h.b1, h.b2, h.d, a);
            compute_surface_interaction(p0, p1, p2, nullptr, h.t, h.b1, h.b2, h.d, b);
            bad += si_diff(a, b) != 0; ++checked;
        }
    }
    return bad;
}

// the emitter tables of a mesh of `n` faces as the host builds them (distr_1d.h:55-87: CDF accumulated in double, stored float)
struct Emitter { std::vector<float> tri, vnorm, pmf, cdf, face_n; MeshSampler m; };
static void make_emitter(Emitter &e, const std::vector<Case> &cases, size_t first, uint32_t n, bool with_vn) {
    e.tri.clear(); e.vnorm.clear(); e.pmf.clear(); e.cdf.clear(); e.face_n.clear();
    double sum = 0.0;
    uint32_t lo = 0xffffffffu, hi = 0;
    for (uint32_t f = 0; f < n; ++f) {
        const Case &c = cases[(first + f) % cases.size()];
        e.tri.insert(e.tri.end(), c.p, c.p + 9);
        e.vnorm.insert(e.vnorm.end(), c.vn, c.vn + 9);
        const V3 p0 = ld3(c.p), p1 = ld3(c.p + 3), p2 = ld3(c.p + 6);
        float a = face_area(p0, p1, p2);
        if (!(a > 0.f) || !isfinite_(a)) a = 0.f;
        e.pmf.push_back(a);
        sum += (double) a;
        e.cdf.push_back((float) sum);
        if (a > 0.f) { if (lo == 0xffffffffu) lo = f; hi = f; }
        const V3 fn = face_normal(p0, p1, p2);             // the table record: 4 floats per face
        e.face_n.push_back(fn.x); e.face_n.push_back(fn.y); e.face_n.push_back(fn.z); e.face_n.push_back(0.f);
    }
    if (lo == 0xffffffffu) lo = hi = 0;
    e.m.tri = e.tri.data(); e.m.vnorm = with_vn ? e.vnorm.data() : nullptr; e.m.pmf = e.pmf.data(); e.m.cdf = e.cdf.data();
    e.m.count = n; e.m.valid_lo = lo; e.m.valid_hi = hi; e.m.sum = (float) sum; e.m.normalization = (float) (1.0 / sum);
}
static long run_emitters(const std::vector<Case> &cases, Rng &rng, size_t meshes, long &checked) {
    long bad = 0;
    Emitter e;
    size_t first = 0;
    for (size_t k = 0; k < meshes; ++k) {
        const uint32_t n = 1u + (uint32_t) (rng.next() % 7u);
        const bool with_vn = (rng.next() & 3u) == 0u;
        make_emitter(e, cases, first, n, with_vn);
        first += n;
        if (!(e.m.sum > 0.f) || !isfinite_(e.m.sum)) continue;          // a mesh without area is no emitter (the host refuses it)
        for (int s = 0; s < 4; ++s) {
            const V2 u = v2(rng.uni(), rng.uni());
            const PositionSample a = legacy_mesh_sample_position(e.m, u), b = mesh_sample_position(e.m, u),
                                 t = mesh_sample_position(e.m, u, FaceNormalTable{ e.face_n.data() });
            const int d1 = ps_diff(a, b), d2 = ps_diff(a, t);
            if ((d1 || d2) && bad < 8) fprintf(stderr, "emitter mesh %zu sample %d: classic differs in %d words, table in %d\n", k, s, d1, d2);
            bad += (d1 != 0) + (d2 != 0);
            checked += 2;
        }
    }
    return bad;
}

int main(int argc, char **argv) {
    const size_t n_random = argc > 1 ? (size_t) atol(argv[1]) : 100000;
    Rng rng{ 0x7ea1f4a3e5ull };
    std::vector<HitIn> hits;
    for (int i = 0; i < 4096; ++i) {
        HitIn h;
        const float a = rng.uni(), b = rng.uni();
        h.b1 = a + b > 1.f ? 1.f - a : a; h.b2 = a + b > 1.f ? 1.f - b : b;
        h.t = rng.uni() * 1000.f + 1e-3f;
        h.d = normalize(v3(rng.sym(1.f), rng.sym(1.f), rng.sym(1.f) + 1e-3f));
        hits.push_back(h);
    }
    // a few hits on the rim and outside (what Moeller-Trumbore may hand over at grazing angles)
    hits[0].b1 = 0.f; hits[0].b2 = 0.f; hits[1].b1 = 1.f; hits[1].b2 = 0.f; hits[2].b1 = 0.f; hits[2].b2 = 1.f; hits[3].b1 = .5f; hits[3].b2 = .5f;

    // ---- set 1: the fixed list ----
    std::vector<Case> fixed;
    const float vn_smooth[9] = { 0.f, 0.6f, 0.8f, 0.6f, 0.f, 0.8f, -0.48f, 0.64f, 0.6f };
    const float vn_axis[9] = { 0.f, 0.f, 1.f, 0.f, 1.f, 0.f, 1.f, 0.f, 0.f };
    const float tc_zero[6] = { 0.25f, 0.25f, 0.5f, 0.5f, 0.75f, 0.75f };             // collinear uv: determinant 0
    const float tc_same[6] = { 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f };                 // one point: determinant 0
    const float tc_unit[6] = { 0.f, 0.f, 1.f, 0.f, 1.f, 1.f };
    const float tc_skew[6] = { 0.1f, 0.9f, 0.7f, 0.2f, -0.3f, 0.4f };
    auto add_all = [&](const float p[9]) {
        const float *vns[3] = { nullptr, vn_smooth, vn_axis };
        const float *tcs[5] = { nullptr, tc_zero, tc_same, tc_unit, tc_skew };
        for (const float *vn : vns) for (const float *tc : tcs) fixed.push_back(make_case(p, vn, tc));
    };
    const float tris[][9] = {
        { 0, 0, 0, 0, 1, 0, 0, 0, 1 },                       // normal +x
        { 0, 0, 0, 0, 0, 1, 0, 1, 0 },                       // -x
        { 0, 0, 0, 0, 0, 1, 1, 0, 0 },                       // +y
        { 0, 0, 0, 1, 0, 0, 0, 0, 1 },                       // -y
        { 0, 0, 0, 1, 0, 0, 0, 1, 0 },                       // +z
        { 0, 0, 0, 0, 1, 0, 1, 0, 0 },                       // -z
        { 1, 2, 3, 1, 5, 3, 1, 2, 7 },                       // normal (1, +0, +0): n.z == +0 (cross: 3 * 0 - 0 * 4)
        { 1, 2, 3, 1, 5, 3, 1, 1, 7 },                       // the same with n.z == -0 (cross: fma(+0, -1, -(3 * +0)) = -0 + -0)
        { 0, 0, 0, -1, 0, 0, 0, 1, 0 },                      // -z through negative edges (n.x, n.y = -0 / +0)
        { 0, 0, 0, 1000, 0, 1e-4f, 2000, 1e-4f, 0 },         // a sliver
        { 10, 10, 10, 10.000001f, 10, 10, 10, 500, 10 },     // a sliver one ulp wide
        { 1e-20f, 0, 0, 0, 1e-20f, 0, 0, 0, 1e-20f },        // coordinates of 1e-20 (the cross product underflows)
        { 1e-20f, 2e-20f, 3e-20f, 4e-20f, 1e-20f, 0, -1e-20f, 0, 2e-20f },
        { 1e15f, 0, 0, 0, 1e15f, 0, 0, 0, 1e15f },           // coordinates of 1e+15: the cross product is ~1e30, its squared norm overflows
        { 1e15f, 1e15f, 1e15f, -1e15f, 1e15f, 0, 0, -1e15f, 1e15f },
        { 1e15f, 0, 0, 1e15f, 1e-20f, 0, 1e15f, 0, 1e-20f }, // both at once
        { 1, 1, 1, 2, 2, 2, 3, 3, 3 },                       // zero area, collinear: a NaN frame
        { 4, 5, 6, 4, 5, 6, 4, 5, 6 },                       // zero area, one point
        { 0, 0, 0, 1, 0, 0, 1, 0, 0 },                       // zero area, two vertices equal
        { 343, 548, 227, 343, 548, 332, 213, 548, 332 },     // the Cornell box's light
        { 130, 165, 65, 82, 165, 225, 240, 165, 272 },       // ... and the top of its short block
    };
    for (const auto &p : tris) add_all(p);
    long checked = 0;
    const long bad_fixed = run_cases(fixed, hits, 8, checked);

    // ---- set 2: seeded random triangles x 4 random hits ----
    std::vector<Case> random;
    random.reserve(n_random);
    for (size_t i = 0; i < n_random; ++i) {
        float p[9], vn[9], tc[6];
        const float scale = (rng.next() & 7u) == 0u ? 1e-3f : (rng.next() & 7u) == 0u ? 1e4f : 600.f;
        const V3 c = v3(rng.sym(scale), rng.sym(scale), rng.sym(scale));
        const float size = scale * ((rng.next() & 3u) == 0u ? 1e-3f : 0.3f);
        for (int k = 0; k < 3; ++k) { p[3 * k] = c.x + rng.sym(size); p[3 * k + 1] = c.y + rng.sym(size); p[3 * k + 2] = c.z + rng.sym(size); }
        if ((rng.next() & 15u) == 0u) { p[2] = p[5] = p[8]; }                                       // axis-aligned faces: n.x = n.y = +-0
        for (int k = 0; k < 3; ++k) { const V3 n = normalize(v3(rng.sym(1.f), rng.sym(1.f), rng.sym(1.f) + 1e-3f)); vn[3 * k] = n.x; vn[3 * k + 1] = n.y; vn[3 * k + 2] = n.z; }
        for (int k = 0; k < 6; ++k) tc[k] = rng.sym(2.f);
        const uint32_t kind = (uint32_t) (rng.next() % 3u);
        if (kind == 1u) { tc[2] = tc[0] + 0.25f; tc[3] = tc[1] + 0.5f; tc[4] = tc[0] + 0.5f; tc[5] = tc[1] + 1.f; }   // exactly collinear: determinant 0
        random.push_back(make_case(p, (rng.next() & 1u) ? vn : nullptr, kind == 0u ? nullptr : tc));
    }
    const long bad_random = run_cases(random, hits, 4, checked);

    // ---- mesh_sample_position: emitter meshes of 1 - 7 faces out of both sets ----
    long checked_ps = 0;
    const long bad_ps_fixed = run_emitters(fixed, rng, 400, checked_ps);
    const long bad_ps_random = run_emitters(random, rng, n_random / 4, checked_ps);

    const long bad = bad_fixed + bad_random + bad_ps_fixed + bad_ps_random;
    printf("fixed triangles %zu, random triangles %zu, interactions compared %ld, position samples compared %ld\n", fixed.size(), random.size(), checked, checked_ps);
    printf("mismatches %ld\n", bad);
    return bad == 0 ? 0 : 1;
}
