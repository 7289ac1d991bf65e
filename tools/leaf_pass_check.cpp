// The leaf-box pass of the render kernels' trace2 (device/trace.h) with the widening of the exit distance hoisted out of its loop
// (LeafRay, leaf_ray, leaf_box_test_octant(LeafBox, LeafRay)) against the form it replaces (FastRay, leaf_box_test_octant(LeafBox, FastRay)) —
// tests/test_leaf_pass_cpu.py builds and runs this program (host flags of mitsuba2_amd/build.py; once more with -fsanitize=address,undefined).
//
// Both forms are restated below for the host, statement by statement: a packed fma of the device code is two IEEE fmas (here __builtin_fmaf,
// the host flags have -mfma and no contraction), v_rcp_f32 is 1 / x moved by up to one ulp either way (the instruction's error bound).
// The candidate filter only has to stay conservative, so what is asserted is INCLUSION: every (ray, padded box) pair the old test accepts, the
// new one accepts. Pairs: N random ones (argv[1], default 12 000 000) over scene scales 1e-3, 1 and 1e3, scenes centred up to ten extents away
// from the origin, flat boxes, origins in the scene / on a box face / inside the box / 100 extents away, directions with components 0,
// +-1e-30 and denormal, rays aimed at the edges and corners of the box (entry and exit distance equal up to rounding: where the two forms can
// differ at all), mint at 0 / the ray epsilon / the box's entry or exit distance, maxt infinite / at the box; and a fixed list of the same
// corner cases on exactly representable coordinates. mint >= 0 throughout: the rays of the render kernels (mi_sample keeps the old form).
// Prints how many pairs each form accepts and "violations 0"; returns 0 when there is none.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cmath>
#include <vector>

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float abs_(float a) { return __builtin_fabsf(a); }
static float mulsign(float a, float b) { return u2f(f2u(a) ^ (f2u(b) & 0x80000000u)); }

struct V3 { float x, y, z; };
struct LeafBox { float p[6]; };                     // entry.x exit.x entry.y exit.y entry.z exit.z: the copy staged for the ray's octant
struct F2 { float x, y; };

// ---- device/trace.h, restated ------------------------------------------------------------------------------------------
static int g_rcp_ulp[3];                            // this ray's v_rcp_f32 errors, -1 / 0 / +1 ulp per axis
static float rcp_hw(float x, int k) { float r = 1.f / x; if (r == r && abs_(r) < 3e38f && abs_(r) > 1e-37f) r = u2f(f2u(r) + k); return r; }
struct FastRay { V3 inv_d, neg_o_inv_d; float mint; };
static FastRay fast_ray(V3 o, V3 d, float mint) {
    FastRay r;
    float dx = abs_(d.x) < 1e-30f ? mulsign(1e-30f, d.x) : d.x,
          dy = abs_(d.y) < 1e-30f ? mulsign(1e-30f, d.y) : d.y,
          dz = abs_(d.z) < 1e-30f ? mulsign(1e-30f, d.z) : d.z;
    r.inv_d = V3{ rcp_hw(dx, g_rcp_ulp[0]), rcp_hw(dy, g_rcp_ulp[1]), rcp_hw(dz, g_rcp_ulp[2]) };
    r.neg_o_inv_d = V3{ -(o.x * r.inv_d.x), -(o.y * r.inv_d.y), -(o.z * r.inv_d.z) };
    r.mint = mint;
    return r;
}
static F2 pk_fma(F2 a, F2 b, F2 c) { return F2{ __builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y) }; }
static float widen(float t) { return __builtin_fmaf(abs_(t), 2e-6f, t); }
// the form before this change (and still the one of mi_sample's kernel)
static bool old_test(const LeafBox &b, const FastRay &r, float tmax_wide) {
    const F2 px = { b.p[0], b.p[1] }, py = { b.p[2], b.p[3] }, pz = { b.p[4], b.p[5] };
    const F2 tx = pk_fma(px, F2{ r.inv_d.x, r.inv_d.x }, F2{ r.neg_o_inv_d.x, r.neg_o_inv_d.x }),
             ty = pk_fma(py, F2{ r.inv_d.y, r.inv_d.y }, F2{ r.neg_o_inv_d.y, r.neg_o_inv_d.y }),
             tz = pk_fma(pz, F2{ r.inv_d.z, r.inv_d.z }, F2{ r.neg_o_inv_d.z, r.neg_o_inv_d.z });
    const float tn = __builtin_fmaxf(__builtin_fmaxf(tx.x, ty.x), __builtin_fmaxf(tz.x, r.mint));
    float tf = __builtin_fminf(__builtin_fminf(tx.y, ty.y), tz.y);
    tf = __builtin_fmaf(abs_(tf), 2e-6f, tf);
    return tn <= tf && tn <= tmax_wide;
}
// the hoisted form
struct LeafRay { F2 ix, iy, iz, cx, cy, cz; float mint; };
#define MIW_LEAF_WIDEN 1.0000025f
#define MIW_LEAF_PUSH  4.76837158e-7f
static LeafRay leaf_ray(const FastRay &r, V3 o) {
    LeafRay l;
    l.ix = F2{ r.inv_d.x, r.inv_d.x * MIW_LEAF_WIDEN }; l.iy = F2{ r.inv_d.y, r.inv_d.y * MIW_LEAF_WIDEN }; l.iz = F2{ r.inv_d.z, r.inv_d.z * MIW_LEAF_WIDEN };
    l.cx = F2{ -(o.x * l.ix.x), -(o.x * l.ix.y) }; l.cy = F2{ -(o.y * l.iy.x), -(o.y * l.iy.y) }; l.cz = F2{ -(o.z * l.iz.x), -(o.z * l.iz.y) };
    l.cx.y = __builtin_fmaf(abs_(l.cx.y), MIW_LEAF_PUSH, l.cx.y); l.cy.y = __builtin_fmaf(abs_(l.cy.y), MIW_LEAF_PUSH, l.cy.y); l.cz.y = __builtin_fmaf(abs_(l.cz.y), MIW_LEAF_PUSH, l.cz.y);
    l.mint = r.mint;
    return l;
}
static bool new_test(const LeafBox &b, const LeafRay &r, float tmax_wide) {
    const F2 px = { b.p[0], b.p[1] }, py = { b.p[2], b.p[3] }, pz = { b.p[4], b.p[5] };
    const F2 tx = pk_fma(px, r.ix, r.cx), ty = pk_fma(py, r.iy, r.cy), tz = pk_fma(pz, r.iz, r.cz);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(tx.x, ty.x), tz.x);
    const float tf = __builtin_fminf(__builtin_fminf(tx.y, ty.y), tz.y);
    return tn <= tf && r.mint <= tf && tn <= tmax_wide;
}
static uint32_t ray_octant(const FastRay &r) { return (r.inv_d.x < 0.f ? 1u : 0u) | (r.inv_d.y < 0.f ? 2u : 0u) | (r.inv_d.z < 0.f ? 4u : 0u); }
// stage_to_lds: the copy of a box for octant o
static LeafBox octant_copy(const float lo[3], const float hi[3], uint32_t o) {
    LeafBox k;
    for (int a = 0; a < 3; ++a) { const bool neg = (o >> a) & 1u; k.p[2 * a] = neg ? hi[a] : lo[a]; k.p[2 * a + 1] = neg ? lo[a] : hi[a]; }
    return k;
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t) (g_state >> 32); }
static float uni() { return (rnd() >> 8) * (1.f / 16777216.f); }            // [0, 1)
static float sym() { return 2.f * uni() - 1.f; }

static unsigned long long n_pairs, n_old, n_new, n_bad;
static unsigned long long n_free, free_old, free_new;            // of these: the pairs that are not borderline by construction (origin not on a face, direction not aimed at an edge)

static void check(V3 o, V3 d, float mint, float maxt, const float lo[3], const float hi[3]) {
    const FastRay r = fast_ray(o, d, mint);
    const LeafRay q = leaf_ray(r, o);
    const LeafBox b = octant_copy(lo, hi, ray_octant(r));
    const float wide = widen(maxt);
    const bool a_old = old_test(b, r, wide), a_new = new_test(b, q, wide);
    ++n_pairs; n_old += a_old; n_new += a_new;
    if (a_old && !a_new) {
        if (n_bad++ < 8)
            printf("VIOLATION o %a %a %a d %a %a %a mint %a maxt %a box %a %a %a .. %a %a %a\n", o.x, o.y, o.z, d.x, d.y, d.z, mint, maxt,
                   lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    }
}

static float odd_component(uint32_t k) {
    static const float v[] = { 0.f, -0.f, 1e-30f, -1e-30f, 1e-40f, -1e-40f, 1.4e-45f, 1e-31f };
    return v[k & 7u];
}

static void random_pair() {
    static const float scales[3] = { 1e-3f, 1.f, 1e3f };
    const float s = scales[rnd() % 3u];
    const uint32_t kind = rnd();
    // where the scene lies: at the origin, or up to ten extents away (plane * inv_d and -o * inv_d cancel)
    const float off = (kind & 1u) ? 0.f : 10.f * s;
    const V3 c = { off * sym(), off * sym(), off * sym() };
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const float u = c.x * (a == 0) + c.y * (a == 1) + c.z * (a == 2) + s * sym(), w = s * uni() * (((kind >> 1) & 3u) == 0 ? 0.05f : 1.f);
        lo[a] = u; hi[a] = u + w;
    }
    if (((kind >> 3) & 3u) == 0) { const int a = rnd() % 3u; hi[a] = lo[a]; }                 // a flat box (an axis-aligned wall)
    const float pad = 1e-5f * 2.f * s;                                                           // bvh_build.h: 1e-5 x the scene extent
    for (int a = 0; a < 3; ++a) { lo[a] -= pad; hi[a] += pad; }
    for (int a = 0; a < 3; ++a) g_rcp_ulp[a] = (int) (rnd() % 3u) - 1;
    // origin
    V3 o;
    const uint32_t ok = (kind >> 5) & 7u;
    float *oc[3] = { &o.x, &o.y, &o.z };
    if (ok == 0) { o = V3{ c.x + 100.f * 2.f * s * sym(), c.y + 100.f * 2.f * s * sym(), c.z + 100.f * 2.f * s * sym() }; }       // 100 extents away
    else if (ok <= 2) { for (int a = 0; a < 3; ++a) *oc[a] = lo[a] + (hi[a] - lo[a]) * uni(); }   // inside the box
    else { o = V3{ c.x + 2.f * s * sym(), c.y + 2.f * s * sym(), c.z + 2.f * s * sym() }; }     // in the scene
    if (ok == 2 || ok == 3) { const int a = rnd() % 3u; *oc[a] = (rnd() & 1u) ? lo[a] : hi[a]; } // on a face (of the padded box), inside or in its plane outside
    if (ok == 4) { const int a = rnd() % 3u; *oc[a] = (rnd() & 1u) ? lo[a] + pad : hi[a] - pad; } // on the unpadded face: where a path vertex lies
    // direction
    V3 d;
    const uint32_t dk = (kind >> 8) & 7u;
    if (dk <= 3) {                                                                               // aimed at an edge or corner point of the box (or through its inside)
        float t[3];
        for (int a = 0; a < 3; ++a) { const uint32_t e = rnd() % 3u; t[a] = e == 0 ? lo[a] : e == 1 ? hi[a] : lo[a] + (hi[a] - lo[a]) * uni(); }
        d = V3{ t[0] - o.x, t[1] - o.y, t[2] - o.z };
    } else {
        d = V3{ sym(), sym(), sym() };
    }
    float len = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    if (!(len > 0.f)) { d = V3{ 0.f, 0.f, 1.f }; len = 1.f; }
    d = V3{ d.x / len, d.y / len, d.z / len };
    if (dk == 3 || dk == 7) {                                                                    // one or two components 0, +-1e-30, denormal
        float *dc[3] = { &d.x, &d.y, &d.z };
        const int a = rnd() % 3u; *dc[a] = odd_component(rnd());
        if (rnd() & 1u) { *dc[(a + 1) % 3] = odd_component(rnd()); }
        if (d.x == 0.f && d.y == 0.f && d.z == 0.f) d.z = 1.f;
    }
    // interval: mint >= 0
    const FastRay r = fast_ray(o, d, 0.f);
    const LeafBox b = octant_copy(lo, hi, ray_octant(r));
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(b.p[0], r.inv_d.x, r.neg_o_inv_d.x), __builtin_fmaf(b.p[2], r.inv_d.y, r.neg_o_inv_d.y)), __builtin_fmaf(b.p[4], r.inv_d.z, r.neg_o_inv_d.z));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaf(b.p[1], r.inv_d.x, r.neg_o_inv_d.x), __builtin_fmaf(b.p[3], r.inv_d.y, r.neg_o_inv_d.y)), __builtin_fmaf(b.p[5], r.inv_d.z, r.neg_o_inv_d.z));
    float mint = 0.f, maxt = __builtin_inff();
    switch ((kind >> 11) & 7u) {
        case 0: mint = 8.9406967e-05f * s; break;                     // the ray epsilon of a scene of this size
        case 1: if (tn > 0.f && tn == tn) mint = tn; break;          // mint at the box: entry
        case 2: if (tf > 0.f && tf == tf) mint = tf; break;          //                  exit
        case 3: if (tf > 0.f && tf == tf) mint = u2f(f2u(tf) + 1u - 2u * (rnd() & 1u)); break;
        default: break;
    }
    switch ((kind >> 14) & 7u) {
        case 0: if (tn > 0.f && tn == tn) maxt = tn; break;          // maxt at the box
        case 1: if (tf > 0.f && tf == tf) maxt = tf; break;
        case 2: if (tn > 0.f && tn == tn) maxt = u2f(f2u(tn) + 1u - 2u * (rnd() & 1u)); break;
        case 3: maxt = 4.f * s * uni(); break;
        default: break;
    }
    if (!(mint >= 0.f) || mint > 3e38f) mint = 0.f;
    if (mint > maxt) maxt = __builtin_inff();                        // (an empty interval is no ray of the kernels: the new form does not ask mint <= maxt)
    const unsigned long long o0 = n_old, n0 = n_new;
    check(o, d, mint, maxt, lo, hi);
    if (dk > 3 && (ok < 2 || ok > 4)) { ++n_free; free_old += n_old - o0; free_new += n_new - n0; }
}

static void fixed_list() {
    static const float scales[3] = { 1e-3f, 1.f, 1e3f };
    memset(g_rcp_ulp, 0, sizeof g_rcp_ulp);
    for (float s : scales) {
        const float pad = 1e-5f * 2.f * s;
        // a unit-ish box and three flat ones, padded
        const float boxes[4][6] = { { 0.25f * s, 0.5f * s, -0.75f * s, 0.5f * s, 0.f, s },  { 0.f, 0.f, -s, s, -s, s }, { -s, s, s, s, -s, s }, { -s, s, -s, s, -0.5f * s, -0.5f * s } };
        const float comps[] = { 0.f, -0.f, 1e-30f, -1e-30f, 1e-40f, -1e-40f, 1.f, -1.f };
        for (const auto &bx : boxes) {
            float lo[3] = { bx[0] - pad, bx[2] - pad, bx[4] - pad }, hi[3] = { bx[1] + pad, bx[3] + pad, bx[5] + pad };
            // origins: every face (padded and unpadded plane) at the centre of the face, the centre of the box, the corners, 100 extents out on each axis
            std::vector<V3> origins;
            const V3 mid = { 0.5f * (lo[0] + hi[0]), 0.5f * (lo[1] + hi[1]), 0.5f * (lo[2] + hi[2]) };
            origins.push_back(mid);
            for (int a = 0; a < 3; ++a)
                for (int side = 0; side < 4; ++side) {
                    V3 o = mid; float *oc[3] = { &o.x, &o.y, &o.z };
                    *oc[a] = side == 0 ? lo[a] : side == 1 ? hi[a] : side == 2 ? lo[a] + pad : hi[a] - pad;
                    origins.push_back(o);
                    V3 far = mid; float *fc[3] = { &far.x, &far.y, &far.z };
                    *fc[a] += (side & 1 ? 200.f : -200.f) * s;
                    origins.push_back(far);
                }
            for (int k = 0; k < 8; ++k) origins.push_back(V3{ (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2] });
            for (const V3 &o : origins)
                for (float dx : comps) for (float dy : comps) for (float dz : comps) {
                    if (dx == 0.f && dy == 0.f && dz == 0.f) continue;
                    const V3 d = { dx, dy, dz };                     // (unnormalised on purpose: the test does not ask for a unit direction)
                    const FastRay r = fast_ray(o, d, 0.f);
                    const LeafBox b = octant_copy(lo, hi, ray_octant(r));
                    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaf(b.p[1], r.inv_d.x, r.neg_o_inv_d.x), __builtin_fmaf(b.p[3], r.inv_d.y, r.neg_o_inv_d.y)), __builtin_fmaf(b.p[5], r.inv_d.z, r.neg_o_inv_d.z));
                    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(b.p[0], r.inv_d.x, r.neg_o_inv_d.x), __builtin_fmaf(b.p[2], r.inv_d.y, r.neg_o_inv_d.y)), __builtin_fmaf(b.p[4], r.inv_d.z, r.neg_o_inv_d.z));
                    const float mints[4] = { 0.f, 8.9406967e-05f * s, (tn > 0.f && tn < 3e38f) ? tn : 0.f, (tf > 0.f && tf < 3e38f) ? tf : 0.f };
                    const float maxts[3] = { __builtin_inff(), (tn > 0.f && tn < 3e38f) ? tn : s, (tf > 0.f && tf < 3e38f) ? tf : s };
                    for (float mint : mints) for (float maxt : maxts) if (mint <= maxt) check(o, d, mint, maxt, lo, hi);
                }
        }
    }
}

int main(int argc, char **argv) {
    const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 12000000ull;
    fixed_list();
    const unsigned long long n_fixed = n_pairs, fixed_old = n_old, fixed_new = n_new;
    for (unsigned long long i = 0; i < n; ++i) random_pair();
    printf("fixed pairs %llu: old accepts %llu, new accepts %llu\n", n_fixed, fixed_old, fixed_new);
    printf("random pairs %llu: old accepts %llu, new accepts %llu (%llu more, %.4f %% of the old form's)\n", n, n_old - fixed_old, n_new - fixed_new,
           (n_new - fixed_new) - (n_old - fixed_old), 100.0 * (double) ((n_new - fixed_new) - (n_old - fixed_old)) / (double) ((n_old - fixed_old) ? (n_old - fixed_old) : 1));
    printf("  of these, origin off the faces and direction not aimed at an edge %llu: old accepts %llu, new accepts %llu (%llu more)\n", n_free, free_old, free_new, free_new - free_old);
    printf("violations %llu\n", n_bad);
    return n_bad ? 1 : 0;
}
