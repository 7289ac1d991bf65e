// Which instantiation of the path kernels a scene gets: the rules mi_render and mi_sample (csrc/miwave.hip) both follow, stated once.
// Plain C++17 without HIP types, so that a host program can enumerate them (tests/test_kernel_pick.py).
//
// A rule maps the scene facts to (tiny, material class, analytic) = the leading template arguments of k_path_resident / k_sample_rays
// (device/resident_kernel.h, device/sample_kernel.h), or to (class, analytic) of k_path_phased / k_path_pooled. The lists of tuples that
// EXIST as instantiations live beside the launches in miwave.hip (MIW_*_LIST); a pick outside its list is an error there, never a default.
// The order of the tests inside a rule is part of it: it also decides what combinations no scene has (lights_on without nested) get.
#pragma once

namespace miw_pick {

// the material classes, by the values of miw/path.h's MATS_* (miwave.hip static_asserts the match)
enum : int { ALL = 0, DIFFUSE = 1, PLAIN = 2, TRIO = 3, NESTED = 4, LIGHTS = 5 };

struct Facts {
    bool tiny;            // packet scene: LDS brute-force sweep instead of the tree (TraceLds::brute)
    bool small;           // tri_count <= 32: 32-bit candidate masks
    bool diffuse_only, trio, nested, textured, lights_on;   // mi_ctx, set by mi_scene_upload
    bool no_rects;        // no analytic rectangles
    bool trio_on;         // MIW_TRIO is not 0
};

struct Pick {
    int tiny;             // 0: tree, 1: packets with 64-bit candidate masks, 2: with 32-bit masks
    int mats;             // material class
    bool analytic;        // analytic shapes compiled in
};
inline bool operator==(const Pick &a, const Pick &b) { return a.tiny == b.tiny && a.mats == b.mats && a.analytic == b.analytic; }

// the MATS_TRIO class serves the scene (52 KB of code instead of MATS_PLAIN's 84)
inline bool trio_kernel(const Facts &f) { return f.trio && f.trio_on && f.no_rects && !f.textured; }

// resident path: k_path_resident<true, ..., INTEG_PATH> and the path side of k_sample_rays. The two differ in one line: mi_sample has a
// MATS_TRIO tree kernel (with_trio), mi_render's lock-step tree kernel has none (its MATS_TRIO scenes run the phase machine).
inline Pick resident_path(const Facts &f, bool with_trio) {
    if (f.tiny && f.diffuse_only) return { f.small ? 2 : 1, DIFFUSE, false };   // no BSDF dispatch at all
    if (f.lights_on) return { f.tiny ? 1 : 0, LIGHTS, !f.tiny };
    if (f.nested) return { f.tiny ? 1 : 0, NESTED, !f.tiny };                   // + wrapper resolution, null / thindielectric
    if (f.textured) return { f.tiny ? 1 : 0, ALL, !f.tiny };                    // texture coordinates / bitmap lookups compiled in
    if (f.tiny) return { f.small ? 2 : 1, PLAIN, false };
    if (with_trio && trio_kernel(f)) return { 0, TRIO, false };
    return { 0, PLAIN, !f.no_rects };
}

// resident direct: k_path_resident<true, ..., INTEG_DIRECT> and the direct side of k_sample_rays
inline Pick resident_direct(const Facts &f) {
    const int mats = f.lights_on ? LIGHTS : f.nested ? NESTED : f.textured ? ALL : PLAIN;
    return { f.tiny ? 1 : 0, mats, !f.tiny };
}

// the float64-atomics film (k_path_resident<false, ...>, path and direct alike): three classes, analytic shapes in every tree kernel
inline Pick resident_atomic(const Facts &f) {
    return { f.tiny ? 1 : 0, f.lights_on ? LIGHTS : f.nested ? NESTED : ALL, !f.tiny };
}

// tree class: k_path_phased and k_path_pooled (which refuses LIGHTS and NESTED)
inline Pick tree_class(const Facts &f) {
    if (f.lights_on) return { 0, LIGHTS, true };
    if (f.nested) return { 0, NESTED, true };
    if (f.textured) return { 0, ALL, true };
    if (trio_kernel(f)) return { 0, TRIO, false };
    return { 0, PLAIN, !f.no_rects };
}

// ---- scene features of the packet path kernels --------------------------------------------------------------------------------------
// Beside the class, k_path_resident<true, tiny != 0, ..., INTEG_PATH> takes a mask of the scene features compiled INTO it (miw/scene.h's FEAT_*
// are these values, by name): routes whose test is false for every record of a scene that lacks the feature.
enum : unsigned { FEAT_ENV = 1u, FEAT_SHAPE_NORMALS = 2u, FEAT_EMITTER_NORMALS = 4u, FEAT_MOMENT = 8u, FEAT_ALL = 15u, FEAT_NONE = 0u };
// One more value of that template argument, beyond the scene features and never combined with one: the FRAME twin of a lean kernel (no scene feature, and the facts of a
// full frame's launch compiled in: frame_twin below). A value of the mask rather than a parameter of its own, so that the kernels that do not have it keep their names.
enum : unsigned { FEAT_FRAME = 16u };

// the features a render needs: the scene has an environment map / a shape with vertex normals / an area emitter whose mesh has them
// (mi_scene_upload), and the moment integrator wraps this render (mi_render_cfg::moment_pass)
inline unsigned packet_features(bool has_env, bool shape_normals, bool emitter_normals, bool moment) {
    return (has_env ? FEAT_ENV : 0u) | (shape_normals ? FEAT_SHAPE_NORMALS : 0u) | (emitter_normals ? FEAT_EMITTER_NORMALS : 0u) | (moment ? FEAT_MOMENT : 0u);
}
// the masks that EXIST as instantiations: all and none, not sixteen
inline bool packet_features_exist(unsigned mask) { return mask == FEAT_ALL || mask == FEAT_NONE; }
// the mask a render gets. Unlike a class outside its list (an error), a mask outside falls back to FEAT_ALL: the full kernel is correct
// for every scene, the lean one (FEAT_NONE) only for a scene with none of the four. `lean_on`: the MIW_LEAN switch.
inline unsigned packet_features_kernel(unsigned needed, bool lean_on) { return lean_on && packet_features_exist(needed) ? needed : (unsigned) FEAT_ALL; }
// the picks of resident_path() that have a lean twin (miwave.hip: MIW_LEAN_LIST): the packet kernels of the plain-diffuse and the MATS_PLAIN class
inline bool packet_lean_class(const Pick &p) { return p.tiny != 0 && !p.analytic && (p.mats == DIFFUSE || p.mats == PLAIN); }

// ---- the frame twins of the lean packet kernels -------------------------------------------------------------------------------------
// k_path_resident<true, tiny, class, false, INTEG_PATH, false, 0, FEAT_FRAME> (device/resident_kernel.h): a lean twin with the facts the
// launch of a full frame fixes for its whole duration compiled in, instead of tested inside the pixel loop with the other side of each test behind it.
struct LaunchFacts {
    bool job_chunks;      // LaneQueues::job_chunk != 0: chunk jobs from the one queue
    bool log_rec16;       // LaneQueues::log_rec: the 16-byte sample log (a filter with class tables)
    bool one_queue;       // TraceLds::queues == 1: no placed queues
    bool tail_prio;       // TraceLds::tail_prio: least-progress-first wave priorities
    bool leaf_filter;     // TraceLds::leaves != 0: not uploaded with MI_BVH_NO_LEAF_FILTER
    bool group_counts;    // LaneQueues::group_done: the film replay runs beside the render
};
// the launch that takes the twin: one that would launch the lean twin of `p` (the path integrator, the mask FEAT_NONE, a class of MIW_LEAN_LIST) with every
// fact as the twin has it compiled in. `twin_on`: the MIW_FRAME_TWIN switch. Anything else launches what it launched before.
inline bool frame_twin(const Pick &p, bool direct, unsigned feat, const LaunchFacts &l, bool twin_on) {
    return twin_on && !direct && feat == FEAT_NONE && packet_lean_class(p) &&
           l.job_chunks && l.log_rec16 && l.one_queue && !l.tail_prio && l.leaf_filter && !l.group_counts;
}

}  // namespace miw_pick
