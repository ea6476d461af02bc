// The plan of the signature-group ("Gram") assembly and its back substitution (csrc/gram_path.h) against a second implementation of its rules -- the expressions as
// the solver stated them before the plan existed, kept here on their own -- field by field over both camera block sizes, task sets of one class, all classes and
// classes with gaps, task counts on both sides of every threshold, every environment and lab knob; then the landmarks of the shipped decision by name, the launch
// contracts, the class of the planner's cost model, and the layout of a wave's LDS slice.  Stand-alone: includes gram_path.h only.  Prints GRAM_PATH_OK.
#include <cstdio>
#include <vector>
#include "../../spherical_sfm_amd/csrc/gram_path.h"

using namespace ssfm;

static int g_failed = 0;
static long g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 40) { std::printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } } } while (0)

// ---- the second implementation ---------------------------------------------------------------------------------------------------------------
static int ref_tile_class(int DC, int K, bool t4) { const int rows = DC * K; return rows <= 16 ? 0 : (rows <= 20 && t4) ? 1 : rows <= 32 ? 2 : (rows <= 36 && t4) ? 3 : 4; }
// the planner's cost model had its own numbering: 8 + full tiles for the tail classes, the tile count otherwise
static int ref_cost_class(int DC, int K) { const int rows = DC * K, nt_full = rows / 16, tail = rows - 16 * nt_full; return (tail > 0 && tail <= 4 && nt_full >= 1) ? 8 + nt_full : (rows + 15) / 16; }
static const int REF_CAMREC = 34, REF_TAIL = 8 * REF_CAMREC + 48 + 28 / 2 + 8 / 2, REF_VEC = 4 * 6 * 8;
static int ref_g_off(int R) { const int t = R >> 4; return 128 * t * t + 144 * t + (R & 15) * (16 * t + 17); }

struct RefLaunch { int cls, t0, t1, rows_alloc, W, grid, block; size_t lds; bool split; int max_sub; };
struct Ref {
    bool fuse_lin, any_ok; RefLaunch any; std::vector<RefLaunch> launches; int n_cls;
    bool grouped, all_grouped; int gbs_split, gbs_grid; size_t gbs_lds; int lpp;
};
static Ref reference(const GramPathIn& in, const GramPathLab& lab) {
    Ref r{}; const int DC = in.DC, ng = in.ng; const int* rec = in.gr_rec;
    int cls_end[5];
    for (int cl = 0; cl < 5; cl++) cls_end[cl] = 0;
    for (int t = 0; t < ng; t++) { const int c0 = ref_tile_class(DC, rec[(size_t)t * 48 + 2], lab.t4); for (int cl = c0; cl < 5; cl++) cls_end[cl] = t + 1; }
    int n_cls = 0; for (int cl = 0; cl < 5; cl++) if (cls_end[cl] > (cl ? cls_end[cl - 1] : 0)) n_cls++;
    r.n_cls = n_cls;
    // read_knobs
    r.fuse_lin = in.env_fuse != 0 && !in.det && in.nP > 0 && ng > 0 && in.gram_points == in.nP && !in.pair_tasks && !in.cam_sum_tasks && !(in.gram_any && n_cls > 1) && cls_end[4] == cls_end[3];
    const bool unsplit = in.det || lab.gram_waves != 1 || lab.emit_skip != 0 || lab.stamps || (in.gram_any && n_cls > 1);
    int gram_split[5];
    int max_sub_of[5];
    for (int cl = 0; cl < 5; cl++) {
        const int t0 = cl ? cls_end[cl - 1] : 0, t1 = cls_end[cl];
        gram_split[cl] = 1; max_sub_of[cl] = 1;
        if (t1 <= t0) continue;
        int max_sub = 1;
        for (int t = t0; t < t1; t++) max_sub = std::max(max_sub, (rec[(size_t)t * 48 + 1] + 8 - 1) / 8);
        max_sub_of[cl] = max_sub;
        if (unsplit) continue;
        const int ntask = t1 - t0, by_count = ntask <= 2 * in.num_cus ? 4 : ntask <= 4 * in.num_cus ? 2 : 1;
        gram_split[cl] = (in.env_split >= 1 && in.env_split <= 4) ? in.env_split : std::min(max_sub, by_count);
    }
    // launch_gram (a launch that is not stamped: gram_dbg = null)
    const int gram_waves = std::min(4, std::max(1, lab.gram_waves));
    r.any_ok = in.gram_any && n_cls > 1 && gram_waves == 1 && !r.fuse_lin;
    if (ng > 0) {
        const int rows_alloc = DC * rec[(size_t)(ng - 1) * 48 + 2];
        r.any = RefLaunch{ref_tile_class(DC, rec[(size_t)(ng - 1) * 48 + 2], lab.t4), 0, ng, rows_alloc, 1, ng, 64, ((size_t)rows_alloc * SSFM_GRAM_LD + REF_TAIL) * sizeof(double), false, 1};
    }
    for (int cl = 0; cl < (DC == 6 ? 5 : 3); cl++) {
        const int t0 = cl ? cls_end[cl - 1] : 0, t1 = cls_end[cl];
        if (t1 <= t0) continue;
        const int W = (gram_waves == 1 && !lab.emit_skip) ? gram_split[cl] : 1;
        const int rows_alloc = DC * rec[(size_t)(t1 - 1) * 48 + 2];
        const size_t gram_lds = W > 1 ? (size_t)W * ((size_t)rows_alloc * SSFM_GRAM_LD + REF_TAIL + REF_VEC) * sizeof(double)
                                      : (size_t)gram_waves * ((size_t)rows_alloc * SSFM_GRAM_LD + REF_TAIL) * sizeof(double);
        r.launches.push_back(RefLaunch{cl, t0, t1, rows_alloc, W, W > 1 ? t1 - t0 : (t1 - t0 + gram_waves - 1) / gram_waves, W > 1 ? 64 * W : 64 * gram_waves, gram_lds, W > 1, max_sub_of[cl]});
    }
    // back_substitute / gram_backsub
    r.grouped = !lab.publish_fused && ng > 0 && (in.env_backsub < 0 ? in.gram_obs >= 6 * in.gram_points : in.env_backsub != 0);
    r.all_grouped = r.grouped && in.gram_points == in.nP;
    const int gbs_wave_target = 14 * in.num_cus;
    r.gbs_split = in.env_gbs_split > 0 ? std::min(8, in.env_gbs_split) : std::max(1, std::min(4, (gbs_wave_target + ng - 1) / std::max(1, ng)));
    r.gbs_grid = (ng * r.gbs_split + 4 - 1) / 4;
    r.gbs_lds = (size_t)4 * (8 * (REF_CAMREC + 12 + 6) + 2 * 8 * 18) * sizeof(double);
    const int bs_lpp = lab.backsub_lpp > 0 ? lab.backsub_lpp : ((int64_t)4 * in.M > (int64_t)33 * in.nP ? 2 : 1);
    r.lpp = bs_lpp == 2 ? 2 : 1;
    return r;
}

// ---- task sets ---------------------------------------------------------------------------------------------------------------------------------
// ng tasks sorted by K over the given Ks (spread evenly), every task of `sub` sub-chunks except the first of 1 (so the longest decides)
static std::vector<int> make_tasks(const std::vector<int>& Ks, int ng, int sub) {
    std::vector<int> rec((size_t)ng * GRAM_REC, 0);
    for (int t = 0; t < ng; t++) {
        rec[(size_t)t * GRAM_REC + 1] = (t == 0 && ng > 1) ? 5 : 8 * (sub - 1) + 3;
        rec[(size_t)t * GRAM_REC + 2] = Ks[(size_t)t * Ks.size() / ng];
    }
    return rec;
}

static void compare(const GramPathIn& in, const GramPathLab& lab, const char* what) {
    const GramPath p = gram_path(in, lab); const Ref r = reference(in, lab); g_cases++;
    const int DC = in.DC, ng = in.ng;
    CHECK(p.fuse_lin == r.fuse_lin && p.n_cls == r.n_cls, "%s DC %d ng %d: fuse_lin %d / %d, classes %d / %d", what, DC, ng, p.fuse_lin, r.fuse_lin, p.n_cls, r.n_cls);
    CHECK(p.any == r.any_ok, "%s DC %d ng %d: any %d / %d", what, DC, ng, p.any, r.any_ok);
    if (r.any_ok) {
        const GramLaunch& a = p.any_launch;
        CHECK(a.t0 == 0 && a.t1 == ng && a.rows_alloc == r.any.rows_alloc && a.grid == r.any.grid && a.block == 64 && a.lds == r.any.lds && !a.split && a.waves == 1 && a.cls == r.any.cls,
              "%s DC %d ng %d: any launch rows %d grid %d lds %zu", what, DC, ng, a.rows_alloc, a.grid, a.lds);
        CHECK(a.lds <= 64 * 1024, "%s: any launch of %zu bytes", what, a.lds);
    }
    CHECK(p.n_launch == (int)r.launches.size(), "%s DC %d ng %d: %d launches / %zu", what, DC, ng, p.n_launch, r.launches.size());
    int next = 0;
    for (int i = 0; i < p.n_launch && i < (int)r.launches.size(); i++) {
        const GramLaunch& l = p.launch[i]; const RefLaunch& q = r.launches[i];
        CHECK(l.cls == q.cls && l.t0 == q.t0 && l.t1 == q.t1 && l.rows_alloc == q.rows_alloc && l.waves == q.W && l.split == q.split && l.grid == q.grid && l.block == q.block && l.lds == q.lds && l.max_sub == q.max_sub,
              "%s DC %d ng %d launch %d: class %d/%d tasks [%d, %d)/[%d, %d) rows %d/%d waves %d/%d grid %d/%d block %d/%d lds %zu/%zu", what, DC, ng, i, l.cls, q.cls, l.t0, l.t1, q.t0, q.t1,
              l.rows_alloc, q.rows_alloc, l.waves, q.W, l.grid, q.grid, l.block, q.block, l.lds, q.lds);
        // contracts: a partition of [0, ng) in order; room for every task; bytes = waves of the block x the slice; within 64 KiB; a class the cameras can have
        CHECK(l.t0 == next && l.t1 > l.t0, "%s DC %d ng %d launch %d: [%d, %d) after %d", what, DC, ng, i, l.t0, l.t1, next); next = l.t1;
        for (int t = l.t0; t < l.t1; t++) {
            CHECK(l.rows_alloc >= DC * in.K(t), "%s DC %d launch %d task %d: %d rows for K %d", what, DC, i, t, l.rows_alloc, in.K(t));
            CHECK(gram_tile_class(DC, in.K(t), lab.t4) == l.cls, "%s DC %d launch %d task %d: class", what, DC, i, t);
        }
        CHECK(l.lds == (size_t)(l.block / 64) * gram_slice_doubles(l.rows_alloc, l.split) * 8, "%s DC %d launch %d: %zu bytes", what, DC, i, l.lds);
        CHECK(l.lds <= 64 * 1024, "%s DC %d launch %d: %zu bytes", what, DC, i, l.lds);
        CHECK(l.split == (l.waves > 1) && l.waves >= 1 && l.waves <= 4 && l.block <= 256 && (l.split ? l.grid == l.t1 - l.t0 : l.grid * (l.block / 64) >= l.t1 - l.t0), "%s DC %d launch %d", what, DC, i);
        CHECK(DC == 6 || GRAM_CLASS_DC3[l.cls], "%s: 3-dof cameras in class %d", what, l.cls);
        CHECK(!p.fuse_lin || GRAM_CLASS_FUSED[l.cls], "%s: fused launch of class %d", what, l.cls);
        if (p.unsplit) CHECK(!l.split, "%s: split launch of an unsplit plan", what);
    }
    CHECK(next == ng, "%s DC %d: the launches end at %d of %d tasks", what, DC, next, ng);
    if (p.any) CHECK(!p.fuse_lin && p.unsplit, "%s: the mixed-class launch is unfused and unsplit", what);
    CHECK(p.grouped == r.grouped && p.all_grouped == r.all_grouped && p.gbs_split == r.gbs_split && p.gbs_grid == r.gbs_grid && p.gbs_lds == r.gbs_lds && p.backsub_lpp == r.lpp,
          "%s DC %d ng %d: grouped %d/%d all %d/%d waves %d/%d grid %d/%d bytes %zu/%zu lanes %d/%d", what, DC, ng, p.grouped, r.grouped, p.all_grouped, r.all_grouped, p.gbs_split, r.gbs_split,
          p.gbs_grid, r.gbs_grid, p.gbs_lds, r.gbs_lds, p.backsub_lpp, r.lpp);
    CHECK(p.t4 == lab.t4 && p.focal_free == in.focal_free && p.lab.emit_skip == lab.emit_skip, "%s: kernel arguments", what);
}

static GramPathIn base_in(int DC, const std::vector<int>& rec, int num_cus = 256) {
    GramPathIn in; in.DC = DC; in.gr_rec = rec.data(); in.ng = (int)(rec.size() / GRAM_REC); in.num_cus = num_cus;
    int64_t pts = 0, obs = 0; for (int t = 0; t < in.ng; t++) { pts += in.cnt(t); obs += (int64_t)in.cnt(t) * in.K(t); }
    in.gram_points = pts; in.gram_obs = obs; in.nP = pts; in.M = obs;
    return in;
}

int main() {
    // ---- the plan against the second implementation
    for (int DC : {3, 6}) {
        // one class only, for each class; all classes present; classes with gaps (K sorted ascending, K <= GRAM_KMAX)
        std::vector<std::vector<int>> sets;
        if (DC == 6) sets = {{2}, {3}, {4, 5}, {6}, {7, 8}, {8}, {2, 3, 4, 6, 7}, {3, 4, 5, 6, 7, 8}, {2, 6}, {3, 8}, {2, 4, 8}, {3, 6}};
        else sets = {{3}, {4, 5}, {6}, {7, 8}, {3, 6, 7}, {3, 4, 5, 6, 7, 8}, {3, 8}, {5, 6}, {6, 8}};
        for (const auto& Ks : sets) for (int ng : {1, 511, 512, 513, 1023, 1024, 1025, 5000}) for (int sub = 1; sub <= 5; sub++) {
            const std::vector<int> rec = make_tasks(Ks, ng, sub);
            for (int num_cus : {256, 304}) for (int det = 0; det < 2; det++) for (int any = 0; any < 2; any++) {
                if (num_cus != 256 && (sub != 3 || det)) continue;      // (the second device: the thresholds move with it, nothing else)
                GramPathIn in = base_in(DC, rec, num_cus); in.det = det != 0; in.gram_any = any != 0;
                compare(in, GramPathLab(), "default");
                if (sub != 2 && sub != 5) continue;                      // the knobs on two task lengths
                for (int pairs = 0; pairs < 2; pairs++) for (int sums = 0; sums < 2; sums++) for (int below = 0; below < 2; below++) {
                    GramPathIn v = in; v.pair_tasks = pairs != 0; v.cam_sum_tasks = sums != 0; v.focal_free = below != 0;
                    if (below) { v.nP = in.nP + 1000; v.M = in.M + 9000; }      // points outside the groups, with long tracks
                    compare(v, GramPathLab(), "pair / camera-sum tasks, loose points");
                }
                for (int e : {0, 1}) { GramPathIn v = in; v.env_fuse = e; compare(v, GramPathLab(), "SSFM_GRAM_FUSE"); }
                for (int e : {0, 1, 2, 3, 4, 5}) { GramPathIn v = in; v.env_split = e; compare(v, GramPathLab(), "SSFM_GRAM_SPLIT"); }
                for (int e : {-1, 0, 1}) for (int k = 0; k < 2; k++) { GramPathIn v = in; v.env_backsub = e; if (k) v.gram_obs = 5 * v.gram_points; compare(v, GramPathLab(), "SSFM_GRAM_BACKSUB"); }
                for (int e : {0, 1, 3, 8, 12}) { GramPathIn v = in; v.env_gbs_split = e; compare(v, GramPathLab(), "SSFM_GBS_SPLIT"); }
                for (int e : {0, 1, 2, 4, 7}) { GramPathLab lab; lab.gram_waves = e; compare(in, lab, "SSFM_GRAM_WAVES"); }
                { GramPathLab lab; lab.t4 = false; compare(in, lab, "SSFM_GRAM_T4"); }
                { GramPathLab lab; lab.emit_skip = 1; compare(in, lab, "SSFM_GRAM_EMIT_SKIP"); }
                { GramPathLab lab; lab.stamps = true; compare(in, lab, "SSFM_GRAM_STAMPS"); }
                for (int e : {0, 1, 2, 3}) { GramPathLab lab; lab.backsub_lpp = e; GramPathIn v = in; v.nP += 10; v.M += 100; compare(v, lab, "SSFM_BACKSUB_LPP"); }
                { GramPathLab lab; lab.publish_fused = true; compare(in, lab, "SSFM_PUBLISH_FUSED"); }
            }
        }
        { GramPathIn in; in.DC = DC; compare(in, GramPathLab(), "no groups"); }
    }
    // ---- landmarks, by name
    {
        const std::vector<int> r900 = make_tasks({6}, 900, 14), r512 = make_tasks({6}, 512, 14), r5000 = make_tasks({8}, 5000, 14);
        GramPathIn in = base_in(6, r900);
        GramPath p = gram_path(in);
        CHECK(p.n_launch == 1 && p.launch[0].waves == 2 && p.launch[0].split && p.launch[0].grid == 900 && p.launch[0].block == 128 && p.fuse_lin && !p.any, "900 one-class tasks on 256 CUs: 2 waves per task, fused");
        CHECK(p.grouped && p.all_grouped && p.gbs_split == 4 && p.gbs_grid == 900 && p.backsub_lpp == 1, "900 tasks of K = 6: grouped back substitution, four waves per task");
        CHECK(gram_path(base_in(6, r512)).launch[0].waves == 4 && gram_path(base_in(6, make_tasks({6}, 100, 14))).launch[0].waves == 4, "at most 512 tasks: 4 waves per task");
        CHECK(gram_path(base_in(6, make_tasks({6}, 100, 3))).launch[0].waves == 3, "never more waves than the longest task has sub-chunks");
        const GramPath big = gram_path(base_in(6, r5000));
        CHECK(big.launch[0].waves == 1 && !big.launch[0].split && big.launch[0].block == 64 && big.gbs_split == 1, "5000 tasks: 1 wave per task");
        CHECK(!big.fuse_lin && big.launch[0].cls == 4, "a three-tile task turns fuse_lin off");
        { const std::vector<int> r367 = make_tasks({3, 6, 7}, 900, 14); GramPathIn m = base_in(6, r367); m.gram_any = false; CHECK(!gram_path(m).fuse_lin && gram_path(m).n_launch == 3, "a three-tile task among others turns fuse_lin off"); }
        for (int e : {0, 2, 4}) { GramPathIn d = in; d.det = true; d.env_split = e; const GramPath q = gram_path(d); CHECK(q.launch[0].waves == 1 && !q.launch[0].split && !q.fuse_lin, "det: 1 wave per task whatever SSFM_GRAM_SPLIT = %d says", e); }
        { const std::vector<int> r346 = make_tasks({3, 4, 6}, 900, 14); GramPathIn m = base_in(6, r346); const GramPath q = gram_path(m);
          CHECK(q.any && !q.fuse_lin && q.unsplit && q.any_launch.grid == 900 && q.any_launch.block == 64 && q.any_launch.rows_alloc == 36, "several classes with gram_any: one launch, unsplit and unfused");
          m.gram_any = false; const GramPath s = gram_path(m); CHECK(!s.any && s.n_launch == 3 && s.fuse_lin && s.launch[0].split, "several classes without gram_any: a launch per class"); }
        for (int K = 1; K <= GRAM_KMAX; K++) for (int t4 = 0; t4 < 2; t4++) CHECK(gram_tile_class(3, K, t4 != 0) <= 2 && GRAM_CLASS_DC3[gram_tile_class(3, K, t4 != 0)], "3-dof cameras never get classes 3 or 4 (K %d)", K);
        // the largest launch: 4 waves with a 48-row slice
        const GramPath w = gram_path(base_in(6, make_tasks({8}, 512, 14)));
        CHECK(w.launch[0].waves == 4 && w.launch[0].rows_alloc == 48 && w.launch[0].lds == (size_t)4 * (48 * GRAM_LD + 338 + 192) * 8, "4 waves x 48 rows: %zu bytes", w.launch[0].lds);
#if SSFM_GRAM_LD == 28
        CHECK(w.launch[0].lds == 59968, "4 x (48 x 28 + 338 + 192) x 8 = 59 968 B, not %zu", w.launch[0].lds);
#endif
    }
    // ---- tile classes: the rule, its tables, and the cost model's class = the launch's class
    for (int DC : {3, 6}) for (int K = 1; K <= GRAM_KMAX; K++) {
        for (int t4 = 0; t4 < 2; t4++) {
            const int c = gram_tile_class(DC, K, t4 != 0);
            CHECK(c == ref_tile_class(DC, K, t4 != 0) && c >= 0 && c < GRAM_CLASSES, "DC %d K %d: class %d", DC, K, c);
            CHECK(16 * GRAM_CLASS_NT[c] + (GRAM_CLASS_TI[c] > 0 ? 4 : 0) >= DC * K, "DC %d K %d: class %d holds %d rows", DC, K, c, DC * K);
            CHECK(c == 0 || 16 * GRAM_CLASS_NT[c - 1] + (GRAM_CLASS_TI[c - 1] > 0 && t4 ? 4 : 0) < DC * K || (!t4 && GRAM_CLASS_TI[c - 1] > 0), "DC %d K %d: class %d is not the smallest", DC, K, c);
            if (GRAM_CLASS_TI[c] > 0) CHECK(16 * GRAM_CLASS_TI[c] >= DC * K && t4, "DC %d K %d: the tail's column tiles", DC, K);
        }
        // (what the planner computes: gram_tile_class(DC, K, true); two K share a class there exactly when they shared one in its old numbering)
        for (int K2 = 1; K2 <= GRAM_KMAX; K2++)
            CHECK((gram_tile_class(DC, K, true) == gram_tile_class(DC, K2, true)) == (ref_cost_class(DC, K) == ref_cost_class(DC, K2)), "DC %d: K %d and %d in the cost model", DC, K, K2);
        std::vector<int> rec = make_tasks({K}, 10, 2);
        const GramPath p = gram_path(base_in(DC, rec));
        CHECK(p.n_launch == 1 && p.launch[0].cls == gram_tile_class(DC, K, true), "DC %d K %d: the cost model's class %d is the launch's %d", DC, K, gram_tile_class(DC, K, true), p.launch[0].cls);
    }
    CHECK(!GRAM_CLASS_FUSED[4] && GRAM_CLASS_FUSED[0] && GRAM_CLASS_FUSED[1] && GRAM_CLASS_FUSED[2] && GRAM_CLASS_FUSED[3], "only the three-tile class has no fused form");
    // ---- the slice of a wave: offsets inside the slice, aligned, in order; the overlay of G
    CHECK(GRAM_TAIL == REF_TAIL && GRAM_VEC == REF_VEC && GRAM_CAMREC == REF_CAMREC, "tail %d, vectors %d", GRAM_TAIL, GRAM_VEC);
    for (int rows = 1; rows <= 6 * GRAM_KMAX; rows++) for (int split = 0; split < 2; split++) {
        const GramSlice s = gram_slice(rows, split != 0);
        CHECK(s.len == gram_slice_doubles(rows, split != 0) && s.len == rows * GRAM_LD + REF_TAIL + (split ? REF_VEC : 0), "rows %d split %d: %d doubles", rows, split, s.len);
        CHECK(s.cam == rows * GRAM_LD && s.scale == s.cam + GRAM_KMAX * GRAM_CAMREC && s.slot == s.scale + 48, "rows %d: camera records %d, scales %d, slots %d", rows, s.cam, s.scale, s.slot);
        CHECK(0 < s.cam && s.cam < s.scale && s.scale + 6 * GRAM_KMAX <= s.slot, "rows %d: order", rows);
        const int slot_end_ints = 2 * s.slot + s.diag + GRAM_KMAX;       // in ints from the start of the slice
        CHECK(s.diag == GRAM_NPAIR && slot_end_ints <= 2 * s.vec && (2 * s.slot * 4) % 8 == 0, "rows %d: the slot table begins on an 8-byte boundary and ends in front of the vectors", rows);
        CHECK(s.vec == s.cam + GRAM_TAIL && 2 * s.vec >= slot_end_ints && s.vec + (split ? GRAM_VEC : 0) == s.len, "rows %d: the vectors begin behind the diagonal slots", rows);
        CHECK(GRAM_KMAX * 4 * 6 <= GRAM_VEC, "the vectors of %d cameras", GRAM_KMAX);
        // a slice begins on a 16-byte boundary only if its length is even -- the kernel's 16-byte reads of Y need no more than 8 (LD = 28: rows of 224 B)
        for (int w = 0; w < 4; w++) CHECK(((size_t)w * s.len * 8) % 8 == 0, "wave %d", w);
    }
    for (int DC : {3, 6}) {
        CHECK(gram_overlay_fits(DC), "DC %d: overlay", DC);
        for (int K = 1; K <= GRAM_KMAX; K++) {
            const int R = DC * K, last = gram_g_off(R - 1) + R - 1, room = R * GRAM_LD + GRAM_KMAX * GRAM_CAMREC;
            CHECK(gram_g_off(R - 1) == ref_g_off(R - 1) && last < room, "DC %d K %d: the last entry of G at %d of %d doubles", DC, K, last, room);
            for (int t4 = 0; t4 < 2; t4++) for (int ra = R; ra <= DC * GRAM_KMAX; ra += DC)
                CHECK(gram_g_extent(gram_tile_class(DC, K, t4 != 0), ra) <= gram_slice(ra, false).scale, "DC %d K %d in %d rows: the tiles store %d doubles", DC, K, ra, gram_g_extent(gram_tile_class(DC, K, t4 != 0), ra));
            // rows of G do not overlap: row R ends where row R + 1 begins (band t: 16 (t + 1) + 1 columns)
            for (int r = 0; r + 1 < R; r++) CHECK(gram_g_off(r + 1) - gram_g_off(r) >= r + 1 && gram_g_off(r + 1) - gram_g_off(r) >= 16 * (r >> 4) + 16, "row %d of G", r);
        }
    }
#if SSFM_GRAM_LD == 28
    CHECK(48 * GRAM_LD + GRAM_KMAX * GRAM_CAMREC - (gram_g_off(47) + 47 + 1) == 33, "K = 8 at 28: 33 doubles to spare");
#endif
    CHECK(gbs2_lds_bytes() == (size_t)GBS_WAVES * GBS2_TAIL * 8 && GBS2_TAIL == GBS_TAIL + 2 * GRAM_SUB_PTS * GBS2_PT && gbs2_lds_bytes() <= 48 * 1024, "k_gram_backsub2: %zu bytes", gbs2_lds_bytes());
    std::printf("%ld plans compared\n", g_cases);
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("GRAM_PATH_OK\n");
    return 0;
}
