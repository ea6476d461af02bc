// spherical_sfm_amd -- what the signature-group ("Gram") half of an LM iteration is launched with: the tile class of a task (written once, for the launch, the
// mixed-class kernel, the kernel tables and the planner's cost model), the LDS slice of a wave of schur_gram_task (one description: the kernel's pointers and the
// host's byte count), the share of a split task that a wave takes, and the plan of one solve (GramPath): the Gram launches of the assembly and the grouped back
// substitution.  Host-compilable, no HIP calls, no getenv: tests/native/gram_path_check.cpp holds the plan against a second implementation of its rules and walks
// the layout; the few functions the kernels call (ba_kernels.h) carry SSFM_GRAM_HD.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SSFM_GRAM_HD __host__ __device__ __forceinline__
#else
#define SSFM_GRAM_HD inline
#endif

namespace ssfm {

// ---- a task (BAFlat::gr_rec, ba_flatten.h) -------------------------------------------------------------------------------------------------
// runs of >= GRAM_MIN_RUN consecutive points observed by the same K cameras, GRAM_KMIN <= K <= GRAM_KMAX; GRAM_REC ints per task ([1] points, [2] K), GRAM_NPAIR pair
// slots; every kernel walks a task in sub-chunks of GRAM_SUB_PTS points
constexpr int GRAM_KMAX = 8, GRAM_NPAIR = 28, GRAM_REC = 48, GRAM_MIN_RUN = 32, GRAM_KMIN = 3, GRAM_SUB_PTS = 8;

// ---- tile classes ---------------------------------------------------------------------------------------------------------------------------
// The tasks are sorted by K, i.e. by rows = DC K of the Gram matrix: rows <= 16 -> one row tile of 16; 17..20 -> one tile + a tail of <= 4 rows through the 4x4x4
// instruction (t4); <= 32 -> two tiles; 33..36 -> two tiles + tail; else three tiles.  NT / TI = the template arguments of schur_gram_task for the class.
constexpr int GRAM_CLASSES = 5;
constexpr int GRAM_CLASS_NT[GRAM_CLASSES] = {1, 1, 2, 2, 3}, GRAM_CLASS_TI[GRAM_CLASSES] = {0, 2, 0, 3, 0};
constexpr bool GRAM_CLASS_DC3[GRAM_CLASSES] = {true, true, true, false, false};       // 3-dof cameras (rows <= 24) never reach the classes behind the third
// the three-tile class has no fused form: k_schur_gram<6, 3, 0> sits at its 256 registers and the point-pass prologue costs it 16 B more scratch -- a problem with
// such tasks keeps k_point_lin (gram_path: fuse_lin)
constexpr bool GRAM_CLASS_FUSED[GRAM_CLASSES] = {true, true, true, true, false};
SSFM_GRAM_HD constexpr int gram_tile_class(int DC, int K, bool t4) {
    const int rows = DC * K;
    return rows <= 16 ? 0 : (rows <= 20 && t4) ? 1 : rows <= 32 ? 2 : (rows <= 36 && t4) ? 3 : 4;
}

// ---- the LDS slice of one wave of schur_gram_task (ba_kernels.h) --------------------------------------------------------------------------------
#ifndef SSFM_GRAM_LD
#define SSFM_GRAM_LD 28      // row stride of the half products in LDS, doubles (swept in round 4: scripts/gpu_gram_ld.sh, profiles/r04_notes.md)
#endif
constexpr int GRAM_CAMREC = 34, GRAM_LD = SSFM_GRAM_LD;
constexpr int GRAM_SCALES = 48;                                              // Jacobi scale of Gram row DC k + d: 6 GRAM_KMAX
constexpr int GRAM_TAIL = GRAM_KMAX * GRAM_CAMREC + GRAM_SCALES + (GRAM_NPAIR + GRAM_KMAX) / 2;      // what follows the rows of Y, doubles
constexpr int GRAM_VEC = 4 * 6 * GRAM_KMAX;      // split task: behind a wave's slice, its cameras' vectors [K][diag U | Jc^T r | coupling term | S_fc][DC]
static_assert(GRAM_SCALES >= 6 * GRAM_KMAX && (GRAM_NPAIR + GRAM_KMAX) % 2 == 0 && GRAM_NPAIR == GRAM_KMAX * (GRAM_KMAX - 1) / 2, "the tail of a Gram slice");
// [rows_alloc][GRAM_LD] Y | camera records [GRAM_KMAX][GRAM_CAMREC] | scales | int pair slots [GRAM_NPAIR] | int diagonal slots [GRAM_KMAX] | split: the vectors.
// Offsets in doubles from the start of the slice, except diag: ints from the start of the slot table.
struct GramSlice { int cam, scale, slot, diag, vec, len; };
SSFM_GRAM_HD constexpr GramSlice gram_slice(int rows_alloc, bool split) {
    GramSlice s{};
    s.cam = rows_alloc * GRAM_LD; s.scale = s.cam + GRAM_KMAX * GRAM_CAMREC; s.slot = s.scale + GRAM_SCALES; s.diag = GRAM_NPAIR;
    s.vec = s.cam + GRAM_TAIL; s.len = s.vec + (split ? GRAM_VEC : 0);
    return s;
}
SSFM_GRAM_HD constexpr int gram_slice_doubles(int rows_alloc, bool split) { return gram_slice(rows_alloc, split).len; }
// Behind the sub-chunk loop the scaled tiles go back to LDS as the lower triangle of G, OVER the rows of Y and the camera records (both done by then): bands of 16
// rows, band t with 16 (t + 1) + 1 columns.  gram_g_off(R) = where row R begins.
SSFM_GRAM_HD constexpr int gram_g_off(int R) { const int t = R >> 4; return 128 * t * t + 144 * t + (R & 15) * (16 * t + 17); }
// doubles of G a task of class cls touches in a slice of rows_alloc rows: its full tiles store 16 columns per tile of every row < rows_alloc, the tail its 4 rows
constexpr int gram_g_extent(int cls, int rows_alloc) {
    const int NT = GRAM_CLASS_NT[cls], TI = GRAM_CLASS_TI[cls], full = std::min(16 * NT, rows_alloc);
    const int a = gram_g_off(full - 1) + 16 * ((full - 1) >> 4) + 16, b = TI > 0 ? gram_g_off(16 * NT + 3) + 16 * TI : 0;
    return std::max(a, b);
}
// the overlay stays in front of the scales and the slot tables, which the emission still reads: for every K of a launch sized for rows_alloc >= DC K rows
constexpr bool gram_overlay_fits(int DC) {
    for (int K = 1; K <= GRAM_KMAX; K++)
        for (int t4 = 0; t4 < 2; t4++)
            for (int rows_alloc = DC * K; rows_alloc <= DC * GRAM_KMAX; rows_alloc += DC) {
                const int room = rows_alloc * GRAM_LD + GRAM_KMAX * GRAM_CAMREC;
                if (gram_g_off(DC * K - 1) + DC * K - 1 >= room) return false;                       // the last entry of G
                if (gram_g_extent(gram_tile_class(DC, K, t4 != 0), rows_alloc) > room) return false;      // and whatever the tiles store beside it
            }
    return true;
}
static_assert(gram_overlay_fits(3) && gram_overlay_fits(6), "SSFM_GRAM_LD is too small: G, laid over the rows of Y and the camera records, would run into the scales and slot tables of the slice");

// ---- the share of a split task that one wave takes (schur_gram_task<..., SPLIT = true>) ---------------------------------------------------------
// A task is a run of cnt points walked in sub-chunks of GRAM_SUB_PTS points; with W waves per task, wave w takes a contiguous run of WHOLE sub-chunks
// [s_begin, s_end) (in points; only the task's last sub-chunk may be partial).  The nsub = ceil(cnt / 8) sub-chunks are dealt evenly: nsub / W each, the
// first nsub % W waves one more -- the longest share is ceil(nsub / W), and a share is empty only when there are fewer sub-chunks than waves (the rule of
// k_gram_backsub2, ceil(nsub / W) for every wave until none are left, has the same longest share but leaves a wave idle at e.g. 5 sub-chunks on 4 waves).
// tests/native/gram_split_check.cpp.
SSFM_GRAM_HD void gram_share(int cnt, int W, int w, int& s_begin, int& s_end) {
    const int nsub = (cnt + GRAM_SUB_PTS - 1) / GRAM_SUB_PTS, base = nsub / W, rem = nsub - base * W;
    const int b = w * base + (w < rem ? w : rem), n = base + (w < rem ? 1 : 0);
    s_begin = b * GRAM_SUB_PTS < cnt ? b * GRAM_SUB_PTS : cnt;
    s_end = (b + n) * GRAM_SUB_PTS < cnt ? (b + n) * GRAM_SUB_PTS : cnt;
}

// ---- the LDS slice of one wave of k_gram_backsub2 (ba_kernels.h) -----------------------------------------------------------------------------
// camera records | candidate records [GRAM_KMAX][GBS_CAMC] | the cameras' steps [GRAM_KMAX][6] | point records, two buffers [GRAM_SUB_PTS][GBS2_PT]
constexpr int GBS_CAMC = 12, GBS_TAIL = GRAM_KMAX * (GRAM_CAMREC + GBS_CAMC + 6), GBS_WAVES = 4;
constexpr int GBS2_PT = 18, GBS2_STAGE = 2 * GRAM_SUB_PTS * GBS2_PT, GBS2_TAIL = GBS_TAIL + GBS2_STAGE;
inline size_t gbs2_lds_bytes() { return (size_t)GBS_WAVES * GBS2_TAIL * sizeof(double); }

// ---- the plan of one solve -------------------------------------------------------------------------------------------------------------------
// Lab knobs that change the plan (knobs.h: live in the lab library only).  The defaults are the shipped values; ba_solver.hip fills the struct from SSFM_LAB_KNOB.
struct GramPathLab {
    int gram_waves = 1;             // SSFM_GRAM_WAVES      tasks (a wave each) per workgroup: 1 measured best (2: +14 %, 4: +13 % at the configs[4] size)
    bool t4 = true;                 // SSFM_GRAM_T4         the tail classes
    int emit_skip = 0;              // SSFM_GRAM_EMIT_SKIP  timing study: tasks without emission
    bool stamps = false;            // SSFM_GRAM_STAMPS     timing study: per-task phase stamps of the first Gram launch of the process
    int backsub_lpp = 0;            // SSFM_BACKSUB_LPP     > 0: lanes per point of k_point_backsub
    bool publish_fused = false;     // SSFM_PUBLISH_FUSED   the hand-over in the last workgroup of k_point_backsub: no grouped back substitution
};

struct GramPathIn {
    int DC = 6;
    const int* gr_rec = nullptr; int ng = 0;      // the task records, GRAM_REC ints each, sorted by K (BAFlat::gr_rec)
    int64_t gram_points = 0, gram_obs = 0, nP = 0, M = 0;      // points / observations in groups, points / observations of the problem
    bool pair_tasks = false, cam_sum_tasks = false;            // the assembly also runs k_schur_pairs2 / k_cam_sums2
    bool gram_any = true;           // SSFM_GRAM_ANY as the PLAN read it: one value for the cost model (ba_flatten.h) and the launch
    bool det = false;               // SSFM_DETERMINISTIC
    bool focal_free = false;
    int num_cus = 256;
    int env_fuse = 1;               // SSFM_GRAM_FUSE     0: k_point_lin + the unfused kernel (profiles/r09_notes.md)
    int env_split = 0;              // SSFM_GRAM_SPLIT    1..4 forces the waves per task of the Gram launches
    int env_backsub = -1;           // SSFM_GRAM_BACKSUB  0 / 1 forces k_gram_backsub2 off / on
    int env_gbs_split = 0;          // SSFM_GBS_SPLIT     > 0: waves per task of k_gram_backsub2
    int cnt(int t) const { return gr_rec[(size_t)t * GRAM_REC + 1]; }
    int K(int t) const { return gr_rec[(size_t)t * GRAM_REC + 2]; }
};

// one launch of k_schur_gram / k_schur_gram_split over the tasks [t0, t1) of one tile class, or of k_schur_gram_any over all of them (cls = the largest class)
struct GramLaunch {
    int cls = 0, t0 = 0, t1 = 0;
    int rows_alloc = 0;             // rows of Y in a slice: DC x the largest K of the range (its last task)
    int max_sub = 1;                // sub-chunks of the longest task of the range
    int waves = 1;                  // waves per task
    bool split = false;             // waves > 1: one task per workgroup, shared by its waves, a slice of LDS (+ the vectors) each; else a task per wave
    int grid = 0, block = 0; size_t lds = 0;
};

struct GramPath {
    GramPathLab lab;
    bool t4 = true, focal_free = false;       // arguments of the kernels, fixed for the solve
    bool fuse_lin = false;          // the Gram task does the point pass of its own points (ba_kernels.h: FUSE); k_point_lin does not run
    bool unsplit = false;           // every launch keeps one wave per task, whatever the counts say
    bool any = false;               // every tile class in ONE launch (k_schur_gram_any): any_launch, else launch[0 .. n_launch)
    GramLaunch any_launch;
    int n_cls = 0, n_launch = 0;    // classes in use (= launches of the per-class form)
    GramLaunch launch[GRAM_CLASSES];
    // back substitution
    bool grouped = false;           // the points of the groups take k_gram_backsub2, k_point_backsub skips them
    bool all_grouped = false;       // ... and k_point_backsub does not run: the residual check's workgroup rides with k_gram_backsub2
    int gbs_split = 1, gbs_grid = 0; size_t gbs_lds = 0;      // k_gram_backsub2: waves per task, workgroups (without the residual check's), bytes
    int backsub_lpp = 1;            // k_point_backsub: lanes per point (1 or 2)
};

inline GramPath gram_path(const GramPathIn& in, const GramPathLab& lab = GramPathLab()) {
    GramPath p; p.lab = lab; p.t4 = lab.t4; p.focal_free = in.focal_free;
    const int DC = in.DC, ng = in.ng;
    // one launch per tile class over a contiguous task range: cls_end[cl] = end of class cl's range
    int cls_end[GRAM_CLASSES] = {0, 0, 0, 0, 0};
    for (int t = 0; t < ng; t++) for (int cl = gram_tile_class(DC, in.K(t), lab.t4); cl < GRAM_CLASSES; cl++) cls_end[cl] = t + 1;
    for (int cl = 0; cl < GRAM_CLASSES; cl++) if (cls_end[cl] > (cl ? cls_end[cl - 1] : 0)) p.n_cls++;
    const int gram_waves = std::min(4, std::max(1, lab.gram_waves));
    const bool mixed = in.gram_any && p.n_cls > 1;      // tracks of mixed length: the classes side by side in one launch, LDS and registers of the largest class
    // Every point in a signature group, one Gram launch per tile class and nothing else in the assembly: the Gram task does the point pass of its own points in a
    // prologue and k_point_lin does not run; the speculative launch behind k_publish is then the Gram kernel of the NEXT iteration, accumulating into the next zone.
    // Not with pair or camera-sum tasks (they read PS of points other tasks own), not in the mixed-class launch, not with SSFM_DETERMINISTIC=1 (the fused epilogue
    // adds its sums with plain atomics), not with a task of the three-tile class (GRAM_CLASS_FUSED).
    bool all_fused = true;
    for (int cl = 0; cl < GRAM_CLASSES; cl++) if (!GRAM_CLASS_FUSED[cl] && cls_end[cl] > (cl ? cls_end[cl - 1] : 0)) all_fused = false;
    p.fuse_lin = in.env_fuse != 0 && !in.det && in.nP > 0 && ng > 0 && in.gram_points == in.nP && !in.pair_tasks && !in.cam_sum_tasks && !mixed && all_fused;
    // Waves per task of k_schur_gram (ba_kernels.h: SPLIT).  A wave of it takes half a SIMD's registers, so the chip holds 8 waves per CU: a launch with fewer
    // tasks than that gives every task W of them, W <= 4 and at most one per sub-chunk of the launch's longest task (config 2: 900 tasks -> 2; <= 512 -> 4;
    // the configs[4] size, thousands of tasks -> 1 = the unsplit kernel).  SSFM_GRAM_SPLIT=1..4 forces W.  SSFM_DETERMINISTIC=1 keeps W = 1 whatever the knob
    // says: its per-task partial buffer takes plain stores of ONE wave per task (det_acc.h), and the limbs' order independence is tested on the unsplit kernel.
    // The lab shapes and the mixed-class launch stay unsplit too.
    p.unsplit = in.det || lab.gram_waves != 1 || lab.emit_skip != 0 || lab.stamps || mixed;
    for (int cl = 0; cl < GRAM_CLASSES; cl++) {
        GramLaunch l; l.cls = cl; l.t0 = cl ? cls_end[cl - 1] : 0; l.t1 = cls_end[cl];
        if (l.t1 <= l.t0) continue;
        l.rows_alloc = DC * in.K(l.t1 - 1);
        for (int t = l.t0; t < l.t1; t++) l.max_sub = std::max(l.max_sub, (in.cnt(t) + GRAM_SUB_PTS - 1) / GRAM_SUB_PTS);
        // a workgroup lives on ONE CU: 8 / W of them fit there, so 4 waves per task while the tasks fit 2 per CU, 2 while they fit 4 per CU (3 holds no more
        // workgroups per CU than 4 does: 600 tasks x 3 waves ran in two rounds, 58.6 us against 51.8 with 2 -- profiles/r11_notes.md)
        const int ntask = l.t1 - l.t0, by_count = ntask <= 2 * in.num_cus ? 4 : ntask <= 4 * in.num_cus ? 2 : 1;
        l.waves = p.unsplit ? 1 : (in.env_split >= 1 && in.env_split <= 4) ? in.env_split : std::min(l.max_sub, by_count);
        l.split = l.waves > 1;
        l.grid = l.split ? ntask : (ntask + gram_waves - 1) / gram_waves;
        l.block = 64 * (l.split ? l.waves : gram_waves);
        l.lds = (size_t)(l.block / 64) * gram_slice_doubles(l.rows_alloc, l.split) * sizeof(double);
        p.launch[p.n_launch++] = l;
    }
    p.any = mixed && gram_waves == 1 && !p.fuse_lin;
    if (ng > 0) {
        GramLaunch& a = p.any_launch;
        a.cls = gram_tile_class(DC, in.K(ng - 1), lab.t4); a.t0 = 0; a.t1 = ng; a.rows_alloc = DC * in.K(ng - 1);
        a.grid = ng; a.block = 64; a.lds = (size_t)gram_slice_doubles(a.rows_alloc, false) * sizeof(double);
    }
    // Back substitution: the points of signature groups take k_gram_backsub2 (lane = observation, camera records in LDS); k_point_backsub keeps the others.  Its time
    // follows the POINTS (8 lanes per point whatever K), k_point_backsub's the observations: measured (rounds 3-5, k_gram_backsub) 27.3 / 28.1 us at K = 6 / 8 against
    // 23.4 / 31.7 (100k points) and 271 / 278 against 284 / 379 (1.5 M points).  Round 6, k_gram_backsub2: 195 us at 1.5 M points (K = 8), 21.1 against 23.0 us at
    // config 2 (K = 6, four waves per task): on from 6 observations per point on average.
    p.grouped = !lab.publish_fused && ng > 0 && (in.env_backsub < 0 ? in.gram_obs >= 6 * in.gram_points : in.env_backsub != 0);
    p.all_grouped = p.grouped && in.gram_points == in.nP;
    // waves per task: a small problem (config 2: 900 tasks on 1024 SIMDs) runs with several waves per SIMD, each with a share of its task's sub-chunks (config 2,
    // hipEvent: 1 wave per task 26.3 us, 2: 24, 4: 21.1, 6 / 8: 24; k_point_backsub 23.0).  Target: 14 waves per CU, ~3.5 per SIMD in flight (config 2: 900 tasks
    // x 4; 1200 tasks x 1 took 31 us, x 3: see profiles/r06_notes.md r06i)
    const int gbs_wave_target = 14 * in.num_cus;
    p.gbs_split = in.env_gbs_split > 0 ? std::min(8, in.env_gbs_split) : std::max(1, std::min(4, (gbs_wave_target + ng - 1) / std::max(1, ng)));
    p.gbs_grid = (ng * p.gbs_split + GBS_WAVES - 1) / GBS_WAVES;
    p.gbs_lds = gbs2_lds_bytes();
    // k_point_backsub with two lanes per point: half the dependent camera gathers per lane, twice the waves.  Measured at config 2 (scripts/lab/ab_lpp.sh, hipEvent
    // averages): 25.1-25.3 us against 23.0-23.5 with one lane per point; 2.557 against 2.538-2.552 ms per solve.  On LONG tracks it pays (r05ai) -- 300 cameras,
    // tracks of 3 ... 14 (8.5 observations per point, 70 000 points = one wave per SIMD): 40.1 -> 33.0 us; tracks 3 ... 8 (5.5 per point): 26.7 -> 28.7.  Two lanes
    // per point from 8.25 observations per point on.
    const int lpp = lab.backsub_lpp > 0 ? lab.backsub_lpp : (4 * in.M > 33 * in.nP ? 2 : 1);
    p.backsub_lpp = lpp == 2 ? 2 : 1;
    return p;
}

}  // namespace ssfm
