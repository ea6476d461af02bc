/* ssfm.h -- C ABI of the MI355X-native spherical-sfm optimisation core (libssfm_hip.so).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every entry point names the reference
 * interface (file:line under jonathanventura/spherical-sfm) that it replaces.  Matrices crossing this
 * boundary are COLUMN-MAJOR 3x3 (Eigen's default; the reference hands `Matrix3d::data()` to Ceres at
 * src/rotation_averaging.cpp:28-29), cameras are 6 doubles [t;r] (include/sphericalsfm/sfm_types.h:9,
 * src/sfm.cpp:104-105), points 3 doubles, observations principal-point-centred pixels
 * (examples/spherical_sfm_tools.cpp:907-908).
 *
 * Return value: 0 = ok, <0 = error (ssfm_last_error gives the text).  No exceptions cross the ABI.
 * A context is bound to one GPU and one HIP stream and is not thread-safe (one per host thread / rank).
 */
#ifndef SSFM_H
#define SSFM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSFM_OK 0
#define SSFM_ERR_INVALID -1
#define SSFM_ERR_HIP -2
#define SSFM_ERR_NO_DEVICE -3
#define SSFM_ERR_COMM -4

/* termination_type of ceres::Solver::Summary as the reference reads it (src/sfm.cpp:278-289) */
#define SSFM_CONVERGENCE 0
#define SSFM_NO_CONVERGENCE 1
#define SSFM_FAILURE 2
#define SSFM_NOTHING_TO_DO 3 /* src/sfm.cpp:230,265-268: Optimize() returns false before solving */

typedef struct ssfm_ctx ssfm_ctx;

/* ---- context ------------------------------------------------------------------------------ */
/* device < 0: current device.  stream: a hipStream_t passed as void*, NULL = context-owned stream. */
int ssfm_ctx_create(int32_t device, void* stream, ssfm_ctx** out);
void ssfm_ctx_destroy(ssfm_ctx* ctx);
const char* ssfm_last_error(const ssfm_ctx* ctx); /* ctx may be NULL: last creation error */
int ssfm_version(void);

/* Multi-GPU (one process per GPU; RCCL over xGMI).  Rank 0 obtains an id, the host side broadcasts the
 * 128 bytes with whatever it has (torch.distributed in bench.py), every rank calls ssfm_comm_init. */
int ssfm_comm_unique_id(uint8_t id[128]);
int ssfm_comm_init(ssfm_ctx* ctx, const uint8_t id[128], int32_t nranks, int32_t rank);
/* Alternative to RCCL: the caller supplies the collective (MPI, gloo, a test harness).  The library stages each reduction
 * through pinned host memory and calls fn(user, buf, n, op) with op = SSFM_REDUCE_SUM / SSFM_REDUCE_MAX; fn must leave the
 * element-wise reduction over all ranks in buf and return 0.  Same sharding and the same reductions as the RCCL path. */
enum { SSFM_REDUCE_SUM = 0, SSFM_REDUCE_MAX = 1 };
typedef int (*ssfm_host_allreduce_fn)(void* user, double* buf, uint64_t n, int32_t op);
int ssfm_comm_init_host(ssfm_ctx* ctx, int32_t nranks, int32_t rank, ssfm_host_allreduce_fn fn, void* user);

/* Timing probe of bench.py (`timing_without_collective`), not a product setting: while on, the bundle-adjustment reductions of this context return at once, so
 * every rank iterates on its own shard (kernels and sizes of the sharded solve, results meaningless).  Warns on stderr when switched on. */
int ssfm_debug_timing_skip_collectives(ssfm_ctx* ctx, int32_t on);

/* Measured device copy bandwidth ("denominator = measured device copy bandwidth on the box, nominal also quoted"): `reps` launches of a float4
 * grid-stride copy of `bytes` bytes (>= 256 MB: beyond the Infinity Cache); GBs_out = bytes read + bytes written per second, in GB/s.  bench.py reports it. */
int ssfm_debug_copy_bandwidth(ssfm_ctx* ctx, uint64_t bytes, int32_t reps, double* GBs_out);

/* ---- bundle adjustment: replaces the body of sphericalsfm::SfM::Optimize (src/sfm.cpp:228-290) --- */
typedef struct {
    int32_t num_cameras;
    int32_t num_points;
    int64_t num_observations;
    double* cameras;            /* [num_cameras*6] [t;r], in/out  (GetCameraPtr, src/sfm.cpp:89-92) */
    double* points;             /* [num_points*3], in/out         (GetPointPtr,  src/sfm.cpp:94-97) */
    double* focal;              /* &intrinsics.focal, in/out      (src/sfm.cpp:220) */
    const double* obs_xy;       /* [M*2] */
    const int32_t* obs_cam;     /* [M] */
    const int32_t* obs_pt;      /* [M] */
    const uint8_t* rot_fixed;   /* [num_cameras] rotationFixed, NULL = all free     (src/sfm.cpp:224) */
    const uint8_t* trans_fixed; /* [num_cameras] translationFixed, NULL = all free  (src/sfm.cpp:223) */
    const uint8_t* pt_fixed;    /* [num_points] pointFixed, NULL = all free         (src/sfm.cpp:225) */
    int32_t focal_fixed;        /* focalFixed                                        (src/sfm.cpp:222) */
} ssfm_ba_problem;

typedef struct {
    /* ConfigureSolverOptions / PreOptimize values (src/sfm.cpp:194-212), rest Ceres 2.2.0 defaults */
    int32_t max_num_iterations;                /* 2000 */
    int32_t max_num_consecutive_invalid_steps; /* 100 */
    double function_tolerance;                 /* 1e-6 */
    double gradient_tolerance;                 /* 1e-10 */
    double parameter_tolerance;                /* 1e-8 */
    double initial_trust_region_radius;        /* 1e4 */
    double max_trust_region_radius;            /* 1e16 */
    double min_trust_region_radius;            /* 1e-32 */
    double min_lm_diagonal, max_lm_diagonal;   /* 1e-6, 1e32 */
    double min_relative_decrease;              /* 1e-3 */
    int32_t loss_type;                         /* 0 trivial, 1 Cauchy, 2 SoftLOne; default 1 */
    double loss_scale;                         /* 1.0 */
    int32_t jacobi_scaling;                    /* 1 */
    /* reduced-camera-system solver.  The reference solves it directly (SPARSE_SCHUR: sparse Cholesky, src/sfm.cpp:205) and so does this build by
     * default: an exact block-banded Cholesky in Cuthill-McKee order (twisted / substructured for long components).  The PCG of
     * north_star survives as a REFINEMENT that runs only when |rhs - S y| > pcg_tolerance |rhs| after the direct solve -- never observed, 0 sweeps in
     * every measured solve -- and as the block-Jacobi comparison solver (preconditioner = 1).  The "pcg" in field names below is historical: they time
     * and count the reduced solve, whichever solver ran. */
    int32_t pcg_max_iterations;                /* 1000 */
    double pcg_tolerance;                      /* |r| <= tol |b|, default 1e-10 (tracks a direct solve) */
    int32_t preconditioner;                    /* 0: block-banded Cholesky (exact on the Cuthill-McKee band) + PCG
                                                  refinement; 1: block-Jacobi PCG */
    int32_t verbose;                           /* 1: one line per LM iteration (minimizer_progress_to_stdout) */
} ssfm_ba_options;

typedef struct {
    int32_t termination;          /* SSFM_CONVERGENCE ... */
    int32_t iterations;
    int32_t num_successful_steps, num_unsuccessful_steps;
    int32_t num_linearizations;   /* n_LM of SURVEY 8d: every assemble+solve, accepted or rejected */
    int32_t pcg_iterations_total;
    double initial_cost, final_cost;
    int64_t num_residual_blocks;  /* observations that entered the problem (this rank) */
    int64_t num_residual_blocks_global;
    int32_t num_points_used;
    int32_t camera_dof;           /* 3 = spherical (all translations fixed), 6 = general */
    double t_flatten_s, t_upload_s, t_solve_s, t_download_s;   /* host wall-clock */
    double t_kernel_linearize_ms, t_kernel_schur_ms, t_kernel_pcg_ms, t_kernel_update_ms; /* hipEvent sums; "pcg" = the reduced solve (banded Cholesky + back substitution) */
    int32_t reduced_blocks;       /* non-zero DCxDC blocks of the reduced camera system */
    int32_t band_half_width;      /* block half-bandwidth of S in the Cuthill-McKee order */
    int32_t band_segments;        /* workgroups of the reduced-system factorisation: connected components, long ones cut */
    int32_t band_separators;      /* into segments by this many separators of band_half_width block rows (0 = none cut) */
    /* bounded problems (ssfm_posegraph_focal_solve): Ceres' projected line search inside the trust-region loop */
    int32_t num_line_search_evaluations;   /* function evaluations beyond the candidate's */
    int32_t num_line_search_contractions;  /* iterations whose step the search shortened */
} ssfm_ba_summary;

void ssfm_ba_default_options(ssfm_ba_options* o);

/* Test probe for the reduced-system solver (the stand-in for Ceres' SPARSE_SCHUR Cholesky, src/sfm.cpp:276-279): factor + solve
 * a caller-supplied symmetric positive definite block band.  band: [N][b+1][dc*dc], block d of row i = (i, i-d), rows in band
 * order; comp_ptr: [ncomp+1] contiguous row ranges of independent components; Y: [2][N*dc] right-hand sides in, solutions out.
 * segs_seps_fail: [3] = factorisation workgroups, separators (0 = no component was cut), non-positive-pivot flag.
 * Zdump [b*dc][N*dc], Ddump [seps][b*dc][b*dc], Tdump [seps][2][b*dc]: intermediates of the substructured path, or NULL. */
int ssfm_band_solve_probe(ssfm_ctx* ctx, int32_t dc, int32_t N, int32_t b, int32_t ncomp, const int32_t* comp_ptr, const double* band,
                          double* Y, int32_t* segs_seps_fail, double* Zdump, double* Ddump, double* Tdump);

/* Test probe (round 6): the supernodal ring / chain solver of the reduced camera system alone (csrc/snode.h; it takes the place of the sparse Cholesky
 * inside Ceres' SPARSE_SCHUR, reference src/sfm.cpp:205,273, whenever every component of the camera graph is a chain or a closed loop whose tracks span
 * <= 30 / dc cameras).  S: block-CSR (row_ptr [Nc + 1], col_idx), every coupled pair of cameras stored once in either orientation plus the diagonal blocks,
 * row-major dc x dc blocks; rhs2: [2][Nc * dc]; nr = 1 | 2 right-hand sides; Y: [2][Nc * dc] out (camera order).
 * info: [4] = {1 if the plan applies (else nothing ran), workgroups, rows of the closing separator, non-positive-pivot flag}. */
int ssfm_snode_solve_probe(ssfm_ctx* ctx, int32_t dc, int32_t Nc, const int32_t* row_ptr, const int32_t* col_idx, const double* S_val, const double* rhs2,
                           int32_t nr, double* Y, int32_t* info);
/* Host-only (no GPU): the plan of that solver for a block structure.  sizes: [8] = {applies, workgroups, rows reserved for the closing separator, cameras per supernode,
 * capacity of a node's camera list, ints of half_rec, of step_rec, of node_cam}; the tables (layouts: csrc/snode.h) are copied out when the pointers are non-null;
 * tab_len: capacity of tab in, its length out. */
int ssfm_snode_plan_probe(int32_t dc, int32_t Nc, const int32_t* row_ptr, const int32_t* col_idx, int32_t num_cus, int32_t* sizes, int32_t* half_rec, int32_t* step_rec,
                          int32_t* node_cam, int32_t* tab, int32_t* tab_len);

/* Host-only planning (no GPU needed): what the flatten rules of src/sfm.cpp:240-263 keep, how the used points
 * are sharded over ranks (contiguous ranges balanced by observations), and the camera elimination order. */
typedef struct {
    int32_t camera_dof, num_points_used, num_points_used_global, reduced_blocks, band_half_width, max_row_blocks;
    int64_t num_observations_used, num_observations_used_global;
    int32_t band_segments, band_separators;   /* as in ssfm_ba_summary (SSFM_BAND_SEGMENTS=1 disables cutting, =P forces P per component) */
    /* round 3: points of this rank whose Schur blocks are assembled as Gram products on the matrix cores (runs of >= 32 consecutive points with the same 3..8
     * cameras; everything else goes through the sorted pair lists), their observations, and the wave tasks they are cut into */
    int64_t num_points_grouped, num_observations_grouped;
    int32_t group_tasks, reserved;
} ssfm_ba_plan_info;
/* point_ids: [num_points] capacity or NULL (receives the original ids of this rank's used points, in order);
 * obs_used: [num_observations] or NULL (1 where the observation enters this rank's problem);
 * cam_pos: [num_cameras] or NULL (camera -> position in the elimination order). */
int ssfm_ba_plan(const ssfm_ba_problem* p, int32_t nranks, int32_t rank, ssfm_ba_plan_info* info, int32_t* point_ids,
                 uint8_t* obs_used, int32_t* cam_pos);

/* One call = flatten (src/sfm.cpp:240-263 rules) + upload + device LM loop + scatter back.
 * The context keeps the resident plan of the last problem STRUCTURE it solved (observation ids in order, fixed masks, which
 * points are zero, sizes): a call with the same structure only uploads parameters and pixels -- the drivers' Optimize ->
 * Retriangulate -> Optimize pattern.  summary.t_flatten_s is 0 on such a call.  SSFM_NO_PLAN_CACHE=1 in the environment
 * disables the cache; ssfm_ctx_destroy releases it.
 * Reproducibility: by default the assembly of the reduced camera system adds with fp64 atomics, so repeated solves agree to ~1e-11, not bit for bit (Ceres' own
 * multi-threaded evaluation behind src/sfm.cpp:276 is in the same position).  SSFM_DETERMINISTIC=1 in the environment, read when a handle is created, switches a
 * single-GPU handle to order-independent accumulation (csrc/det_acc.h): bit-identical repeats.  A problem whose points all sit in signature groups takes the
 * atomics-free Gram emission + fold at +3...7 % of the iteration time; the others add fixed-point limbs with integer atomics at ~1.2x.
 * A context with a communicator refuses it (SSFM_ERR_INVALID). */
int ssfm_ba_solve(ssfm_ctx* ctx, ssfm_ba_problem* p, const ssfm_ba_options* o, ssfm_ba_summary* s);

/* Staged form: problem stays resident in HBM between runs (bench.py, multi-GPU sharding). */
typedef struct ssfm_ba_handle ssfm_ba_handle;
int ssfm_ba_create(ssfm_ctx* ctx, const ssfm_ba_problem* p, const ssfm_ba_options* o, ssfm_ba_handle** out);
int ssfm_ba_reset(ssfm_ba_handle* h);                          /* restore the uploaded initial parameters */
int ssfm_ba_run(ssfm_ba_handle* h, ssfm_ba_summary* s);        /* device LM loop only */
int ssfm_ba_download(ssfm_ba_handle* h, ssfm_ba_problem* p);   /* scatter parameters back */
void ssfm_ba_destroy(ssfm_ba_handle* h);
/* one evaluation at the uploaded state, for kernel parity tests: cost, residuals [M*2] (robustified),
 * jacobians [M*2*10] (focal | t | r | X, robustified, unscaled); entries of unused observations are 0. */
int ssfm_ba_evaluate(ssfm_ba_handle* h, double* cost, double* residuals, double* jacobians);
/* on != 0: bracket every kernel launch of ssfm_ba_run with hipEvents (slower; for bench.py's profile leg) */
int ssfm_ba_set_profiling(ssfm_ba_handle* h, int32_t on);
/* per-kernel timing of the last run: name -> (launches, total ms); returns number of entries written */
int ssfm_ba_kernel_times(ssfm_ba_handle* h, int32_t max_entries, char names[][32], int64_t* launches, double* total_ms);

/* ---- SO(3) pose graphs ------------------------------------------------------------------------------
 * rotations: [n*9] column-major 3x3 (std::vector<Eigen::Matrix3d>), in/out; index0/index1/rel_rotations: the fields of
 * sphericalsfm::RelativeRotation (include/sphericalsfm/rotation_averaging.h:9-14), rel = R1 * R0^T, column-major.
 * Options: ssfm_ba_options with the pose-graph defaults (Ceres defaults: 50 iterations, 5 invalid steps;
 * SoftLOneLoss(0.03)).  summary->final_cost is the value the reference functions return. */
void ssfm_rotavg_default_options(ssfm_ba_options* o);
/* optimize_rotations (src/rotation_averaging.cpp:44-91).
 * LARGE GRAPHS AND THE 50-ITERATION CAP (src/rotation_averaging.cpp:75-80 solves with Ceres' default max_num_iterations = 50): from about 2000 nodes on the
 * capped run has NOT converged, and where it stops depends on the order in which the implementation sums -- ANY implementation, Ceres with another thread count
 * included.  Measured on the 2000 / 4000-node rings of tests/test_rotavg_gpu.py: this library and the CPU oracle, two summation orders of the same algorithm, end
 * up to 0.3 rad apart in single rotations with final costs within 5 %.  What IS reproducible is the converged minimum: with max_num_iterations raised until the
 * tolerances fire, this library's answer is a fixed point of the oracle to < 1e-5 rad (the oracle restarted from it moves less than that).  A caller who needs
 * north_star's 1e-5 on such graphs must raise options->max_num_iterations (a few hundred suffice); with the reference's cap the contract is "same cost band". */
int ssfm_rotavg_solve(ssfm_ctx* ctx, int32_t n, double* rotations, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                      const double* rel_rotations, const ssfm_ba_options* o, ssfm_ba_summary* s);
/* get_cost (src/uncalibrated_pose_graph.cpp:116-145) */
int ssfm_rotavg_cost(ssfm_ctx* ctx, int32_t n, const double* rotations, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                     const double* rel_rotations, double* cost);
/* optimize_rotations_and_focal_length (src/uncalibrated_pose_graph.cpp:147-203); *focal_length is multiplied by the
 * optimised multiplier, which is kept inside [min_focal, max_focal] / focal_length */
int ssfm_posegraph_focal_solve(ssfm_ctx* ctx, int32_t n, double* rotations, int32_t num_edges, const int32_t* index0,
                               const int32_t* index1, const double* rel_rotations, double* focal_length, double min_focal,
                               double max_focal, const ssfm_ba_options* o, ssfm_ba_summary* s);

/* ---- batched spherical relative-pose RANSAC ----------------------------------------------------------
 * Replaces the OpenMP loop body of estimate_pairwise (examples/spherical_sfm_tools.cpp:332-420): per image pair
 * LocallyOptimizedMSAC<..., SphericalEstimator>::EstimateModel (include/RansacLib/ransac.h:128) with the action-matrix
 * minimal solver, final least squares, inlier mask and Decompose.  Pair p owns rays [pair_ptr[p], pair_ptr[p+1]) of
 * u / v ([total*3]; u = first view, v = second view, as RayPair, include/sphericalsfm/ray.h:8-10).
 * squared_inlier_threshold = (inlier_threshold_px * Kinv(0,0))^2 (spherical_sfm_tools.cpp:315).
 * Outputs (any may be NULL): E, R [num_pairs*9] column-major; inlier_mask [total]; num_inliers, scores [num_pairs].
 * R is the identity where num_inliers <= min_num_inliers (the reference skips such pairs, :410).
 *
 * mode: how the hypotheses of a pair are generated.
 *   SSFM_RANSAC_REFERENCE_TRACE (default): RansacLib's LocallyOptimizedMSAC control flow, draw for draw -- both std::mt19937 streams
 *     (seeded with `seed`, include/RansacLib/sampling.h:52, ransac.h:145-146) and libstdc++'s uniform_int_distribution are restated
 *     on the device, so a pair evaluates the reference's minimal samples, runs LocalOptimization (ransac.h:341-407: the initial
 *     least-squares fit on <= min_sample_multiplicator * 3 shuffled inliers, then num_lo_steps x [NonMinimalSolver + iterated fits])
 *     at the reference's iterations, adapts max_num_iterations from the inlier ratio (utils.h:110-140) and stops where the reference
 *     stops.  Differences to a CPU build are floating-point rounding.  A chunk of iterations is evaluated in parallel, one lane each.
 *     Rounding caveats of that sweep: the Sampson quotient of the hypothesis phase uses the hardware reciprocal + two Newton steps (~1 ulp)
 *     where the CPU divides, so a strict "<" between two scores that agree to the last bits may go the other way (never observed to change a
 *     result: 256 of 256 test pairs and 200 sampled pairs of the full BASELINE configs[3] run replay the oracle's trace); and with LO steps
 *     on, NonMinimalSolver on an ill-conditioned sample can differ from a CPU eigen-solver by far more than rounding (tolerances).
 *   SSFM_RANSAC_FIXED_BUDGET: num_hypotheses counter-based samples per pair scored in parallel, best one refined on its inliers
 *     (no LO, no adaptive stopping; statistically equivalent result, more arithmetic). */
#define SSFM_RANSAC_FIXED_BUDGET 0
#define SSFM_RANSAC_REFERENCE_TRACE 1
typedef struct {
    int32_t num_hypotheses;      /* FIXED_BUDGET: minimal samples per pair (default 1024) */
    uint32_t seed;               /* RansacOptions::random_seed_ (default 0) */
    int32_t min_num_inliers;     /* acceptance threshold of estimate_pairwise */
    int32_t final_least_squares; /* LORansacOptions::final_least_squares_ (default 1, spherical_sfm_tools.cpp:318) */
    int32_t inward;              /* SphericalEstimator(..., inward) */
    int32_t use_poly_solver;     /* SphericalEstimator(..., use_poly_solver, ...): 0 = action matrix (estimate_pairwise's choice), 1 = quartic */
    int32_t mode;                /* SSFM_RANSAC_REFERENCE_TRACE */
    uint32_t min_num_iterations, max_num_iterations;   /* RansacOptions: 100, 10000 (ransac.h:50-51) */
    double success_probability;  /* 0.9999 (ransac.h:52) */
    int32_t num_lo_steps;        /* estimate_pairwise sets 0 (spherical_sfm_tools.cpp:316); LORansacOptions default 10 */
    int32_t num_lsq_iterations;  /* estimate_pairwise sets 0 (:317); default 4 */
    double threshold_multiplier; /* sqrt(2) (ransac.h:67) */
    int32_t min_sample_multiplicator;   /* 7: least-squares fits use <= 7 * 3 inliers (ransac.h:69,412); 1..21 */
    int32_t non_min_sample_multiplier;  /* 3: non-minimal samples hold max(4, min(3 * 3, inliers / 2)) rays (ransac.h:70,369-373); 1..3 */
    uint32_t lo_starting_iterations;    /* 50 (ransac.h:71) */
    int32_t fast_shuffle;        /* 1: the draws of a Fisher-Yates tail that is thrown away are only checked for rejections, in parallel (same stream) */
} ssfm_ransac_options;
void ssfm_ransac_default_options(ssfm_ransac_options* o);
/* stats: [num_pairs*2] = RansacStatistics::num_iterations, number_lo_iterations per pair (zeros in FIXED_BUDGET mode), or NULL.
 * Pairs are streamed through the GPU in slabs (two pinned staging buffers, the upload of slab k+1 under the kernels of slab k), so one
 * call may hold any number of pairs (BASELINE configs[3]: 2000 frames = 1 999 000 pairs); pairs with more than ~2700 correspondences
 * keep their rays in HBM/L2 instead of LDS. */
int ssfm_ransac_batch(ssfm_ctx* ctx, int32_t num_pairs, const int32_t* pair_ptr, const double* u, const double* v,
                      double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R, uint8_t* inlier_mask,
                      int32_t* num_inliers, double* scores, uint32_t* stats);
/* Multi-GPU form of the same call (BASELINE configs[3]: exhaustive pairwise RANSAC over several GPUs; the reference's
 * counterpart is the `#pragma omp parallel for` over matches, spherical_sfm_tools.cpp:332).  Every rank of the context's
 * communicator (ssfm_comm_init / ssfm_comm_init_host) passes the SAME full arguments; rank r estimates pairs r, r + nranks, ...
 * with the random streams of their global indices, and one sum all-reduce returns every pair's result on every rank --
 * bit-identical to ssfm_ransac_batch on one GPU.  Without a communicator it is ssfm_ransac_batch. */
int ssfm_ransac_batch_sharded(ssfm_ctx* ctx, int32_t num_pairs, const int32_t* pair_ptr, const double* u, const double* v,
                              double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R,
                              uint8_t* inlier_mask, int32_t* num_inliers, double* scores, uint32_t* stats);
/* The same estimation from what estimate_pairwise really holds (examples/spherical_sfm_tools.cpp:340-375): per-frame feature lists and per-pair
 * match lists.  feat_rays[feat_ptr[f] + k] = Kinv (x, y, 1) of feature k of frame f (:362-370, computed once per feature instead of once per
 * match); pair p matches feature match_idx0[i] of frame pair_frame0[p] with feature match_idx1[i] of frame pair_frame1[p] for i in
 * [match_ptr[p], match_ptr[p+1]).  The feature rays are uploaded once, the match lists stream through the pinned double buffer (8 bytes per
 * correspondence instead of the 48 of ssfm_ransac_batch: BASELINE configs[3] moves 8 GB instead of 48 GB) and a gather kernel lays the ray
 * pairs out on the device.  Outputs and random streams exactly as ssfm_ransac_batch on the gathered rays (inlier_mask indexed like the matches). */
int ssfm_ransac_batch_indexed(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const double* feat_rays,
                              int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1, const int32_t* match_ptr,
                              const int32_t* match_idx0, const int32_t* match_idx1,
                              double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R, uint8_t* inlier_mask,
                              int32_t* num_inliers, double* scores, uint32_t* stats);
/* The indexed form over the ranks of the context's communicator (multi-GPU estimate_pairwise, BASELINE configs[3]): every rank passes the SAME full
 * arguments, uploads the feature rays of all frames and the match lists of ITS pairs (r, r + nranks, ...), and the result table of
 * ssfm_ransac_batch_sharded is all-reduced -- bit-identical to ssfm_ransac_batch_indexed on one GPU.  Without a communicator it is that call. */
int ssfm_ransac_batch_indexed_sharded(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const double* feat_rays,
                                      int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1, const int32_t* match_ptr,
                                      const int32_t* match_idx0, const int32_t* match_idx1,
                                      double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R, uint8_t* inlier_mask,
                                      int32_t* num_inliers, double* scores, uint32_t* stats);
/* Measurement aid (the RANSAC leg is priced in FP64 flop/s of Sampson scoring, not GB/s): device time of the kernels of this context's last
 * ssfm_ransac_batch* call, summed over its slabs (hipEvent brackets on the solver stream; uploads and read-backs are outside).  No reference counterpart. */
int ssfm_ransac_last_kernel_ms(ssfm_ctx* ctx, double* ms);
/* ---- general relative pose: five-point LO-MSAC per image pair (examples/spherical_sfm_tools.cpp:433-573, `-fivepoint`) ----------------
 * estimate_pairwise_five_point per pair: LocallyOptimizedMSAC over SteweniusEstimator (evaluation/five_point/stewenius_estimator.cpp) with the
 * one-sided epipolar-line residual of FivePointEstimator::EvaluateModelOnPoint (five_point_estimator.cpp:115-125: line = E (u / u2),
 * (v . line)^2 / (line0^2 + line1^2); v is not renormalised), inlier flags by residual < threshold, acceptance num_inliers > min_num_inliers,
 * then PoseFromEssentialMatrix on the inliers (:15-113).  No spherical-motion assumption: R is a general rotation and t a unit translation
 * (x1 = R x0 + t), R = identity and t = 0 where the pair is not accepted.  u, v, pair_ptr, E, inlier_mask, num_inliers, scores, stats and the
 * slabs, random streams and ssfm_ransac_last_kernel_ms are those of ssfm_ransac_batch; t: [num_pairs*3].  Rays need a nonzero third component.
 *
 * Options: the struct of ssfm_ransac_batch as it is.  Used: seed, min_num_inliers, min_num_iterations, max_num_iterations,
 * success_probability, threshold_multiplier, lo_starting_iterations, fast_shuffle.  IGNORED: inward, use_poly_solver, num_lo_steps,
 * num_lsq_iterations (estimate_pairwise_five_point sets both 0), non_min_sample_multiplier, min_sample_multiplicator,
 * final_least_squares and mode (reference-trace only; there is no fixed-budget form).
 *
 * The control flow is RansacLib's for a minimal sample of five, draw for draw (n = 5..7 take ShuffleSample, n >= 8 DrawSample; fewer than
 * five correspondences: no model).  SteweniusEstimator::NonMinimalSolver returns 0 and LeastSquares is empty, so LocalOptimization and the
 * final least squares change no model: LocalOptimization still runs where the reference runs it (it counts in stats and its shuffle of the
 * relaxed inlier list advances the second random stream), the final least squares -- a re-score of the same model -- is not run.
 *
 * Departures from the reference, all stated here:
 *  * The minimal solver is written from the mathematics (nullspace, the ten cubic constraints, elimination to a degree-10 polynomial in
 *    one coordinate, real roots by bracketing), not from the reference's generated code, and returns the REAL solutions only, in ascending
 *    order of that coordinate.  The reference also returns the real parts of complex eigenvectors (stewenius_estimator.cpp:40-57), which
 *    satisfy no constraint; they can only win an iteration's score by accident.  A sample whose 5x9 system is rank-deficient (a row's part
 *    outside the others below 1e-10 of its length) or whose elimination meets a pivot below 1e-12 yields no model.
 *  * Agreement with a build of the reference's solver_stewenius is not pinned (it needs Eigen); tests compare with a numpy restatement.
 *  * num_inliers counts the inlier flags (the existing call's convention); RansacLib's returned count is that of the same model.
 *  * With two equal singular values, which rotation DecomposeEssentialMatrix calls R1 and the sign of t are the SVD routine's choice.  Here
 *    the entry of t of largest magnitude is made positive and R1 is the rotation with <[t]x R1, E> > 0; the four candidates are then
 *    (R1, t) (R2, t) (R1, -t) (R2, -t) and the last one with the largest vote wins, as in the reference.  The order matters only in a tie. */
int ssfm_ransac5_batch(ssfm_ctx* ctx, int32_t num_pairs, const int32_t* pair_ptr, const double* u, const double* v,
                       double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R, double* t,
                       uint8_t* inlier_mask, int32_t* num_inliers, double* scores, uint32_t* stats);
/* The same from feature tables and match lists: the arguments of ssfm_ransac_batch_indexed plus t. */
int ssfm_ransac5_batch_indexed(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const double* feat_rays,
                               int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1, const int32_t* match_ptr,
                               const int32_t* match_idx0, const int32_t* match_idx1,
                               double squared_inlier_threshold, const ssfm_ransac_options* o, double* E, double* R, double* t,
                               uint8_t* inlier_mask, int32_t* num_inliers, double* scores, uint32_t* stats);
/* Probes of the pieces; each runs the device function the batch kernel runs.
 * ssfm_fivepoint_solver_probe: the minimal solver on S samples (samples [S*5] ray indices) -> Es [S*10*9] (column-major 3x3, zero beyond
 *   counts[s]), counts [S].
 * ssfm_fivepoint_residual_probe: the residual of T models (Es [T*9]) on every ray -> errors [T*n].
 * ssfm_fivepoint_pose_probe: PoseFromEssentialMatrix of task k on the rays lists[task_ptr[k] .. task_ptr[k+1]) with E [tasks*9] ->
 *   R [tasks*9], t [tasks*3], votes [tasks*4] (the four candidates in the order above).
 * ssfm_fivepoint_max_lds_rays: the largest pair whose rays the batch kernel keeps in LDS (5 doubles per ray beside the generator states);
 *   larger pairs, or every pair while SSFM_RANSAC5_FORCE_GLOBAL=1 is set (read at call time), read their rays from global memory. */
int ssfm_fivepoint_solver_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t S, const int32_t* samples, double* Es, int32_t* counts);
int ssfm_fivepoint_residual_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t T, const double* Es, double* errors);
int ssfm_fivepoint_pose_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t tasks, const int32_t* task_ptr,
                              const int32_t* lists, const double* E, double* R, double* t, int32_t* votes);
int32_t ssfm_fivepoint_max_lds_rays(void);
/* ---- brute-force descriptor matching: match() / match_exhaustive() (examples/spherical_sfm_tools.cpp:235-251, :575-600) ---------------
 * Per pair, train = the descriptors of frame pair_frame0[p] (n0 x dim floats), query = those of pair_frame1[p] (n1 x dim).  For every query i:
 * its nearest train j1 and second nearest j2 by L2 distance (cv::BFMatcher::knnMatch(query, train, 2)), dist = sqrtf(sum (q - t)^2) as a float;
 * if (double)dist1 < ratio * (double)dist2 then m01[j1] = i.  m01 is a std::map, so a later query overwrites an earlier one: the list of a pair is
 * (j, i) in ascending j, each j once, i the LARGEST passing query whose nearest train is j -- what ImageMatch::matches holds and what
 * ssfm_ransac_batch_indexed takes as match_idx0 / match_idx1.
 * Device: distances as a tiled T . Q^T on the f32-input matrix instruction (exact f32), ranked by |t|^2 - 2 q.t with a running best / second best
 * per query (the n1 x n0 matrix is never stored); the two finalists of a query are then re-evaluated as sum (q - t)^2 in f32, square-rooted
 * (correctly rounded) and compared as above; an atomic max per train slot and a scan produce the lists.  Bit-identical from run to run.
 * EXACT for SIFT descriptors (floats holding integers 0..255): every partial sum is an integer < 2^24, so every summation order and the product form
 * give the same f32 and the lists equal the reference's.  For general floats the finalists may differ from OpenCV's where two candidates are within
 * f32 rounding of each other (parity unpinned: OpenCV is not part of this build).
 * Defined here, undefined in the reference: a pair whose train frame has fewer than 2 features yields no matches (the reference indexes past
 * matches[i]); equal distances rank the lower train index first (this only shows for ratio >= 1: with ratio < 1 a tie dist1 == dist2 never passes
 * and only the VALUE of dist2 enters the test). */
typedef struct {
    double ratio;       /* 0.75 (spherical_sfm_tools.h:70) */
    int32_t dim;        /* 128; a multiple of 4, 4..128 */
    int32_t reserved;
} ssfm_match_options;
void ssfm_match_default_options(ssfm_match_options* o);
/* Frame f owns descriptors [feat_ptr[f], feat_ptr[f+1]) of descs ([feat_ptr[num_frames] * dim] floats, uploaded once per call).  Any number of pairs:
 * they are processed in slabs that bound the slot buffer (environment SSFM_MATCH_SLAB_PAIRS, read at every call, forces the slab length).
 * match_ptr [num_pairs + 1] is always written; match_idx0 / match_idx1 [capacity] may both be NULL (counts only).  If the total exceeds capacity the
 * call returns SSFM_ERR_INVALID with the needed total in match_ptr[num_pairs] (the lists written so far are those of whole slabs that fitted).
 * Arguments are checked before any launch (frame ids, dim, ratio > 0, ascending feat_ptr). */
int ssfm_match_pairs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, int32_t num_pairs,
                     const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* o, int64_t capacity,
                     int32_t* match_ptr, int32_t* match_idx0, int32_t* match_idx1);
/* Parity probe of ONE pair: per query i the finalists nn[2 i] = {j1, j2} (-1: the train set has no such row) and their float distances
 * dist[2 i] = {dist1, dist2} (+inf where the index is -1).  nn [n1 * 2], dist [n1 * 2]. */
int ssfm_match_knn_probe(ssfm_ctx* ctx, int32_t n0, const float* train, int32_t n1, const float* query, int32_t dim, int32_t* nn, float* dist);
/* Device time of the kernels of this context's last ssfm_match_pairs call, summed over its slabs (like ssfm_ransac_last_kernel_ms). */
int ssfm_match_last_kernel_ms(ssfm_ctx* ctx, double* ms);
/* ---- guided matching: rematch a verified pair under its essential matrix (no reference counterpart; COLMAP's guided_matching) ----------------
 * Lowe's test over the whole train frame drops a feature on repeated structure before geometry is consulted.  Once a pair has an E, the test is
 * repeated among the train features inside the query's epipolar band only.  THE RULE, for pair p with train = frame pair_frame0[p] (n0 features,
 * rays u_j), query = frame pair_frame1[p] (n1 features, rays v_i) and E_p (9 doubles, column-major) in the convention of ssfm_sampson_probe,
 * v_i^T E u_j = 0 for a true correspondence:
 *     b_j = E u_j      a_i = E^T v_i      d = v_i . b_j      den = b_j.x^2 + b_j.y^2 + a_i.x^2 + a_i.y^2
 *     cand(i, j)  <=>  d * d < squared_threshold * den
 * evaluated in fp64 without a division; a NaN, or 0 < 0, is "no", so a zero E or a zero threshold admits nothing.  This is
 * SphericalEstimator::EvaluateModelOnPoint (src/spherical_estimator.cpp:67-78) below the threshold, in the unit of the squared_inlier_threshold of the
 * RANSAC calls.  Per query i: AMONG ITS CANDIDATES ONLY, j1 and j2 are the nearest and second nearest train rows by the distance of ssfm_match_pairs (float
 * sqrtf(sum (q - t)^2), the finalists re-evaluated in the direct form, equal distances rank the lower j first).  Query i is accepted iff j1 exists, and
 * dist1 <= max_distance, and j2 does not exist or (double)dist1 < ratio * (double)dist2.  Then m01[j1] = i, the largest accepted i keeps a train slot: the
 * list of a pair is (j, i) in ascending j, each j and each i at most once -- the match_idx0 / match_idx1 shape of ssfm_match_pairs.  The mask applies BEFORE
 * the ranking ("plain match, then filter" is another, weaker rule); a lone candidate is accepted, so a train frame of one feature can match here.
 * E of ssfm_ransac5_batch_indexed / ssfm_pairwise5_from_features has this convention as returned (the residual there is taken on v^T E u; checked on the
 * call's own inliers in tests/test_guided_match_gpu.py), no transposition is needed; for the spherical front end, which returns R only, E = [t]x R with
 * t = R e_z - e_z, negated when inward (make_spherical_essential_matrix, src/spherical_utils.cpp:9-14).
 * Device: k_guided_dist, the tiling of the plain distance kernel with (E u_j, b.x^2 + b.y^2) of a staged train tile and (v_i, a.x^2 + a.y^2) of the query
 * tile in LDS (8 KB more); the predicates of a tile are packed into a bit mask per query that the ranking epilogue tests.  Bit-identical from run to run. */
typedef struct {
    double ratio;              /* 0.75 */
    double squared_threshold;  /* 0: the caller sets it (nothing is admitted at 0) */
    float max_distance;        /* +inf */
    int32_t dim;               /* 128; a multiple of 4, 4..128 */
} ssfm_guided_match_options;   /* 24 bytes */
void ssfm_guided_match_default_options(ssfm_guided_match_options* o);
/* Feature tables, pair list, slabs (SSFM_MATCH_SLAB_PAIRS), capacity protocol (match_ptr always written, NULL lists = counts only, SSFM_ERR_INVALID with
 * the needed total in match_ptr[num_pairs]) and argument checks before any launch: those of ssfm_match_pairs.  In addition feat_rays
 * ([feat_ptr[num_frames] * 3], as ssfm_ransac_batch_indexed takes them) and E ([9 * num_pairs]) must not be NULL when num_pairs > 0, squared_threshold >= 0
 * and not NaN, max_distance >= 0.  Single-GPU: a context with a communicator is refused.  Up: the descriptors, 24 bytes per feature, 72 per pair; down: the
 * count scan and 8 bytes per match. */
int ssfm_guided_match_pairs(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays, int32_t num_pairs,
                            const int32_t* pair_frame0, const int32_t* pair_frame1, const double* E, const ssfm_guided_match_options* o, int64_t capacity,
                            int32_t* match_ptr, int32_t* match_idx0, int32_t* match_idx1);
/* Parity probe of ONE pair (train rows with rays u, query rows with rays v): nn [n1 * 2] the two finalists among the candidates (-1 where absent),
 * dist [n1 * 2] their float distances (+inf where absent), cand_count [n1] the number of train rows inside the band of query i -- the predicate is
 * evaluated for all n0 x n1 entries here. */
int ssfm_guided_knn_probe(ssfm_ctx* ctx, int32_t n0, const float* train, const double* u, int32_t n1, const float* query, const double* v, int32_t dim,
                          const double* E, double squared_threshold, int32_t* nn, float* dist, int32_t* cand_count);
/* Device time of the kernels of this context's last ssfm_guided_match_pairs call, summed over its slabs (like ssfm_match_last_kernel_ms). */
int ssfm_guided_match_last_kernel_ms(ssfm_ctx* ctx, double* ms);

/* ---- the pairwise front end in one call: match_exhaustive + estimate_pairwise (examples/spherical_sfm_tools.cpp:575-600, :309-420) -------------
 * For the given frame pairs, from the per-frame feature tables (descs: dim floats per feature; feat_rays: Kinv (x, y, 1), 3 doubles per feature; both
 * indexed by feat_ptr like ssfm_match_pairs / ssfm_ransac_batch_indexed).  DEFINED by composition -- the outputs are, bit for bit, those of
 *   1. ssfm_match_pairs on all pairs;
 *   2. the candidates: pairs with count >= min_num_inliers and count > 0 (:353), in pair order;
 *   3. ssfm_ransac_batch_indexed on exactly that candidate list (candidate k gets the random stream the indexed call gives its pair k);
 *   4. the candidates with num_inliers > min_num_inliers (:410) and a non-empty inlier list; of these the INLIER matches only, ascending train index.
 * The same kernels run with the same launch parameters; the match lists stay on the device between 1 and 3 and the inlier mask never leaves it: per pair
 * only its match count (4 bytes) and, for candidates, num_inliers + stats come back, and for accepted pairs R, the count and the inlier lists.
 * Outputs (capacity protocol): accepted_pair [pair_capacity] indices into the pair list, ascending; R [9 * pair_capacity] column-major;
 * num_inliers [pair_capacity]; inl_ptr [pair_capacity + 1]; inl_idx0 / inl_idx1 [inlier_capacity] (features of frame0 / frame1).  All are required.
 * needed[0] = accepted pairs, needed[1] = inlier matches, always written; if either exceeds its capacity the call returns SSFM_ERR_INVALID (no partial
 * lists are promised) and is to be repeated with those sizes.  Optional per input pair: match_count [num_pairs], num_inliers_all [num_pairs] (-1 where
 * the pair was no candidate), stats [2 * num_pairs] (iterations, LO runs; 0 where no candidate).  num_pairs = 0 and num_frames = 0 are fine.
 * The argument checks run before any launch.  Single-GPU: a context with a communicator is refused (use ssfm_match_pairs +
 * ssfm_ransac_batch_indexed_sharded there). */
int ssfm_pairwise_from_features(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays,
                                int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* match_opt,
                                const ssfm_ransac_options* ransac_opt, double squared_inlier_threshold, int64_t pair_capacity, int64_t inlier_capacity,
                                int64_t* needed, int32_t* accepted_pair, double* R, int32_t* num_inliers, int32_t* inl_ptr, int32_t* inl_idx0,
                                int32_t* inl_idx1, int32_t* match_count, int32_t* num_inliers_all, uint32_t* stats);
/* The same front end with general relative pose in the third place: match_exhaustive + estimate_pairwise_five_point (:575-600, :433-573), what
 * run_spherical_sfm_uncalib -match -fivepoint runs.  DEFINED by composition -- the outputs are, bit for bit, those of
 *   1. ssfm_match_pairs on all pairs;
 *   2. the candidates: pairs with count >= min_num_inliers and count > 0 (:475), in pair order;
 *   3. ssfm_ransac5_batch_indexed on exactly that candidate list (candidate k gets random stream k);
 *   4. the candidates with num_inliers > min_num_inliers (:534) and a non-empty inlier list; of these the INLIER matches only, ascending train index.
 * The match kernels and the five-point LO-MSAC kernel run unchanged with the launch parameters of the two public calls, the slab plans are made from the
 * same counts, and SSFM_MATCH_SLAB_PAIRS, SSFM_RANSAC_SLAB_PAIRS, SSFM_RANSAC_SLAB_RAYS and SSFM_RANSAC5_FORCE_GLOBAL act as they do there.  The options
 * are the struct of ssfm_ransac_batch; the fields used and the fields IGNORED are those listed at ssfm_ransac5_batch (reference-trace mode only).
 * Arguments, capacity protocol, optional per-pair outputs and refusals are those of ssfm_pairwise_from_features; in addition
 *   t [3 * pair_capacity]   the unit translation of every accepted pair (x1 = R x0 + t); required;
 *   E [9 * pair_capacity]   column-major, the matrix ssfm_ransac5_batch_indexed returns for the pair, with that call's sign; may be NULL.
 * Per accepted pair 24 bytes (t) come back beside what the spherical call brings back, and 72 bytes more when E is asked for; E, the scores and the masks
 * of the other candidates stay on the device.  Messages are prefixed ssfm_pairwise5_from_features.  Single-GPU: a context with a communicator is
 * refused (the sharded calls have no five-point form). */
int ssfm_pairwise5_from_features(ssfm_ctx* ctx, int32_t num_frames, const int32_t* feat_ptr, const float* descs, const double* feat_rays,
                                 int32_t num_pairs, const int32_t* pair_frame0, const int32_t* pair_frame1, const ssfm_match_options* match_opt,
                                 const ssfm_ransac_options* ransac_opt, double squared_inlier_threshold, int64_t pair_capacity, int64_t inlier_capacity,
                                 int64_t* needed, int32_t* accepted_pair, double* R, double* t, double* E /* may be NULL */, int32_t* num_inliers,
                                 int32_t* inl_ptr, int32_t* inl_idx0, int32_t* inl_idx1, int32_t* match_count, int32_t* num_inliers_all, uint32_t* stats);
/* Device time of the kernels of this context's last ssfm_pairwise_from_features or ssfm_pairwise5_from_features call (whichever came last): the brackets of ssfm_match_last_kernel_ms and
 * ssfm_ransac_last_kernel_ms, the latter with the hand-over kernels inside.  NOT included: the device-to-device copies that append every match slab's lists
 * to the call's list (8 bytes per match, once; copied again when the list has to grow), which run between the two brackets. */
int ssfm_pairwise_front_last_kernel_ms(ssfm_ctx* ctx, double* ms);
/* ---- the reference's estimator interface for ONE pair (rays resident on the device) ------------------------------------------------
 * One entry point per virtual of sphericalsfm::Estimator<Eigen::Matrix3d> / EssentialEstimator (include/sphericalsfm/estimator.h:7-29) as
 * SphericalEstimator implements them (include/sphericalsfm/spherical_estimator.h:8-35, src/spherical_estimator.cpp:67-164): what a host-side
 * RANSAC driver such as ransac_lib::LocallyOptimizedMSAC (include/RansacLib/ransac.h:128) calls.  The C++ mirror of the class is
 * spherical_sfm_amd/csrc/shim/spherical_estimator.h.  Thousands of pairs go through ssfm_ransac_batch instead.  Matrices column-major.
 *   create(u, v [n*3], use_poly_solver, inward)      SphericalEstimator(correspondences, use_poly_solver, inward)   spherical_estimator.h:15
 *   minimal_solver(sample [3..9]) -> Es [36], 0 | 4    MinimalSolver: always four candidates, real parts of complex ones       :80-84
 *   non_minimal_solver(sample [3..9]) -> E, ok         NonMinimalSolver                                                          :86-108
 *   evaluate_model(E) -> errors [n]                    EvaluateModelOnPoint(E, i) for every i                                     :67-78
 *   least_squares(sample [0..n], E in/out)             LeastSquares                                                              :110-157
 *   decompose(E) -> R [9], t [3]                       Decompose                                                                  :159-164 */
typedef struct ssfm_estimator ssfm_estimator;
int ssfm_estimator_create(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t use_poly_solver, int32_t inward, ssfm_estimator** out);
void ssfm_estimator_destroy(ssfm_estimator* e);
int ssfm_estimator_minimal_solver(ssfm_estimator* e, const int32_t* sample, int32_t sample_size, double* Es, int32_t* num_models);
int ssfm_estimator_non_minimal_solver(ssfm_estimator* e, const int32_t* sample, int32_t sample_size, double* E, int32_t* ok);
int ssfm_estimator_evaluate_model(ssfm_estimator* e, const double* E, double* errors);
int ssfm_estimator_least_squares(ssfm_estimator* e, const int32_t* sample, int32_t sample_size, double* E);
int ssfm_estimator_decompose(ssfm_estimator* e, const double* E, double* R, double* t);

/* ---- deterministic probes of the estimator's pieces (parity tests; one workgroup per task) --------------------------------------
 * ssfm_sampson_refine_probe: SphericalEstimator::LeastSquares (src/spherical_estimator.cpp:110-157) -- task t refines E_inout[t] (column-
 *   major, in/out) on the rays lists[task_ptr[t] .. task_ptr[t+1]) of the ONE pair (u, v).  The fit has SIX free parameters [r1; t1]: the
 *   reference sets r0, t0, u, v constant (:140-144) and leaves t1 free; t1 is dropped when E is rebuilt from so3exp(r1) (:156).
 * ssfm_sampson_refine_probe_ex: the same with its trace -- variant 0 = the workgroup-cooperative fit, 1 = the one-wave fit of the batched
 *   LO-MSAC kernel; trace [tasks*10] = [r1; t1], Levenberg-Marquardt iterations, status (0 converged / 1 iteration limit / 2 invalid
 *   steps / 3 evaluation failure), initial cost, final cost (may be NULL).
 * ssfm_decompose_probe: decompose_spherical_essential_matrix (src/spherical_utils.cpp:16-66) + so3exp = SphericalEstimator::Decompose
 *   (src/spherical_estimator.cpp:159-164): r_out [tasks*3] angle-axis, R_out [tasks*9] column-major (either may be NULL).
 * ssfm_nonminimal_probe: SphericalEstimator::NonMinimalSolver (src/spherical_estimator.cpp:86-108) on samples of 3..9 rays.
 * ssfm_so3_probe (row a9): what = 0 so3exp (src/so3.cpp:16-23), 1 so3ln (:25-69), 2 ceres::AngleAxisToRotationMatrix,
 *   3 ceres::RotationMatrixToAngleAxis, as the device code evaluates them; matrices column-major.
 * ssfm_mt19937_probe: nraw raw words of std::mt19937(seed), then uniform_int_distribution<int>(lo[i], hi[i]) draws from the same
 *   engine, through the device generator of the reference-trace mode.
 * ssfm_minimal_solver_probe: SphericalEstimator::MinimalSolver as the reference returns it (src/spherical_estimator.cpp:80-84): always four
 *   candidates per 3-point sample, the real parts of complex solutions included; Es [S*36] column-major, counts [S] (0 or 4).
 * ssfm_sampson_probe: EvaluateModelOnPoint (src/spherical_estimator.cpp:67-78) of T models on every ray: errors [T*n]. */
int ssfm_minimal_solver_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t S, const int32_t* samples, int32_t use_poly_solver,
                              double* Es, int32_t* counts);
int ssfm_sampson_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t T, const double* Es, double* errors);
int ssfm_sampson_refine_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t tasks, const int32_t* task_ptr,
                              const int32_t* lists, int32_t inward, double* E_inout);
int ssfm_sampson_refine_probe_ex(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t tasks, const int32_t* task_ptr,
                                 const int32_t* lists, int32_t inward, int32_t variant, double* E_inout, double* trace);
int ssfm_decompose_probe(ssfm_ctx* ctx, int32_t tasks, const double* E, int32_t inward, double* r_out, double* R_out);
int ssfm_nonminimal_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t tasks, const int32_t* task_ptr,
                          const int32_t* lists, double* E_out, int32_t* ok_out);
int ssfm_so3_probe(ssfm_ctx* ctx, int32_t what, int32_t n, const double* in, double* out);
int ssfm_mt19937_probe(ssfm_ctx* ctx, uint32_t seed, int32_t n, const int32_t* lo, const int32_t* hi, int32_t* draws, int32_t nraw, uint32_t* raw);
/* parity probe: spherical_solver_action_matrix (src/spherical_solvers.cpp:102-311) on S given 3-point samples
 * (samples: [S*3] indices into the n rays).  Es: [S*36] = up to 4 column-major 3x3 per sample (real solutions only),
 * counts: [S]. */
int ssfm_spherical_solver_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t S, const int32_t* samples,
                                double* Es, int32_t* counts);
/* same for spherical_solver_polynomial (src/spherical_solvers.cpp:313-660, SolveQuartic :15-69) */
int ssfm_spherical_solver_poly_probe(ssfm_ctx* ctx, int32_t n, const double* u, const double* v, int32_t S, const int32_t* samples,
                                     double* Es, int32_t* counts);

/* ---- focal-length search around the pose graph (examples/spherical_sfm_tools.cpp:1418-1496, find_best_focal_length_random)
 * costs[t] = loop_constraint_cost_fn(focals[t]) (:1138-1157): every match's essential matrix (rebuilt from its rotation,
 * :1429-1433) is rescaled by T = diag(f/f0, f/f0, 1) on both sides and decomposed again (transform_image_matches, :1118-1132),
 * the rotations are chained over the matches (k-1, k) (initialize_rotations_sequential, :794-813; the -sequential mode, the
 * GraphOptim initialisation is out of scope) and get_cost (src/uncalibrated_pose_graph.cpp:116-145) is evaluated -- one
 * workgroup per trial.  The reference draws the trial focals from std::random_device; here the caller supplies them.
 * best_trial: first minimum (strict <, :1467-1474); rotations_best [n*9]: the chained rotations at that focal, column-major,
 * rel_rotations_best [num_edges*9]: the matches' rotations re-derived at that focal (what run_optimization, :1160-1188, feeds to
 * optimize_rotations_and_focal_length = ssfm_posegraph_focal_solve).  Any output may be NULL. */
int ssfm_focal_search(ssfm_ctx* ctx, int32_t n, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                      const double* rel_rotations, int32_t inward, double focal_guess, int32_t num_trials, const double* focals,
                      double* costs, int32_t* best_trial, double* rotations_best, double* rel_rotations_best);

/* ---- general view graphs: unordered image sets (the sequential == false branch, examples/run_spherical_sfm.cpp:73-76) -----------
 * The edge list is what estimate_pairwise leaves: edge e = (index0[e], index1[e]) carries rel_rotations[9 e ..], column-major, with the
 * convention of the whole code base R_index1 = R_e R_index0.  All three calls are single-GPU: a context with a communicator is refused
 * (SSFM_ERR_INVALID).
 *
 * ssfm_triplet_filter: filter_image_matches (examples/spherical_sfm_tools.cpp:1031-1082) as a sparse join on the device.  A triplet is an
 *   ordered triple of LIST POSITIONS (i, j, k) with index1[i] == index0[j], index0[k] == index0[i], index1[k] == index1[j] -- the reference's
 *   three loops literally: no distinctness test, so duplicate edges, self loops and edges with index0 > index1 take part as they do there.
 *   err < err_thresh_rad (fp64, strict) sets good_out[i] = good_out[j] = good_out[k] = 1; every other entry is 0.  *num_triplets_out counts
 *   every triplet.  The result depends on the inputs alone (idempotent flags, integer counts, no floating-point sum across lanes).
 *   order: which product the error is taken of --
 *     SSFM_TRIPLET_ORDER_REFERENCE  |so3ln(Rij Rjk Rik^T)|  spherical_sfm_tools.cpp:1055 as written
 *     SSFM_TRIPLET_ORDER_COMPOSED   |so3ln(Rjk Rij Rik^T)|  what R_b = R_ab R_a implies: a consistent triangle has Rik = Rjk Rij
 *   The two agree only where the rotations commute (nearly so for the one-axis motion of a spherical capture).
 *   Records: if triplet_edges_out is not NULL (then triplet_err_out must not be either), the first min(num_triplets, max_records) triplets are
 *   written, (i, j, k) as list positions and err in radians, in THIS order: i ascending; within an i, j ascending by (index1[j], j); within a
 *   j, k ascending.  For a list sorted by (index0, index1) -- what estimate_pairwise produces from match_exhaustive -- that is the order of
 *   the lines of the reference's filter.txt.  Nothing is written past max_records.
 *   An index outside [0, num_cameras) gives SSFM_ERR_INVALID before anything is launched; num_edges == 0 is valid.
 *
 * ssfm_view_graph_tree (host only, no context): breadth-first spanning tree from `root`.  A popped node scans its incident edges in
 *   ascending list position and adopts every neighbour not seen yet.  Output in visiting order (= level order), num_reached entries:
 *   node_out[0] = root with parent_out / edge_out = -1; reversed_out = 1 when the tree edge is stored as (child, parent);
 *   level l = positions level_ptr[l] .. level_ptr[l + 1], l < *num_levels.  Self loops and duplicates are harmless; unreached cameras are not
 *   listed.  Arrays hold num_cameras entries (level_ptr num_cameras + 1); the rest is filled with -1 (reversed 0, level_ptr num_reached).
 *
 * ssfm_focal_search_graph: ssfm_focal_search with the same transform_image_matches step, the same get_cost and the same first-minimum
 *   rule, but the rotations of every trial are chained along the tree of ssfm_view_graph_tree(root), built once per call: a forward tree
 *   edge gives R_child = R_e R_parent, a reversed one R_child = R_e^T R_parent, unreached cameras keep the identity.  One workgroup per
 *   trial walks the tree level by level.  This is the project's own initialisation for a graph without a chain; the reference's
 *   initialize_rotations_gopt (GraphOptim, third party) is not restated. */
#define SSFM_TRIPLET_ORDER_REFERENCE 0
#define SSFM_TRIPLET_ORDER_COMPOSED 1
int ssfm_triplet_filter(ssfm_ctx* ctx, int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                        const double* rel_rotations, double err_thresh_rad, int32_t order, uint8_t* good_out, int64_t* num_triplets_out,
                        int64_t max_records, int32_t* triplet_edges_out, double* triplet_err_out);
int ssfm_view_graph_tree(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, int32_t root,
                         int32_t* num_reached, int32_t* node_out, int32_t* parent_out, int32_t* edge_out, uint8_t* reversed_out,
                         int32_t* num_levels, int32_t* level_ptr);
int ssfm_focal_search_graph(ssfm_ctx* ctx, int32_t n, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                            const double* rel_rotations, int32_t inward, double focal_guess, int32_t num_trials, const double* focals,
                            int32_t root, double* costs, int32_t* best_trial, double* rotations_best, double* rel_rotations_best);

/* ---- robust rotation initialisation for a view graph: L1 iteratively reweighted least squares on the device ------------------------
 * ssfm_rot_l1_init: a start for ssfm_rotavg_solve that does not inherit the wrong edges of a spanning tree (Chatterjee & Govindu's robust
 *   rotation averaging with the L1 weight, written from the mathematics; GraphOptim's initialize_rotations_gopt is not restated).  Edges as
 *   above: R_index1 = R_e R_index0, rel_rotations column-major.  Single-GPU: a context with a communicator is refused.
 *   Used edges: index0 != index1 and both ends reached from `root` by the walk of ssfm_view_graph_tree.  Free nodes: every reached camera but
 *   the root.  The rotations start from the tree chain of `root` (the root and every unreached camera: identity, and they stay so).
 *   Outer iteration k = 1 .. max_iterations:
 *     1. per used edge e = (a, b): v_e = so3ln(R_b^T R_e R_a) (body frame), w_e = 1 / max(|v_e|, weight_floor);
 *     2. min sum_e w_e |x_b - x_a - v_e|^2 with x_root = 0: one weighted graph Laplacian, three right-hand sides --
 *        L_ii = sum w_e, L_ij = -sum w_e over the edges between i and j, g_i = sum_{b = i} w_e v_e - sum_{a = i} w_e v_e;
 *     3. Jacobi-preconditioned conjugate gradients from x = 0, the three columns in lockstep with their own scalars.  Before each iteration a
 *        column with |r|^2 <= pcg_tolerance^2 |g|^2 stops (a zero column at once); at pcg_max_iterations (0: 4 x the free node count) the
 *        solve stops as it is and counts in pcg_solves_capped.  pcg_iterations_total adds the lockstep iterations of every solve;
 *     4. R_i <- R_i so3exp(x_i), step = max_i |x_i|; step < step_tolerance ends with SSFM_CONVERGENCE (the update is applied first),
 *        the iteration cap with SSFM_NO_CONVERGENCE.  step_tolerance = 0 therefore runs exactly max_iterations.
 *   Afterwards residual_out[e] = |v_e| at the returned rotations (-1 for an unused edge; may be NULL), final_cost = sum |v_e|; initial_cost is
 *   the same sum at the tree start.  Cutting the edges whose residual exceeds a threshold (2 degrees in the drivers) before the refinement is
 *   what removes the outliers' bias: DESIGN.md 4, "Robust rotation initialisation".
 *   Reproducible: no floating-point atomics, every sum is taken in a fixed order -- two calls on the same input return the same bits.
 *   SSFM_ERR_INVALID before anything is launched: an index or the root outside [0, num_cameras), max_iterations <= 0, weight_floor <= 0,
 *   pcg_tolerance <= 0, step_tolerance < 0, pcg_max_iterations < 0 (checked in this order: arguments, options, indices, root, then the
 *   context).  num_edges == 0 or a root without used edges is valid: identities, 0 iterations, SSFM_CONVERGENCE.
 *   Defaults: max_iterations 30, step_tolerance 1e-4, weight_floor 1e-3 (rad), pcg_tolerance 1e-10, pcg_max_iterations 0.
 *   kernel_ms: device time between the first and the last launch of the call (one hipEvent pair). */
typedef struct {
    int32_t max_iterations;
    double step_tolerance;
    double weight_floor;
    double pcg_tolerance;
    int32_t pcg_max_iterations;
} ssfm_rot_l1_options;
typedef struct {
    int32_t iterations, termination, num_free, num_edges_used, pcg_solves_capped;
    int64_t pcg_iterations_total;
    double initial_cost, final_cost, last_step, kernel_ms;
} ssfm_rot_l1_summary;
void ssfm_rot_l1_default_options(ssfm_rot_l1_options* o);
int ssfm_rot_l1_init(ssfm_ctx* ctx, int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                     const double* rel_rotations, int32_t root, const ssfm_rot_l1_options* opt /* NULL = defaults */,
                     double* rotations_out /* 9 n, column-major */, double* residual_out /* E, may be NULL */, ssfm_rot_l1_summary* s);

/* ---- robust focal search for a view graph: one L1 solve per trial focal on the device --------------------------------------------------
 * ssfm_focal_search_l1: ssfm_focal_search_graph whose trials do not inherit the wrong edges of the spanning tree.  Defined per trial t by
 *   composition of the two calls above:
 *     1. rel_t: the matches re-derived at focals[t] -- the transform_image_matches step of ssfm_focal_search_graph, the same device functions
 *        in the same order (its rel_rotations_best for the single trial focals[t]);
 *     2. (R_t, residual_t, iterations_t): the algorithm of ssfm_rot_l1_init on (index0, index1, rel_t, root, opt) as stated above -- used
 *        edges and free nodes by the walk of ssfm_view_graph_tree(root), the tree chain as the start, w_e = 1 / max(|v_e|, weight_floor),
 *        the three columns in lockstep through Jacobi-preconditioned CG with the stopping test before each iteration and the cap, the update
 *        R_i <- R_i so3exp(x_i), the end after the update when step < step_tolerance or at max_iterations;
 *     3. costs[t] = sum |v_e| over the used edges at R_t (final_cost); get_costs[t] = the cost ssfm_focal_search_graph takes, at R_t and
 *        rel_t; iterations[t] = the outer iterations run.
 *   *best_trial: the first minimum of costs (strict <).  rotations_best (9 n) and rel_rotations_best (9 E), column-major, are those of the
 *   best trial; residual_best[e] = |v_e| there, -1 for an unused edge.  Every output may be NULL.
 *   The tree and the adjacency are built once per call; the whole iteration of a trial runs inside one launch, a workgroup per trial.  The
 *   sums of a trial are taken in an order fixed by (n, num_edges, adjacency): its outputs do not depend on its position among the trials, on
 *   num_trials, on the slab of trials it is run in (SSFM_FOCAL_L1_SLAB_TRIALS overrides the slab size) or on where the solver's vectors
 *   are kept (LDS when they fit, SSFM_FOCAL_L1_FORCE_GLOBAL=1 forces global memory); two calls return the same bits.
 *   The sums are not taken in the order of ssfm_rot_l1_init (a lane per node here, a wave per node there): the two agree to rounding.
 *   SSFM_ERR_INVALID before anything is launched, the message prefixed "ssfm_focal_search_l1": what ssfm_focal_search_graph refuses
 *   (n, num_edges, num_trials <= 0, a NULL input), the options ssfm_rot_l1_init refuses, an index or the root out of range (in this order),
 *   then a NULL context or one with a communicator.
 *   ssfm_focal_l1_default_options: ssfm_rot_l1_default_options with max_iterations = 10 ("Robust focal search").
 *   costs is not normalised by the size of the relative rotations, which grow with the trial focal: where a large part of the edges is wrong,
 *   the lower end of a wide trial range can undercut the true focal ("Robust focal search", Open).
 *   kernel_ms: device time of the launches, summed over the slabs. */
void ssfm_focal_l1_default_options(ssfm_rot_l1_options* o);
int ssfm_focal_search_l1(ssfm_ctx* ctx, int32_t n, int32_t num_edges, const int32_t* index0, const int32_t* index1,
                         const double* rel_rotations, int32_t inward, double focal_guess, int32_t num_trials, const double* focals,
                         int32_t root, const ssfm_rot_l1_options* opt /* NULL = ssfm_focal_l1_default_options */,
                         double* costs, double* get_costs, int32_t* iterations, int32_t* best_trial,
                         double* rotations_best, double* rel_rotations_best, double* residual_best, double* kernel_ms);

/* ---- keypoint selection: adaptive non-maximal suppression, batched over frames ---------------------------------------------------------
 * ssfm_anms_batch: adaptiveNonMaximalSuppresion (examples/spherical_sfm_tools.cpp:76-123), the thinning step of DetectorTracker::detect (:179-208),
 *   for every frame in one device call.  Frame f owns the keypoints kp_ptr[f] .. kp_ptr[f + 1] of xy ([2 * total]: x, y) and response ([total]).
 *   Per frame, with n keypoints and k = num_to_keep[f]:
 *     n < k: the keypoints are returned unchanged -- keep_idx is 0 .. n-1, the radii are DBL_MAX.
 *     Otherwise, in the total order (response descending, original index ascending), precedes(j, i) = response_j > response_i ||
 *     (response_j == response_i && j < i):
 *       thr_i    = response_i * 1.11f (a float product),
 *       radius_i = sqrt(min over {j : response_j > thr_i && precedes(j, i)} of (double)dx * dx + (double)dy * dy), dx and dy float differences;
 *                  DBL_MAX when no j qualifies (a difference that overflows to infinity, or is NaN, never lowers a radius: std::min in the reference),
 *       decision = element k (0-based) of the radii sorted descending,
 *       kept: every i with radius_i >= decision, in the total order.  At least k + 1 keypoints survive, more when radii tie.
 *     This is the reference's loop (sort by response; for each i the prefix of j with response_j > thr_i) for every tie order std::sort may pick when the
 *     responses are non-negative, and for the stable order when some are negative.
 *   keep_ptr [num_frames + 1], keep_idx: frame-local original indices, frame f's at keep_ptr[f] .. keep_ptr[f + 1]; a frame never keeps more than it has, so
 *   capacity `total` always suffices and there is no counting call.  radius: [total], per INPUT keypoint, may be NULL.
 *   Three deviations from the reference:
 *     n == k: the reference reads one element past its radii array; here every keypoint is returned, in the total order;
 *     a NaN response (undefined behaviour in std::sort) is refused;
 *     among equal responses the output order is by original index (std::sort leaves it unspecified).
 *   SSFM_ERR_INVALID before anything is launched, the message prefixed with the function's name: kp_ptr not starting at 0 or not ascending, a negative
 *   num_to_keep, a NaN response, force_j_chunks < 0 (arguments, options, kp_ptr, num_to_keep, responses, then the context).  num_frames = 0 and empty frames
 *   are valid.  Single-GPU: a context with a communicator is refused.
 *   force_j_chunks: 0 lets the planner decide how many chunks a frame's j range is cut into (frames that cannot fill the device alone are cut); k > 0 cuts
 *   every frame into k chunks.  The chunks combine by integer atomics only: the result is the same bits for every cut and every run.
 * ssfm_anms_batch_host: the same contract on the host (sort, prefix loop with the early exit, selection), num_threads threads over frames and blocks of a
 *   frame.  No context; the native check and the CPU side of scripts/anms_timing.py.  Never called by ssfm_anms_batch.
 * ssfm_anms_last_kernel_ms: device time between the first and the last launch of the context's last ssfm_anms_batch call (one hipEvent pair). */
typedef struct {
    int32_t force_j_chunks;   /* 0 = planner decides */
    int32_t reserved;
} ssfm_anms_options;
void ssfm_anms_default_options(ssfm_anms_options* o);
int ssfm_anms_batch(ssfm_ctx* ctx, int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep,
                    const ssfm_anms_options* opt /* NULL = defaults */, int32_t* keep_ptr, int32_t* keep_idx, double* radius /* may be NULL */);
int ssfm_anms_batch_host(int32_t num_frames, const int32_t* kp_ptr, const float* xy, const float* response, const int32_t* num_to_keep, int32_t num_threads,
                         int32_t* keep_ptr, int32_t* keep_idx, double* radius /* may be NULL */);
int ssfm_anms_last_kernel_ms(ssfm_ctx* ctx, double* ms);

/* ---- SfM::Retriangulate (src/sfm.cpp:156-192) ------------------------------------------------------------------
 * Re-estimates EVERY point of the problem from its observations and the current cameras/focal with the per-point
 * ransac_lib::LocallyOptimizedMSAC<Point, ..., TriangulationEstimator> of the reference (src/triangulation_estimator.cpp:46-127,
 * include/RansacLib/ransac.h:128-428; squared inlier threshold 4 px^2, final least squares on, every other option a LORansacOptions
 * default), one GPU lane per point.  The default mode REPLAYS THE REFERENCE'S TRACE: both std::mt19937 streams run from seed 0 for
 * every point, so the sampler's pair sequence (a function of the track length only) and the raw words of the local optimisation's
 * stream are drawn once on the host with libstdc++'s generators, and the device walks RansacLib's control flow draw for draw -- same
 * iteration counts, same local-optimisation runs, same inlier sets as a CPU build (tests/test_retriangulate_gpu.py compares with the
 * oracle bit for bit).  p->points is overwritten; points with < 3 observations or < 3 inliers become (0,0,0) exactly as in the
 * reference (which removes them from later Optimize calls).  num_inliers_out: [num_points] or NULL.  The *_fixed masks are ignored,
 * like the reference does.  SSFM_RETRI_ENUMERATE=1 selects the enumerating kernel of rounds 1-2 (every observation pair once, no random
 * stream: statistical agreement only, ~2.5x faster) as the default of the two forms without a mode argument; ssfm_retriangulate_mode
 * takes the mode explicitly (SSFM_RETRI_MODE_TRACE / SSFM_RETRI_MODE_ENUMERATE).
 * WHAT "THE REFERENCE'S TRACE" MEANS: bit-for-bit agreement is with this repository's CPU restatement (oracle/triangulation_oracle.cpp: one-sided
 * Jacobi SVD for the DLT, a hand-written Levenberg-Marquardt with Ceres' rules), compiled without fused multiply-adds.  A real build of the reference
 * computes the DLT with Eigen::JacobiSVD and the point refinement with Ceres; last bits decide every `score < best` branch and therefore every later
 * draw, so against such a build the replay is the same ALGORITHM and random streams, statistically equivalent results (same inlier sets for all but
 * marginal observations), not the same trace.  Parity of this row is "unpinned" like the rest of the oracle.
 * ssfm_retriangulate_ex: the same with its trace -- stats_out [2*num_points] = RansacStatistics::num_iterations, number_lo_iterations
 *   of every point's run; inlier_flags_out [num_observations] = 1 where the observation is in the final stats.inlier_indices of its
 *   point (either may be NULL; trace mode only).
 * ssfm_tri_probe: TriangulationEstimator's pieces, one lane per task, on point task_pt[t] with the observation subset
 *   lists[task_ptr[t] .. task_ptr[t+1]) (positions in the point's observation list, cameras ascending); out [tasks*4]:
 *   what 0 NonMinimalSolver (1..6 observations) -> X, 0;  what 1 LeastSquares from X_in[t] -> X, Levenberg-Marquardt iterations;
 *   what 2 ScoreModel / GetInliers of X_in[t] -> MSAC score at 4, inliers at 4, inliers at 4 sqrt 2, error of observation 0. */
#define SSFM_RETRI_MODE_TRACE 0
#define SSFM_RETRI_MODE_ENUMERATE 1
int ssfm_retriangulate(ssfm_ctx* ctx, ssfm_ba_problem* p, int32_t* num_inliers_out);
int ssfm_retriangulate_mode(ssfm_ctx* ctx, ssfm_ba_problem* p, int32_t mode, int32_t* num_inliers_out, uint32_t* stats_out, uint8_t* inlier_flags_out);
int ssfm_retriangulate_ex(ssfm_ctx* ctx, ssfm_ba_problem* p, int32_t* num_inliers_out, uint32_t* stats_out, uint8_t* inlier_flags_out);
int ssfm_tri_probe(ssfm_ctx* ctx, ssfm_ba_problem* p, int32_t what, int32_t tasks, const int32_t* task_pt, const int32_t* task_ptr, const int32_t* lists,
                   const double* X_in, double* out);

/* ---- feature tracks: the integer part of build_sfm (examples/spherical_sfm_tools.cpp:862-950), host only ------
 * Keyframe k owns features [feat_ptr[k], feat_ptr[k+1]) of feat_xy ([total*2] pixels).  Match set s links keyframes
 * (ms_index0[s], ms_index1[s]) with pairs (m_f0[m], m_f1[m]), m in [ms_ptr[s], ms_ptr[s+1]), feature indices local to their
 * keyframe, first index ascending (std::map order).  Outputs: tracks [total] (-1 = unmatched; ids bit-exact with the
 * reference's AddPoint sequence), num_points (ids issued, merged ones included), point_alive [>= num match pairs] (0 =
 * removed by MergePoint), observations camera-major / point-ascending (the iteration order of SfM's maps), centred by
 * (centerx, centery); obs_* need capacity 2 * (number of match pairs) and may be NULL to only count. */
int ssfm_build_tracks(int32_t num_keyframes, const int32_t* feat_ptr, const double* feat_xy, int32_t num_match_sets,
                      const int32_t* ms_index0, const int32_t* ms_index1, const int32_t* ms_ptr, const int32_t* m_f0, const int32_t* m_f1,
                      double centerx, double centery, int32_t merge, int32_t* tracks, int32_t* num_points, uint8_t* point_alive,
                      int64_t* num_observations, int32_t* obs_cam, int32_t* obs_pt, double* obs_xy);

/* ---- feature tracks on the device: the track pass of build_sfm (merge = true) as connected components --------------------------------
 * ssfm_build_tracks_device: the inputs of ssfm_build_tracks, all host pointers.  A global feature id is feat_ptr[k] + local index;
 *   total = feat_ptr[num_keyframes].
 *   Tracks.  tracks [total]: -1 for a feature that no match names; for every other feature the id of its connected component in the graph
 *     whose edges are the matches.
 *   Canonical ids.  The components are numbered 0 .. P-1 in ascending order of their smallest global feature id; *num_points = P; there are
 *     no dead ids.
 *   Observations.  Every (camera, track) pair that holds at least one feature gets one observation: that of the feature with the smallest
 *     index among them.  Its pixel is feat_xy - (centerx, centery) in double: one subtraction, bit-equal to the host's.
 *   Output order.  Observations come out in ascending global feature id of the winning feature.  obs_cam, obs_pt and obs_feat (the local
 *     index of the winning feature) hold up to `total` entries, obs_xy 2 * total; the four may be NULL together, to count only.
 *     *num_observations is always written.
 *   Conflicts.  point_conflict (capacity `total`, may be NULL): 1 for a track that holds two or more features of one frame -- such a track is
 *     inconsistent and the caller may drop it -- 0 otherwise; P entries are written.
 *   Order independence.  The result does not depend on the order of the match sets, on the order of the matches inside a set (ascending
 *     m_f0 is not required here), on repeated matches or on the run: repeats are bit-identical.  A component's root is its smallest member
 *     whatever the schedule of the device, and everything else is a function of the roots.
 *   A match set with index0 == index1 is accepted: its two features share a frame, so the track is flagged in point_conflict.  A match of a
 *   feature with itself makes a track of one feature.
 *   Four departures from ssfm_build_tracks:
 *     the ids are canonical, not the AddPoint sequence (which issues an id per track ever started and leaves the merged ones dead);
 *     where a track holds two features of one frame the observation is that of the smallest feature index, not of the last write;
 *     the observations are ordered by winning feature, not camera-major / point-ascending;
 *     there is no merge = 0 form: that mode is the order-dependent bookkeeping itself.
 *   Where the two calls agree, on every input: the partition of the features into tracks, the set of (camera, track) observation keys after
 *   relabelling, and the pixel of every key that holds one feature.
 *   SSFM_ERR_INVALID before anything is launched and before the context is looked at, the message prefixed "ssfm_build_tracks_device": a NULL
 *   feat_ptr / tracks / num_points / num_observations, some but not all of the four observation arrays, a NULL ms_index0 / ms_index1 / ms_ptr
 *   with num_match_sets > 0 or num_match_sets < 0, num_keyframes <= 0, feat_ptr[0] != 0, a descending feat_ptr, more than 2^30 features,
 *   a NULL feat_xy where observations are asked for, ms_ptr[0] != 0, a descending ms_ptr, a NULL m_f0 / m_f1 with matches, a frame index out
 *   of range (in this order); then a NULL context ("ctx is null") or one with a communicator (the call is single-GPU).  A feature index
 *   outside its frame is caught by a flag raised in the first kernel: SSFM_ERR_INVALID, "feature index out of range", no output is promised,
 *   the context stays usable.  num_match_sets = 0 and empty sets are valid: all -1, zero points, zero observations.
 *   Transfers: 8 bytes per match up; 4 bytes per feature, 1 per point and 8 per observation down (the camera, the local index and the pixel
 *   of an observation follow from its global feature id on the host).  The scratch buffers and the pinned staging are kept in the context and
 *   grown on demand.
 * ssfm_tracks_last_kernel_ms: device time between the first and the last launch of the context's last ssfm_build_tracks_device call (one
 *   hipEvent pair; 0 when the call had nothing to launch).  -1 on NULL arguments. */
int ssfm_build_tracks_device(ssfm_ctx* ctx, int32_t num_keyframes, const int32_t* feat_ptr, const double* feat_xy,
                             int32_t num_match_sets, const int32_t* ms_index0, const int32_t* ms_index1, const int32_t* ms_ptr,
                             const int32_t* m_f0, const int32_t* m_f1, double centerx, double centery,
                             int32_t* tracks, int32_t* num_points, uint8_t* point_conflict, int64_t* num_observations,
                             int32_t* obs_cam, int32_t* obs_pt, int32_t* obs_feat, double* obs_xy);
int ssfm_tracks_last_kernel_ms(ssfm_ctx* ctx, double* ms);

/* ---- stereo panorama: make_stereo_panoramas (examples/stereo_panorama_tools.cpp:404-637) from poses, frames and optical flow -------------
 * One cylindrical panorama per viewing angle phi.  Every output column is synthesised from one pair of consecutive keyframes k -> (k+1) mod n:
 * a plane-induced column map into both frames (:69-106), optionally corrected by the optical flow between them (:135-188), two bilinear
 * remaps and a blend.  The flow estimator stays outside, like SIFT: flows are an input; without them the call computes
 * synthesize_column_linear (:108-133).  R is ROW-MAJOR [n*9] here (x_cam = R x_world + t), t [n*3]; the poses are expected levelled and scaled
 * as estimate_plane leaves them (:276-358; csrc/shim/stereo_panorama_tools.h: level_keyframes).
 *
 * ssfm_pano_plan (host only, no GPU): the column jobs of :521-616.  A job is a (pair, thetanum, phinum) that passes the angle tests of
 *   :582-592, listed pair-major, then thetanum, then phinum.  job_col = (thetanum + round(phi / theta_step)) mod pano_width, made non-negative;
 *   job_ok = 1 when get_synthetic_column_maps would return true (XL(2) > 0 and XR(2) > 0 on every row); job_alpha = |angle_LD| / |angle_LR|;
 *   job_consts [10 per job] = tan(phi), synth_R[9] row-major -- every transcendental of the stage is taken here, the kernel uses + - * / only.
 *   owner [num_phi * pano_width]: the pair index of the ok job of the HIGHEST pair index that writes the column (the reference overwrites pair
 *   by pair), -1 where none does.  *num_jobs: capacity of the job arrays in, number of jobs out; a capacity that is too small returns
 *   SSFM_ERR_INVALID with the needed count in *num_jobs and the job arrays untouched (owner is still written).  Any output array may be NULL.
 * ssfm_pano_synthesize: panoramas [num_phi][height][pano_width][3] bytes, every byte defined (columns nobody owns are 0).  frames [n] pointers to
 *   height*width*3 bytes (channel order kept as is); flow_fwd [n] pointers to height*width*2 floats (dx, dy), entry k the flow of frame k ->
 *   (k+1) mod n, flow_bwd entry k that of frame (k+1) mod n -> k; both arrays NULL = linear mode.  Entries of pairs that do not exist (the last
 *   one of an open sweep) are not read.  Per pixel, the map in double in the order written in csrc/pano_host.h, rounded to float; then in fp32,
 *   flow mode: xs_L = xL * 1 + ((xR - xL) - bilinear(flow_fwd, xL)) * (float)alpha, xs_R = xR * 1 + ((xL - xR) - bilinear(flow_bwd, xR)) *
 *   (float)(1 - alpha); out = bilinear(frame_k, xs_L) * (float)(1 - alpha) + bilinear(frame_k+1, xs_R) * (float)alpha, rounded half to even and
 *   clamped to 0..255 (NaN -> 0).  bilinear: x0 = floor(x), fx = x - x0, weights (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx formed first, the four
 *   products summed left to right, a tap outside the image is 0, a non-finite coordinate or one beyond +-2^30 samples 0; with subpixel_bits = 5
 *   a valid coordinate is first replaced by rint(x * 32) / 32 (the grid cv::remap interpolates on).  No multiply-add is fused.
 *   on_device = 0: frames / flows / panoramas are host memory, staged pair slab by pair slab within max_slab_bytes (0 = 1 GiB; at least one pair)
 *   through a pinned buffer of the context.  on_device = 1: the pointer arrays are host arrays of DEVICE pointers and panoramas is a device pointer;
 *   nothing is copied, the work is queued on the context's stream and the call returns after it has finished.  owner_out (host, or NULL) receives
 *   the owner map of the plan.
 *   SSFM_ERR_INVALID before the device is touched: flow arrays given only one way, a null frame or flow pointer of an existing pair, pano_width < 2,
 *   num_phi < 1, width or height < 1, a null context.
 * ssfm_pano_last_kernel_ms: device time of the kernels of the context's last ssfm_pano_synthesize call (one hipEvent pair per slab). */
typedef struct {
    int32_t num_phi;             /* 9      (:485) */
    int32_t is_loop;             /* 1: the last keyframe pairs with the first (:525-528) */
    double  phi_step_deg;        /* 1.0    phi_i = (i - (num_phi-1)/2) * step; num_phi == 1 -> 0 (:486-494) */
    double  depth;               /* 10.0   (:30) */
    double  synth_radius;        /* 0.5    (:31) */
    double  synth_focal_factor;  /* 1.2    (:32) */
    int32_t subpixel_bits;       /* 0: sample at the float coordinate; 5: coordinates rounded to 1/32 px first */
    int32_t on_device;           /* 0: frames / flows / panoramas are host pointers; 1: device pointers (no copies) */
    int64_t max_slab_bytes;      /* 0 = default; device staging budget for frames + flows when on_device == 0 */
} ssfm_pano_options;
void ssfm_pano_default_options(ssfm_pano_options* opt);
int ssfm_pano_plan(const ssfm_pano_options* opt, int32_t n, const double* R, const double* t, double focal, double cx, double cy,
                   int32_t width, int32_t height, int32_t pano_width, int32_t* num_jobs, int32_t* job_pair, int32_t* job_theta, int32_t* job_phi,
                   int32_t* job_col, uint8_t* job_ok, double* job_alpha, double* job_consts, int32_t* owner);
int ssfm_pano_synthesize(ssfm_ctx* ctx, const ssfm_pano_options* opt, int32_t n, const double* R, const double* t, double focal, double cx, double cy,
                         int32_t width, int32_t height, const uint8_t* const* frames, const float* const* flow_fwd, const float* const* flow_bwd,
                         int32_t pano_width, uint8_t* panoramas, int32_t* owner_out);
int ssfm_pano_last_kernel_ms(ssfm_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif
