// spherical_sfm_amd -- the part of examples/spherical_sfm_tools.{h,cpp} that sits on the optimisation hot path, over the C ABI:
// find_best_focal_length_random (spherical_sfm_tools.cpp:1418-1496) with its run_optimization (:1160-1188).
// POD stand-ins for the Eigen types, as in sfm.h.  Host code only.
#pragma once
#include <array>
#include <cstddef>
#include <limits>
#include <map>
#include <string>
#include <vector>
#include "../../../include/ssfm.h"
#include "sfm.h"

namespace sphericalsfm {

typedef std::array<double, 9> Mat3;                       // column-major like Eigen::Matrix3d::data()
typedef std::map<std::size_t, std::size_t> Matches;                 // spherical_sfm_tools.h:20

struct ImageMatch {                                       // spherical_sfm_tools.h:41-50
    int index0, index1;
    Matches matches;
    Mat3 R;
    ImageMatch(int _index0, int _index1, const Matches& _matches, const Mat3& _R) : index0(_index0), index1(_index1), matches(_matches), R(_R) {}
};

struct Point2f { float x, y; };
struct Features {                                         // spherical_sfm_tools.h:19-28 (cv::Mat descs -> flat 128 floats per feature)
    std::vector<int> tracks;
    std::vector<Point2f> points;
    std::vector<std::array<unsigned char, 3>> colors;
    std::vector<float> descs;
    int size() const { return (int)points.size(); }
    bool empty() const { return points.empty(); }
};
struct Keyframe {                                         // spherical_sfm_tools.h:30-39 (images are not part of this path)
    int index; std::string name; Features features;
    Keyframe(int _index, const std::string& _name, const Features& _features) : index(_index), name(_name), features(_features) {}
};

struct KeyPoint {                                         // cv::KeyPoint's data members, as a POD
    Point2f pt; float size, angle, response; int octave, class_id;
};

// adaptiveNonMaximalSuppresion (spherical_sfm_tools.cpp:76-123) over ssfm_anms_batch, the reference's signature plus the context argument: fewer keypoints than
// numToKeep are left as they are; otherwise the survivors replace `keypoints`, strongest response first.  Where the reference is open or undefined (include/ssfm.h):
// equal responses come out by their position in the input, keypoints.size() == numToKeep returns all of them sorted, a NaN response is an error.
// The batched overload thins every frame in ONE device call (the reference runs one frame per OpenMP thread, :299-306).  Exits on an error of the library.
void adaptiveNonMaximalSuppresion(ssfm_ctx* ctx, std::vector<KeyPoint>& keypoints, const int numToKeep);
void adaptiveNonMaximalSuppresion(ssfm_ctx* ctx, std::vector<std::vector<KeyPoint>>& keypoints_per_frame, const std::vector<int>& numToKeep);

// The selection of DetectorTracker::detect (:186-198) without the detector: ntokeep = max(0, 4000 - features.points.size()); 0 selects nothing (keypoints is
// emptied, features stays); otherwise keypoints is thinned to ntokeep and the survivors' positions are appended to features.points, as :202-207 does.  The
// descriptors and colours of the appended points need the image (sift->compute, sample_image) and are the caller's to append.  The batched form makes one
// device call for all frames.
void select_keypoints(ssfm_ctx* ctx, Features& features, std::vector<KeyPoint>& keypoints);
void select_keypoints(ssfm_ctx* ctx, std::vector<Features*>& features, std::vector<std::vector<KeyPoint>>& keypoints_per_frame);

// keyframes.txt / features.dat / matches.dat (examples/spherical_sfm_io.cpp:10-120).  The reference prints the keyframe name with
// "%s" of a std::string object and reads back only the indices; here the name is written as text and skipped on input.
void write_feature_tracks(const std::string& outputpath, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches);
bool read_feature_tracks(const std::string& outputpath, std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches);

// estimate_pairwise (spherical_sfm_tools.cpp:309-431): every candidate pair (index0 < index1) with at least min_num_inliers matches goes
// through the spherical 3-point LO-MSAC -- all pairs in ONE ssfm_ransac_batch launch instead of the OpenMP loop; pairs with more than
// min_num_inliers inliers come back with their inlier matches and R = so3exp(decompose(E)).  Returns the number of loop closures
// (accepted pairs that are not consecutive).  COLLECTIVE if ctx carries a communicator: every rank calls it with the same arguments (pairs are sharded, one all-reduce
// returns all results everywhere); a context without a communicator runs all pairs locally.
int estimate_pairwise(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches,
                      double inlier_threshold, int min_num_inliers, bool inward, std::vector<ImageMatch>& image_matches_out);

// estimate_pairwise_five_point (spherical_sfm_tools.cpp:433-573, the `-fivepoint` branch of run_spherical_sfm_uncalib): the same candidate rule (the first
// stored match set of every pair index0 < index1; `m01.size() < min_num_inliers` skips) and the same output order as estimate_pairwise, but general relative pose --
// LO-MSAC over the five-point estimator and PoseFromEssentialMatrix on the inliers -- through ssfm_ransac5_batch_indexed.  No `inward`: nothing ties t to R.
// Single GPU (the sharded forms have no five-point counterpart).  Returns the loop-closure count.
int estimate_pairwise_five_point(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches,
                                 double inlier_threshold, int min_num_inliers, std::vector<ImageMatch>& image_matches_out);

// match (spherical_sfm_tools.cpp:235-251) and match_exhaustive (:575-600) over ssfm_match_pairs: features0 is the train set, features1 the query set, m01 maps a
// feature of features0 to the LAST query that chose it; match_exhaustive appends one ImageMatch per pair index0 < index1 -- every pair, also one without a match,
// as the reference does -- where index0 / index1 are the POSITIONS in `keyframes` (the reference's loop counters; what estimate_pairwise,
// find_largest_connected_component, initialize_rotations_sequential and build_sfm read them as), not Keyframe::index.  Its rotation is the identity (the
// reference leaves it uninitialised).  The reference's signatures plus the context argument.
void match(ssfm_ctx* ctx, const Features& features0, const Features& features1, Matches& m01, double ratio = 0.75);
void match_exhaustive(ssfm_ctx* ctx, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches);

// find_largest_connected_component (:736-792), on the host with union-find: the vertices are 0 .. the largest index an edge names, components are numbered in order
// of their smallest vertex, the first largest one wins a tie; keyframes and matches of that component are kept and renumbered in place (Keyframe::index keeps the
// original frame number).  DEFINED here: keyframes beyond the last vertex that any edge names are in no component and are dropped (the reference reads its
// component table out of range for them); with no edges at all everything is dropped.
void find_largest_connected_component(std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches);

// keyframes.txt + features.dat without matches.dat
bool read_features(const std::string& outputpath, std::vector<Keyframe>& keyframes);

// match_exhaustive + estimate_pairwise in one device call (ssfm_pairwise_from_features) for all pairs index0 < index1 of keyframes[index]: the match lists never come
// back to the host, only the accepted pairs' inlier matches and rotations do.  Same result and return value as match_exhaustive followed by estimate_pairwise.
// Single-GPU: the context must not carry a communicator.
int estimate_pairwise_from_features(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, double inlier_threshold, int min_num_inliers,
                                    bool inward, std::vector<ImageMatch>& image_matches_out);

// match_exhaustive + estimate_pairwise_five_point in one device call (ssfm_pairwise5_from_features), built like estimate_pairwise_from_features: all pairs
// index0 < index1, capacity bounds that cannot miss, the loop-closure count.  Same result and return value as match_exhaustive followed by
// estimate_pairwise_five_point.  Single-GPU: the context must not carry a communicator.
// Es_out (optional): the essential matrix of every appended ImageMatch, column-major, v^T E u = 0 with u in index0 -- what guided_match takes.
int estimate_pairwise_five_point_from_features(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, double inlier_threshold,
                                               int min_num_inliers, std::vector<ImageMatch>& image_matches_out, std::vector<Mat3>* Es_out = nullptr);

// Guided matching (ssfm_guided_match_pairs; no reference counterpart): `matches` of every ImageMatch is replaced by its guided list -- Lowe's test among the
// features of keyframes[index0] inside the epipolar band of each feature of keyframes[index1] -- under E = [t]x R, t = R e_z - e_z, negated if inward
// (make_spherical_essential_matrix of the match's R).  The threshold is inlier_threshold^2 * Kinv(0)^2, as in estimate_pairwise.  index0 / index1 are positions in
// `keyframes` (call it before find_largest_connected_component renumbers them); R stays.  One device call for all matches.  Single GPU.
// The overload takes one E per ImageMatch instead (column-major, v^T E u = 0): the five-point path, where R alone does not give E.
void guided_match(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, double inlier_threshold,
                  bool inward, double ratio = 0.75, float max_distance = std::numeric_limits<float>::infinity());
void guided_match(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, const std::vector<Mat3>& Es,
                  double inlier_threshold, double ratio = 0.75, float max_distance = std::numeric_limits<float>::infinity());

void initialize_rotations_sequential(int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations);   // tools.cpp:794-813
double refine_rotations(ssfm_ctx* ctx, int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations); // tools.cpp:851-860
// tools.cpp:862-955: tracks (ssfm_build_tracks, ids bit-exact with the reference's AddPoint sequence), cameras, observations, Retriangulate
void build_sfm(std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches, const std::vector<Mat3>& rotations, SfM& sfm,
               bool spherical, bool merge, bool inward, int fix_camera = 0, bool device_tracks = false);
// device_tracks (with merge): the tracks come from ssfm_build_tracks_device on sfm.GetContext() -- connected components of the matches with canonical ids, P points
// added and none removed, the observations added as returned (include/ssfm.h states where that call and ssfm_build_tracks agree).  With merge == false the host
// pass runs and a line on stdout says so.  Default false: the host pass, unchanged.

// filter_image_matches (spherical_sfm_tools.cpp:1031-1082) over ssfm_triplet_filter: every ordered triple of matches (i, j, k) with i = (a, b), j = (b, c), k = (a, c)
// is a triplet; a triplet whose rotation error is below err_thresh_rad marks its three matches good; the good matches come back in list order.  order: which product
// the error is taken of -- the reference's own Rij Rjk Rik^T (the default) or Rjk Rij Rik^T, which is what R_b = R_ab R_a implies (include/ssfm.h).  Prints the
// reference's "good edges" line; the per-triplet lines of filter.txt ("%d %d %d %f": index0, index1 of match i, index1 of match j, degrees) are written only when
// log_path is given (the reference always writes them, and prints each to stdout); the log costs a second run of the filter, because the number of records
// has to be known before they can be asked for.  Single-GPU: the context must not carry a communicator.
std::vector<ImageMatch> filter_image_matches(ssfm_ctx* ctx, std::vector<ImageMatch>& image_matches, double err_thresh_rad, int order = SSFM_TRIPLET_ORDER_REFERENCE,
                                             const char* log_path = nullptr);
// the host half of it (tools_host.cpp): the kept matches from the flags, the "good edges" line, the log from the records (num_records triples of list positions + radians)
std::vector<ImageMatch> apply_triplet_filter(const std::vector<ImageMatch>& image_matches, const std::vector<uint8_t>& good, int64_t num_records,
                                             const int32_t* triplet_edges, const double* triplet_err, const char* log_path);

// Rotation initialisation over a general view graph, in place of the reference's initialize_rotations_gopt (GraphOptim, third party, not restated): the relative
// rotations chained along the breadth-first spanning tree of ssfm_view_graph_tree(root) -- forward tree edge R_child = R_e R_parent, reversed R_child = R_e^T R_parent;
// cameras the tree does not reach keep the identity.  The robust refine_rotations that follows does the averaging.  Host code.
void initialize_rotations_tree(int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations, int root = 0);

// Robust rotation initialisation over a general view graph (ssfm_rot_l1_init: L1 iteratively reweighted least squares from the tree chain of `root`, on the device):
// rotations as initialize_rotations_tree returns them, residuals[e] = |so3ln(R_b^T R_e R_a)| in radians at those rotations (-1 for a match that is not used: a self
// loop, or cameras `root` does not reach).  Default options.  Exits on an error of the library, like refine_rotations.
void initialize_rotations_l1(ssfm_ctx* ctx, int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations, std::vector<double>& residuals,
                             int root = 0, ssfm_rot_l1_summary* summary = nullptr);
// The matches whose residual lies in [0, thresh_rad], in list order (host code, tools_host.cpp).  Together with the start above this is what keeps gross outliers
// out of refine_rotations: DESIGN.md 4, "Robust rotation initialisation".
std::vector<ImageMatch> filter_image_matches_by_residual(const std::vector<ImageMatch>& image_matches, const std::vector<double>& residuals, double thresh_rad);
// find_largest_connected_component with per-camera rotations carried along: kept cameras keep their rotation, re-gauged so that the new camera 0 has the identity
// (R_i <- R_i R_0^T leaves every R_b R_a^T as it is).  Host code.
void find_largest_connected_component(std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations);

// The reference seeds std::mt19937 from std::random_device and draws inside an OpenMP loop; here the draw is sequential from
// `seed` (deterministic), everything after it follows the reference: costs of all trials in one GPU launch, first minimum,
// the initial rotations at the best focal, then the joint rotation + focal refinement.  sequential = true chains the matches (k-1, k)
// (ssfm_focal_search); sequential = false chains along the spanning tree from camera 0 (ssfm_focal_search_graph), where the reference
// calls GraphOptim.  Returns false on an error of the library.
bool find_best_focal_length_random(ssfm_ctx* ctx, int num_cameras, std::vector<ImageMatch>& image_matches, bool inward, bool sequential,
                                   double focal_guess, double min_focal, double max_focal, int num_trials, std::vector<Mat3>& rotations,
                                   double& best_focal, unsigned seed = 0, const char* costs_path = "costs.txt");

// find_best_focal_length_random on a view graph whose matches may carry wrong rotations (ssfm_focal_search_l1; DESIGN.md 4, "Robust focal search"):
//   1. the trial focals are drawn as find_best_focal_length_random draws them (the same seed gives the same focals);
//   2. ssfm_focal_search_l1 from camera 0 with its defaults: one L1 solve per trial, the trial with the smallest sum of residuals wins; costs_path gets
//      "%d %lf %lf %lf": trial, focal, the sum, get_cost at the L1 rotations;
//   3. the matches take their rotations at the found focal, and initialize_rotations_l1 (defaults: 30 iterations) gives converged residuals there --
//      the search stops at 10 iterations, where the weights have not settled;
//   4. filter_image_matches_by_residual(thresh_rad), then find_largest_connected_component with the rotations carried along and re-gauged: keyframes and
//      image_matches shrink as in the calibrated driver with -rotinit l1;
//   5. ssfm_posegraph_focal_solve from those rotations on the kept matches, inside [min_focal, max_focal].
// The cut is applied only at the found focal: at a focal that is still off, clean loops do not close and a 2 degree cut would drop clean matches.
// summary->frame0 / frame1 / residual list every match that entered step 3 (Keyframe::index of its two cameras, radians, -1 = not used).
// Returns false on an error of the library or when no match survives the cut.  find_best_focal_length_random itself is untouched.
struct FocalL1Summary {
    size_t edges_in = 0, edges_kept = 0, cameras_in = 0, cameras_kept = 0;
    int best_trial = 0; double focal_search = 0.0, search_cost = 0.0, search_kernel_ms = 0.0;
    ssfm_rot_l1_summary l1{};
    std::vector<int> frame0, frame1; std::vector<double> residual;
};
bool find_best_focal_length_random_l1(ssfm_ctx* ctx, std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, bool inward, double focal_guess,
                                      double min_focal, double max_focal, int num_trials, std::vector<Mat3>& rotations, double& best_focal, unsigned seed = 0,
                                      const char* costs_path = "costs.txt", double thresh_rad = 2.0 * 3.14159265358979323846 / 180.0, FocalL1Summary* summary = nullptr);

}  // namespace sphericalsfm
