// Drop-in driver for the uncalibrated pipeline from the feature tracks on (examples/run_spherical_sfm_uncalib.cpp:101-228):
// focal guess (width + height) / 2, matches whose rotations were estimated at that guess, 1024-trial focal search around the pose
// graph + joint refinement (find_best_focal_length_random), build_sfm at the found focal, shared focal FREE in every bundle
// adjustment: spherical BA -> Retriangulate -> BA, with -generalba: unfix translations -> BA -> Normalize -> Retriangulate -> BA ->
// Normalize; poses.txt, OBJ files, COLMAP text model, calib.txt.  Everything numerical runs in libssfm_hip.so.
// -match: no matches.dat -- match_exhaustive + estimate_pairwise at the guessed focal in one device call (estimate_pairwise_from_features), then
// find_largest_connected_component (:96-122).
// -viewgraph: the frames need not be in capture order -- the focal search chains its trial rotations along a breadth-first spanning tree of the matches
// (find_best_focal_length_random with sequential = false -> ssfm_focal_search_graph) instead of along the matches (k-1, k).  Without it nothing changes.
// -rotinit l1 (with -viewgraph; default: tree) [-rotinitthresh DEG, default 2]: the focal search solves the rotations of every trial robustly and judges the trial
// by the sum of the residuals (find_best_focal_length_random_l1 -> ssfm_focal_search_l1): a wrong match on a tree edge no longer spoils the cost of every trial.
// At the found focal the matches whose converged L1 residual exceeds the threshold are dropped, find_largest_connected_component runs once more, and the joint
// refinement starts from the L1 rotations of what is left; rotinit.txt lists every pair with its residual, ROTINIT_RESULT the counts.
// -fivepoint: the pairwise stage is general relative pose (estimate_pairwise_five_point, examples/run_spherical_sfm_uncalib.cpp:107-110) instead of the spherical
// three-point estimator: with -match in one device call from the feature tables (estimate_pairwise_five_point_from_features: the match lists stay on the
// device), without it on the matches of matches.dat, whose rotations it replaces.
// -guided (with -match): the accepted pairs are rematched under their own essential matrix at the guessed focal -- E(R) of the spherical estimator, the E of
// the five-point estimator with -fivepoint -- before find_largest_connected_component (guided_match -> ssfm_guided_match_pairs).  GUIDED_RESULT reports the counts.
//   run_spherical_sfm_uncalib -output <dir with keyframes.txt, features.dat, matches.dat> -width W -height H [-generalba] [-inward]
//                             [-match [-guided]] [-fivepoint] [-inlierthresh T] [-mininliers N] [-viewgraph [-rotinit tree|l1] [-rotinitthresh DEG]] [-devicetracks]
// -devicetracks: build_sfm's track pass runs on the device (ssfm_build_tracks_device: connected components, canonical point ids).  Without it nothing changes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "tools.h"
using namespace sphericalsfm;

int main(int argc, char** argv) {
    std::string output; bool inward = false, generalba = false, match_mode = false, viewgraph = false, fivepoint = false; int width = 0, height = 0, num_trials = 1024, mininliers = 100; unsigned seed = 0; double inlierthresh = 2.0;
    bool rotinit_l1 = false, device_tracks = false, guided = false; double rotinit_thresh_deg = 2.0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-output" && i + 1 < argc) output = argv[++i];
        else if (a == "-width" && i + 1 < argc) width = std::atoi(argv[++i]);
        else if (a == "-height" && i + 1 < argc) height = std::atoi(argv[++i]);
        else if (a == "-trials" && i + 1 < argc) num_trials = std::atoi(argv[++i]);
        else if (a == "-seed" && i + 1 < argc) seed = (unsigned)std::atoi(argv[++i]);
        else if (a == "-inward") inward = true;
        else if (a == "-devicetracks") device_tracks = true;                // build_sfm's track pass on the device (ssfm_build_tracks_device); default: the host pass
        else if (a == "-generalba") generalba = true;
        else if (a == "-match") match_mode = true;
        else if (a == "-fivepoint") fivepoint = true;
        else if (a == "-guided") guided = true;                             // with -match: rematch the accepted pairs under their E
        else if (a == "-inlierthresh" && i + 1 < argc) inlierthresh = std::atof(argv[++i]);
        else if (a == "-mininliers" && i + 1 < argc) mininliers = std::atoi(argv[++i]);
        else if (a == "-sequential") viewgraph = false;
        else if (a == "-viewgraph") viewgraph = true;
        else if (a == "-rotinit" && i + 1 < argc) {
            const std::string o = argv[++i];
            if (o == "l1") rotinit_l1 = true; else if (o == "tree") rotinit_l1 = false;
            else { std::cout << "unknown rotation initialisation " << o << " (tree or l1)\n"; return 2; }
        }
        else if (a == "-rotinitthresh" && i + 1 < argc) rotinit_thresh_deg = std::atof(argv[++i]);
        else { std::cout << "unknown argument " << a << "\n"; return 2; }
    }
    if (output.empty() || width <= 0 || height <= 0) { std::cout << "usage: run_spherical_sfm_uncalib -output <dir> -width W -height H [-generalba] [-inward]\n"; return 2; }
    if (rotinit_l1 && !viewgraph) { std::cout << "-rotinit l1 needs -viewgraph\n"; return 2; }
    if (guided && !match_mode) { std::cout << "error: -guided needs -match\n"; return 1; }
    std::vector<Keyframe> keyframes; std::vector<ImageMatch> image_matches;
    const double focal_guess = (width + height) / 2, centerx = width / 2, centery = height / 2;     // :101-103 (integer division as in the reference)
    if (match_mode ? !read_features(output, keyframes) : (!read_feature_tracks(output, keyframes, image_matches) || image_matches.empty())) { std::cout << "error: no matches found\n"; return 1; }
    std::cout << "initial focal: " << focal_guess << "\n";
    const double min_focal = focal_guess / 4, max_focal = focal_guess * 2;                          // :141-142

    SfM sfm_probe(Intrinsics(focal_guess, centerx, centery));                                       // owns the library context for the pairwise stage and the search
    int loop_closures = -1;
    std::vector<Mat3> guided_Es;                                                                    // -fivepoint -guided: the E of every accepted pair
    auto rematch = [&]() {                                                                          // -guided: before the component step renumbers the frames
        size_t before = 0, after = 0;
        for (const ImageMatch& im : image_matches) before += im.matches.size();
        if (fivepoint) guided_match(sfm_probe.GetContext(), Intrinsics(focal_guess, centerx, centery), keyframes, image_matches, guided_Es, inlierthresh);
        else guided_match(sfm_probe.GetContext(), Intrinsics(focal_guess, centerx, centery), keyframes, image_matches, inlierthresh, inward);
        for (const ImageMatch& im : image_matches) after += im.matches.size();
        std::printf("GUIDED_RESULT pairs=%zu matches_before=%zu matches_after=%zu\n", image_matches.size(), before, after);
    };
    if (fivepoint) {                                                                                // :107-110
        if (match_mode) loop_closures = estimate_pairwise_five_point_from_features(sfm_probe.GetContext(), Intrinsics(focal_guess, centerx, centery), keyframes, inlierthresh, mininliers, image_matches,
                                                                                   guided ? &guided_Es : nullptr);
        else {
            std::vector<ImageMatch> all; all.swap(image_matches);
            loop_closures = estimate_pairwise_five_point(sfm_probe.GetContext(), Intrinsics(focal_guess, centerx, centery), keyframes, all, inlierthresh, mininliers, image_matches);
        }
        if (loop_closures == 0) { std::cout << "error: no loop closures found\n"; return 1; }
        if (guided) rematch();
        find_largest_connected_component(keyframes, image_matches);
        if (image_matches.empty()) { std::cout << "error: no matches found\n"; return 1; }
    } else if (match_mode) {                                                                        // :96-122
        loop_closures = estimate_pairwise_from_features(sfm_probe.GetContext(), Intrinsics(focal_guess, centerx, centery), keyframes, inlierthresh, mininliers, inward, image_matches);
        if (loop_closures == 0) { std::cout << "error: no loop closures found\n"; return 1; }
        if (guided) rematch();
        find_largest_connected_component(keyframes, image_matches);
        if (image_matches.empty()) { std::cout << "error: no matches found\n"; return 1; }
    }
    std::vector<Mat3> rotations; double focal_new = focal_guess;
    if (rotinit_l1) {
        FocalL1Summary l1;
        const bool ok = find_best_focal_length_random_l1(sfm_probe.GetContext(), keyframes, image_matches, inward, focal_guess, min_focal, max_focal, num_trials, rotations,
                                                         focal_new, seed, (output + "/costs.txt").c_str(), rotinit_thresh_deg * M_PI / 180.0, &l1);
        if (FILE* f = std::fopen((output + "/rotinit.txt").c_str(), "w")) {                          // frame numbers of the pair, residual in degrees, 1 = kept
            for (size_t e = 0; e < l1.residual.size(); e++)
                std::fprintf(f, "%d %d %f %d\n", l1.frame0[e], l1.frame1[e], l1.residual[e] * 180.0 / M_PI,
                             l1.residual[e] >= 0.0 && l1.residual[e] <= rotinit_thresh_deg * M_PI / 180.0 ? 1 : 0);
            std::fclose(f);
        }
        if (!ok) { std::cout << "ERROR: could not find any acceptable focal length\n"; return 1; }
        std::printf("ROTINIT_RESULT edges_in=%zu edges_kept=%zu cameras_in=%zu cameras_kept=%zu iterations=%d cg_iterations=%lld cost_initial=%.6e cost_final=%.6e "
                    "focal_search_l1=%.6f search_kernel_ms=%.3f\n", l1.edges_in, l1.edges_kept, l1.cameras_in, l1.cameras_kept, l1.l1.iterations,
                    (long long)l1.l1.pcg_iterations_total, l1.l1.initial_cost, l1.l1.final_cost, l1.focal_search, l1.search_kernel_ms);
    }
    else if (!find_best_focal_length_random(sfm_probe.GetContext(), (int)keyframes.size(), image_matches, inward, !viewgraph, focal_guess, min_focal, max_focal,
                                       num_trials, rotations, focal_new, seed, (output + "/costs.txt").c_str())) {
        std::cout << "ERROR: could not find any acceptable focal length\n"; return 1;
    }
    std::cout << " best focal: " << focal_new << "\n";
    const double focal_search = focal_new;
    Intrinsics intrinsics(focal_new, centerx, centery);

    std::cout << "building sfm\n";
    SfM sfm(intrinsics);
    build_sfm(keyframes, image_matches, rotations, sfm, true, true, inward, 0, device_tracks);
    sfm.SetFocalFixed(false);
    sfm.WriteCOLMAP(output + "/sparse-pre-spherical-ba", width, height);
    sfm.WritePointsOBJ(output + "/points-pre-spherical-ba.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras-pre-spherical-ba.obj");
    const bool ok1 = sfm.Optimize();
    sfm.Retriangulate();
    const bool ok2 = sfm.Optimize();
    sfm.WriteCOLMAP(output + "/sparse-pre-general-ba", width, height);
    sfm.WritePointsOBJ(output + "/points-pre-general-ba.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras-pre-general-ba.obj");
    const double focal_spherical = sfm.GetFocal();
    std::cout << "focal after spherical BA: " << focal_spherical << "\n";
    bool ok3 = true, ok4 = true;
    if (generalba) {
        for (int i = 1; i < sfm.GetNumCameras(); i++) sfm.SetTranslationFixed(i, false);
        std::cout << "running general optimization\n";
        ok3 = sfm.Optimize();
        sfm.Normalize(inward);
        sfm.Retriangulate();
        ok4 = sfm.Optimize();
        sfm.Normalize(inward);
        std::cout << "done.\n";
        std::cout << "focal after general BA: " << sfm.GetFocal() << "\n";
    }
    std::vector<int> keyframe_indices(keyframes.size());
    for (size_t i = 0; i < keyframes.size(); i++) keyframe_indices[i] = keyframes[i].index;
    sfm.WritePoses(output + "/poses.txt", keyframe_indices);
    sfm.WritePointsOBJ(output + "/points.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras.obj");
    sfm.WriteCOLMAP(output + "/sparse", width, height);
    sfm.WriteCalib(output + "/calib.txt");
    std::printf("PAIRWISE_RESULT pairs=%zu loop_closures=%d\n", image_matches.size(), loop_closures);
    std::printf("PIPELINE_RESULT ok=%d%d%d%d cameras=%d focal_guess=%.3f focal_search=%.6f focal_spherical=%.6f focal_final=%.6f cost=%.6e residuals=%lld\n", ok1, ok2, ok3, ok4,
                sfm.GetNumCameras(), focal_guess, focal_search, focal_spherical, sfm.GetFocal(), sfm.LastSummary().final_cost, (long long)sfm.LastSummary().num_residual_blocks);
    return 0;
}
