// Drop-in driver for the calibrated pipeline from the feature tracks on (examples/run_spherical_sfm.cpp:71-121, the flow the
// reference intends past its debugging exit(0) at :81): read keyframes.txt / features.dat / matches.dat, sequential rotation
// initialisation, rotation averaging, build_sfm, spherical BA -> Retriangulate -> BA, general BA -> Normalize -> Retriangulate -> BA
// -> Normalize, then poses.txt, points.obj, cameras.obj and the COLMAP text model.  Everything numerical runs in libssfm_hip.so.
// Feature detection over images (the OpenCV front end) is outside this build.  With -match the driver starts from keyframes.txt + features.dat alone, as the
// reference's driver does after detect_features (:49-55): match_exhaustive + estimate_pairwise in one device call (estimate_pairwise_from_features), then
// find_largest_connected_component.  Without it, it starts from a matches.dat (-pairwise: that file holds raw matches, estimate_pairwise runs first).
// -viewgraph: the frames need not be in capture order (the reference's sequential == false branch, :73-76): filter_image_matches(2 degrees) on the device, then
// find_largest_connected_component AGAIN -- the filter can split the graph; the reference does not guard against that, this driver does -- then the rotations chained
// along a breadth-first spanning tree (initialize_rotations_tree, in place of GraphOptim) and the same rotation averaging.  -tripletorder composed selects the product
// order that the edge convention implies instead of the reference's (include/ssfm.h).  Without -viewgraph nothing changes.
// -rotinit l1 (with -viewgraph; default: tree): the start is the robust one of ssfm_rot_l1_init instead of the tree chain, the matches whose residual at that start
// exceeds -rotinitthresh degrees (default 2) are dropped, find_largest_connected_component runs once more, and refine_rotations starts from the L1 rotations of the
// cameras that are left; rotinit.txt lists every pair with its residual.  One wrong match on a tree edge no longer rotates a whole subtree, and the gross outliers no longer bias the averaging.
// -guided (with -match): the accepted pairs are rematched under their own E(R) (guided_match -> ssfm_guided_match_pairs) before find_largest_connected_component:
// features on repeated structure, which Lowe's test over the whole frame drops, come back.  GUIDED_RESULT reports the counts.  Without it nothing changes.
//   run_spherical_sfm -intrinsics <file: focal cx cy> -output <dir with the feature tracks> [-match [-guided] | -pairwise] [-inward] [-width W -height H]
//                     [-viewgraph [-tripletorder reference|composed] [-rotinit tree|l1] [-rotinitthresh DEG]] [-devicetracks]
// -devicetracks: build_sfm's track pass runs on the device (ssfm_build_tracks_device: connected components, canonical point ids).  Without it nothing changes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include "tools.h"
using namespace sphericalsfm;

int main(int argc, char** argv) {
    std::string intrinsics_path, output; bool inward = false, pairwise = false, match_mode = false, viewgraph = false; int triplet_order = SSFM_TRIPLET_ORDER_REFERENCE, width = 1920, height = 1080, mininliers = 100; double inlierthresh = 2.0;
    bool rotinit_l1 = false, device_tracks = false, guided = false; double rotinit_thresh_deg = 2.0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-intrinsics" && i + 1 < argc) intrinsics_path = argv[++i];
        else if (a == "-output" && i + 1 < argc) output = argv[++i];
        else if (a == "-width" && i + 1 < argc) width = std::atoi(argv[++i]);
        else if (a == "-height" && i + 1 < argc) height = std::atoi(argv[++i]);
        else if (a == "-inward") inward = true;
        else if (a == "-devicetracks") device_tracks = true;                // build_sfm's track pass on the device (ssfm_build_tracks_device); default: the host pass
        else if (a == "-pairwise") pairwise = true;                         // matches.dat holds raw matches: run estimate_pairwise (GPU RANSAC) first
        else if (a == "-match") match_mode = true;                          // no matches.dat: features -> verified image matches on the device
        else if (a == "-guided") guided = true;                             // with -match: rematch the accepted pairs under their E
        else if (a == "-inlierthresh" && i + 1 < argc) inlierthresh = std::atof(argv[++i]);
        else if (a == "-mininliers" && i + 1 < argc) mininliers = std::atoi(argv[++i]);
        else if (a == "-sequential") viewgraph = false;                     // the default: rotations chained over the matches (k-1, k)
        else if (a == "-viewgraph") viewgraph = true;                       // any pair may carry a rotation: triplet filter + spanning-tree initialisation
        else if (a == "-tripletorder" && i + 1 < argc) {
            const std::string o = argv[++i];
            if (o == "composed") triplet_order = SSFM_TRIPLET_ORDER_COMPOSED; else if (o == "reference") triplet_order = SSFM_TRIPLET_ORDER_REFERENCE;
            else { std::cout << "unknown triplet order " << o << "\n"; return 2; }
        }
        else if (a == "-rotinit" && i + 1 < argc) {
            const std::string o = argv[++i];
            if (o == "l1") rotinit_l1 = true; else if (o == "tree") rotinit_l1 = false;
            else { std::cout << "unknown rotation initialisation " << o << "\n"; return 2; }
        }
        else if (a == "-rotinitthresh" && i + 1 < argc) rotinit_thresh_deg = std::atof(argv[++i]);
        else { std::cout << "unknown argument " << a << "\n"; return 2; }
    }
    if (rotinit_l1 && !viewgraph) { std::cout << "-rotinit l1 needs -viewgraph\n"; return 2; }
    if (guided && !match_mode) { std::cout << "error: -guided needs -match\n"; return 1; }
    if (intrinsics_path.empty() || output.empty()) { std::cout << "usage: run_spherical_sfm -intrinsics <file> -output <dir> [-inward]\n"; return 2; }
    double focal, centerx, centery;
    std::ifstream intrinsicsf(intrinsics_path);
    if (!(intrinsicsf >> focal >> centerx >> centery)) { std::cout << "error: could not read " << intrinsics_path << "\n"; return 1; }
    std::cout << "intrinsics : " << focal << ", " << centerx << ", " << centery << "\n";
    Intrinsics intrinsics(focal, centerx, centery);

    std::vector<Keyframe> keyframes; std::vector<ImageMatch> image_matches;
    if (match_mode) { if (!read_features(output, keyframes)) { std::cout << "error: no features in " << output << "\n"; return 1; } }
    else {
        if (!read_feature_tracks(output, keyframes, image_matches)) { std::cout << "error: no feature tracks in " << output << "\n"; return 1; }
        if (image_matches.empty()) { std::cout << "error: no loop closures found\n"; return 1; }
    }

    SfM sfm(intrinsics);
    int loop_closures = -1;
    if (match_mode) {                                                        // run_spherical_sfm.cpp:49-55
        std::cout << "matching and detecting loop closures\n";
        const size_t nframes = keyframes.size();
        loop_closures = estimate_pairwise_from_features(sfm.GetContext(), intrinsics, keyframes, inlierthresh, mininliers, inward, image_matches);
        if (loop_closures == 0) { std::cout << "error: no loop closures found\n"; return 1; }
        if (guided) {
            size_t before = 0, after = 0;
            for (const ImageMatch& im : image_matches) before += im.matches.size();
            guided_match(sfm.GetContext(), intrinsics, keyframes, image_matches, inlierthresh, inward);
            for (const ImageMatch& im : image_matches) after += im.matches.size();
            std::printf("GUIDED_RESULT pairs=%zu matches_before=%zu matches_after=%zu\n", image_matches.size(), before, after);
        }
        find_largest_connected_component(keyframes, image_matches);
        std::cout << "kept " << keyframes.size() << " of " << nframes << " keyframes, " << image_matches.size() << " image pairs, " << loop_closures << " loop closures\n";
    } else if (pairwise) {                                                          // run_spherical_sfm.cpp:56-63
        std::cout << "detecting loop closures\n";
        std::vector<ImageMatch> all_image_matches; all_image_matches.swap(image_matches);
        loop_closures = estimate_pairwise(sfm.GetContext(), intrinsics, keyframes, all_image_matches, inlierthresh, mininliers, inward, image_matches);
        if (loop_closures == 0) { std::cout << "error: no loop closures found\n"; return 1; }
        std::cout << "kept " << image_matches.size() << " of " << all_image_matches.size() << " image pairs, " << loop_closures << " loop closures\n";
    }
    if (viewgraph) {                                                         // run_spherical_sfm.cpp:73-76
        std::cout << "filtering image matches\n";
        const size_t nframes = keyframes.size(), nmatches = image_matches.size();
        image_matches = filter_image_matches(sfm.GetContext(), image_matches, 2.0 * M_PI / 180.0, triplet_order);
        if (image_matches.empty()) { std::cout << "error: no image match survived the triplet filter\n"; return 1; }
        find_largest_connected_component(keyframes, image_matches);          // the filter may have split the graph
        std::cout << "after the triplet filter: " << keyframes.size() << " of " << nframes << " keyframes, " << image_matches.size() << " of " << nmatches << " image pairs\n";
    }
    std::cout << "initializing rotations\n";
    std::vector<Mat3> rotations;
    if (viewgraph && rotinit_l1) {
        std::vector<double> residuals; ssfm_rot_l1_summary l1;
        const size_t edges_in = image_matches.size(), frames_in = keyframes.size();
        initialize_rotations_l1(sfm.GetContext(), (int)keyframes.size(), image_matches, rotations, residuals, 0, &l1);
        if (FILE* f = std::fopen((output + "/rotinit.txt").c_str(), "w")) {             // frame numbers of the pair, residual in degrees, 1 = kept
            for (size_t e = 0; e < edges_in; e++)
                std::fprintf(f, "%d %d %f %d\n", keyframes[image_matches[e].index0].index, keyframes[image_matches[e].index1].index, residuals[e] * 180.0 / M_PI,
                             residuals[e] >= 0.0 && residuals[e] <= rotinit_thresh_deg * M_PI / 180.0 ? 1 : 0);
            std::fclose(f);
        }
        image_matches = filter_image_matches_by_residual(image_matches, residuals, rotinit_thresh_deg * M_PI / 180.0);
        if (image_matches.empty()) { std::cout << "error: no image match survived the residual cut\n"; return 1; }
        find_largest_connected_component(keyframes, image_matches, rotations);          // the cut may have split the graph
        std::printf("ROTINIT_RESULT edges_in=%zu edges_kept=%zu cameras_in=%zu cameras_kept=%zu iterations=%d cg_iterations=%lld cost_initial=%.6e cost_final=%.6e\n", edges_in,
                    image_matches.size(), frames_in, keyframes.size(), l1.iterations, (long long)l1.pcg_iterations_total, l1.initial_cost, l1.final_cost);
    }
    else if (viewgraph) initialize_rotations_tree((int)keyframes.size(), image_matches, rotations);
    else initialize_rotations_sequential((int)keyframes.size(), image_matches, rotations);

    std::cout << "refining rotations\n";
    const double rot_cost = refine_rotations(sfm.GetContext(), (int)keyframes.size(), image_matches, rotations);

    std::cout << "building sfm\n";
    build_sfm(keyframes, image_matches, rotations, sfm, true, true, inward, 0, device_tracks);
    sfm.WritePointsOBJ(output + "/points-pre-spherical-ba.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras-pre-spherical-ba.obj");

    const bool ok1 = sfm.Optimize();
    sfm.Retriangulate();
    const bool ok2 = sfm.Optimize();
    const double cost_spherical = sfm.LastSummary().final_cost;
    sfm.WritePointsOBJ(output + "/points-pre-ba.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras-pre-ba.obj");

    // --- general SFM ---
    for (int i = 1; i < sfm.GetNumCameras(); i++) sfm.SetTranslationFixed(i, false);
    std::cout << "running general optimization\n";
    const bool ok3 = sfm.Optimize();
    sfm.Normalize(inward);
    sfm.Retriangulate();
    const bool ok4 = sfm.Optimize();
    sfm.Normalize(inward);
    std::cout << "done.\n";

    std::vector<int> keyframe_indices(keyframes.size());
    for (size_t i = 0; i < keyframes.size(); i++) keyframe_indices[i] = keyframes[i].index;
    sfm.WritePoses(output + "/poses.txt", keyframe_indices);
    sfm.WritePointsOBJ(output + "/points.obj");
    sfm.WriteCameraCentersOBJ(output + "/cameras.obj");
    sfm.WriteCOLMAP(output, width, height);
    std::printf("PAIRWISE_RESULT pairs=%zu loop_closures=%d\n", image_matches.size(), loop_closures);
    std::printf("PIPELINE_RESULT ok=%d%d%d%d cameras=%d points=%d rot_cost=%.6e cost_spherical=%.6e cost_general=%.6e residuals=%lld\n", ok1, ok2, ok3, ok4,
                sfm.GetNumCameras(), sfm.GetNumPoints(), rot_cost, cost_spherical, sfm.LastSummary().final_cost, (long long)sfm.LastSummary().num_residual_blocks);
    return 0;
}
