// The C++ mirrors of match / match_exhaustive (shim/tools.h) on a feature directory, and the two ways from there to verified image matches:
//   match_exhaustive + estimate_pairwise   against   estimate_pairwise_from_features
//   demo_match <dir with keyframes.txt, features.dat> <focal> <cx> <cy> <inlier threshold px> <min inliers>
// Writes <dir>/match_exhaustive.txt (one line per pair: index0 index1 n, then n x "j i") and <dir>/match_ratio.txt (match() of the first two keyframes with
// ratio 1.5, same format) for the test to compare with its own matcher; prints DEMO_MATCH_RESULT.  Then estimate_pairwise_five_point on the same lists:
// <dir>/five_point.txt (one line per accepted pair: index0 index1 n, n x "j i", the nine entries of R column-major as %.17g) and DEMO_FIVEPOINT_RESULT.
// Then the same keyframes through estimate_pairwise_five_point_from_features: <dir>/five_point_front.txt in the same format and
// DEMO_FIVEPOINT_FRONT_RESULT, whose equal compares with the two-call result.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "tools.h"
using namespace sphericalsfm;

static void write_line(FILE* f, int a, int b, const Matches& m) {
    std::fprintf(f, "%d %d %zu", a, b, m.size());
    for (auto& kv : m) std::fprintf(f, " %zu %zu", kv.first, kv.second);
    std::fprintf(f, "\n");
}

static void write_five(const std::string& path, const std::vector<ImageMatch>& ms) {
    if (FILE* f = std::fopen(path.c_str(), "w")) {
        for (const ImageMatch& m : ms) {
            std::fprintf(f, "%d %d %zu", m.index0, m.index1, m.matches.size());
            for (auto& kv : m.matches) std::fprintf(f, " %zu %zu", kv.first, kv.second);
            for (int q = 0; q < 9; q++) std::fprintf(f, " %.17g", m.R[q]);
            std::fprintf(f, "\n");
        }
        std::fclose(f);
    }
}

int main(int argc, char** argv) {
    if (argc < 7) { std::cout << "usage: demo_match <dir> <focal> <cx> <cy> <inlier threshold> <min inliers>\n"; return 2; }
    const std::string dir = argv[1];
    const Intrinsics intrinsics(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]));
    const double thresh = std::atof(argv[5]); const int min_inliers = std::atoi(argv[6]);
    std::vector<Keyframe> keyframes;
    if (!read_features(dir, keyframes) || keyframes.size() < 2) { std::cout << "error: no features in " << dir << "\n"; return 1; }
    SfM sfm(intrinsics);                                                       // owns the library context
    std::vector<ImageMatch> all;
    match_exhaustive(sfm.GetContext(), keyframes, all);
    if (FILE* f = std::fopen((dir + "/match_exhaustive.txt").c_str(), "w")) { for (const ImageMatch& m : all) write_line(f, m.index0, m.index1, m.matches); std::fclose(f); }
    Matches m01, m15;
    match(sfm.GetContext(), keyframes[0].features, keyframes[1].features, m01);
    match(sfm.GetContext(), keyframes[0].features, keyframes[1].features, m15, 1.5);
    if (FILE* f = std::fopen((dir + "/match_ratio.txt").c_str(), "w")) { write_line(f, 0, 1, m15); std::fclose(f); }
    const int match_same = !all.empty() && all[0].index0 == 0 && all[0].index1 == 1 && all[0].matches == m01;
    std::vector<ImageMatch> a, b;
    const int loops_a = estimate_pairwise(sfm.GetContext(), intrinsics, keyframes, all, thresh, min_inliers, false, a);
    const int loops_b = estimate_pairwise_from_features(sfm.GetContext(), intrinsics, keyframes, thresh, min_inliers, false, b);
    int equal = a.size() == b.size() && loops_a == loops_b;
    for (size_t k = 0; equal && k < a.size(); k++) equal = a[k].index0 == b[k].index0 && a[k].index1 == b[k].index1 && a[k].matches == b[k].matches && a[k].R == b[k].R;
    std::printf("DEMO_MATCH_RESULT keyframes=%zu pairs=%zu match_same=%d accepted_a=%zu accepted_b=%zu loops_a=%d loops_b=%d equal=%d\n", keyframes.size(), all.size(),
                match_same, a.size(), b.size(), loops_a, loops_b, equal);
    std::vector<ImageMatch> five;
    const int loops5 = estimate_pairwise_five_point(sfm.GetContext(), intrinsics, keyframes, all, thresh, min_inliers, five);
    write_five(dir + "/five_point.txt", five);
    std::printf("DEMO_FIVEPOINT_RESULT accepted=%zu loops=%d\n", five.size(), loops5);
    std::vector<ImageMatch> front;
    const int loops5f = estimate_pairwise_five_point_from_features(sfm.GetContext(), intrinsics, keyframes, thresh, min_inliers, front);
    write_five(dir + "/five_point_front.txt", front);
    int equal5 = five.size() == front.size() && loops5 == loops5f;
    for (size_t k = 0; equal5 && k < five.size(); k++)
        equal5 = five[k].index0 == front[k].index0 && five[k].index1 == front[k].index1 && five[k].matches == front[k].matches && five[k].R == front[k].R;
    std::printf("DEMO_FIVEPOINT_FRONT_RESULT accepted=%zu loops=%d equal=%d\n", front.size(), loops5f, equal5);
    return 0;
}
