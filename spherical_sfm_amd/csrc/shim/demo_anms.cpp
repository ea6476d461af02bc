// The C++ mirrors of adaptiveNonMaximalSuppresion and of DetectorTracker::detect's selection (shim/tools.h) on a keypoint file:
//   demo_anms <file>
// <file>, binary, native byte order: int32 F; per frame int32 n, int32 numToKeep, int32 existing, then n x (float x, float y, float response).
// Prints, per frame, "ANMS_FRAME f count idx ..." from the batched overload (one device call; idx: the survivors' positions in the input, carried in class_id),
// "ANMS_SINGLE f equal=0|1" for the single-frame overload against it, and "ANMS_SELECT f points_before points_after count" for select_keypoints on a
// Features that already holds `existing` points; then DEMO_ANMS_RESULT.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "tools.h"
using namespace sphericalsfm;

int main(int argc, char** argv) {
    if (argc < 2) { std::cout << "usage: demo_anms <keypoint file>\n"; return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t F = 0;
    if (!f || std::fread(&F, 4, 1, f) != 1 || F < 0) { std::cout << "error: cannot read " << argv[1] << "\n"; return 1; }
    std::vector<std::vector<KeyPoint>> frames((size_t)F); std::vector<int> keep((size_t)F), existing((size_t)F);
    for (int32_t k = 0; k < F; k++) {
        int32_t h[3];
        if (std::fread(h, 4, 3, f) != 3 || h[0] < 0) { std::cout << "error: truncated file\n"; return 1; }
        keep[(size_t)k] = h[1]; existing[(size_t)k] = h[2];
        for (int32_t i = 0; i < h[0]; i++) {
            float v[3];
            if (std::fread(v, 4, 3, f) != 3) { std::cout << "error: truncated file\n"; return 1; }
            frames[(size_t)k].push_back(KeyPoint{Point2f{v[0], v[1]}, 1.f, -1.f, v[2], 0, i});
        }
    }
    std::fclose(f);
    SfM sfm(Intrinsics(1.0, 0.0, 0.0));                                        // owns the library context
    ssfm_ctx* ctx = sfm.GetContext();
    std::vector<std::vector<KeyPoint>> batched = frames;
    adaptiveNonMaximalSuppresion(ctx, batched, keep);
    int all_equal = 1;
    for (int32_t k = 0; k < F; k++) {
        std::printf("ANMS_FRAME %d %zu", k, batched[(size_t)k].size());
        for (const KeyPoint& kp : batched[(size_t)k]) std::printf(" %d", kp.class_id);
        std::printf("\n");
        std::vector<KeyPoint> single = frames[(size_t)k];
        adaptiveNonMaximalSuppresion(ctx, single, keep[(size_t)k]);
        int equal = single.size() == batched[(size_t)k].size();
        for (size_t q = 0; equal && q < single.size(); q++) equal = single[q].class_id == batched[(size_t)k][q].class_id && single[q].response == batched[(size_t)k][q].response;
        std::printf("ANMS_SINGLE %d equal=%d\n", k, equal);
        all_equal &= equal;
    }
    std::vector<Features> feats((size_t)F); std::vector<Features*> fs;
    for (int32_t k = 0; k < F; k++) { feats[(size_t)k].points.assign((size_t)std::max(existing[(size_t)k], 0), Point2f{0.f, 0.f}); fs.push_back(&feats[(size_t)k]); }
    std::vector<std::vector<KeyPoint>> sel = frames;
    select_keypoints(ctx, fs, sel);
    for (int32_t k = 0; k < F; k++) {
        std::printf("ANMS_SELECT %d %d %zu %zu", k, existing[(size_t)k], feats[(size_t)k].points.size(), sel[(size_t)k].size());
        for (const KeyPoint& kp : sel[(size_t)k]) std::printf(" %d", kp.class_id);
        std::printf("\n");
    }
    std::printf("DEMO_ANMS_RESULT frames=%d single_equals_batched=%d\n", F, all_equal);
    return 0;
}
