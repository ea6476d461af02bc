// see tools.h
#include "tools.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>

#include "../ssfm_math.h"

namespace sphericalsfm {

int estimate_pairwise(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches,
                      double inlier_threshold, int min_num_inliers, bool inward, std::vector<ImageMatch>& image_matches_out) {
    const double kinv = 1.0 / intrinsics.focal;                                           // Kinv(0,0)
    const double sq_thresh = inlier_threshold * inlier_threshold * kinv * kinv;           // :315
    // the reference enumerates all (index0 < index1) and takes the FIRST stored match set of each pair
    std::map<std::pair<int, int>, const ImageMatch*> first;
    for (const ImageMatch& m : image_matches) if (m.index0 < m.index1) first.emplace(std::make_pair(m.index0, m.index1), &m);
    std::vector<const ImageMatch*> cand;
    for (auto& kv : first) if ((int)kv.second->matches.size() >= min_num_inliers && !kv.second->matches.empty()) cand.push_back(kv.second);   // :353
    if (cand.empty()) return 0;
    // per-frame feature rays Kinv * (x, y, 1) (:362-376, once per feature) + per-pair match lists: ssfm_ransac_batch_indexed gathers the ray pairs on the device
    const int nf = (int)keyframes.size();
    std::vector<int32_t> feat_ptr(nf + 1, 0);
    for (int f = 0; f < nf; f++) feat_ptr[f + 1] = feat_ptr[f] + (int32_t)keyframes[f].features.points.size();
    std::vector<double> rays((size_t)3 * std::max(1, (int)feat_ptr[nf]));
    for (int f = 0; f < nf; f++) {
        const Features& ft = keyframes[f].features;
        for (size_t k = 0; k < ft.points.size(); k++) {
            double* r = &rays[3 * ((size_t)feat_ptr[f] + k)];
            r[0] = (ft.points[k].x - intrinsics.centerx) * kinv; r[1] = (ft.points[k].y - intrinsics.centery) * kinv; r[2] = 1.0;
        }
    }
    std::vector<int32_t> pair_ptr(1, 0), pf0, pf1, m0, m1;
    for (const ImageMatch* m : cand) {
        pf0.push_back(m->index0); pf1.push_back(m->index1);
        for (auto& kv : m->matches) { m0.push_back((int32_t)kv.first); m1.push_back((int32_t)kv.second); }
        pair_ptr.push_back((int32_t)m0.size());
    }
    ssfm_ransac_options O; ssfm_ransac_default_options(&O);
    O.min_num_inliers = min_num_inliers; O.inward = inward ? 1 : 0; O.final_least_squares = 1;                                 // :316-318
    const int P = (int)cand.size();
    std::vector<double> R((size_t)9 * P); std::vector<uint8_t> mask(std::max<size_t>(1, m0.size())); std::vector<int32_t> nin(P);
    // COLLECTIVE when the context carries a communicator (ssfm_comm_init / ssfm_comm_init_host): every rank of the job must make this call with the same
    // keyframes and matches, or the ranks that did wait in the result all-reduce forever -- a rank-0-only pairwise stage needs a context of its own without a
    // communicator.  Without one this is the plain single-GPU indexed batch.  (The result table is summed: a -0.0 entry of a rotation comes back as +0.0 on the
    // ranks that did not compute it; every other bit equals the single-GPU result.)
    if (ssfm_ransac_batch_indexed_sharded(ctx, nf, feat_ptr.data(), rays.data(), P, pf0.data(), pf1.data(), pair_ptr.data(), m0.data(), m1.data(), sq_thresh, &O, nullptr, R.data(),
                                  mask.data(), nin.data(), nullptr, nullptr) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    int loop_closure_count = 0;
    for (int k = 0; k < P; k++) {
        if (!(nin[k] > min_num_inliers)) continue;                                        // :410
        Matches inl; size_t j = (size_t)pair_ptr[k];
        for (auto& kv : cand[k]->matches) { if (mask[j++]) inl[kv.first] = kv.second; }
        if (inl.empty()) continue;
        Mat3 Rk; for (int q = 0; q < 9; q++) Rk[q] = R[9 * (size_t)k + q];
        if (cand[k]->index0 + 1 != cand[k]->index1) loop_closure_count++;
        image_matches_out.push_back(ImageMatch(cand[k]->index0, cand[k]->index1, inl, Rk));
    }
    return loop_closure_count;
}

int estimate_pairwise_five_point(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches,
                      double inlier_threshold, int min_num_inliers, std::vector<ImageMatch>& image_matches_out) {
    const double kinv = 1.0 / intrinsics.focal;                                           // Kinv(0,0)
    const double sq_thresh = inlier_threshold * inlier_threshold * kinv * kinv;           // :440
    // the reference enumerates all (index0 < index1) and takes the FIRST stored match set of each pair
    std::map<std::pair<int, int>, const ImageMatch*> first;
    for (const ImageMatch& m : image_matches) if (m.index0 < m.index1) first.emplace(std::make_pair(m.index0, m.index1), &m);
    std::vector<const ImageMatch*> cand;
    for (auto& kv : first) if ((int)kv.second->matches.size() >= min_num_inliers && !kv.second->matches.empty()) cand.push_back(kv.second);   // :476
    if (cand.empty()) return 0;
    // per-frame feature rays Kinv * (x, y, 1) (:484-500, once per feature) + per-pair match lists: ssfm_ransac5_batch_indexed gathers the ray pairs on the device
    const int nf = (int)keyframes.size();
    std::vector<int32_t> feat_ptr(nf + 1, 0);
    for (int f = 0; f < nf; f++) feat_ptr[f + 1] = feat_ptr[f] + (int32_t)keyframes[f].features.points.size();
    std::vector<double> rays((size_t)3 * std::max(1, (int)feat_ptr[nf]));
    for (int f = 0; f < nf; f++) {
        const Features& ft = keyframes[f].features;
        for (size_t k = 0; k < ft.points.size(); k++) {
            double* r = &rays[3 * ((size_t)feat_ptr[f] + k)];
            r[0] = (ft.points[k].x - intrinsics.centerx) * kinv; r[1] = (ft.points[k].y - intrinsics.centery) * kinv; r[2] = 1.0;
        }
    }
    std::vector<int32_t> pair_ptr(1, 0), pf0, pf1, m0, m1;
    for (const ImageMatch* m : cand) {
        pf0.push_back(m->index0); pf1.push_back(m->index1);
        for (auto& kv : m->matches) { m0.push_back((int32_t)kv.first); m1.push_back((int32_t)kv.second); }
        pair_ptr.push_back((int32_t)m0.size());
    }
    ssfm_ransac_options O; ssfm_ransac_default_options(&O);
    O.min_num_inliers = min_num_inliers;                                                  // :441-445 (the LO options it sets have no effect on this estimator)
    const int P = (int)cand.size();
    std::vector<double> R((size_t)9 * P); std::vector<uint8_t> mask(std::max<size_t>(1, m0.size())); std::vector<int32_t> nin(P);
    if (ssfm_ransac5_batch_indexed(ctx, nf, feat_ptr.data(), rays.data(), P, pf0.data(), pf1.data(), pair_ptr.data(), m0.data(), m1.data(), sq_thresh, &O, nullptr, R.data(), nullptr,
                                   mask.data(), nin.data(), nullptr, nullptr) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    int loop_closure_count = 0;
    for (int k = 0; k < P; k++) {
        if (!(nin[k] > min_num_inliers)) continue;                                        // :535
        Matches inl; size_t j = (size_t)pair_ptr[k];
        for (auto& kv : cand[k]->matches) { if (mask[j++]) inl[kv.first] = kv.second; }
        if (inl.empty()) continue;
        Mat3 Rk; for (int q = 0; q < 9; q++) Rk[q] = R[9 * (size_t)k + q];
        if (cand[k]->index0 + 1 != cand[k]->index1) loop_closure_count++;
        image_matches_out.push_back(ImageMatch(cand[k]->index0, cand[k]->index1, inl, Rk));
    }
    return loop_closure_count;
}

// per-frame tables of the C ABI: feat_ptr, descriptors (128 floats per feature), optionally the rays Kinv (x, y, 1)
static void feature_tables(const std::vector<const Features*>& fs, const Intrinsics* intrinsics, std::vector<int32_t>& feat_ptr, std::vector<float>& descs, std::vector<double>* rays) {
    const int nf = (int)fs.size();
    feat_ptr.assign(nf + 1, 0);
    for (int f = 0; f < nf; f++) feat_ptr[f + 1] = feat_ptr[f] + (int32_t)fs[f]->points.size();
    descs.assign((size_t)128 * std::max(1, (int)feat_ptr[nf]), 0.0f);
    if (rays) rays->assign((size_t)3 * std::max(1, (int)feat_ptr[nf]), 0.0);
    for (int f = 0; f < nf; f++) {
        const Features& ft = *fs[f];
        const size_t n = ft.points.size(), have = std::min(n, ft.descs.size() / 128);
        if (have) std::copy(ft.descs.begin(), ft.descs.begin() + have * 128, descs.begin() + (size_t)feat_ptr[f] * 128);
        if (rays) {
            const double kinv = 1.0 / intrinsics->focal;
            for (size_t k = 0; k < n; k++) {
                double* r = &(*rays)[3 * ((size_t)feat_ptr[f] + k)];
                r[0] = (ft.points[k].x - intrinsics->centerx) * kinv; r[1] = (ft.points[k].y - intrinsics->centery) * kinv; r[2] = 1.0;
            }
        }
    }
}

static void exhaustive_pairs(const std::vector<Keyframe>& keyframes, std::vector<int32_t>& pf0, std::vector<int32_t>& pf1) {
    for (size_t a = 0; a < keyframes.size(); a++) for (size_t b = a + 1; b < keyframes.size(); b++) { pf0.push_back((int32_t)a); pf1.push_back((int32_t)b); }   // :577-586
}

static void match_lists(ssfm_ctx* ctx, const std::vector<const Features*>& fs, const std::vector<int32_t>& pf0, const std::vector<int32_t>& pf1, double ratio,
                        std::vector<int32_t>& mp, std::vector<int32_t>& m0, std::vector<int32_t>& m1) {
    std::vector<int32_t> feat_ptr; std::vector<float> descs;
    feature_tables(fs, nullptr, feat_ptr, descs, nullptr);
    ssfm_match_options O; ssfm_match_default_options(&O); O.ratio = ratio;
    const int P = (int)pf0.size();
    mp.assign(P + 1, 0);
    int64_t cap = 0;
    for (int p = 0; p < P; p++) cap += std::min(feat_ptr[pf0[p] + 1] - feat_ptr[pf0[p]], feat_ptr[pf1[p] + 1] - feat_ptr[pf1[p]]);       // a pair has at most min(n0, n1) matches
    m0.assign((size_t)std::max<int64_t>(cap, 1), 0); m1.assign((size_t)std::max<int64_t>(cap, 1), 0);
    if (ssfm_match_pairs(ctx, (int32_t)fs.size(), feat_ptr.data(), descs.data(), P, pf0.data(), pf1.data(), &O, cap, mp.data(), m0.data(), m1.data()) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
}

void match(ssfm_ctx* ctx, const Features& features0, const Features& features1, Matches& m01, double ratio) {
    std::vector<int32_t> mp, m0, m1;
    match_lists(ctx, {&features0, &features1}, {0}, {1}, ratio, mp, m0, m1);
    for (int32_t k = mp[0]; k < mp[1]; k++) m01[(size_t)m0[k]] = (size_t)m1[k];
}

void adaptiveNonMaximalSuppresion(ssfm_ctx* ctx, std::vector<std::vector<KeyPoint>>& keypoints_per_frame, const std::vector<int>& numToKeep) {
    const int F = (int)keypoints_per_frame.size();
    if ((int)numToKeep.size() != F) { std::cout << "error: adaptiveNonMaximalSuppresion: one numToKeep per frame\n"; std::exit(1); }
    std::vector<int32_t> kp_ptr((size_t)F + 1, 0), keep(numToKeep.begin(), numToKeep.end()), keep_ptr((size_t)F + 1, 0);
    for (int f = 0; f < F; f++) kp_ptr[(size_t)f + 1] = kp_ptr[(size_t)f] + (int32_t)keypoints_per_frame[(size_t)f].size();
    const size_t total = (size_t)kp_ptr[(size_t)F];
    std::vector<float> xy(2 * std::max<size_t>(total, 1)), response(std::max<size_t>(total, 1));
    std::vector<int32_t> keep_idx(std::max<size_t>(total, 1));
    for (int f = 0; f < F; f++)
        for (size_t k = 0; k < keypoints_per_frame[(size_t)f].size(); k++) {
            const KeyPoint& kp = keypoints_per_frame[(size_t)f][k]; const size_t g = (size_t)kp_ptr[(size_t)f] + k;
            xy[2 * g] = kp.pt.x; xy[2 * g + 1] = kp.pt.y; response[g] = kp.response;
        }
    if (ssfm_anms_batch(ctx, F, kp_ptr.data(), xy.data(), response.data(), keep.data(), nullptr, keep_ptr.data(), keep_idx.data(), nullptr) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    for (int f = 0; f < F; f++) {
        std::vector<KeyPoint>& kps = keypoints_per_frame[(size_t)f];
        if ((int)kps.size() < numToKeep[(size_t)f]) continue;                               // :79, left as they are
        std::vector<KeyPoint> anmsPts;
        for (int32_t q = keep_ptr[(size_t)f]; q < keep_ptr[(size_t)f + 1]; q++) anmsPts.push_back(kps[(size_t)keep_idx[(size_t)q]]);
        anmsPts.swap(kps);
    }
}

void adaptiveNonMaximalSuppresion(ssfm_ctx* ctx, std::vector<KeyPoint>& keypoints, const int numToKeep) {
    std::vector<std::vector<KeyPoint>> one(1); one[0].swap(keypoints);
    adaptiveNonMaximalSuppresion(ctx, one, std::vector<int>(1, numToKeep));
    keypoints.swap(one[0]);
}

void select_keypoints(ssfm_ctx* ctx, std::vector<Features*>& features, std::vector<std::vector<KeyPoint>>& keypoints_per_frame) {
    if (features.size() != keypoints_per_frame.size()) { std::cout << "error: select_keypoints: one Features per frame\n"; std::exit(1); }
    std::vector<std::vector<KeyPoint>> live; std::vector<int> ntokeep; std::vector<size_t> frame;
    for (size_t f = 0; f < features.size(); f++) {
        const int n = std::max(0, 4000 - (int)features[f]->points.size());                  // :186
        if (n == 0) { keypoints_per_frame[f].clear(); continue; }                           // :187
        live.emplace_back(); live.back().swap(keypoints_per_frame[f]); ntokeep.push_back(n); frame.push_back(f);
    }
    adaptiveNonMaximalSuppresion(ctx, live, ntokeep);
    for (size_t k = 0; k < live.size(); k++) {
        for (const KeyPoint& kp : live[k]) features[frame[k]]->points.push_back(kp.pt);     // :204
        keypoints_per_frame[frame[k]].swap(live[k]);
    }
}

void select_keypoints(ssfm_ctx* ctx, Features& features, std::vector<KeyPoint>& keypoints) {
    std::vector<Features*> fs(1, &features); std::vector<std::vector<KeyPoint>> one(1); one[0].swap(keypoints);
    select_keypoints(ctx, fs, one);
    keypoints.swap(one[0]);
}

void match_exhaustive(ssfm_ctx* ctx, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches) {
    if (keyframes.size() < 2) return;
    std::vector<const Features*> fs; for (const Keyframe& k : keyframes) fs.push_back(&k.features);
    std::vector<int32_t> pf0, pf1, mp, m0, m1;
    exhaustive_pairs(keyframes, pf0, pf1);
    match_lists(ctx, fs, pf0, pf1, 0.75, mp, m0, m1);
    const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (size_t p = 0; p < pf0.size(); p++) {                                             // every pair is stored, also one without a match (:577-586), under its POSITIONS
        Matches m; for (int32_t k = mp[p]; k < mp[p + 1]; k++) m[(size_t)m0[k]] = (size_t)m1[k];
        image_matches.push_back(ImageMatch(pf0[p], pf1[p], m, I));
    }
}

// the two one-call front ends: exhaustive pairs, capacity bounds that cannot miss, the loop-closure count (five: ssfm_pairwise5_from_features, no `inward`)
static int pairwise_front(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, double inlier_threshold, int min_num_inliers,
                          bool five, bool inward, std::vector<ImageMatch>& image_matches_out, std::vector<Mat3>* Es_out = nullptr) {
    if (keyframes.size() < 2) return 0;
    const double kinv = 1.0 / intrinsics.focal;
    const double sq_thresh = inlier_threshold * inlier_threshold * kinv * kinv;           // :315, :440
    std::vector<const Features*> fs; for (const Keyframe& k : keyframes) fs.push_back(&k.features);
    std::vector<int32_t> feat_ptr, pf0, pf1; std::vector<float> descs; std::vector<double> rays;
    feature_tables(fs, &intrinsics, feat_ptr, descs, &rays);
    exhaustive_pairs(keyframes, pf0, pf1);
    ssfm_ransac_options O; ssfm_ransac_default_options(&O);
    O.min_num_inliers = min_num_inliers;
    if (!five) { O.inward = inward ? 1 : 0; O.final_least_squares = 1; }                  // :316-318 (five: :441-445, the LO options it sets have no effect on that estimator)
    const int P = (int)pf0.size();
    int64_t pair_cap = P, inl_cap = 0, needed[2] = {0, 0};
    for (int p = 0; p < P; p++) inl_cap += std::min(feat_ptr[pf0[p] + 1] - feat_ptr[pf0[p]], feat_ptr[pf1[p] + 1] - feat_ptr[pf1[p]]);   // a pair has at most min(n0, n1) matches: never a miss
    std::vector<int32_t> acc, nin, ptr, i0, i1; std::vector<double> R, t, E;
    for (int attempt = 0; attempt < 2; attempt++) {                                       // the capacity protocol (the bounds above cannot miss; a retry would repeat all the work)
        acc.assign((size_t)std::max<int64_t>(pair_cap, 1), 0); nin.assign(acc.size(), 0); ptr.assign((size_t)pair_cap + 1, 0); R.assign(9 * acc.size(), 0.0);
        i0.assign((size_t)std::max<int64_t>(inl_cap, 1), 0); i1.assign(i0.size(), 0);
        if (five) t.assign(3 * acc.size(), 0.0);                                          // (ImageMatch has no place for t; E only for a caller that goes on to guided_match)
        if (five && Es_out) E.assign(9 * acc.size(), 0.0);
        const int rc = five ? ssfm_pairwise5_from_features(ctx, (int32_t)fs.size(), feat_ptr.data(), descs.data(), rays.data(), P, pf0.data(), pf1.data(), nullptr, &O, sq_thresh,
                                                           pair_cap, inl_cap, needed, acc.data(), R.data(), t.data(), Es_out ? E.data() : nullptr, nin.data(), ptr.data(), i0.data(), i1.data(),
                                                           nullptr, nullptr, nullptr)
                            : ssfm_pairwise_from_features(ctx, (int32_t)fs.size(), feat_ptr.data(), descs.data(), rays.data(), P, pf0.data(), pf1.data(), nullptr, &O, sq_thresh,
                                                          pair_cap, inl_cap, needed, acc.data(), R.data(), nin.data(), ptr.data(), i0.data(), i1.data(), nullptr, nullptr, nullptr);
        if (rc == SSFM_OK) break;
        if (attempt == 0 && (needed[0] > pair_cap || needed[1] > inl_cap)) { pair_cap = needed[0]; inl_cap = needed[1]; continue; }
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    int loop_closure_count = 0;
    for (int64_t a = 0; a < needed[0]; a++) {
        const int index0 = pf0[acc[a]], index1 = pf1[acc[a]];                             // positions in `keyframes`, as estimate_pairwise reads ImageMatch::index0 / index1
        Matches inl; for (int32_t k = ptr[a]; k < ptr[a + 1]; k++) inl[(size_t)i0[k]] = (size_t)i1[k];
        Mat3 Rk; for (int q = 0; q < 9; q++) Rk[q] = R[9 * (size_t)a + q];
        if (index0 + 1 != index1) loop_closure_count++;
        image_matches_out.push_back(ImageMatch(index0, index1, inl, Rk));
        if (five && Es_out) { Mat3 Ek; for (int q = 0; q < 9; q++) Ek[q] = E[9 * (size_t)a + q]; Es_out->push_back(Ek); }
    }
    return loop_closure_count;
}

int estimate_pairwise_from_features(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, double inlier_threshold, int min_num_inliers,
                                    bool inward, std::vector<ImageMatch>& image_matches_out) {
    return pairwise_front(ctx, intrinsics, keyframes, inlier_threshold, min_num_inliers, false, inward, image_matches_out);
}

int estimate_pairwise_five_point_from_features(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, double inlier_threshold,
                                               int min_num_inliers, std::vector<ImageMatch>& image_matches_out, std::vector<Mat3>* Es_out) {
    return pairwise_front(ctx, intrinsics, keyframes, inlier_threshold, min_num_inliers, true, false, image_matches_out, Es_out);
}

void guided_match(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, const std::vector<Mat3>& Es,
                  double inlier_threshold, double ratio, float max_distance) {
    if (Es.size() != image_matches.size()) { std::cout << "error: guided_match: one E per image match\n"; std::exit(1); }
    if (image_matches.empty()) return;
    const double kinv = 1.0 / intrinsics.focal;
    std::vector<const Features*> fs; for (const Keyframe& k : keyframes) fs.push_back(&k.features);
    std::vector<int32_t> feat_ptr, pf0, pf1; std::vector<float> descs; std::vector<double> rays, E;
    feature_tables(fs, &intrinsics, feat_ptr, descs, &rays);
    int64_t cap = 0;
    for (size_t p = 0; p < image_matches.size(); p++) {
        const int a = image_matches[p].index0, b = image_matches[p].index1;
        if (a < 0 || b < 0 || a >= (int)fs.size() || b >= (int)fs.size()) { std::cout << "error: guided_match: an image match names a keyframe that is not there\n"; std::exit(1); }
        pf0.push_back(a); pf1.push_back(b); E.insert(E.end(), Es[p].begin(), Es[p].end());
        cap += std::min(feat_ptr[a + 1] - feat_ptr[a], feat_ptr[b + 1] - feat_ptr[b]);      // a pair has at most min(n0, n1) matches
    }
    ssfm_guided_match_options O; ssfm_guided_match_default_options(&O);
    O.ratio = ratio; O.max_distance = max_distance; O.squared_threshold = inlier_threshold * inlier_threshold * kinv * kinv;     // the unit of estimate_pairwise (:315)
    const int P = (int)pf0.size();
    std::vector<int32_t> mp((size_t)P + 1, 0), m0((size_t)std::max<int64_t>(cap, 1), 0), m1((size_t)std::max<int64_t>(cap, 1), 0);
    if (ssfm_guided_match_pairs(ctx, (int32_t)fs.size(), feat_ptr.data(), descs.data(), rays.data(), P, pf0.data(), pf1.data(), E.data(), &O, cap, mp.data(), m0.data(),
                                m1.data()) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    for (int p = 0; p < P; p++) {
        Matches m; for (int32_t k = mp[p]; k < mp[p + 1]; k++) m[(size_t)m0[k]] = (size_t)m1[k];
        image_matches[(size_t)p].matches.swap(m);
    }
}

void guided_match(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, double inlier_threshold,
                  bool inward, double ratio, float max_distance) {
    std::vector<Mat3> Es;
    for (const ImageMatch& im : image_matches) {                                          // make_spherical_essential_matrix (src/spherical_utils.cpp:9-14); Mat3 is column-major
        const Mat3& R = im.R;
        double t[3] = {R[6], R[7], R[8] - 1.0};                                           // R e_z - e_z
        if (inward) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
        Mat3 E;
        for (int c = 0; c < 3; c++) {                                                     // column c of [t]x R = t x (column c of R)
            const double* r = &R[3 * c];
            E[3 * c] = t[1] * r[2] - t[2] * r[1]; E[3 * c + 1] = t[2] * r[0] - t[0] * r[2]; E[3 * c + 2] = t[0] * r[1] - t[1] * r[0];
        }
        Es.push_back(E);
    }
    guided_match(ctx, intrinsics, keyframes, image_matches, Es, inlier_threshold, ratio, max_distance);
}

void initialize_rotations_sequential(int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations) {
    const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    rotations.assign(num_cameras, I);
    Mat3 R = I;
    for (int index = 1; index < num_cameras; index++)
        for (size_t i = 0; i < image_matches.size(); i++)
            if (image_matches[i].index0 == index - 1 && image_matches[i].index1 == index) {
                Mat3 Rn;                                                              // R = match.R * R, column-major 3x3
                for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int k = 0; k < 3; k++) s += image_matches[i].R[r + 3 * k] * R[k + 3 * c]; Rn[r + 3 * c] = s; }
                R = Rn; rotations[index] = R;
                break;
            }
}

std::vector<ImageMatch> filter_image_matches(ssfm_ctx* ctx, std::vector<ImageMatch>& image_matches, double err_thresh_rad, int order, const char* log_path) {
    const int E = (int)image_matches.size();
    int num_cameras = 0;
    std::vector<int32_t> i0(E), i1(E); std::vector<double> rel((size_t)9 * E);
    for (int e = 0; e < E; e++) {
        i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; num_cameras = std::max(num_cameras, std::max(i0[e], i1[e]) + 1);
        for (int k = 0; k < 9; k++) rel[9 * (size_t)e + k] = image_matches[e].R[k];
    }
    std::vector<uint8_t> good((size_t)E, 0); int64_t num_triplets = 0;
    std::vector<int32_t> tri; std::vector<double> err;
    for (int pass = 0; pass < (log_path ? 2 : 1); pass++) {                               // the log needs the count first: with a log_path the WHOLE call runs twice (filter kernel included), the second time asking for that many records
        if (pass == 1) { tri.assign((size_t)std::max<int64_t>(3 * num_triplets, 1), 0); err.assign((size_t)std::max<int64_t>(num_triplets, 1), 0.0); }
        if (ssfm_triplet_filter(ctx, num_cameras, E, i0.data(), i1.data(), rel.data(), err_thresh_rad, order, good.data(), &num_triplets, pass ? num_triplets : 0,
                                pass ? tri.data() : nullptr, pass ? err.data() : nullptr) != SSFM_OK) {
            std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
        }
    }
    return apply_triplet_filter(image_matches, good, log_path ? num_triplets : 0, tri.data(), err.data(), log_path);
}

void initialize_rotations_tree(int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations, int root) {
    const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    rotations.assign(std::max(num_cameras, 0), I);
    const int E = (int)image_matches.size();
    if (num_cameras <= 0) return;
    std::vector<int32_t> i0(E), i1(E), node(num_cameras), parent(num_cameras), edge(num_cameras), level_ptr((size_t)num_cameras + 1); std::vector<uint8_t> rev(num_cameras);
    for (int e = 0; e < E; e++) { i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; }
    int32_t reached = 0, levels = 0;
    if (ssfm_view_graph_tree(num_cameras, E, i0.data(), i1.data(), root, &reached, node.data(), parent.data(), edge.data(), rev.data(), &levels, level_ptr.data()) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(nullptr) << "\n"; std::exit(1);
    }
    for (int k = 1; k < reached; k++) {                                                   // column-major 3x3: R_child = R_e R_parent, or R_e^T R_parent for an edge stored (child, parent)
        const Mat3& Re = image_matches[edge[k]].R; const Mat3& Rp = rotations[parent[k]];
        Mat3 Rn;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int q = 0; q < 3; q++) s += (rev[k] ? Re[q + 3 * r] : Re[r + 3 * q]) * Rp[q + 3 * c]; Rn[r + 3 * c] = s; }
        rotations[node[k]] = Rn;
    }
}

void initialize_rotations_l1(ssfm_ctx* ctx, int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations, std::vector<double>& residuals,
                             int root, ssfm_rot_l1_summary* summary) {
    const int E = (int)image_matches.size();
    std::vector<int32_t> i0(E), i1(E); std::vector<double> rel((size_t)9 * E), rot((size_t)9 * std::max(num_cameras, 0));
    for (int e = 0; e < E; e++) { i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; for (int k = 0; k < 9; k++) rel[9 * (size_t)e + k] = image_matches[e].R[k]; }
    residuals.assign((size_t)E, -1.0);
    ssfm_rot_l1_summary S;
    if (ssfm_rot_l1_init(ctx, num_cameras, E, i0.data(), i1.data(), rel.data(), root, nullptr, rot.data(), residuals.data(), &S) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
    }
    rotations.resize(std::max(num_cameras, 0));
    for (int i = 0; i < num_cameras; i++) for (int k = 0; k < 9; k++) rotations[i][k] = rot[9 * (size_t)i + k];
    if (summary) *summary = S;
}

double refine_rotations(ssfm_ctx* ctx, int num_cameras, const std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations) {
    const int E = (int)image_matches.size();
    std::vector<int32_t> i0(E), i1(E); std::vector<double> rel((size_t)9 * E), rot((size_t)9 * num_cameras);
    for (int e = 0; e < E; e++) { i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; for (int k = 0; k < 9; k++) rel[9 * (size_t)e + k] = image_matches[e].R[k]; }
    for (int i = 0; i < num_cameras; i++) for (int k = 0; k < 9; k++) rot[9 * (size_t)i + k] = rotations[i][k];
    ssfm_ba_summary S;
    if (ssfm_rotavg_solve(ctx, num_cameras, rot.data(), E, i0.data(), i1.data(), rel.data(), nullptr, &S) != SSFM_OK || S.termination == SSFM_FAILURE) {
        std::cout << "error: ceres failed.\n"; std::exit(1);                          // src/rotation_averaging.cpp:82-86
    }
    for (int i = 0; i < num_cameras; i++) for (int k = 0; k < 9; k++) rotations[i][k] = rot[9 * (size_t)i + k];
    return S.final_cost;
}

void build_sfm(std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches, const std::vector<Mat3>& rotations, SfM& sfm,
               bool spherical, bool merge, bool inward, int fix_camera, bool device_tracks) {
    std::cout << "building tracks\n";
    const int nk = (int)keyframes.size();
    std::vector<int32_t> feat_ptr(nk + 1, 0);
    for (int i = 0; i < nk; i++) feat_ptr[i + 1] = feat_ptr[i] + keyframes[i].features.size();
    std::vector<double> feat_xy((size_t)feat_ptr[nk] * 2);
    for (int i = 0; i < nk; i++) for (int j = 0; j < keyframes[i].features.size(); j++) {
        feat_xy[2 * ((size_t)feat_ptr[i] + j)] = keyframes[i].features.points[j].x; feat_xy[2 * ((size_t)feat_ptr[i] + j) + 1] = keyframes[i].features.points[j].y; }
    std::vector<int32_t> ms0, ms1, ms_ptr(1, 0), f0, f1;
    for (const ImageMatch& m : image_matches) {
        ms0.push_back(m.index0); ms1.push_back(m.index1);
        for (auto& kv : m.matches) { f0.push_back((int32_t)kv.first); f1.push_back((int32_t)kv.second); }
        ms_ptr.push_back((int32_t)f0.size());
    }
    const size_t nm = f0.size();
    if (device_tracks && !merge) { std::cout << "device tracks need merge = true: the host track pass runs\n"; device_tracks = false; }
    const size_t nobs_cap = device_tracks ? (size_t)feat_ptr[nk] + 1 : 2 * nm + 1;
    std::vector<int32_t> tracks(feat_ptr[nk]), ocam(nobs_cap), opt(nobs_cap); std::vector<uint8_t> alive(device_tracks ? 1 : nm + 1); std::vector<double> oxy(2 * nobs_cap);
    int32_t npts = 0; int64_t nobs = 0;
    std::cout << "adding cameras\n";
    for (int index = 0; index < nk; index++) {
        double Rm[9], r[3];                                                          // so3ln of the column-major rotation
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rm[3 * a + b] = rotations[index][a + 3 * b];
        ssfm::so3ln(Rm, r);
        const int camera = sfm.AddCamera(Pose(Vec3(0, 0, inward ? 1 : -1), Vec3(r[0], r[1], r[2])), keyframes[index].name);
        sfm.SetRotationFixed(camera, index == fix_camera);
        sfm.SetTranslationFixed(camera, spherical ? true : (index == fix_camera));
    }
    std::cout << "adding tracks\nnumber of keyframes is " << nk << "\n";
    if (device_tracks) {                                                             // connected components with canonical ids: every id is alive
        std::vector<int32_t> ofeat(nobs_cap);
        ssfm_ctx* ctx = sfm.GetContext();
        if (ssfm_build_tracks_device(ctx, nk, feat_ptr.data(), feat_xy.data(), (int32_t)image_matches.size(), ms0.data(), ms1.data(), ms_ptr.data(), f0.data(), f1.data(),
                                     sfm.GetIntrinsics().centerx, sfm.GetIntrinsics().centery, tracks.data(), &npts, nullptr, &nobs, ocam.data(), opt.data(), ofeat.data(),
                                     oxy.data()) != SSFM_OK) {
            std::cout << "error: " << ssfm_last_error(ctx) << "\n"; std::exit(1);
        }
        std::cout << "device tracks: " << npts << " points, " << nobs << " observations\n";
    }
    else ssfm_build_tracks(nk, feat_ptr.data(), feat_xy.data(), (int32_t)image_matches.size(), ms0.data(), ms1.data(), ms_ptr.data(), f0.data(), f1.data(),
                           sfm.GetIntrinsics().centerx, sfm.GetIntrinsics().centery, merge ? 1 : 0, tracks.data(), &npts, alive.data(), &nobs, ocam.data(), opt.data(), oxy.data());
    for (int i = 0; i < nk; i++) keyframes[i].features.tracks.assign(tracks.begin() + feat_ptr[i], tracks.begin() + feat_ptr[i + 1]);
    for (int j = 0; j < npts; j++) { const int p = sfm.AddPoint(Point(0, 0, 0)); sfm.SetPointFixed(p, false); }
    if (!device_tracks) for (int j = 0; j < npts; j++) if (!alive[j]) sfm.RemovePoint(j);   // points consumed by MergePoint
    for (int64_t o = 0; o < nobs; o++) sfm.AddObservation(ocam[o], opt[o], Observation(oxy[2 * o], oxy[2 * o + 1]));
    std::cout << "retriangulating...\n";
    sfm.Retriangulate();
}

bool find_best_focal_length_random(ssfm_ctx* ctx, int num_cameras, std::vector<ImageMatch>& image_matches, bool inward, bool sequential,
                                   double focal_guess, double min_focal, double max_focal, int num_trials, std::vector<Mat3>& rotations,
                                   double& best_focal, unsigned seed, const char* costs_path) {
    const int E = (int)image_matches.size();
    std::vector<int32_t> i0(E), i1(E); std::vector<double> rel((size_t)9 * E);
    for (int e = 0; e < E; e++) { i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; for (int k = 0; k < 9; k++) rel[9 * (size_t)e + k] = image_matches[e].R[k]; }
    std::mt19937 gen(seed);
    std::uniform_real_distribution<double> dist(min_focal, max_focal);                    // spherical_sfm_tools.cpp:1449-1451
    std::vector<double> focals(num_trials), costs(num_trials);
    for (int t = 0; t < num_trials; t++) focals[t] = dist(gen);
    int32_t best = 0;
    std::vector<double> rot((size_t)9 * num_cameras), rel_best((size_t)9 * E);
    const int rc = sequential ? ssfm_focal_search(ctx, num_cameras, E, i0.data(), i1.data(), rel.data(), inward ? 1 : 0, focal_guess, num_trials, focals.data(), costs.data(),
                                                  &best, rot.data(), rel_best.data())
                              : ssfm_focal_search_graph(ctx, num_cameras, E, i0.data(), i1.data(), rel.data(), inward ? 1 : 0, focal_guess, num_trials, focals.data(), 0,
                                                        costs.data(), &best, rot.data(), rel_best.data());
    if (rc != SSFM_OK) { std::cout << "error: " << ssfm_last_error(ctx) << "\n"; return false; }
    if (costs_path) {                                                                     // :1463-1468
        if (FILE* f = std::fopen(costs_path, "w")) { for (int t = 0; t < num_trials; t++) std::fprintf(f, "%d %lf %lf\n", t, focals[t], costs[t]); std::fclose(f); }
    }
    best_focal = focals[best];
    std::cout << "before optimization: " << best_focal << "\n";
    // run_optimization (:1160-1188): matches at the best focal, joint refinement of rotations and focal inside [min, max]
    ssfm_ba_summary S;
    if (ssfm_posegraph_focal_solve(ctx, num_cameras, rot.data(), E, i0.data(), i1.data(), rel_best.data(), &best_focal, min_focal, max_focal, nullptr, &S) != SSFM_OK
        || S.termination == SSFM_FAILURE) { std::cout << "error: ceres failed.\n"; return false; }
    rotations.resize(num_cameras);
    for (int i = 0; i < num_cameras; i++) for (int k = 0; k < 9; k++) rotations[i][k] = rot[9 * (size_t)i + k];
    std::cout << "after optimization: " << best_focal << "\n";
    return true;
}

bool find_best_focal_length_random_l1(ssfm_ctx* ctx, std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, bool inward, double focal_guess,
                                      double min_focal, double max_focal, int num_trials, std::vector<Mat3>& rotations, double& best_focal, unsigned seed,
                                      const char* costs_path, double thresh_rad, FocalL1Summary* summary) {
    const int num_cameras = (int)keyframes.size(), E = (int)image_matches.size();
    std::vector<int32_t> i0(E), i1(E); std::vector<double> rel((size_t)9 * E);
    for (int e = 0; e < E; e++) { i0[e] = image_matches[e].index0; i1[e] = image_matches[e].index1; for (int k = 0; k < 9; k++) rel[9 * (size_t)e + k] = image_matches[e].R[k]; }
    std::mt19937 gen(seed);
    std::uniform_real_distribution<double> dist(min_focal, max_focal);                    // as find_best_focal_length_random draws
    std::vector<double> focals(std::max(num_trials, 0)), costs(focals.size()), get_costs(focals.size());
    for (int t = 0; t < num_trials; t++) focals[t] = dist(gen);
    int32_t best = 0; double kernel_ms = 0.0;
    std::vector<double> rel_best((size_t)9 * E);
    if (ssfm_focal_search_l1(ctx, num_cameras, E, i0.data(), i1.data(), rel.data(), inward ? 1 : 0, focal_guess, num_trials, focals.data(), 0, nullptr, costs.data(),
                             get_costs.data(), nullptr, &best, nullptr, rel_best.data(), nullptr, &kernel_ms) != SSFM_OK) {
        std::cout << "error: " << ssfm_last_error(ctx) << "\n"; return false;
    }
    if (costs_path) {
        if (FILE* f = std::fopen(costs_path, "w")) { for (int t = 0; t < num_trials; t++) std::fprintf(f, "%d %lf %lf %lf\n", t, focals[t], costs[t], get_costs[t]); std::fclose(f); }
    }
    best_focal = focals[best];
    std::cout << "before optimization: " << best_focal << "\n";
    FocalL1Summary S;
    S.edges_in = (size_t)E; S.cameras_in = keyframes.size(); S.best_trial = best; S.focal_search = best_focal; S.search_cost = costs[best]; S.search_kernel_ms = kernel_ms;
    // the matches at the found focal; converged residuals there, the cut, the component
    for (int e = 0; e < E; e++) for (int k = 0; k < 9; k++) image_matches[e].R[k] = rel_best[9 * (size_t)e + k];
    std::vector<double> residuals;
    initialize_rotations_l1(ctx, num_cameras, image_matches, rotations, residuals, 0, &S.l1);
    S.frame0.resize(E); S.frame1.resize(E); S.residual = residuals;
    for (int e = 0; e < E; e++) { S.frame0[e] = keyframes[image_matches[e].index0].index; S.frame1[e] = keyframes[image_matches[e].index1].index; }
    image_matches = filter_image_matches_by_residual(image_matches, residuals, thresh_rad);
    if (image_matches.empty()) { std::cout << "error: no image match survived the residual cut\n"; if (summary) *summary = S; return false; }
    find_largest_connected_component(keyframes, image_matches, rotations);                // the cut may have split the graph
    S.edges_kept = image_matches.size(); S.cameras_kept = keyframes.size();
    if (summary) *summary = S;
    // run_optimization (:1160-1188) from the L1 rotations on the kept matches
    const int nk = (int)keyframes.size(), Ek = (int)image_matches.size();
    std::vector<int32_t> k0(Ek), k1(Ek); std::vector<double> relk((size_t)9 * Ek), rot((size_t)9 * nk);
    for (int e = 0; e < Ek; e++) { k0[e] = image_matches[e].index0; k1[e] = image_matches[e].index1; for (int k = 0; k < 9; k++) relk[9 * (size_t)e + k] = image_matches[e].R[k]; }
    for (int i = 0; i < nk; i++) for (int k = 0; k < 9; k++) rot[9 * (size_t)i + k] = rotations[i][k];
    ssfm_ba_summary B;
    if (ssfm_posegraph_focal_solve(ctx, nk, rot.data(), Ek, k0.data(), k1.data(), relk.data(), &best_focal, min_focal, max_focal, nullptr, &B) != SSFM_OK
        || B.termination == SSFM_FAILURE) { std::cout << "error: ceres failed.\n"; return false; }
    for (int i = 0; i < nk; i++) for (int k = 0; k < 9; k++) rotations[i][k] = rot[9 * (size_t)i + k];
    std::cout << "after optimization: " << best_focal << "\n";
    return true;
}

}  // namespace sphericalsfm
