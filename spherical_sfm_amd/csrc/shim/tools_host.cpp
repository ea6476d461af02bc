// see tools.h -- the part of the mirror that never calls the library: the on-disk formats and find_largest_connected_component.  Kept in a unit of its own so
// that it builds and runs (tests/native/front_tools_check.cpp) without libssfm_hip.so.
#include "tools.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <iostream>

namespace sphericalsfm {

void write_feature_tracks(const std::string& outputpath, const std::vector<Keyframe>& keyframes, const std::vector<ImageMatch>& image_matches) {
    if (FILE* f = std::fopen((outputpath + "/keyframes.txt").c_str(), "w")) {
        std::fprintf(f, "%d\n", (int)keyframes.size());
        for (const Keyframe& k : keyframes) std::fprintf(f, "%d %s\n", k.index, k.name.c_str());
        std::fclose(f);
    }
    if (FILE* f = std::fopen((outputpath + "/features.dat").c_str(), "w")) {
        for (const Keyframe& k : keyframes) {
            const int nfeatures = k.features.size();
            std::fwrite(&nfeatures, sizeof(int), 1, f);
            for (int j = 0; j < nfeatures; j++) {
                std::fwrite(&k.features.points[j].x, sizeof(float), 1, f); std::fwrite(&k.features.points[j].y, sizeof(float), 1, f);
                static const float zeros[128] = {0};
                std::fwrite(k.features.descs.size() >= (size_t)(j + 1) * 128 ? &k.features.descs[(size_t)j * 128] : zeros, sizeof(float), 128, f);
            }
        }
        std::fclose(f);
    }
    if (FILE* f = std::fopen((outputpath + "/matches.dat").c_str(), "w")) {
        const int n = (int)image_matches.size(); std::fwrite(&n, sizeof(int), 1, f);
        for (const ImageMatch& m : image_matches) {
            std::fwrite(&m.index0, sizeof(int), 1, f); std::fwrite(&m.index1, sizeof(int), 1, f);
            const int nm = (int)m.matches.size(); std::fwrite(&nm, sizeof(int), 1, f);
            for (auto& kv : m.matches) { const int a = (int)kv.first, b = (int)kv.second; std::fwrite(&a, sizeof(int), 1, f); std::fwrite(&b, sizeof(int), 1, f); }
            std::fwrite(m.R.data(), sizeof(double), 9, f);                              // Eigen column-major
        }
        std::fclose(f);
    }
}

bool read_features(const std::string& outputpath, std::vector<Keyframe>& keyframes) {
    FILE* kf = std::fopen((outputpath + "/keyframes.txt").c_str(), "r");
    if (!kf) return false;
    int nkeyframes = 0;
    if (std::fscanf(kf, "%d\n", &nkeyframes) != 1 || nkeyframes < 0) { std::fclose(kf); return false; }
    std::vector<int> indices(nkeyframes);
    for (int i = 0; i < nkeyframes; i++) {
        if (std::fscanf(kf, "%d", &indices[i]) != 1) { std::fclose(kf); return false; }
        int ch; while ((ch = std::fgetc(kf)) != EOF && ch != '\n') {}                  // the rest of the line is the name
    }
    std::fclose(kf);
    std::cout << "read " << indices.size() << " indices\n";
    FILE* ff = std::fopen((outputpath + "/features.dat").c_str(), "r");
    if (!ff) return false;
    for (int i = 0; i < nkeyframes; i++) {
        int nfeatures = 0;
        if (std::fread(&nfeatures, sizeof(int), 1, ff) != 1 || nfeatures < 0) { std::fclose(ff); return false; }
        Features features; features.points.resize(nfeatures); features.descs.resize((size_t)nfeatures * 128);
        for (int j = 0; j < nfeatures; j++) {
            if (std::fread(&features.points[j].x, sizeof(float), 1, ff) != 1 || std::fread(&features.points[j].y, sizeof(float), 1, ff) != 1 ||
                std::fread(&features.descs[(size_t)j * 128], sizeof(float), 128, ff) != 128) { std::fclose(ff); return false; }
        }
        char name[1024]; std::snprintf(name, sizeof name, "%06d.jpg", indices[i] + 1);
        keyframes.push_back(Keyframe(indices[i], name, features));
    }
    std::fclose(ff);
    return true;
}

bool read_feature_tracks(const std::string& outputpath, std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches) {
    if (!read_features(outputpath, keyframes)) return false;
    FILE* mf = std::fopen((outputpath + "/matches.dat").c_str(), "r");
    if (!mf) return false;
    int nmatches = 0;
    if (std::fread(&nmatches, sizeof(int), 1, mf) != 1) { std::fclose(mf); return false; }
    for (int i = 0; i < nmatches; i++) {
        int index0, index1, nm;
        if (std::fread(&index0, sizeof(int), 1, mf) != 1 || std::fread(&index1, sizeof(int), 1, mf) != 1 || std::fread(&nm, sizeof(int), 1, mf) != 1) { std::fclose(mf); return false; }
        Matches m;
        for (int j = 0; j < nm; j++) { int a, b; if (std::fread(&a, sizeof(int), 1, mf) != 1 || std::fread(&b, sizeof(int), 1, mf) != 1) { std::fclose(mf); return false; } m[a] = b; }
        Mat3 R; if (std::fread(R.data(), sizeof(double), 9, mf) != 9) { std::fclose(mf); return false; }
        image_matches.push_back(ImageMatch(index0, index1, m, R));
    }
    std::fclose(mf);
    return true;
}

std::vector<ImageMatch> apply_triplet_filter(const std::vector<ImageMatch>& image_matches, const std::vector<uint8_t>& good, int64_t num_records,
                                             const int32_t* triplet_edges, const double* triplet_err, const char* log_path) {
    const size_t E = image_matches.size();
    if (log_path) {
        if (FILE* f = std::fopen(log_path, "w")) {                                        // spherical_sfm_tools.cpp:1057
            for (int64_t t = 0; t < num_records; t++) {
                const int32_t i = triplet_edges[3 * t], j = triplet_edges[3 * t + 1];
                if (i < 0 || j < 0 || (size_t)i >= E || (size_t)j >= E) continue;
                std::fprintf(f, "%d %d %d %f\n", image_matches[(size_t)i].index0, image_matches[(size_t)i].index1, image_matches[(size_t)j].index1, triplet_err[t] * 180 / M_PI);
            }
            std::fclose(f);
        }
    }
    int count = 0;
    std::vector<ImageMatch> image_matches_new;
    for (size_t i = 0; i < E && i < good.size(); i++)
        if (good[i]) { count++; image_matches_new.push_back(image_matches[i]); }
    std::cout << count << " / " << E << " good edges\n";                                  // :1079
    return image_matches_new;
}

void find_largest_connected_component(std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches) {
    int nv = 0;
    for (const ImageMatch& m : image_matches) nv = std::max(nv, std::max(m.index0, m.index1) + 1);
    std::vector<int> parent(nv);
    for (int i = 0; i < nv; i++) parent[i] = i;
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (const ImageMatch& m : image_matches) {
        if (m.index0 < 0 || m.index1 < 0) continue;
        const int a = find(m.index0), b = find(m.index1);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);                              // the root of a component is its smallest vertex
    }
    // components in order of their smallest vertex = ascending root; the first largest wins
    std::vector<int> size(nv, 0);
    for (int i = 0; i < nv; i++) size[find(i)]++;
    int best = -1;
    for (int i = 0; i < nv; i++) if (parent[i] == i && (best < 0 || size[i] > size[best])) best = i;
    std::vector<int> renumber(nv, -1);
    std::vector<Keyframe> kept;
    for (int i = 0; i < nv && i < (int)keyframes.size(); i++)
        if (best >= 0 && find(i) == best) { renumber[i] = (int)kept.size(); kept.push_back(keyframes[i]); }
    std::vector<ImageMatch> kept_matches;
    for (const ImageMatch& m : image_matches) {
        if (m.index0 < 0 || m.index1 < 0 || renumber[m.index0] < 0 || renumber[m.index1] < 0) continue;
        kept_matches.push_back(ImageMatch(renumber[m.index0], renumber[m.index1], m.matches, m.R));
    }
    keyframes.swap(kept); image_matches.swap(kept_matches);
}

std::vector<ImageMatch> filter_image_matches_by_residual(const std::vector<ImageMatch>& image_matches, const std::vector<double>& residuals, double thresh_rad) {
    std::vector<ImageMatch> kept;
    for (size_t e = 0; e < image_matches.size() && e < residuals.size(); e++)
        if (residuals[e] >= 0.0 && residuals[e] <= thresh_rad) kept.push_back(image_matches[e]);
    return kept;
}

void find_largest_connected_component(std::vector<Keyframe>& keyframes, std::vector<ImageMatch>& image_matches, std::vector<Mat3>& rotations) {
    // Keyframe::index is the one field the component pass carries through untouched: lend it the position for the duration of the call
    std::vector<int> index(keyframes.size());
    for (size_t i = 0; i < keyframes.size(); i++) { index[i] = keyframes[i].index; keyframes[i].index = (int)i; }
    find_largest_connected_component(keyframes, image_matches);
    const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<Mat3> kept(keyframes.size(), I);
    for (size_t k = 0; k < keyframes.size(); k++) {
        const size_t pos = (size_t)keyframes[k].index;
        keyframes[k].index = index[pos];
        if (pos < rotations.size()) kept[k] = rotations[pos];
    }
    if (!kept.empty()) {
        const Mat3 R0 = kept[0];
        for (Mat3& R : kept) {                                                            // R <- R R0^T, column-major
            Mat3 Rn;
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = 0; for (int q = 0; q < 3; q++) s += R[r + 3 * q] * R0[c + 3 * q]; Rn[r + 3 * c] = s; }
            R = Rn;
        }
    }
    rotations.swap(kept);
}

}  // namespace sphericalsfm
