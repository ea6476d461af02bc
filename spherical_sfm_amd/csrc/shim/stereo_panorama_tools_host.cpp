// spherical_sfm_amd -- the host half of the stereo panorama mirror (stereo_panorama_tools.h): poses, levelling, thetas, loop trimming, PPM / .flo files.
// No GPU and no libssfm_hip: tests/native/pano_host_check.cpp compiles this file alone under ASan + UBSan.
#include "stereo_panorama_tools.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../ssfm_math.h"

namespace stereopanotools {

static void center_of(const Keyframe& kf, double c[3]) {               // c = -R^T t
    double m[3]; ssfm::mat3_tvec(kf.R, kf.t, m);
    for (int i = 0; i < 3; i++) c[i] = -m[i];
}

bool load_keyframes(const std::string& posespath, std::vector<Keyframe>& keyframes) {
    FILE* posesf = std::fopen(posespath.c_str(), "r");
    if (!posesf) return false;
    while (true) {
        int index; double t[3], r[3];
        const int nread = std::fscanf(posesf, "%d %lf %lf %lf %lf %lf %lf\n", &index, t + 0, t + 1, t + 2, r + 0, r + 1, r + 2);
        if (nread != 7) break;
        Keyframe kf;
        kf.index = index;
        for (int i = 0; i < 3; i++) { kf.t[i] = t[i]; kf.r[i] = r[i]; }
        ssfm::so3exp(kf.r, kf.R);
        keyframes.push_back(kf);
    }
    std::fclose(posesf);
    return true;
}

// Eigenvector of the smallest eigenvalue of the scatter of the centres about their mean, by cyclic Jacobi rotations (a symmetric 3x3 converges in a few sweeps).
void plane_normal(const std::vector<Keyframe>& keyframes, double up[3]) {
    up[0] = 0; up[1] = 1; up[2] = 0;
    const size_t n = keyframes.size();
    if (n < 3) return;
    std::vector<double> c(3 * n); double mean[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++) { center_of(keyframes[i], &c[3 * i]); for (int k = 0; k < 3; k++) mean[k] += c[3 * i + k]; }
    for (int k = 0; k < 3; k++) mean[k] /= (double)n;
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) A[a][b] += (c[3 * i + a] - mean[a]) * (c[3 * i + b] - mean[b]);
    for (int sweep = 0; sweep < 50; sweep++) {
        const double off = std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]);
        if (off <= 1e-300 || off <= 1e-18 * (std::fabs(A[0][0]) + std::fabs(A[1][1]) + std::fabs(A[2][2]))) break;
        for (int p = 0; p < 2; p++) for (int q = p + 1; q < 3; q++) {
            if (A[p][q] == 0.0) continue;
            const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double tt = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau)), cs = 1.0 / std::sqrt(1.0 + tt * tt), sn = tt * cs;
            for (int k = 0; k < 3; k++) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq; }
            for (int k = 0; k < 3; k++) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk; }
            for (int k = 0; k < 3; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq; }
        }
    }
    int m = 0;
    for (int k = 1; k < 3; k++) if (A[k][k] < A[m][m]) m = k;
    double v[3] = {V[0][m], V[1][m], V[2][m]};
    const double nv = ssfm::norm3(v);
    if (!(nv > 0.0) || !std::isfinite(nv)) return;
    for (int k = 0; k < 3; k++) up[k] = v[k] / nv;
    if (up[1] < 0) for (int k = 0; k < 3; k++) up[k] = -up[k];
}

void get_rotation(const double from[3], const double to[3], double R[9]) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    const double angle = std::acos(ssfm::dot3(from, to));
    if (std::fabs(angle) > 0) {
        double v[3]; ssfm::cross3(from, to, v);
        const double nv = ssfm::norm3(v);
        for (int k = 0; k < 3; k++) v[k] = v[k] / nv * angle;
        ssfm::so3exp(v, R);
    }
}

void level_keyframes(std::vector<Keyframe>& keyframes) {
    if (keyframes.empty()) return;
    double up[3]; plane_normal(keyframes, up);
    const double yaxis[3] = {0, 1, 0};
    double correction[9]; get_rotation(up, yaxis, correction);
    for (Keyframe& kf : keyframes) {                                    // rotate all cameras to correct the up vector: R <- R correction^T
        double Rn[9]; ssfm::mat3_mul_bt(kf.R, correction, Rn);
        std::memcpy(kf.R, Rn, sizeof Rn); ssfm::so3ln(kf.R, kf.r);
    }
    size_t nflip = 0;                                                   // upside-down?
    for (const Keyframe& kf : keyframes) if (kf.R[4] < 0) nflip++;
    if (nflip > keyframes.size() / 2) {
        const double Rflip[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
        for (Keyframe& kf : keyframes) { double Rn[9]; ssfm::mat3_mul(kf.R, Rflip, Rn); std::memcpy(kf.R, Rn, sizeof Rn); ssfm::so3ln(kf.R, kf.r); }
    }
    double min_dist = INFINITY;
    for (const Keyframe& kf : keyframes) { double c[3]; center_of(kf, c); const double d = ssfm::norm3(c); if (d < min_dist) min_dist = d; }
    for (Keyframe& kf : keyframes) for (int k = 0; k < 3; k++) kf.t[k] *= 1. / min_dist;
}

double compute_theta(const double c[3], const double up[3]) {
    const double cu = ssfm::dot3(c, up), x[3] = {1, 0, 0}, xu = ssfm::dot3(x, up);
    double cproj[3], xproj[3], cr[3];
    for (int k = 0; k < 3; k++) { cproj[k] = c[k] - up[k] * cu; xproj[k] = x[k] - up[k] * xu; }
    ssfm::cross3(xproj, cproj, cr);
    return std::atan2(ssfm::dot3(cr, up), ssfm::dot3(xproj, cproj)) + M_PI;
}

void compute_thetas(std::vector<Keyframe>& keyframes) {
    const double up[3] = {0, 1, 0};
    for (Keyframe& kf : keyframes) { double c[3]; center_of(kf, c); kf.theta = compute_theta(c, up); }
}

bool trim_loop(std::vector<Keyframe>& keyframes, bool is_loop) {
    if (keyframes.size() < 2) return false;
    int npos = 0, nneg = 0;
    for (int i = 0; i < 10; i++) {
        if (keyframes[1].theta < keyframes[0].theta) nneg++;
        else if (keyframes[0].theta < keyframes[1].theta) npos++;
    }
    const bool reverse = nneg > npos;
    if (is_loop) {
        if (reverse) { while (keyframes.back().theta < keyframes[0].theta) keyframes.pop_back(); }
        else { while (keyframes.back().theta > keyframes[0].theta) keyframes.pop_back(); }
    }
    return reverse;
}

// one header token of a PPM: skips white space and '#' comments
static bool ppm_int(FILE* f, int& v) {
    int ch = std::fgetc(f);
    while (ch != EOF) {
        if (ch == '#') { while (ch != EOF && ch != '\n') ch = std::fgetc(f); }
        else if (ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r') ch = std::fgetc(f);
        else break;
    }
    if (ch < '0' || ch > '9') return false;
    long long x = 0;
    while (ch >= '0' && ch <= '9') { x = x * 10 + (ch - '0'); if (x > 1 << 24) return false; ch = std::fgetc(f); }
    v = (int)x;                                                           // the character after the number (one white space before the pixels) is consumed
    return true;
}

bool read_ppm(const std::string& path, int& width, int& height, std::vector<uint8_t>& rgb) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    int maxval = 0; bool ok = std::fgetc(f) == 'P' && std::fgetc(f) == '6' && ppm_int(f, width) && ppm_int(f, height) && ppm_int(f, maxval);
    ok = ok && width > 0 && height > 0 && maxval == 255;
    if (ok) {
        rgb.resize((size_t)width * (size_t)height * 3);
        ok = std::fread(rgb.data(), 1, rgb.size(), f) == rgb.size();
    }
    std::fclose(f);
    return ok;
}

bool write_ppm(const std::string& path, int width, int height, const uint8_t* rgb) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t bytes = (size_t)width * (size_t)height * 3;
    bool ok = std::fprintf(f, "P6\n%d %d\n255\n", width, height) > 0 && std::fwrite(rgb, 1, bytes, f) == bytes;
    ok = (std::fclose(f) == 0) && ok;
    return ok;
}

bool read_flo(const std::string& path, int& width, int& height, std::vector<float>& uv) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    char tag[4]; int32_t wh[2] = {0, 0};
    bool ok = std::fread(tag, 1, 4, f) == 4 && std::memcmp(tag, "PIEH", 4) == 0 && std::fread(wh, 4, 2, f) == 2 && wh[0] > 0 && wh[1] > 0 && wh[0] <= 1 << 24 && wh[1] <= 1 << 24;
    if (ok) {
        width = wh[0]; height = wh[1];
        uv.resize((size_t)width * (size_t)height * 2);
        ok = std::fread(uv.data(), sizeof(float), uv.size(), f) == uv.size();
    }
    std::fclose(f);
    return ok;
}

bool write_flo(const std::string& path, int width, int height, const float* uv) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const int32_t wh[2] = {width, height}; const size_t count = (size_t)width * (size_t)height * 2;
    bool ok = std::fwrite("PIEH", 1, 4, f) == 4 && std::fwrite(wh, 4, 2, f) == 2 && std::fwrite(uv, sizeof(float), count, f) == count;
    ok = (std::fclose(f) == 0) && ok;
    return ok;
}

}  // namespace stereopanotools
