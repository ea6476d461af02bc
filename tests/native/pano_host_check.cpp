// Stand-alone check of spherical_sfm_amd/csrc/pano_host.h and of the host half of the stereo panorama mirror (csrc/shim/stereo_panorama_tools_host.cpp), built
// with -fsanitize=address,undefined by tests/test_pano_cpu.py (host code only, no device):
//   1. pano_plan: the `ok` shortcut (two end rows and an error bound) equals the all-rows rule written here, on level, tilted and re-oriented cameras; the owner of a
//      column is the ok job of the highest pair; one thread and several give the same plan; n = 0, 1, 2, pano_width = 2, height = 1; pano_check_params' refusals;
//   2. level_keyframes: cameras on a tilted circle of radius 3 come back with up = y, the smallest centre distance 1 and R still a rotation; an upside-down set is flipped;
//      plane_normal is an eigenvector of the scatter;
//   3. compute_thetas against atan2 of the centre; trim_loop's quirks (reverse from keyframes 0 and 1, end frames dropped only with is_loop, nothing reordered);
//   4. load_keyframes, PPM (with a comment in the header) and .flo round trips, and the refusal of truncated files.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include "../../spherical_sfm_amd/csrc/pano_host.h"
#include "../../spherical_sfm_amd/csrc/shim/stereo_panorama_tools_host.cpp"

using namespace ssfm;
using namespace stereopanotools;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static void yaw_pose(double a, double* R, double* t) {                  // looking outward from the unit circle
    const double c = std::cos(a), s = std::sin(a);
    const double M[9] = {c, 0, -s, 0, 1, 0, s, 0, c};
    std::memcpy(R, M, sizeof M); t[0] = 0; t[1] = 0; t[2] = -1;
}

static void make_circle(int n, std::mt19937& gen, double tilt, std::vector<double>& R, std::vector<double>& t) {
    std::normal_distribution<double> N(0.0, 1.0); std::uniform_real_distribution<double> U(-0.3, 0.3);
    R.assign(9 * (size_t)n, 0.0); t.assign(3 * (size_t)n, 0.0);
    for (int k = 0; k < n; k++) {
        double Y[9], T[9]; yaw_pose((k + U(gen)) * 2 * M_PI / n, Y, &t[3 * (size_t)k]);
        const double r[3] = {tilt * N(gen), 0, tilt * N(gen)}; ssfm::so3exp(r, T);
        ssfm::mat3_mul(T, Y, &R[9 * (size_t)k]);
        for (int i = 0; i < 3; i++) t[3 * (size_t)k + i] += 0.02 * N(gen);
    }
}

static bool all_rows_ok(const PanoJob& J, const double* R, const double* t, int n, double focal, double cy, int height, const PanoParams& P) {
    const PanoRowConsts c = pano_row_consts(J.tan_phi, J.synth_R, P.depth, P.synth_radius);
    const int l = J.pair, r = (J.pair + 1) % n;
    for (int y = 0; y < height; y++) {
        double w[3], XL[3], XR[3];
        pano_world(c, (double)y, cy, focal * P.synth_focal_factor, P.depth, w);
        pano_camera(R + 9 * (size_t)l, t + 3 * (size_t)l, w, XL); pano_camera(R + 9 * (size_t)r, t + 3 * (size_t)r, w, XR);
        if (XL[2] <= 0) return false;
        if (XR[2] <= 0) return false;
    }
    return true;
}

static void check_plan() {
    std::mt19937 gen(5);
    PanoParams P;
    long jobs = 0, not_ok = 0, overwrites = 0;
    for (int rep = 0; rep < 24; rep++) {
        const int cse = rep % 8;
        const int n = cse < 4 ? 7 : 12, pano_width = cse % 2 ? 130 : 193, height = cse == 3 ? 1 : 37;
        const double focal = cse == 6 ? 12.0 : 40.0, cy = 18.5;
        std::vector<double> R, t; make_circle(n, gen, cse >= 4 ? 0.6 : 0.05, R, t);
        if (cse == 2 || cse == 6) {                                      // one camera turned about its own centre
            double c[3], E[9], Rn[9]; ssfm::mat3_tvec(&R[27], &t[9], c);
            const double r[3] = {cse == 6 ? 1.1 : 0.0, cse == 2 ? 1.7 : 0.0, 0}; ssfm::so3exp(r, E);
            ssfm::mat3_mul(E, &R[27], Rn); std::memcpy(&R[27], Rn, sizeof Rn);
            double m[3]; ssfm::mat3_vec(&R[27], c, m); for (int i = 0; i < 3; i++) t[9 + i] = m[i];       // t = -R (-R^T t_old)
        }
        P.is_loop = cse == 1 ? 0 : 1; P.num_phi = cse == 5 ? 1 : 9;
        PanoPlan plan, plan4;
        pano_plan(P, n, R.data(), t.data(), focal, cy, height, pano_width, 1, plan);
        pano_plan(P, n, R.data(), t.data(), focal, cy, height, pano_width, 4, plan4);
        EXPECT(plan.jobs.size() == plan4.jobs.size() && plan.owner == plan4.owner && plan.owner_job == plan4.owner_job);
        EXPECT(plan.num_pairs == (P.is_loop ? n : n - 1));
        std::vector<int32_t> owner((size_t)P.num_phi * pano_width, -1);
        for (size_t j = 0; j < plan.jobs.size(); j++) {
            const PanoJob& J = plan.jobs[j];
            EXPECT(J.pair >= 0 && J.pair < plan.num_pairs && J.col >= 0 && J.col < pano_width && J.phi >= 0 && J.phi < P.num_phi && J.theta >= 0 && J.theta < pano_width);
            EXPECT(j == 0 || plan.jobs[j - 1].pair < J.pair || (plan.jobs[j - 1].pair == J.pair && (plan.jobs[j - 1].theta < J.theta || (plan.jobs[j - 1].theta == J.theta && plan.jobs[j - 1].phi < J.phi))));
            EXPECT(J.alpha > 0.0);
            const bool ok = all_rows_ok(J, R.data(), t.data(), n, focal, cy, height, P);
            EXPECT(ok == (J.ok != 0));
            jobs++; not_ok += ok ? 0 : 1;
            if (ok) { int32_t& o = owner[(size_t)J.phi * pano_width + J.col]; if (o >= 0) overwrites++; EXPECT(o <= J.pair); o = J.pair; }
            if (j < plan4.jobs.size()) EXPECT(std::memcmp(&plan4.jobs[j].alpha, &J.alpha, sizeof(double)) == 0 && plan4.jobs[j].col == J.col && plan4.jobs[j].ok == J.ok);
        }
        EXPECT(owner == plan.owner);
        for (size_t c = 0; c < owner.size(); c++) EXPECT((plan.owner_job[c] < 0) == (owner[c] < 0) && (owner[c] < 0 || plan.jobs[(size_t)plan.owner_job[c]].pair == owner[c]));
    }
    EXPECT(jobs > 5000 && not_ok > 0 && overwrites > 0);
    std::printf("plan: %ld jobs, %ld not ok, %ld overwrites\n", jobs, not_ok, overwrites);
    // degenerate sizes
    P = PanoParams();
    std::vector<double> R, t; make_circle(2, gen, 0.05, R, t);
    for (int n = 0; n <= 2; n++) for (int loop = 0; loop < 2; loop++) {
        PanoPlan plan; P.is_loop = loop;
        pano_plan(P, n, R.data(), t.data(), 40.0, 18.5, 37, n == 2 ? 2 : 64, 3, plan);
        EXPECT(plan.num_pairs == (n == 0 ? 0 : loop ? n : n - 1));
        if (n < 2) EXPECT(plan.jobs.empty());
        EXPECT(plan.owner.size() == (size_t)9 * (n == 2 ? 2 : 64));
    }
    P = PanoParams();
    EXPECT(pano_check_params(P, 2, R.data(), t.data(), 40.0, 48, 37, 193) == nullptr);
    EXPECT(pano_check_params(P, -1, R.data(), t.data(), 40.0, 48, 37, 193) != nullptr);
    EXPECT(pano_check_params(P, 2, nullptr, t.data(), 40.0, 48, 37, 193) != nullptr);
    EXPECT(pano_check_params(P, 2, R.data(), t.data(), 40.0, 48, 37, 1) != nullptr);
    EXPECT(pano_check_params(P, 2, R.data(), t.data(), 0.0, 48, 37, 193) != nullptr);
    EXPECT(pano_check_params(P, 2, R.data(), t.data(), 40.0, 0, 37, 193) != nullptr);
    P.num_phi = 0; EXPECT(pano_check_params(P, 2, R.data(), t.data(), 40.0, 48, 37, 193) != nullptr);
    P = PanoParams();
    EXPECT(pano_phi(P, 4) == 0.0 && pano_phi(P, 0) == -4.0 * M_PI / 180. && pano_phi(P, 8) == 4.0 * M_PI / 180.);
    P.num_phi = 1; EXPECT(pano_phi(P, 0) == 0.0);
}

static std::vector<Keyframe> tilted_circle(int n, const double* tilt_r, double radius, bool upside_down) {
    std::vector<Keyframe> kfs((size_t)n);
    double T[9]; ssfm::so3exp(tilt_r, T);
    for (int k = 0; k < n; k++) {
        double Y[9], t0[3]; yaw_pose(k * 2 * M_PI / n * 0.9, Y, t0);
        Keyframe& kf = kfs[(size_t)k];
        kf.index = 3 * k;
        if (upside_down) { const double F[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}; double Z[9]; ssfm::mat3_mul(Y, F, Z); std::memcpy(Y, Z, sizeof Z); }
        ssfm::mat3_mul_bt(Y, T, kf.R);                                   // world tilted by T: R = Y T^T, centre = T * (circle point)
        for (int i = 0; i < 3; i++) kf.t[i] = t0[i] * radius * (1.0 + 0.1 * (k % 3));
        ssfm::so3ln(kf.R, kf.r);
    }
    return kfs;
}

static void check_levelling() {
    const double tilt[3] = {0.3, 0.0, -0.2};
    for (int flip = 0; flip < 2; flip++) {
        std::vector<Keyframe> kfs = tilted_circle(11, tilt, 3.0, flip == 1);
        double up[3]; plane_normal(kfs, up);
        double T[9]; ssfm::so3exp(tilt, T);
        EXPECT(std::fabs(std::fabs(up[0] * T[1] + up[1] * T[4] + up[2] * T[7]) - 1.0) < 1e-12 && up[1] >= 0);       // the tilted y axis, up to sign
        level_keyframes(kfs);
        double dmin = INFINITY;
        for (const Keyframe& kf : kfs) {
            double c[3]; center_of(kf, c);
            EXPECT(std::fabs(c[1]) < 1e-12);                              // the centres lie in the plane y = 0
            dmin = std::min(dmin, ssfm::norm3(c));
            double I[9]; ssfm::mat3_mul_bt(kf.R, kf.R, I);
            for (int i = 0; i < 9; i++) EXPECT(std::fabs(I[i] - (i % 4 == 0 ? 1.0 : 0.0)) < 1e-12);
            EXPECT(kf.R[4] > 0.99);                                       // upright after the flip rule
            double R2[9]; ssfm::so3exp(kf.r, R2);
            for (int i = 0; i < 9; i++) EXPECT(std::fabs(R2[i] - kf.R[i]) < 1e-9);
        }
        EXPECT(std::fabs(dmin - 1.0) < 1e-12);
        compute_thetas(kfs);
        for (const Keyframe& kf : kfs) {
            double c[3]; center_of(kf, c);
            EXPECT(kf.theta >= 0 && kf.theta <= 2 * M_PI + 1e-12);
            const double up_y[3] = {0, 1, 0};
            EXPECT(kf.theta == compute_theta(c, up_y));
            EXPECT(std::fabs(std::remainder(kf.theta - M_PI - std::atan2(-c[2], c[0]), 2 * M_PI)) < 1e-12);
        }
    }
    std::vector<Keyframe> none; level_keyframes(none); compute_thetas(none); EXPECT(!trim_loop(none, true));
    double R[9]; const double a[3] = {0, 1, 0}, b[3] = {1, 0, 0};
    get_rotation(a, a, R); for (int i = 0; i < 9; i++) EXPECT(R[i] == (i % 4 == 0 ? 1.0 : 0.0));
    get_rotation(a, b, R); double m[3]; ssfm::mat3_vec(R, a, m); EXPECT(std::fabs(m[0] - 1) < 1e-15 && std::fabs(m[1]) < 1e-15 && std::fabs(m[2]) < 1e-15);
}

static void check_trim() {
    auto make = [](std::initializer_list<double> th) { std::vector<Keyframe> k; int i = 0; for (double x : th) { Keyframe f; f.index = i++; f.theta = x; k.push_back(f); } return k; };
    std::vector<Keyframe> k = make({1.0, 2.0, 3.0, 6.0, 0.5, 0.9, 1.5, 1.2});
    EXPECT(!trim_loop(k, true) && k.size() == 6 && k.back().theta == 0.9);             // ascending: the end frames above theta_0 go
    k = make({1.0, 2.0, 3.0, 6.0, 0.5, 1.5});
    EXPECT(!trim_loop(k, false) && k.size() == 6);                                      // an open sweep is left alone
    k = make({5.0, 4.0, 3.0, 0.2, 6.0, 5.5, 4.9});
    EXPECT(trim_loop(k, true) && k.size() == 6 && k.back().theta == 5.5);               // descending: reverse, the end frames below theta_0 go, nothing is reordered
    EXPECT(k[0].index == 0 && k[3].index == 3);
    k = make({2.0, 2.0, 9.0});
    EXPECT(!trim_loop(k, true) && k.size() == 2);                                        // equal thetas: neither count moves, reverse = false
    k = make({1.0, 5.0, 7.0});
    EXPECT(!trim_loop(k, true) && k.size() == 1);                                        // everything beyond theta_0 goes; the first keyframe stops the loop
    k = make({1.0});
    EXPECT(!trim_loop(k, true) && k.size() == 1);
}

static void check_files(const std::string& dir) {
    const std::string poses = dir + "/poses.txt";
    { FILE* f = std::fopen(poses.c_str(), "w"); EXPECT(f != nullptr); std::fprintf(f, "0 0 0 -1 0 0.5 0\n7 0.1 0.2 -1.5 0.01 -0.7 0.02\n9 1 2\n"); std::fclose(f); }
    std::vector<Keyframe> kfs;
    EXPECT(load_keyframes(poses, kfs) && kfs.size() == 2 && kfs[1].index == 7 && kfs[1].t[2] == -1.5 && kfs[1].r[1] == -0.7);
    double R[9]; const double r[3] = {0.01, -0.7, 0.02}; ssfm::so3exp(r, R);
    EXPECT(std::memcmp(R, kfs[1].R, sizeof R) == 0);
    EXPECT(!load_keyframes(dir + "/missing.txt", kfs) && kfs.size() == 2);
    std::mt19937 gen(3);
    for (int cse = 0; cse < 3; cse++) {
        const int w = cse == 0 ? 1 : 13, h = cse == 1 ? 1 : 7;
        std::vector<uint8_t> img((size_t)w * h * 3), back; for (auto& b : img) b = (uint8_t)(gen() & 255);
        if (cse == 2) img[0] = '\n';                                      // pixel bytes that look like white space are not skipped
        const std::string p = dir + "/a.ppm";
        int w2 = 0, h2 = 0;
        EXPECT(write_ppm(p, w, h, img.data()) && read_ppm(p, w2, h2, back) && w2 == w && h2 == h && back == img);
        std::vector<float> uv((size_t)w * h * 2), uv2; for (auto& v : uv) v = (float)(int)(gen() % 2001 - 1000) / 8.f;
        uv[0] = NAN; if (uv.size() > 1) uv[1] = INFINITY;
        const std::string q = dir + "/a.flo";
        EXPECT(write_flo(q, w, h, uv.data()) && read_flo(q, w2, h2, uv2) && w2 == w && h2 == h && uv2.size() == uv.size() &&
               std::memcmp(uv.data(), uv2.data(), uv.size() * sizeof(float)) == 0);
    }
    { FILE* f = std::fopen((dir + "/c.ppm").c_str(), "wb"); std::fprintf(f, "P6\n# a comment\n2 # another\n1\n255\n"); const uint8_t px[6] = {1, 2, 3, 4, 5, 6}; std::fwrite(px, 1, 6, f); std::fclose(f); }
    int w = 0, h = 0; std::vector<uint8_t> img;
    EXPECT(read_ppm(dir + "/c.ppm", w, h, img) && w == 2 && h == 1 && img.size() == 6 && img[5] == 6);
    { FILE* f = std::fopen((dir + "/t.ppm").c_str(), "wb"); std::fprintf(f, "P6\n4 4\n255\n"); std::fwrite("abc", 1, 3, f); std::fclose(f); }
    EXPECT(!read_ppm(dir + "/t.ppm", w, h, img));                          // truncated
    { FILE* f = std::fopen((dir + "/m.ppm").c_str(), "wb"); std::fprintf(f, "P6\n1 1\n65535\n"); std::fwrite("abcdef", 1, 6, f); std::fclose(f); }
    EXPECT(!read_ppm(dir + "/m.ppm", w, h, img));                          // 16-bit samples are not read
    { FILE* f = std::fopen((dir + "/t.flo").c_str(), "wb"); const int32_t wh[2] = {4, 4}; std::fwrite("PIEH", 1, 4, f); std::fwrite(wh, 4, 2, f); std::fwrite(wh, 4, 2, f); std::fclose(f); }
    std::vector<float> uv;
    EXPECT(!read_flo(dir + "/t.flo", w, h, uv));
    { FILE* f = std::fopen((dir + "/b.flo").c_str(), "wb"); const int32_t wh[2] = {1, 1}; std::fwrite("PIEX", 1, 4, f); std::fwrite(wh, 4, 2, f); std::fwrite(wh, 4, 2, f); std::fclose(f); }
    EXPECT(!read_flo(dir + "/b.flo", w, h, uv) && !read_flo(dir + "/missing.flo", w, h, uv) && !read_ppm(dir + "/missing.ppm", w, h, img));
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: pano_host_check <scratch directory>\n"); return 2; }
    check_plan();
    check_levelling();
    check_trim();
    check_files(argv[1]);
    if (g_fail) { std::printf("PANO_HOST_CHECK failed: %d\n", g_fail); return 1; }
    std::printf("PANO_HOST_CHECK ok\n");
    return 0;
}
