// Stand-alone check of spherical_sfm_amd/csrc/anms_host.h, built with -fsanitize=address,undefined by tests/test_anms_cpu.py (host code only, no device):
//   1. the work list of anms_plan covers every (i, j) of every active frame exactly once, at chunk counts 1 .. 7 and the planner's own, at sizes around the block
//      and tile edges; items of a cut frame are marked split, items of an uncut one are not; frames returned unchanged get no item;
//   2. anms_batch_host equals a literal loop written here (std::stable_sort of keypoint structs, the prefix loop with its early exit, a full sort of the
//      radii) and the sort-free set form, keep lists and radii bit for bit, on random, heavily tied and signed input, for 1 and 3 threads;
//   3. anms_check's refusals and their order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "../../spherical_sfm_amd/csrc/anms_host.h"

using namespace ssfm;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct KP { float x, y, response; int index; };

// examples/spherical_sfm_tools.cpp:76-123 with a stable sort; n == numToKeep returns everything (the reference reads past the array there)
static void literal(std::vector<KP>& kps, int numToKeep, std::vector<double>& radius_in) {
    const int n = (int)kps.size();
    radius_in.assign((size_t)n, DBL_MAX);
    if (n < numToKeep) return;
    std::stable_sort(kps.begin(), kps.end(), [](const KP& a, const KP& b) { return a.response > b.response; });
    std::vector<double> radii((size_t)n), sorted((size_t)n);
    const float robustCoeff = 1.11f;
    for (int i = 0; i < n; ++i) {
        const float response = kps[(size_t)i].response * robustCoeff;
        double radius = DBL_MAX;
        for (int j = 0; j < i && kps[(size_t)j].response > response; ++j) {
            const float dx = kps[(size_t)i].x - kps[(size_t)j].x, dy = kps[(size_t)i].y - kps[(size_t)j].y;
            radius = std::min(radius, std::sqrt((double)dx * dx + (double)dy * dy));
        }
        radii[(size_t)i] = sorted[(size_t)i] = radius;
        radius_in[(size_t)kps[(size_t)i].index] = radius;
    }
    std::sort(sorted.begin(), sorted.end(), [](double a, double b) { return a > b; });
    const double decision = numToKeep < n ? sorted[(size_t)numToKeep] : 0.0;
    std::vector<KP> out;
    for (int i = 0; i < n; ++i)
        if (radii[(size_t)i] >= decision) out.push_back(kps[(size_t)i]);
    out.swap(kps);
}

static void set_form(int n, const float* xy, const float* r, int keep, std::vector<int>& kept, std::vector<double>& radius) {
    radius.assign((size_t)n, DBL_MAX); kept.clear();
    if (n < keep) { for (int i = 0; i < n; i++) kept.push_back(i); return; }
    std::vector<int> rank((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        const float thr = r[i] * 1.11f;
        double d2 = INFINITY;
        for (int j = 0; j < n; j++) {
            const bool pre = r[j] > r[i] || (r[j] == r[i] && j < i);
            rank[(size_t)i] += pre;
            if (pre && r[j] > thr) {
                const float dx = xy[2 * i] - xy[2 * j], dy = xy[2 * i + 1] - xy[2 * j + 1];
                const double d = (double)dx * dx + (double)dy * dy;
                if (d < d2) d2 = d;
            }
        }
        if (d2 < INFINITY) radius[(size_t)i] = std::sqrt(d2);
    }
    std::vector<double> s(radius);
    std::sort(s.begin(), s.end(), [](double a, double b) { return a > b; });
    const double decision = keep < n ? s[(size_t)keep] : 0.0;
    std::vector<int> slot((size_t)n, -1);
    for (int i = 0; i < n; i++) { EXPECT(rank[(size_t)i] >= 0 && rank[(size_t)i] < n && slot[(size_t)rank[(size_t)i]] == -1); slot[(size_t)rank[(size_t)i]] = radius[(size_t)i] >= decision ? i : -2; }
    for (int p = 0; p < n; p++) if (slot[(size_t)p] >= 0) kept.push_back(slot[(size_t)p]);
}

static void check_plan(const std::vector<int32_t>& sizes, const std::vector<int32_t>& keep, int32_t force, int32_t num_cus) {
    const int32_t F = (int32_t)sizes.size();
    std::vector<int32_t> ptr((size_t)F + 1, 0);
    for (int32_t f = 0; f < F; f++) ptr[(size_t)f + 1] = ptr[(size_t)f] + sizes[(size_t)f];
    std::vector<AnmsItem> items;
    const int64_t split = anms_plan(F, ptr.data(), keep.data(), force, num_cus, items);
    int64_t seen_split = 0;
    for (int32_t f = 0; f < F; f++) {
        const int32_t n = sizes[(size_t)f];
        std::vector<uint8_t> cover((size_t)n * (size_t)n, 0);
        int chunks_of_block0 = 0;
        for (const AnmsItem& it : items) {
            if (it.kp0 != ptr[(size_t)f] || it.n != n || n == 0) continue;       // (empty frames share kp0 with a neighbour: they have no items, checked below)
            EXPECT(anms_frame_active(n, keep[(size_t)f]));
            EXPECT(it.i0 >= 0 && it.i0 < n && it.i0 % kAnmsBlock == 0 && it.j_lo >= 0 && it.j_lo < it.j_hi && it.j_hi <= n);
            if (it.i0 == 0) chunks_of_block0++;
            for (int32_t i = it.i0; i < std::min(n, it.i0 + kAnmsBlock); i++)
                for (int32_t j = it.j_lo; j < it.j_hi; j++) cover[(size_t)i * (size_t)n + (size_t)j]++;
            seen_split += it.split;
        }
        if (anms_frame_active(n, keep[(size_t)f])) {
            bool once = true;
            for (uint8_t c : cover) once = once && c == 1;
            EXPECT(once);
            for (const AnmsItem& it : items)
                if (it.kp0 == ptr[(size_t)f] && it.n == n) EXPECT((it.split != 0) == (chunks_of_block0 > 1));
            if (force > 0) EXPECT(chunks_of_block0 == std::min(force, (n + (n + force - 1) / force - 1) / ((n + force - 1) / force)));
            else
                for (const AnmsItem& it : items)                                 // the planner's own cut: every chunk but a frame's last is at least the minimum
                    if (it.kp0 == ptr[(size_t)f] && it.n == n && it.j_hi < n) EXPECT(it.j_hi - it.j_lo >= kAnmsMinChunk);
        } else {
            for (const AnmsItem& it : items) EXPECT(!(it.kp0 == ptr[(size_t)f] && it.n == n && n > 0));
        }
    }
    EXPECT(seen_split == split);
}

static void check_frames(const std::vector<std::vector<float>>& xy, const std::vector<std::vector<float>>& resp, const std::vector<int32_t>& keep) {
    const int32_t F = (int32_t)xy.size();
    std::vector<int32_t> ptr((size_t)F + 1, 0);
    std::vector<float> fxy, fr;
    for (int32_t f = 0; f < F; f++) {
        ptr[(size_t)f + 1] = ptr[(size_t)f] + (int32_t)resp[(size_t)f].size();
        fxy.insert(fxy.end(), xy[(size_t)f].begin(), xy[(size_t)f].end()); fr.insert(fr.end(), resp[(size_t)f].begin(), resp[(size_t)f].end());
    }
    const int32_t total = ptr[(size_t)F];
    for (int threads : {1, 3}) {
        std::vector<int32_t> kptr((size_t)F + 1, -1), kidx((size_t)std::max(total, 1), -1);
        std::vector<double> rad((size_t)std::max(total, 1), -1.0);
        EXPECT(anms_check(F, ptr.data(), fxy.data(), fr.data(), keep.data(), nullptr, kptr.data(), kidx.data()) == nullptr);
        anms_batch_host(F, ptr.data(), fxy.data(), fr.data(), keep.data(), threads, kptr.data(), kidx.data(), threads == 1 ? rad.data() : nullptr);
        EXPECT(kptr[0] == 0);
        for (int32_t f = 0; f < F; f++) {
            const int32_t n = ptr[(size_t)f + 1] - ptr[(size_t)f];
            std::vector<KP> kps((size_t)n);
            for (int32_t i = 0; i < n; i++) kps[(size_t)i] = KP{xy[(size_t)f][2 * (size_t)i], xy[(size_t)f][2 * (size_t)i + 1], resp[(size_t)f][(size_t)i], i};
            std::vector<double> r_lit, r_set; std::vector<int> k_set;
            literal(kps, keep[(size_t)f], r_lit);
            set_form(n, xy[(size_t)f].data(), resp[(size_t)f].data(), keep[(size_t)f], k_set, r_set);
            const int32_t got = kptr[(size_t)f + 1] - kptr[(size_t)f];
            EXPECT(got == (int32_t)kps.size() && got == (int32_t)k_set.size());
            if (n >= keep[(size_t)f] && n > 0) EXPECT(got >= std::min(n, keep[(size_t)f] + 1));
            for (int32_t q = 0; q < got && q < (int32_t)kps.size(); q++) {
                EXPECT(kidx[(size_t)kptr[(size_t)f] + (size_t)q] == kps[(size_t)q].index);
                EXPECT(kidx[(size_t)kptr[(size_t)f] + (size_t)q] == k_set[(size_t)q]);
            }
            if (threads == 1)
                for (int32_t i = 0; i < n; i++) {
                    EXPECT(std::memcmp(&rad[(size_t)ptr[(size_t)f] + (size_t)i], &r_lit[(size_t)i], sizeof(double)) == 0);
                    EXPECT(std::memcmp(&r_set[(size_t)i], &r_lit[(size_t)i], sizeof(double)) == 0);
                }
        }
    }
}

int main() {
    // 1. the planner
    const std::vector<int32_t> sizes = {0, 1, 5, 255, 256, 257, 300, 511, 513, 64, 700};
    for (int32_t force = 0; force <= 7; force++)
        for (int32_t cus : {1, 256}) {
            std::vector<int32_t> keep(sizes.size(), 3);
            keep[2] = 6 /* below its target: no item */; keep[6] = 300 /* equal to it: active */;
            check_plan(sizes, keep, force, cus);
        }
    check_plan({1023}, {10}, 0, 256); check_plan({1024}, {10}, 0, 256); check_plan({1025}, {10}, 0, 256); check_plan({1025}, {10}, 3, 256);
    {   // a single large frame is cut, many large frames are not
        std::vector<AnmsItem> items;
        const int32_t p1[2] = {0, 20000}, k1[1] = {4000};
        EXPECT(anms_plan(1, p1, k1, 0, 256, items) == (int64_t)items.size() && items.size() >= 1024 && items[0].j_hi - items[0].j_lo >= kAnmsMinChunk);
        std::vector<int32_t> p300(301), k300(300, 4000);
        for (int f = 0; f <= 300; f++) p300[(size_t)f] = 20000 * f;
        EXPECT(anms_plan(300, p300.data(), k300.data(), 0, 256, items) == 0 && items.size() == (size_t)300 * 79);
    }
    // 2. the host implementation
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    {
        std::vector<std::vector<float>> xy, resp; std::vector<int32_t> keep;
        for (int32_t n : {0, 1, 5, 300, 257, 600, 64}) {
            std::vector<float> a((size_t)2 * n), r((size_t)n);
            for (int32_t i = 0; i < n; i++) { a[2 * (size_t)i] = 1920.f * U(rng); a[2 * (size_t)i + 1] = 1080.f * U(rng); const float u = U(rng); r[(size_t)i] = u * u * u * 0.1f; }
            xy.push_back(a); resp.push_back(r);
        }
        keep = {0, 1, 9, 75, 257, 599, 0};
        check_frames(xy, resp, keep);
        keep = {3, 0, 5, 0, 1, 601, 63};
        check_frames(xy, resp, keep);
    }
    {   // integer grid, responses k/64, duplicated points; and signed responses k/8
        std::vector<std::vector<float>> xy, resp;
        for (int kind = 0; kind < 2; kind++) {
            const int32_t n = 257;
            std::vector<float> a((size_t)2 * n), r((size_t)n);
            for (int32_t i = 0; i < n; i++) {
                a[2 * (size_t)i] = (float)(rng() % 40); a[2 * (size_t)i + 1] = (float)(rng() % 30);
                r[(size_t)i] = kind == 0 ? (float)(rng() % 64) / 64.f : ((float)(rng() % 13) - 6.f) / 8.f;
            }
            for (int32_t i = 0; i < 8; i++) { a[2 * (size_t)(n - 1 - i)] = a[2 * (size_t)i]; a[2 * (size_t)(n - 1 - i) + 1] = a[2 * (size_t)i + 1]; }
            xy.push_back(a); resp.push_back(r);
        }
        check_frames(xy, resp, {64, 64});
        check_frames(xy, resp, {256, 0});
    }
    // 3. refusals, in order
    {
        int32_t ptr[3] = {0, 2, 3}, keep[2] = {1, 1}, kptr[3], kidx[3];
        float xy[6] = {0, 0, 1, 1, 2, 2}, r[3] = {1.f, 2.f, 3.f};
        ssfm_anms_options o{0, 0};
        EXPECT(anms_check(2, ptr, xy, r, keep, &o, kptr, kidx) == nullptr);
        EXPECT(anms_check(0, ptr, nullptr, nullptr, nullptr, nullptr, kptr, nullptr) == nullptr);
        EXPECT(std::strcmp(anms_check(-1, ptr, xy, r, keep, &o, kptr, kidx), "bad arguments") == 0);
        EXPECT(std::strcmp(anms_check(2, ptr, nullptr, r, keep, &o, kptr, kidx), "bad arguments") == 0);
        o.force_j_chunks = -1; EXPECT(std::strcmp(anms_check(2, ptr, xy, r, keep, &o, kptr, kidx), "bad options") == 0); o.force_j_chunks = 0;
        int32_t bad[3] = {0, 3, 2}; keep[0] = -1; r[0] = NAN;
        EXPECT(std::strcmp(anms_check(2, bad, xy, r, keep, &o, kptr, kidx), "kp_ptr is not ascending") == 0);
        int32_t off[3] = {1, 2, 3};
        EXPECT(std::strcmp(anms_check(2, off, xy, r, keep, &o, kptr, kidx), "kp_ptr does not start at 0") == 0);
        EXPECT(std::strcmp(anms_check(2, ptr, xy, r, keep, &o, kptr, kidx), "num_to_keep is negative") == 0); keep[0] = 1;
        EXPECT(std::strcmp(anms_check(2, ptr, xy, r, keep, &o, kptr, kidx), "NaN response") == 0);
    }
    if (g_fail) { std::printf("ANMS_HOST_CHECK failed: %d\n", g_fail); return 1; }
    std::printf("ANMS_HOST_CHECK ok\n");
    return 0;
}
