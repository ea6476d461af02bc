// Stand-alone check of the host side of ssfm_rot_l1_init (spherical_sfm_amd/csrc/rot_l1_host.h: the argument checks, the reach set, the node-major adjacency the
// kernels walk) on the shapes of the tests' fixtures and on random multigraphs, and of the mirror's host half (csrc/shim/tools_host.cpp:
// filter_image_matches_by_residual, find_largest_connected_component with rotations).  No GPU code, no library: built with -fsanitize=address,undefined by
// tests/test_rot_l1_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "../../spherical_sfm_amd/csrc/rot_l1_host.h"
#include "../../spherical_sfm_amd/csrc/shim/tools.h"

using namespace ssfm;

#define CHECK(c) do { if (!(c)) { std::printf("ROT_L1_HOST_CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

typedef std::vector<int32_t> Vi;

static void check_graph(int n, const Vi& i0, const Vi& i1, int root) {
    const int E = (int)i0.size();
    RotL1Graph G;
    CHECK(rot_l1_graph(n, E, i0.data(), i1.data(), root, G));
    // the reach set by brute force: grow until nothing changes
    std::vector<int> reach(n, 0); reach[root] = 1;
    for (bool grew = true; grew;) {
        grew = false;
        for (int e = 0; e < E; e++)
            if (reach[i0[e]] != reach[i1[e]]) { reach[i0[e]] = reach[i1[e]] = 1; grew = true; }
    }
    int nr = 0, used = 0;
    for (int v = 0; v < n; v++) { nr += reach[v]; CHECK(G.reached[v] == reach[v] && G.free_node[v] == (reach[v] && v != root ? 1 : 0)); }
    CHECK(G.num_reached == nr && G.num_free == nr - 1);
    CHECK((int)G.adj_ptr.size() == n + 1 && G.adj_ptr[0] == 0);
    std::vector<int> seen_side((size_t)2 * E, 0);
    for (int e = 0; e < E; e++) used += (i0[e] != i1[e] && reach[i0[e]] && reach[i1[e]]);
    CHECK(G.num_edges_used == used && G.adj_ptr[n] == 2 * used && (int)G.adj_nb.size() == 2 * used && (int)G.adj_es.size() == 2 * used);
    for (int v = 0; v < n; v++) {
        CHECK(G.adj_ptr[v] <= G.adj_ptr[v + 1]);
        if (!reach[v]) CHECK(G.adj_ptr[v] == G.adj_ptr[v + 1]);
        if (G.free_node[v]) CHECK(G.adj_ptr[v] < G.adj_ptr[v + 1]);                 // a free node has the edge to its tree parent: L_ii > 0
        for (int k = G.adj_ptr[v]; k < G.adj_ptr[v + 1]; k++) {
            const int e = (int)(G.adj_es[k] >> 1), side = (int)(G.adj_es[k] & 1u), nb = G.adj_nb[k];
            CHECK(e >= 0 && e < E && nb >= 0 && nb < n && nb != v && reach[nb]);
            CHECK(side ? (i1[e] == v && i0[e] == nb) : (i0[e] == v && i1[e] == nb));
            CHECK(!seen_side[(size_t)2 * e + side]++);
            if (k > G.adj_ptr[v]) {
                const int pe = (int)(G.adj_es[k - 1] >> 1), pnb = G.adj_nb[k - 1];
                CHECK(pnb < nb || (pnb == nb && pe < e));                             // (neighbour, edge id), strictly
            }
        }
    }
    for (int e = 0; e < E; e++) {
        const int want = (i0[e] != i1[e] && reach[i0[e]] && reach[i1[e]]) ? 1 : 0;
        CHECK(seen_side[(size_t)2 * e] == want && seen_side[(size_t)2 * e + 1] == want);
    }
    // the tree the start is chained along covers the reach set
    CHECK(G.t_node[0] == root);
    for (int k = 1; k < nr; k++) CHECK(reach[G.t_node[k]] && G.t_edge[k] >= 0 && G.t_edge[k] < E);
}

static void ring(int n, const std::vector<int>& offsets, std::mt19937& g, Vi& i0, Vi& i1) {
    i0.clear(); i1.clear();
    for (int d : offsets) for (int i = 0; i < n; i++) { int a = i, b = (i + d) % n; if (g() & 1u) std::swap(a, b); i0.push_back(a); i1.push_back(b); }
    for (size_t k = i0.size(); k > 1; k--) { const size_t j = g() % k; std::swap(i0[k - 1], i0[j]); std::swap(i1[k - 1], i1[j]); }
}

static void check_refusals() {
    const int32_t i0[2] = {0, 1}, i1[2] = {1, 2}, bad1[2] = {1, 3}, neg[2] = {0, -1};
    const double rel[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    double out[27]; ssfm_rot_l1_summary s;
    ssfm_rot_l1_options o = {30, 1e-4, 1e-3, 1e-10, 0};
    CHECK(rot_l1_check(3, 2, i0, i1, rel, 0, &o, out, &s) == nullptr);
    CHECK(rot_l1_check(3, 2, i0, i1, rel, 0, nullptr, out, &s) == nullptr);
    CHECK(rot_l1_check(3, 0, nullptr, nullptr, nullptr, 2, nullptr, out, &s) == nullptr);
    auto is = [](const char* got, const char* want) { return got && std::strcmp(got, want) == 0; };
    CHECK(is(rot_l1_check(3, 2, i0, bad1, rel, 0, &o, out, &s), "camera index out of range"));
    CHECK(is(rot_l1_check(3, 2, i0, neg, rel, 0, &o, out, &s), "camera index out of range"));
    CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 3, &o, out, &s), "root out of range"));
    CHECK(is(rot_l1_check(3, 2, i0, i1, rel, -1, &o, out, &s), "root out of range"));
    CHECK(is(rot_l1_check(0, 0, nullptr, nullptr, nullptr, 0, &o, out, &s), "root out of range"));
    CHECK(is(rot_l1_check(3, 2, nullptr, i1, rel, 0, &o, out, &s), "bad arguments"));
    CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &o, nullptr, &s), "bad arguments"));
    CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &o, out, nullptr), "bad arguments"));
    CHECK(is(rot_l1_check(-1, 0, nullptr, nullptr, nullptr, 0, &o, out, &s), "bad arguments"));
    ssfm_rot_l1_options b = o; b.max_iterations = 0; CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s), "bad options"));
    b = o; b.weight_floor = 0.0; CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s), "bad options"));
    b = o; b.pcg_tolerance = -1.0; CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s), "bad options"));
    b = o; b.step_tolerance = -1e-9; CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s), "bad options"));
    b = o; b.pcg_max_iterations = -2; CHECK(is(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s), "bad options"));
    b = o; b.step_tolerance = 0.0; CHECK(rot_l1_check(3, 2, i0, i1, rel, 0, &b, out, &s) == nullptr);
    // options are looked at before the indices, the indices before the root
    b = o; b.max_iterations = -1; CHECK(is(rot_l1_check(3, 2, i0, bad1, rel, 7, &b, out, &s), "bad options"));
    CHECK(is(rot_l1_check(3, 2, i0, bad1, rel, 7, &o, out, &s), "camera index out of range"));
    RotL1Graph G;
    CHECK(!rot_l1_graph(3, 2, i0, bad1, 0, G) && !rot_l1_graph(3, 2, i0, i1, 3, G) && !rot_l1_graph(0, 0, nullptr, nullptr, 0, G));
}

// the mirror: the residual cut, then the component step that carries the rotations along and re-gauges them to the new camera 0
static void check_mirror() {
    using namespace sphericalsfm;
    const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<Keyframe> kf; std::vector<ImageMatch> ms; std::vector<Mat3> rot;
    for (int i = 0; i < 7; i++) {
        kf.push_back(Keyframe(100 + i, "f", Features()));
        const double r[3] = {0.0, 0.3 * i, 0.1 * i}; double R[9]; so3exp(r, R);
        Mat3 M; rm_to_cm(R, M.data()); rot.push_back(M);
    }
    // cameras 0-1 form a small component, 2-5 the largest one, 6 has no match; residuals: one above the cut, one unused (-1)
    const int pairs[][2] = {{0, 1}, {2, 3}, {3, 4}, {5, 4}, {2, 5}, {1, 2}, {3, 3}};
    const double res[] = {0.001, 0.002, 0.0, 0.01, 0.03, 0.5, -1.0};
    for (auto& p : pairs) ms.push_back(ImageMatch(p[0], p[1], Matches(), I));
    std::vector<double> residuals(res, res + 7);
    std::vector<ImageMatch> kept = filter_image_matches_by_residual(ms, residuals, 0.03);
    CHECK(kept.size() == 5 && kept[0].index0 == 0 && kept[4].index0 == 2 && kept[4].index1 == 5);          // <= thresh stays, (1, 2) and the unused loop go
    CHECK(filter_image_matches_by_residual(ms, std::vector<double>(3, 0.0), 1.0).size() == 3);              // a short residual list cuts the rest
    const std::vector<Mat3> before = rot;
    find_largest_connected_component(kf, kept, rot);
    CHECK(kf.size() == 4 && rot.size() == 4 && kept.size() == 4);
    for (int k = 0; k < 4; k++) CHECK(kf[k].index == 102 + k);                                             // the frame numbers are back
    CHECK(kept[0].index0 == 0 && kept[0].index1 == 1 && kept[2].index0 == 3 && kept[2].index1 == 2);       // renumbered
    for (int q = 0; q < 9; q++) CHECK(std::fabs(rot[0][q] - I[q]) < 1e-15);
    for (int k = 0; k < 4; k++) {                                                                          // R_k R_0^T is what it was
        double A[9], B[9], W[9], D[9], v[3];
        cm_to_rm(before[2 + k].data(), A); cm_to_rm(before[2].data(), B); mat3_mul_bt(A, B, W);
        cm_to_rm(rot[k].data(), A); mat3_mul_bt(A, W, D); so3ln(D, v);
        CHECK(norm3(v) < 1e-14);
    }
    // nothing left: everything is dropped, nothing is read out of range
    std::vector<ImageMatch> none; std::vector<Mat3> r2 = before; std::vector<Keyframe> k2; for (int i = 0; i < 3; i++) k2.push_back(Keyframe(i, "f", Features()));
    find_largest_connected_component(k2, none, r2);
    CHECK(k2.empty() && r2.empty());
}

int main() {
    std::mt19937 g(17);
    Vi i0, i1;
    check_refusals();
    check_mirror();
    // the fixtures' shapes: shuffled rings of 60 and 350, the complete graph of 24, a chain, two components and a camera without an edge
    ring(60, {1, 2, 3, 5, 9}, g, i0, i1); check_graph(60, i0, i1, 0); check_graph(60, i0, i1, 59);
    ring(350, {1, 2, 3, 5, 9}, g, i0, i1); check_graph(350, i0, i1, 0);
    i0.clear(); i1.clear();
    for (int a = 0; a < 24; a++) for (int b = a + 1; b < 24; b++) { i0.push_back(a); i1.push_back(b); }
    check_graph(24, i0, i1, 0); check_graph(24, i0, i1, 11);
    i0.clear(); i1.clear();
    for (int k = 0; k + 1 < 40; k++) { if (k % 3 == 0) { i0.push_back(k + 1); i1.push_back(k); } else { i0.push_back(k); i1.push_back(k + 1); } }
    check_graph(40, i0, i1, 0); check_graph(40, i0, i1, 20);
    i0.clear(); i1.clear();
    for (int d = 1; d <= 3; d++) for (int i = 0; i < 30; i++) { i0.push_back(i); i1.push_back((i + d) % 30); if (i < 20 && d < 3) { i0.push_back(30 + i); i1.push_back(30 + (i + d) % 20); } }
    check_graph(51, i0, i1, 0); check_graph(51, i0, i1, 35); check_graph(51, i0, i1, 50);
    // degree 70 (more than one wave), duplicates, a self loop, edges stored as (b, a), a camera without an edge
    i0.clear(); i1.clear();
    for (int c = 1; c <= 70; c++) { i0.push_back(0); i1.push_back(c); }
    for (int c = 1; c < 70; c += 3) { i0.push_back(c); i1.push_back(c + 1); }
    const int extra[][2] = {{75, 0}, {75, 3}, {75, 79}, {76, 0}, {0, 5}, {0, 5}, {5, 0}, {7, 7}, {9, 2}, {30, 0}, {0, 0}};
    for (auto& p : extra) { i0.push_back(p[0]); i1.push_back(p[1]); }
    check_graph(80, i0, i1, 0); check_graph(80, i0, i1, 75); check_graph(80, i0, i1, 78); check_graph(80, i0, i1, 7);
    // no edges at all
    check_graph(5, Vi(), Vi(), 3);
    // random multigraphs
    for (int t = 0; t < 200; t++) {
        const int n = 1 + (int)(g() % 30), E = (int)(g() % (3 * n + 1)), span = (t % 3) ? n : std::max(1, n / 2);
        i0.assign(E, 0); i1.assign(E, 0);
        for (int e = 0; e < E; e++) { i0[e] = (int)(g() % span); i1[e] = (int)(g() % span); }
        if (E > 4) { i0[1] = i0[0]; i1[1] = i1[0]; i1[2] = i0[2]; i0[3] = i1[0]; i1[3] = i0[0]; }
        check_graph(n, i0, i1, (int)(g() % n));
    }
    std::printf("ROT_L1_HOST_CHECK ok\n");
    return 0;
}
