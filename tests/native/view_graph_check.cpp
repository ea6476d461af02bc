// Stand-alone check of the host side of the view-graph calls (spherical_sfm_amd/csrc/view_graph_host.h: the CSR sort, the spanning tree, the join the kernels run)
// and of the mirror's bookkeeping (csrc/shim/tools_host.cpp: apply_triplet_filter) on adversarial lists.  No GPU code, no library: built with
// -fsanitize=address,undefined by tests/test_view_graph_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <set>
#include <string>
#include "../../spherical_sfm_amd/csrc/shim/tools.h"
#include "../../spherical_sfm_amd/csrc/view_graph_host.h"

using namespace ssfm;

#define CHECK(c) do { if (!(c)) { std::printf("VIEW_GRAPH_CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

static void random_rotation(std::mt19937& g, double scale, double* R) {
    std::normal_distribution<double> N(0.0, scale);
    const double r[3] = {N(g), N(g), N(g)};
    so3exp(r, R);
}

static void check_csr(int n, const std::vector<int32_t>& i0, const std::vector<int32_t>& i1) {
    const int E = (int)i0.size();
    ViewGraphCsr G;
    CHECK(view_graph_csr(n, E, i0.data(), i1.data(), G));
    CHECK((int)G.row_ptr.size() == n + 1 && G.row_ptr[0] == 0 && G.row_ptr[n] == E);
    std::set<int> seen;
    for (int p = 0; p < E; p++) {
        const int e = G.perm[p];
        CHECK(e >= 0 && e < E && seen.insert(e).second && G.inv[e] == p && G.s0[p] == i0[e] && G.s1[p] == i1[e]);
        CHECK(p >= G.row_ptr[G.s0[p]] && p < G.row_ptr[G.s0[p] + 1]);
        if (p > 0) {
            const int q = G.perm[p - 1];
            CHECK(i0[q] < i0[e] || (i0[q] == i0[e] && (i1[q] < i1[e] || (i1[q] == i1[e] && q < e))));      // (index0, index1, position)
        }
    }
    // the two bounds delimit exactly the entries with index1 == c
    for (int v = 0; v < n; v++)
        for (int c = -1; c <= n; c++) {
            const int lo = view_graph_bound<false>(G.s1.data(), G.row_ptr[v], G.row_ptr[v + 1], c), hi = view_graph_bound<true>(G.s1.data(), lo, G.row_ptr[v + 1], c);
            int want = 0;
            for (int e = 0; e < E; e++) want += (i0[e] == v && i1[e] == c);
            CHECK(hi - lo == want && lo >= G.row_ptr[v] && hi <= G.row_ptr[v + 1]);
            for (int p = lo; p < hi; p++) CHECK(G.s1[p] == c);
        }
}

static void check_tree(int n, const std::vector<int32_t>& i0, const std::vector<int32_t>& i1, int root) {
    const int E = (int)i0.size();
    std::vector<int32_t> node(n, 7), parent(n, 7), edge(n, 7), lp(n + 1, 7); std::vector<uint8_t> rev(n, 7);
    int32_t reached = -1, levels = -1;
    CHECK(view_graph_tree(n, E, i0.data(), i1.data(), root, &reached, node.data(), parent.data(), edge.data(), rev.data(), &levels, lp.data()) == 0);
    // brute force: the rule of the header, scanning the whole list per popped node
    std::vector<int> q{root}, par{-1}, ed{-1}, rv{0}, lv{0}; std::set<int> seen{root};
    for (size_t h = 0; h < q.size(); h++)
        for (int e = 0; e < E; e++) {
            int v;
            if (i0[e] == q[h]) v = i1[e]; else if (i1[e] == q[h]) v = i0[e]; else continue;
            if (!seen.insert(v).second) continue;
            q.push_back(v); par.push_back(q[h]); ed.push_back(e); rv.push_back(i0[e] == q[h] ? 0 : 1); lv.push_back(lv[h] + 1);
        }
    CHECK(reached == (int)q.size() && levels == lv.back() + 1);
    for (int k = 0; k < n; k++) {
        if (k < reached) CHECK(node[k] == q[k] && parent[k] == par[k] && edge[k] == ed[k] && rev[k] == rv[k]);
        else CHECK(node[k] == -1 && parent[k] == -1 && edge[k] == -1 && rev[k] == 0);
    }
    for (int l = 0; l <= n; l++) {
        int want = reached;
        for (int k = reached - 1; k >= 0; k--) if (lv[k] == l) want = k;
        CHECK(lp[l] == want);
    }
}

static void check_join(std::mt19937& g, int n, const std::vector<int32_t>& i0, const std::vector<int32_t>& i1) {
    const int E = (int)i0.size();
    std::vector<double> R((size_t)9 * E);
    for (int e = 0; e < E; e++) random_rotation(g, 0.02, &R[9 * (size_t)e]);
    ViewGraphCsr G; CHECK(view_graph_csr(n, E, i0.data(), i1.data(), G));
    std::vector<double> Rs((size_t)9 * E);
    for (int p = 0; p < E; p++) for (int k = 0; k < 9; k++) Rs[9 * (size_t)p + k] = R[9 * (size_t)G.perm[p] + k];
    for (int order = 0; order < 2; order++) {
        const double thresh = 0.04;
        std::vector<uint8_t> good(E + 1, 0), want(E + 1, 0);
        const int64_t count = triplet_filter_host(G, Rs.data(), thresh, order, good.data());
        int64_t wcount = 0;
        for (int i = 0; i < E; i++) for (int j = 0; j < E; j++) {                       // examples/spherical_sfm_tools.cpp:1038-1068
            if (i0[j] != i1[i]) continue;
            for (int k = 0; k < E; k++) {
                if (i0[k] != i0[i] || i1[k] != i1[j]) continue;
                double M[9]; triplet_pair_product(&R[9 * (size_t)i], &R[9 * (size_t)j], order, M);
                if (triplet_error(M, &R[9 * (size_t)k]) < thresh) want[i] = want[j] = want[k] = 1;
                wcount++;
            }
        }
        CHECK(count == wcount && good == want && good[E] == 0);
    }
}

int main(int argc, char** argv) {
    const std::string work = argc > 1 ? argv[1] : ".";
    std::mt19937 g(11);
    // hand-made lists: empty, one self loop, duplicates only, everything into one node, a star out of one node, unsorted with reversed edges
    const std::vector<std::pair<int, std::vector<std::pair<int, int>>>> lists = {
        {1, {}}, {3, {}}, {1, {{0, 0}}}, {2, {{0, 1}, {0, 1}, {0, 1}, {1, 0}, {1, 1}}}, {5, {{4, 0}, {3, 0}, {2, 0}, {1, 0}, {0, 0}}},
        {6, {{0, 5}, {0, 4}, {0, 3}, {0, 2}, {0, 1}, {1, 2}, {2, 1}, {5, 3}, {0, 3}}}, {7, {{6, 5}, {5, 4}, {4, 3}, {6, 4}, {5, 3}, {6, 3}, {2, 2}, {1, 0}}}};
    for (auto& L : lists) {
        std::vector<int32_t> i0, i1; for (auto& e : L.second) { i0.push_back(e.first); i1.push_back(e.second); }
        check_csr(L.first, i0, i1); check_join(g, L.first, i0, i1);
        for (int root = 0; root < L.first; root++) check_tree(L.first, i0, i1, root);
    }
    for (int t = 0; t < 40; t++) {                                                        // random multigraphs
        const int n = 1 + (int)(g() % 20), E = (int)(g() % 90);
        std::vector<int32_t> i0(E), i1(E);
        for (int e = 0; e < E; e++) { i0[e] = (int32_t)(g() % n); i1[e] = (int32_t)(g() % n); }
        check_csr(n, i0, i1); check_join(g, n, i0, i1); check_tree(n, i0, i1, (int)(g() % n));
    }
    {   // refusals: indices and roots out of range, no cameras
        ViewGraphCsr G; const int32_t a[2] = {0, 3}, b[2] = {1, 1}, c[2] = {0, -1};
        CHECK(!view_graph_csr(3, 2, a, b, G) && !view_graph_csr(3, 2, b, c, G) && view_graph_csr(0, 0, nullptr, nullptr, G) && G.row_ptr.size() == 1);
        int32_t r = 0, l = 0;
        CHECK(view_graph_tree(3, 2, a, b, 0, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == -1);
        CHECK(view_graph_tree(3, 2, b, c, 0, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == -1);
        CHECK(view_graph_tree(3, 0, nullptr, nullptr, 3, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == -1);
        CHECK(view_graph_tree(3, 0, nullptr, nullptr, -1, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == -1);
        CHECK(view_graph_tree(0, 0, nullptr, nullptr, 0, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == -1);
        CHECK(view_graph_tree(3, 0, nullptr, nullptr, 2, &r, nullptr, nullptr, nullptr, nullptr, &l, nullptr) == 0 && r == 1 && l == 1);
    }
    {   // chaining a noise-free graph along the tree gives back the generating rotations, up to the root's
        const int n = 9; std::vector<double> Rgt((size_t)9 * n);
        for (int i = 0; i < n; i++) random_rotation(g, 0.5, &Rgt[9 * (size_t)i]);
        const std::vector<std::pair<int, int>> es = {{3, 1}, {1, 0}, {4, 0}, {4, 5}, {6, 5}, {2, 6}, {7, 2}, {7, 3}, {0, 0}};   // camera 8 is not reached
        std::vector<int32_t> i0, i1; std::vector<double> rel;
        for (auto& e : es) { i0.push_back(e.first); i1.push_back(e.second); double M[9]; mat3_mul_bt(&Rgt[9 * (size_t)e.second], &Rgt[9 * (size_t)e.first], M); rel.insert(rel.end(), M, M + 9); }
        std::vector<int32_t> node(n), parent(n), edge(n), lp(n + 1); std::vector<uint8_t> rev(n); int32_t reached = 0, levels = 0;
        CHECK(view_graph_tree(n, (int)es.size(), i0.data(), i1.data(), 4, &reached, node.data(), parent.data(), edge.data(), rev.data(), &levels, lp.data()) == 0 && reached == 8);
        std::vector<double> rot((size_t)9 * n);
        view_graph_chain(n, reached, node.data(), parent.data(), edge.data(), rev.data(), rel.data(), rot.data());
        for (int i = 0; i < n; i++) {
            double want[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            if (i != 8) mat3_mul_bt(&Rgt[9 * (size_t)i], &Rgt[9 * 4], want);
            for (int k = 0; k < 9; k++) CHECK(std::fabs(rot[9 * (size_t)i + k] - want[k]) <= 1e-12);
        }
    }
    {   // the mirror's bookkeeping: kept matches in list order, a flag vector shorter than the list, records that name no match, the log's lines
        using namespace sphericalsfm;
        const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::vector<ImageMatch> ms; for (int e = 0; e < 5; e++) ms.push_back(ImageMatch(e, e + 10, Matches{{(size_t)e, (size_t)e}}, I));
        const std::vector<int32_t> tri = {0, 1, 2, 4, 3, 0, -1, 0, 0, 0, 5, 0};
        const std::vector<double> err = {M_PI / 180.0, M_PI / 90.0, 1.0, 1.0};
        const std::string log = work + "/filter.txt";
        std::vector<ImageMatch> kept = apply_triplet_filter(ms, {1, 0, 0, 1, 1}, 4, tri.data(), err.data(), log.c_str());
        CHECK(kept.size() == 3 && kept[0].index0 == 0 && kept[1].index0 == 3 && kept[2].index0 == 4 && kept[2].matches.size() == 1);
        std::ifstream f(log); std::string l1, l2, l3;
        std::getline(f, l1); std::getline(f, l2); CHECK(!std::getline(f, l3));
        CHECK(l1 == "0 10 11 1.000000" && l2 == "4 14 13 2.000000");
        CHECK(apply_triplet_filter(ms, {1, 1}, 0, nullptr, nullptr, nullptr).size() == 2);
        CHECK(apply_triplet_filter({}, {}, 0, nullptr, nullptr, nullptr).empty());
    }
    std::printf("VIEW_GRAPH_CHECK ok\n");
    return 0;
}
