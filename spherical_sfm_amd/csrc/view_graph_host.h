// spherical_sfm_amd -- host side of the view-graph calls (include/ssfm.h: ssfm_triplet_filter, ssfm_view_graph_tree, ssfm_focal_search_graph).
// Plain C++ without a device: view_graph.hip includes it, and so does tests/native/view_graph_check.cpp, which runs it under ASan + UBSan.
#pragma once
#include <cstdint>
#include <vector>
#include "ssfm_math.h"

namespace ssfm {

// The edge list as a CSR by index0: sorted by (index0, index1, list position).  perm[p] is the list position of sorted entry p, inv its inverse;
// out(v) = sorted entries row_ptr[v] .. row_ptr[v + 1], ascending by (index1, position).
struct ViewGraphCsr {
    std::vector<int32_t> row_ptr, s0, s1, perm, inv;
};

// Two stable counting sorts (by index1, then by index0).  Returns false, touching nothing else, when an index lies outside [0, num_cameras).
inline bool view_graph_csr(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, ViewGraphCsr& G) {
    const size_t n = (size_t)(num_cameras > 0 ? num_cameras : 0), E = (size_t)(num_edges > 0 ? num_edges : 0);
    for (size_t e = 0; e < E; e++)
        if (index0[e] < 0 || index0[e] >= num_cameras || index1[e] < 0 || index1[e] >= num_cameras) return false;
    std::vector<int32_t> cnt(n + 1, 0), tmp(E);
    for (size_t e = 0; e < E; e++) cnt[(size_t)index1[e] + 1]++;
    for (size_t v = 0; v < n; v++) cnt[v + 1] += cnt[v];
    for (size_t e = 0; e < E; e++) tmp[(size_t)cnt[index1[e]]++] = (int32_t)e;              // by (index1, position)
    G.row_ptr.assign(n + 1, 0);
    for (size_t e = 0; e < E; e++) G.row_ptr[(size_t)index0[e] + 1]++;
    for (size_t v = 0; v < n; v++) G.row_ptr[v + 1] += G.row_ptr[v];
    std::vector<int32_t> at(G.row_ptr.begin(), G.row_ptr.end() - 1);
    G.perm.assign(E, 0); G.inv.assign(E, 0); G.s0.assign(E, 0); G.s1.assign(E, 0);
    for (size_t q = 0; q < E; q++) { const int32_t e = tmp[q]; G.perm[(size_t)at[index0[e]]++] = e; }   // stable: (index0, index1, position)
    for (size_t p = 0; p < E; p++) { const int32_t e = G.perm[p]; G.inv[(size_t)e] = (int32_t)p; G.s0[p] = index0[e]; G.s1[p] = index1[e]; }
    return true;
}

// first sorted entry of [lo, hi) whose index1 is >= c (UPPER: > c)
template <bool UPPER>
SSFM_HD int view_graph_bound(const int32_t* s1, int lo, int hi, int c) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const bool right = UPPER ? (s1[mid] <= c) : (s1[mid] < c);
        if (right) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// M of one (i, j): Ri Rj as examples/spherical_sfm_tools.cpp:1055 writes it (order 0), Rj Ri as the edge convention R_b = R_ab R_a implies (order 1).  Row-major.
SSFM_HD void triplet_pair_product(const double* Ri, const double* Rj, int order, double* M) {
    if (order == 0) mat3_mul(Ri, Rj, M); else mat3_mul(Rj, Ri, M);
}
// |so3ln(M Rk^T)|: the one definition of the triplet error, for the kernels and for the host
SSFM_HD double triplet_error(const double* M, const double* Rk) {
    double D[9], w[3];
    mat3_mul_bt(M, Rk, D); so3ln(D, w);
    return norm3(w);
}

// Breadth-first spanning tree (ssfm_view_graph_tree; the header states the rules).  Returns 0, or -1 for a root or an index out of range.
// Entries past num_reached: node / parent / edge = -1, reversed = 0; level_ptr past num_levels repeats num_reached.
inline int view_graph_tree(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, int32_t root, int32_t* num_reached,
                           int32_t* node_out, int32_t* parent_out, int32_t* edge_out, uint8_t* reversed_out, int32_t* num_levels, int32_t* level_ptr) {
    if (num_cameras <= 0 || num_edges < 0 || root < 0 || root >= num_cameras) return -1;
    const size_t n = (size_t)num_cameras, E = (size_t)num_edges;
    for (size_t e = 0; e < E; e++)
        if (index0[e] < 0 || index0[e] >= num_cameras || index1[e] < 0 || index1[e] >= num_cameras) return -1;
    // incident edges of every node, ascending list position (a self loop is listed once)
    std::vector<int64_t> ptr(n + 1, 0);
    for (size_t e = 0; e < E; e++) { ptr[(size_t)index0[e] + 1]++; if (index1[e] != index0[e]) ptr[(size_t)index1[e] + 1]++; }
    for (size_t v = 0; v < n; v++) ptr[v + 1] += ptr[v];
    std::vector<int32_t> inc((size_t)ptr[n]); std::vector<int64_t> at(ptr.begin(), ptr.end() - 1);
    for (size_t e = 0; e < E; e++) { inc[(size_t)at[index0[e]]++] = (int32_t)e; if (index1[e] != index0[e]) inc[(size_t)at[index1[e]]++] = (int32_t)e; }
    std::vector<int32_t> node(n, -1), parent(n, -1), edge(n, -1), level(n, 0); std::vector<uint8_t> rev(n, 0), seen(n, 0);
    size_t count = 0;
    node[count++] = root; seen[(size_t)root] = 1;
    for (size_t head = 0; head < count; head++) {                                      // the output arrays are the queue
        const int32_t u = node[head];
        for (int64_t q = ptr[(size_t)u]; q < ptr[(size_t)u + 1]; q++) {
            const int32_t e = inc[(size_t)q];
            const bool fwd = index0[e] == u;
            const int32_t v = fwd ? index1[e] : index0[e];
            if (seen[(size_t)v]) continue;
            seen[(size_t)v] = 1;
            node[count] = v; parent[count] = u; edge[count] = e; rev[count] = fwd ? 0 : 1; level[count] = level[head] + 1;
            count++;
        }
    }
    const int32_t levels = level[count - 1] + 1;
    if (num_reached) *num_reached = (int32_t)count;
    if (num_levels) *num_levels = levels;
    for (size_t k = 0; k < n; k++) {
        if (node_out) node_out[k] = node[k];
        if (parent_out) parent_out[k] = parent[k];
        if (edge_out) edge_out[k] = edge[k];
        if (reversed_out) reversed_out[k] = rev[k];
    }
    if (level_ptr) {
        for (size_t k = 0; k <= n; k++) level_ptr[k] = (int32_t)count;
        for (size_t k = count; k-- > 0;) level_ptr[(size_t)level[k]] = (int32_t)k;     // first position of every level
    }
    return 0;
}

// R_child = R_e R_parent along the tree (reversed: R_e^T R_parent); unreached cameras keep the identity.  rel / rotations: row-major 3x3.
inline void view_graph_chain(int32_t num_cameras, int32_t num_reached, const int32_t* node, const int32_t* parent, const int32_t* edge, const uint8_t* reversed,
                             const double* rel, double* rotations) {
    for (int32_t i = 0; i < num_cameras; i++) for (int k = 0; k < 9; k++) rotations[9 * (size_t)i + k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int32_t k = 1; k < num_reached; k++) {
        const double* Re = rel + 9 * (size_t)edge[k]; const double* Rp = rotations + 9 * (size_t)parent[k];
        double Rn[9];
        if (reversed[k]) mat3_mul_at(Re, Rp, Rn); else mat3_mul(Re, Rp, Rn);
        for (int q = 0; q < 9; q++) rotations[9 * (size_t)node[k] + q] = Rn[q];
    }
}

// The reference loops of filter_image_matches (examples/spherical_sfm_tools.cpp:1038-1068) over the CSR, on the host: the flags and the triplet count.
// What the kernels compute, in the same order; used by the stand-alone check and small enough to read next to them.
inline int64_t triplet_filter_host(const ViewGraphCsr& G, const double* Rs /* sorted order, row-major */, double thresh, int order, uint8_t* good) {
    const int32_t E = (int32_t)G.perm.size();
    int64_t count = 0;
    for (int32_t i = 0; i < E; i++) {
        const int32_t p = G.inv[(size_t)i], a = G.s0[(size_t)p], b = G.s1[(size_t)p];
        for (int32_t pj = G.row_ptr[(size_t)b]; pj < G.row_ptr[(size_t)b + 1]; pj++) {
            const int32_t c = G.s1[(size_t)pj];
            const int lo = view_graph_bound<false>(G.s1.data(), G.row_ptr[(size_t)a], G.row_ptr[(size_t)a + 1], c);
            const int hi = view_graph_bound<true>(G.s1.data(), lo, G.row_ptr[(size_t)a + 1], c);
            if (hi <= lo) continue;
            double M[9]; triplet_pair_product(Rs + 9 * (size_t)p, Rs + 9 * (size_t)pj, order, M);
            for (int pk = lo; pk < hi; pk++) {
                if (triplet_error(M, Rs + 9 * (size_t)pk) < thresh) { good[i] = 1; good[(size_t)G.perm[(size_t)pj]] = 1; good[(size_t)G.perm[(size_t)pk]] = 1; }
                count++;
            }
        }
    }
    return count;
}

}  // namespace ssfm
