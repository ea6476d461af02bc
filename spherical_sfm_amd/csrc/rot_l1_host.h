// spherical_sfm_amd -- host side of ssfm_rot_l1_init (include/ssfm.h): the argument checks, the reach set of the root and the node-major adjacency the
// kernels of rot_l1.hip walk.  Plain C++ without a device: rot_l1.hip includes it, and so does tests/native/rot_l1_host_check.cpp, which runs it under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>
#include "../../include/ssfm.h"
#include "view_graph_host.h"

namespace ssfm {

// nullptr when the call may go on, otherwise the reason it is refused (SSFM_ERR_INVALID).  Arguments and options first, indices next, the root last: the order of
// ssfm_triplet_filter's checks; the context is looked at after all of them.  step_tolerance = 0 is valid (run exactly max_iterations), and so is
// pcg_max_iterations = 0 (4 x the free node count).
inline const char* rot_l1_check(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, const double* rel_rotations, int32_t root,
                                const ssfm_rot_l1_options* o, const double* rotations_out, const ssfm_rot_l1_summary* s) {
    if (num_cameras < 0 || num_cameras > (1 << 29) /* 3 n vector entries */ || num_edges < 0 || num_edges > (1 << 30) /* 2 E adjacency entries, int32 offsets */ || (num_edges > 0 && (!index0 || !index1 || !rel_rotations)) || !rotations_out || !s) return "bad arguments";
    if (o && (o->max_iterations <= 0 || !(o->step_tolerance >= 0.0) || !(o->weight_floor > 0.0) || !(o->pcg_tolerance > 0.0) || o->pcg_max_iterations < 0))
        return "bad options";
    for (int32_t e = 0; e < num_edges; e++)
        if (index0[e] < 0 || index0[e] >= num_cameras || index1[e] < 0 || index1[e] >= num_cameras) return "camera index out of range";
    if (root < 0 || root >= num_cameras) return "root out of range";
    return nullptr;
}

// What the kernels need of the graph.  A used edge has two different ends, both reached from the root; a free node is a reached node other than the root.
// Node i owns the entries adj_ptr[i] .. adj_ptr[i + 1] of adj_nb / adj_es, one per used edge at i, ascending by (neighbour, edge id):
// adj_es = 2 * edge id + side, side 1 when i is the edge's index1 (the edge adds +w v to g_i), 0 when it is its index0 (-w v).  Self loops are left out.
struct RotL1Graph {
    std::vector<int32_t> reached, free_node, adj_ptr, adj_nb;       // reached / free_node: 0 or 1 per camera
    std::vector<uint32_t> adj_es;
    std::vector<int32_t> t_node, t_parent, t_edge; std::vector<uint8_t> t_rev;   // the spanning tree of view_graph_tree, for the start
    int32_t num_reached = 0, num_free = 0, num_edges_used = 0;
};

// The reach set is the node list of view_graph_tree: the same breadth-first walk as ssfm_view_graph_tree.  Returns false for what rot_l1_check refuses.
inline bool rot_l1_graph(int32_t num_cameras, int32_t num_edges, const int32_t* index0, const int32_t* index1, int32_t root, RotL1Graph& G) {
    const size_t n = (size_t)(num_cameras > 0 ? num_cameras : 0), E = (size_t)(num_edges > 0 ? num_edges : 0);
    G.t_node.assign(n, -1); G.t_parent.assign(n, -1); G.t_edge.assign(n, -1); G.t_rev.assign(n, 0);
    int32_t levels = 0;
    if (view_graph_tree(num_cameras, num_edges, index0, index1, root, &G.num_reached, G.t_node.data(), G.t_parent.data(), G.t_edge.data(), G.t_rev.data(), &levels,
                        nullptr) != 0)
        return false;
    G.reached.assign(n, 0); G.free_node.assign(n, 0);
    for (int32_t k = 0; k < G.num_reached; k++) { G.reached[(size_t)G.t_node[(size_t)k]] = 1; G.free_node[(size_t)G.t_node[(size_t)k]] = k > 0 ? 1 : 0; }
    G.num_free = G.num_reached - 1;
    G.adj_ptr.assign(n + 1, 0);
    G.num_edges_used = 0;
    auto used = [&](size_t e) { return index0[e] != index1[e] && G.reached[(size_t)index0[e]] && G.reached[(size_t)index1[e]]; };
    for (size_t e = 0; e < E; e++)
        if (used(e)) { G.adj_ptr[(size_t)index0[e] + 1]++; G.adj_ptr[(size_t)index1[e] + 1]++; G.num_edges_used++; }
    for (size_t v = 0; v < n; v++) G.adj_ptr[v + 1] += G.adj_ptr[v];
    const size_t total = (size_t)G.adj_ptr[n];
    std::vector<std::pair<int32_t, uint32_t>> ent(total);
    std::vector<int32_t> at(G.adj_ptr.begin(), G.adj_ptr.end() - 1);
    for (size_t e = 0; e < E; e++) {
        if (!used(e)) continue;
        ent[(size_t)at[(size_t)index0[e]]++] = {index1[e], 2u * (uint32_t)e};
        ent[(size_t)at[(size_t)index1[e]]++] = {index0[e], 2u * (uint32_t)e + 1u};
    }
    for (size_t v = 0; v < n; v++) std::sort(ent.begin() + G.adj_ptr[v], ent.begin() + G.adj_ptr[v + 1]);      // (neighbour, edge id): the side bit never decides
    G.adj_nb.resize(total); G.adj_es.resize(total);
    for (size_t q = 0; q < total; q++) { G.adj_nb[q] = ent[q].first; G.adj_es[q] = ent[q].second; }
    return true;
}

}  // namespace ssfm
