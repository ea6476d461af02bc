"""Python host side of the view-graph calls (include/ssfm.h: ssfm_triplet_filter, ssfm_view_graph_tree, ssfm_focal_search_graph, ssfm_rot_l1_init, ssfm_focal_search_l1): what the pipeline needs when
the file order of the images is not their capture order, so that any pair (a, b) may carry a relative rotation and no chain (k-1, k) exists.

Rotations are (n,3,3) arrays indexed R[i,j]; edge e = (index0[e], index1[e]) carries R_e with R_index1 = R_e R_index0."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import c_double_p, c_i32_p, c_u8_p
from .rotavg import _edges

ORDER_REFERENCE, ORDER_COMPOSED = 0, 1


def triplet_filter(ctx, num_cameras, index0, index1, rel_rotations, err_thresh_rad, order=ORDER_REFERENCE, max_records=0):
    """filter_image_matches (examples/spherical_sfm_tools.cpp:1031-1082) on the device -> (good (E,) bool, num_triplets) and, with max_records > 0,
    also (triplets (m,3) list positions (i, j, k), errors (m,) radians), m = min(num_triplets, max_records), in the order include/ssfm.h defines."""
    i0, i1, rel = _edges(index0, index1, rel_rotations) if len(index0) else (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    E = len(i0)
    good = np.zeros(max(E, 1), np.uint8); nt = C.c_int64(0)
    m = int(max_records)
    tri = np.zeros(3 * max(m, 1), np.int32); err = np.zeros(max(m, 1))
    _lib.check(_lib.lib().ssfm_triplet_filter(ctx._p if ctx is not None else None, int(num_cameras), E, i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p),
                                              rel.ctypes.data_as(c_double_p), float(err_thresh_rad), int(order), good.ctypes.data_as(c_u8_p), C.byref(nt), m,
                                              tri.ctypes.data_as(c_i32_p) if m > 0 else None, err.ctypes.data_as(c_double_p) if m > 0 else None),
               ctx._p if ctx is not None else None)
    out = (good[:E].astype(bool), int(nt.value))
    if m > 0:
        k = min(m, int(nt.value))
        out += (tri.reshape(-1, 3)[:k].copy(), err[:k].copy())
    return out


def spanning_tree(num_cameras, index0, index1, root=0):
    """Breadth-first spanning tree of the view graph (ssfm_view_graph_tree; host code, no context) -> dict with num_reached, num_levels and the arrays
    node, parent, edge, reversed (num_cameras entries, visiting order, -1 / 0 past num_reached) and level_ptr (num_cameras + 1)."""
    i0 = np.ascontiguousarray(index0, np.int32); i1 = np.ascontiguousarray(index1, np.int32); n = int(num_cameras)
    node = np.zeros(max(n, 1), np.int32); parent = np.zeros_like(node); edge = np.zeros_like(node); rev = np.zeros(max(n, 1), np.uint8)
    lp = np.zeros(max(n, 1) + 1, np.int32); nr = C.c_int32(0); nl = C.c_int32(0)
    _lib.check(_lib.lib().ssfm_view_graph_tree(n, len(i0), i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p), int(root), C.byref(nr), node.ctypes.data_as(c_i32_p),
                                               parent.ctypes.data_as(c_i32_p), edge.ctypes.data_as(c_i32_p), rev.ctypes.data_as(c_u8_p), C.byref(nl),
                                               lp.ctypes.data_as(c_i32_p)))
    return dict(num_reached=nr.value, num_levels=nl.value, node=node, parent=parent, edge=edge, reversed=rev, level_ptr=lp)


def initialize_rotations_tree(num_cameras, index0, index1, rel_rotations, root=0):
    """The relative rotations chained along the spanning tree: forward edge R_child = R_e R_parent, reversed edge R_child = R_e^T R_parent, unreached cameras
    keep the identity -> rotations (n,3,3).  The start for optimize_rotations on a graph without a chain."""
    t = spanning_tree(num_cameras, index0, index1, root)
    rel = np.asarray(rel_rotations, np.float64)
    rot = np.tile(np.eye(3), (int(num_cameras), 1, 1))
    for k in range(1, t["num_reached"]):
        Re = rel[t["edge"][k]]
        rot[t["node"][k]] = (Re.T if t["reversed"][k] else Re) @ rot[t["parent"][k]]
    return rot


def initialize_rotations_l1(ctx, num_cameras, index0, index1, rel_rotations, root=0, **options):
    """Robust start over any view graph (ssfm_rot_l1_init: L1 iteratively reweighted least squares from the tree chain of `root`, conjugate gradients on the device)
    -> (rotations (n,3,3), residuals (E,) = |so3ln(R_b^T R_e R_a)| in radians at those rotations, -1 for an edge that is not used, summary dict).
    options: max_iterations, step_tolerance, weight_floor, pcg_tolerance, pcg_max_iterations (include/ssfm.h states the defaults).  Dropping the edges whose
    residual exceeds a threshold before optimize_rotations is what removes the outliers' bias."""
    L = _lib.lib()
    n = int(num_cameras)
    i0, i1, rel = _edges(index0, index1, rel_rotations) if len(index0) else (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    E = len(i0)
    o = _lib.RotL1OptionsC(); L.ssfm_rot_l1_default_options(C.byref(o))
    for k, v in options.items():
        if k not in dict(o._fields_):
            raise TypeError(f"initialize_rotations_l1: unknown option {k!r}")
        setattr(o, k, v)
    rot = np.zeros(9 * max(n, 1)); res = np.zeros(max(E, 1)); s = _lib.RotL1SummaryC()
    p = ctx._p if ctx is not None else None
    _lib.check(L.ssfm_rot_l1_init(p, n, E, i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p), rel.ctypes.data_as(c_double_p), int(root), C.byref(o),
                                  rot.ctypes.data_as(c_double_p), res.ctypes.data_as(c_double_p), C.byref(s)), p)
    return np.transpose(rot[:9 * n].reshape(-1, 3, 3), (0, 2, 1)).copy(), res[:E].copy(), s.as_dict()


def focal_search_graph(ctx, num_cameras, index0, index1, rel_rotations, focal_guess, focals, inward=False, root=0, return_matches=False):
    """rotavg.focal_search with the rotations of every trial chained along the spanning tree (ssfm_focal_search_graph) -> the same tuple."""
    i0, i1, rel = _edges(index0, index1, rel_rotations)
    fv = np.ascontiguousarray(focals, np.float64); T = len(fv)
    costs = np.zeros(T); best = C.c_int32(0); rot = np.zeros(9 * num_cameras); relb = np.zeros(9 * len(i0))
    _lib.check(_lib.lib().ssfm_focal_search_graph(ctx._p, num_cameras, len(i0), i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p),
                                                  rel.ctypes.data_as(c_double_p), int(bool(inward)), float(focal_guess), T, fv.ctypes.data_as(c_double_p), int(root),
                                                  costs.ctypes.data_as(c_double_p), C.byref(best), rot.ctypes.data_as(c_double_p),
                                                  relb.ctypes.data_as(c_double_p)), ctx._p)
    out = (costs, best.value, np.transpose(rot.reshape(-1, 3, 3), (0, 2, 1)).copy())
    return out + (np.transpose(relb.reshape(-1, 3, 3), (0, 2, 1)).copy(),) if return_matches else out


def focal_search_l1(ctx, num_cameras, index0, index1, rel_rotations, focal_guess, focals, inward=False, root=0, return_matches=False, **options):
    """The robust focal search (ssfm_focal_search_l1): per trial focal the matches are re-derived as in focal_search_graph, the rotations are solved by the L1
    iteration of initialize_rotations_l1 from the tree chain, and the trial is judged by the sum of the residuals |v_e| -> (costs (T,), best, rotations (n,3,3)
    of the best trial, info).  info: get_costs (T,) (focal_search_graph's cost at the L1 rotations), iterations (T,), residual (E,) at the best trial in radians
    (-1 for an edge that is not used), kernel_ms and, with return_matches, matches (E,3,3) at the best focal.
    options: those of initialize_rotations_l1; the default of max_iterations is 10 here."""
    L = _lib.lib()
    n = int(num_cameras)
    i0, i1, rel = _edges(index0, index1, rel_rotations) if len(index0) else (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    E = len(i0)
    o = _lib.RotL1OptionsC(); L.ssfm_focal_l1_default_options(C.byref(o))
    for k, v in options.items():
        if k not in dict(o._fields_):
            raise TypeError(f"focal_search_l1: unknown option {k!r}")
        setattr(o, k, v)
    fv = np.ascontiguousarray(focals, np.float64); T = len(fv)
    costs = np.zeros(max(T, 1)); gc = np.zeros(max(T, 1)); its = np.zeros(max(T, 1), np.int32); best = C.c_int32(0); ms = C.c_double(0.0)
    rot = np.zeros(9 * max(n, 1)); relb = np.zeros(9 * max(E, 1)); res = np.zeros(max(E, 1))
    p = ctx._p if ctx is not None else None
    _lib.check(L.ssfm_focal_search_l1(p, n, E, i0.ctypes.data_as(c_i32_p), i1.ctypes.data_as(c_i32_p), rel.ctypes.data_as(c_double_p), int(bool(inward)),
                                      float(focal_guess), T, fv.ctypes.data_as(c_double_p), int(root), C.byref(o), costs.ctypes.data_as(c_double_p),
                                      gc.ctypes.data_as(c_double_p), its.ctypes.data_as(c_i32_p), C.byref(best), rot.ctypes.data_as(c_double_p),
                                      relb.ctypes.data_as(c_double_p), res.ctypes.data_as(c_double_p), C.byref(ms)), p)
    info = dict(get_costs=gc[:T].copy(), iterations=its[:T].copy(), residual=res[:E].copy(), kernel_ms=ms.value)
    if return_matches:
        info["matches"] = np.transpose(relb[:9 * E].reshape(-1, 3, 3), (0, 2, 1)).copy()
    return costs[:T].copy(), best.value, np.transpose(rot[:9 * n].reshape(-1, 3, 3), (0, 2, 1)).copy(), info
