// spherical_sfm_amd -- which kernels the reduced-system solve (reduced_solve.h) runs for a band of DC x DC blocks with half-width b, and what they are launched with:
// the LDS byte counts of the band kernels (one named function per carve-up, next to nothing else that could drift) and the plan of one solve (BandPath).
// Host-only, no HIP, no getenv: tests/native/band_path_check.cpp walks every (DC, b) and asserts the landmarks and the kernels' launch contracts.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ssfm {

// ---- wave roles of k_band_chol_v2 (band_kernels2.h) --------------------------------------------------------------------------------------
constexpr int CHOL2_LOADERS = 2;
// Role of every PHYSICAL wave of the workgroup (wave p runs on SIMD p % 4): v[p] = the role index the kernel's logic uses (0 look-ahead,
// 1..ntw trailing update, then the loaders, the writer last).  With the identity a nine-wave workgroup puts the look-ahead (the dependent chain of
// the step), a trailing wave and the writer on SIMD 0: their phases took 1.6k / 2.2k / 2.1k cycles against 1.3-1.5k for the trailing waves
// that share a SIMD with one loader only, and the step waits for the slowest (s_memtime stamps, scripts/lab/chol_stamps.hip).
struct CholWaveMap { unsigned char v[16]; };
inline CholWaveMap chol_wave_map(int nw, int ntw, int heavy_tw) {      // heavy_tw: trailing waves that carry block tasks (the rest only right-hand sides)
    CholWaveMap m; for (int i = 0; i < 16; i++) m.v[i] = (unsigned char)i;
    // Measured, not derived: the nine-wave workgroup of config 2 (6x6 blocks, half-width 10) gains 18 % per step; with eleven waves (half-width 14,
    // where both loaders then sit with the look-ahead: 286 -> 340 us per launch at the configs[4] size) and with six (merged 3-dof pairs: 2.18 -> 2.20 ms per
    // solve) the identity is better, so only the shape that was stamped is remapped.
    if (nw != 9) return m;
    int weight[16], order[16];
    for (int r = 0; r < nw; r++) {
        weight[r] = (r == 0) ? 12 : (r <= ntw) ? ((r <= heavy_tw) ? 6 : 2) : (r == nw - 1) ? 5 : 4;
        order[r] = r;
    }
    for (int a = 0; a < nw; a++) for (int c = a + 1; c < nw; c++) if (weight[order[c]] > weight[order[a]]) { const int t = order[a]; order[a] = order[c]; order[c] = t; }
    int load[4] = {0, 0, 0, 0}, used[4] = {0, 0, 0, 0}, cap[4];
    for (int q = 0; q < 4; q++) cap[q] = (nw - q + 3) / 4;                // physical waves q, q + 4, ...
    // SIMD 0: the look-ahead (first in the order) and the LIGHTEST roles for its other waves; everything else heaviest first onto the least
    // loaded of the other three SIMDs
    bool placed[16] = {false};
    m.v[0] = (unsigned char)order[0]; placed[0] = true; used[0] = 1;
    for (int a = nw - 1; a >= 1 && used[0] < cap[0]; a--) { m.v[4 * used[0]] = (unsigned char)order[a]; placed[a] = true; used[0]++; }
    for (int a = 1; a < nw; a++) {
        if (placed[a]) continue;
        int best = -1;
        for (int q = 1; q < 4; q++) if (used[q] < cap[q] && (best < 0 || load[q] < load[best])) best = q;
        m.v[best + 4 * used[best]] = (unsigned char)order[a];
        load[best] += weight[order[a]]; used[best]++;
    }
    return m;
}

// ---- dynamic LDS of the band kernels: each function states the carve-up at the top of its kernel -------------------------------------------
// k_band_chol_v2 (band_kernels2.h): window ring + panel + right-hand-side rows + y_j + G + scratch block, then the pair table
inline size_t chol2_lds_bytes(int DC, int b, int NR) {
    const size_t BB = (size_t)DC * DC;
    return ((size_t)(b + 1) * (b + 1) * BB + (size_t)b * BB + (size_t)(b + 1) * NR * DC + (size_t)NR * DC + 2 * BB) * sizeof(double) + ((size_t)b * (b + 1) / 2 + 2) * sizeof(int);
}
// k_band_chol_v2p (band_kernels2p.h, 6x6 blocks): the live triangle of the window instead of the ring; T6 keeps a transposed copy of the panel
inline size_t chol2p_lds_bytes(int b, int NR, bool t6 = false) {
    constexpr int DC = 6, BB = 36;
    return ((size_t)(b + 1) * (b + 2) / 2 * BB + (size_t)b * BB * (t6 ? 2 : 1) + (size_t)(b + 1) * NR * DC + NR * DC + 2 * BB) * sizeof(double) + ((size_t)b * (b + 1) / 2 + 2) * sizeof(int);
}
// k_band_chol (band_kernels.h, the window stays in global memory): G + diagonal block + y_j + panel
inline size_t band_chol_lds_bytes(int DC, int b, int NR) { return ((size_t)2 * DC * DC + (size_t)NR * DC + (size_t)b * DC * DC) * sizeof(double); }
// k_band_fwd / k_band_back / k_band_fwd_lds (band_kernels.h): ring of the last b solutions + partial products + one row sum
inline size_t band_subst_lds_bytes(int DC, int b, int NR) { return ((size_t)2 * b * NR * DC + (size_t)NR * DC) * sizeof(double); }
// k_sub_sep_chain / k_sub_sep_chain_mfma (band_sub.h), Q = b DC: one packed triangle (two with ping-pong) + F + the vectors t, w
inline size_t chain_lds_bytes(int Q, int NR, bool two_triangles) {
    return ((size_t)Q * (Q + 1) / 2 * (two_triangles ? 2 : 1) + (size_t)Q * Q + (size_t)2 * NR * Q) * sizeof(double);
}
// k_sub_apply_left (band_sub.h): the separator's solution + one partial sum per (slice, row, right-hand side)
constexpr int APPLY_ROWS = 64, APPLY_SLICES = 4;
inline size_t sub_apply_lds_bytes(int Q, int NR) { return ((size_t)NR * Q + (size_t)APPLY_SLICES * APPLY_ROWS * NR) * sizeof(double); }
constexpr int RING_BACK_P = 8;                    // threads that share one entry of F^T x in ring_back_node (band_ring.h)

// ---- the plan of one solve -------------------------------------------------------------------------------------------------------------------
// Lab knobs that change the plan (knobs.h: live in the lab library only).  The defaults are the shipped values; reduced_solve.h fills the struct from SSFM_LAB_KNOB.
struct BandPathLab {
    bool chol_wave_map = true;      // SSFM_CHOL_WAVE_MAP
    int band_mfma = 0;              // SSFM_BAND_MFMA   bit 0: matrix-core panel, bit 1: matrix-core trailing update
    bool band_early = false;        // SSFM_BAND_EARLY  early look-ahead
    bool chol_fuse = false;         // SSFM_CHOL_FUSE   segments and twisted separators in one launch
    bool chain_pingpong = true;     // SSFM_CHAIN_PINGPONG
    bool chain_twist = true;        // SSFM_CHAIN_TWIST
    int spike_nc = 0;               // SSFM_SPIKE_NC    > 0: columns per wave of the spike kernel
    int ring_roles = 0;             // SSFM_RING_ROLES  > 0: workgroups per ring elimination
};

enum BandFactor {
    BAND_FACTOR_GLOBAL,             // k_band_chol: one workgroup, the window in global memory
    BAND_FACTOR_SQUARE,             // k_band_chol_v2: (b+1)^2 ring of blocks in LDS
    BAND_FACTOR_PACKED3,            // k_band_chol_v2p<2, 3, npb, pre>: packed window, 3x3 tiles
    BAND_FACTOR_PACKED_T6           // k_band_chol_v2p<2, 1, 2, 8, true>: packed window, 6x6 tiles
};

struct BandPath {
    int DC = 0, b = 0, num_cus = 0;
    BandPathLab lab;
    // factorisation (two right-hand-side columns)
    BandFactor factor = BAND_FACTOR_GLOBAL;
    int npb = 0, pre = 0;           // PACKED3: panel entries per thread, prefetch rounds (template arguments of the kernel)
    size_t chol_lds = 0;            // dynamic LDS of the factorisation kernel chosen
    int chol_threads = 0;
    int chol_ntw = 0, chol_heavy = 0;     // SQUARE: trailing-update waves, and how many of them carry block tasks (chol_wave_map)
    CholWaveMap chol_map;           // SQUARE
    int chol_mf = 0; bool chol_early = false;     // SQUARE, lab: matrix-core bits / early look-ahead
    // back substitution: task sets per lane of the single-wave k_band_back_v2 (b DC <= 64 / 128 / 192); 0 = k_band_back (GLOBAL)
    int back_sets = 0;
    // long components through segments, spikes and separators (band_sub.h): taken when the plan holds one and the factorisation is LDS-resident
    bool substructured = false;
    int Q = 0;                      // rows of a separator block
    size_t chain_lds = 0; int chain_pp = 0;       // separator chain: bytes, 1 = two triangles take turns (ping-pong)
    int ring_back_threads = 0, ring_cr_threads = 0;

    bool lds_factor() const { return factor != BAND_FACTOR_GLOBAL; }
    bool packed() const { return factor == BAND_FACTOR_PACKED3 || factor == BAND_FACTOR_PACKED_T6; }
    // The substructured factor has no stand-alone substitution kernels: a second solve with it (PCG refinement) rebuilds the band and factors again.
    bool needs_refactor() const { return substructured; }
    size_t subst_lds(int NR) const { return band_subst_lds_bytes(DC, b, NR); }
    size_t apply_lds() const { return sub_apply_lds_bytes(Q, 2); }
    // one launch for the segments AND the separators of twisted components: the waiting workgroups must all be resident (one per compute unit)
    bool fused_factor(int nseg, int ntwist) const { return lab.chol_fuse && !packed() && ntwist > 0 && nseg + ntwist <= num_cus; }
    // Spike columns per wave: what decides is how many one-wave workgroups the launch has -- one column per wave until the chip is full (~3000 waves), then two, then
    // three (us per launch at NC = 1 / 2 / 3: 4 arcs b = 13: 35 / 45 / 58; 8 arcs b = 7: 18.5 / 24.8 / 32.0; 32 arcs b = 5: 19 / 23 / 29; 128 arcs b = 7: 70 / 52.6 / 58.7)
    int spike_cols(int nleft) const {
        if (lab.spike_nc > 0) return std::min(lab.spike_nc, 4);
        const long long waves = (long long)nleft * Q;
        return waves <= 3000 ? 1 : waves <= 6000 ? 2 : 3;
    }
    // Chains of three or more separators are eliminated from both ends by two workgroups each, which wait for each other through flags in global memory: both must be
    // RESIDENT.  A chain workgroup (1024 threads, > 100 KB of LDS) owns a compute unit, so the two-sided form is only used while all 2 x nchain workgroups fit the device
    // at once; beyond that the one-sided kernel runs (nothing waits on anything in it).
    bool chain_two_sided(int nchain) const { return lab.chain_twist && 2 * nchain <= num_cus; }
    // workgroups per ring elimination (band_ring.h, phase 3): three while the step leaves compute units idle, fewer when it fills the chip by itself
    int ring_elim_roles(int nodes) const {
        if (lab.ring_roles > 0) return lab.ring_roles;
        return (Q < 40) ? 1 : (3 * nodes <= num_cus ? 3 : (2 * nodes <= num_cus ? 2 : 1));
    }
};

// Bands too wide for the square window ring (6x6 blocks, half-width 21..30) keep an LDS-resident factorisation through the PACKED window of band_kernels2p.h (the live
// triangle only: 109 KB at half-width 26) and the single-wave back substitution with three task sets per lane; twisted components included (the planner twists up to
// half-width 30 when this path is on, ba_flatten.h: band_wide_max).  One connected ring of 300 cameras at half-width 26: 4.0 us per block row against 6.2 for the
// global-memory kernel (scripts/lab/chol_lab3.hip, profiles/r04_notes.md).  packed_enabled = SSFM_BAND_PACKED, 0 keeps the global-memory kernels.
inline bool band_wide_packed(int DC, int b, bool square, bool packed_enabled) {
    if (square || DC != 6 || b < 1 || !packed_enabled) return false;
    const int tasks2p = (b * (b + 1) / 2) * 4 - 4 + b * DC;
    return chol2p_lds_bytes(b, 2) <= 160 * 1024 && tasks2p <= 3 * 12 * 64 && b * 36 <= 2 * 1024 && (b + 1) * 36 + 2 * DC <= 9 * 128 && b * DC <= 192;
}

// substructured_plan: the handle's plan holds segments (BandSub::enabled); packed_enabled: SSFM_BAND_PACKED; num_cus: compute units of the device
inline BandPath band_path(int DC, int b, bool substructured_plan, bool packed_enabled, int num_cus, const BandPathLab& lab = BandPathLab()) {
    BandPath p; p.DC = DC; p.b = b; p.num_cus = num_cus; p.lab = lab;
    const int BB = DC * DC;
    const size_t lds_win = chol2_lds_bytes(DC, b, 2);
    const bool square = lds_win <= 140 * 1024 && b >= 1;
    const bool wide2p = band_wide_packed(DC, b, square, packed_enabled);
    // up to half-width 26 the 6x6-tile variant (one block per lane, twelve waves, 168 VGPRs): 3.45 against 4.02 us per block row at 26, 2.72 against 3.31 at 22
    const bool t6 = wide2p && (b * (b + 1) / 2 - 1 + b * DC) <= 8 * 64 && b * BB <= 2 * 768 && (b + 1) * BB + 2 * DC <= 8 * 128 && chol2p_lds_bytes(b, 2, true) <= 160 * 1024;
    // wave roles of k_band_chol_v2: 1 look-ahead + trailing-update waves (one block task per lane) + loaders + 1 writer
    // (block tasks and right-hand-side tasks on waves of their own when seven waves allow it: see the trailing role of the kernel)
    const int tpb = (DC % 3 == 0) ? (DC / 3) * (DC / 3) : DC * DC, blk_tasks = (b * (b + 1) / 2) * tpb - tpb, rhs_tasks = b * DC;
    const int tr_waves_split = (std::max(blk_tasks, 1) + 63) / 64 + (rhs_tasks + 63) / 64, tr_waves_packed = (blk_tasks + rhs_tasks + 63) / 64;
    const int ntw = std::min(std::max(tr_waves_split <= 7 ? tr_waves_split : tr_waves_packed, 1), 7);
    const int square_threads = 64 * (2 + CHOL2_LOADERS + ntw);
    if (t6) { p.factor = BAND_FACTOR_PACKED_T6; p.npb = 2; p.pre = 8; p.chol_lds = chol2p_lds_bytes(b, 2, true); p.chol_threads = 768; }
    else if (wide2p) {
        p.factor = BAND_FACTOR_PACKED3; p.chol_lds = chol2p_lds_bytes(b, 2); p.chol_threads = 1024;
        if (b * BB <= 1024 && (b + 1) * BB + 2 * DC <= 8 * 128) { p.npb = 1; p.pre = 8; } else { p.npb = 2; p.pre = 9; }
    } else if (square) {
        p.factor = BAND_FACTOR_SQUARE; p.chol_lds = lds_win; p.chol_threads = square_threads;
        p.chol_ntw = ntw; p.chol_heavy = tr_waves_split <= 7 ? (std::max(blk_tasks, 1) + 63) / 64 : ntw;
        p.chol_mf = (DC == 6 && b * DC <= 127) ? (lab.band_mfma & 3) : 0;
        p.chol_early = lab.band_early && p.chol_mf == 0 && b * BB <= BB + square_threads - 64;
    } else { p.factor = BAND_FACTOR_GLOBAL; p.chol_lds = band_chol_lds_bytes(DC, b, 2); p.chol_threads = 1024; }
    p.chol_map = (p.factor == BAND_FACTOR_SQUARE && lab.chol_wave_map) ?chol_wave_map(square_threads / 64, p.chol_ntw, p.chol_heavy) : chol_wave_map(0, 0, 0);
    // single-wave back substitution: up to two task sets per lane behind the square window, three behind the packed one
    const bool back_v2 = (square && b * DC <= 128) || wide2p;
    p.back_sets = !back_v2 ? 0 : b * DC > 128 ? 3 : b * DC > 64 ? 2 : 1;
    p.substructured = substructured_plan && p.lds_factor() && back_v2;
    p.Q = b * DC;
    // a second packed triangle when it fits (Q <= 96): the chain kernel then brings the next separator's D in while it factors this one (band_sub.h: pingpong)
    p.chain_pp = (lab.chain_pingpong && chain_lds_bytes(p.Q, 2, true) <= 160 * 1024) ? 1 : 0;
    p.chain_lds = chain_lds_bytes(p.Q, 2, p.chain_pp != 0);
    p.ring_back_threads = p.Q < 40 ? 256 : std::min(1024, std::max(256, ((RING_BACK_P * 2 * p.Q + 255) / 256) * 256));     // RING_BACK_P threads per entry of F^T x
    p.ring_cr_threads = p.Q > 48 ? 1024 : 512;            // (rows of the tall factorisation: 3 Q + 2 <= 256 either way; fewer waves make cheaper barriers)
    return p;
}

}  // namespace ssfm
