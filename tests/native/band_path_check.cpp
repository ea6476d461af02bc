// The plan of the reduced-system solve (csrc/band_path.h) over every camera block size and half-width: which factorisation and back substitution a band gets,
// with how many threads and how much LDS -- the landmarks of the shipped decision, and the launch contracts the kernels state in their headers.
// Stand-alone: includes band_path.h only.  Prints BAND_PATH_OK.
#include <cstdio>
#include <cstring>
#include "../../spherical_sfm_amd/csrc/band_path.h"

using namespace ssfm;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed++; std::printf("FAILED %s:%d  %s  [", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("]\n"); } } while (0)

static int in_range(int b, int lo, int hi) { return b >= lo && b <= hi; }

// factorisation threads of the square window: 64 x (look-ahead + trailing waves + two loaders + writer)
static int square_threads_dc6(int b) { return b <= 5 ? 384 : b <= 7 ? 448 : b <= 9 ? 512 : b <= 10 ? 576 : 704; }
static int square_threads_dc3(int b) { return b <= 10 ? 384 : b <= 15 ? 448 : b <= 19 ? 512 : b <= 21 ? 576 : b <= 22 ? 640 : 704; }

int main() {
    const size_t LDS_MAX = 160 * 1024;
    const int num_cus = 256;
    for (int DC : {3, 6}) for (int b = 1; b <= 64; b++) for (int packed_on = 0; packed_on < 2; packed_on++) for (int sub = 0; sub < 2; sub++) {
        const BandPath p = band_path(DC, b, sub != 0, packed_on != 0, num_cus);
        const int Q = b * DC;
        // ---- landmarks
        BandFactor want;
        if (DC == 6) want = b <= 20 ? BAND_FACTOR_SQUARE : (!packed_on || b > 30) ? BAND_FACTOR_GLOBAL : b <= 26 ? BAND_FACTOR_PACKED_T6 : BAND_FACTOR_PACKED3;
        else want = b <= 42 ? BAND_FACTOR_SQUARE : BAND_FACTOR_GLOBAL;
        CHECK(p.factor == want, "DC %d b %d packed %d: factor %d, expected %d", DC, b, packed_on, (int)p.factor, (int)want);
        if (want == BAND_FACTOR_SQUARE) CHECK(p.chol_threads == (DC == 6 ? square_threads_dc6(b) : square_threads_dc3(b)), "DC %d b %d: %d threads", DC, b, p.chol_threads);
        if (want == BAND_FACTOR_PACKED_T6) CHECK(p.chol_threads == 768 && p.npb == 2 && p.pre == 8, "b %d: T6 with %d threads <.., %d, %d>", b, p.chol_threads, p.npb, p.pre);
        if (want == BAND_FACTOR_PACKED3) {
            CHECK(p.chol_threads == 1024, "b %d: %d threads", b, p.chol_threads);
            if (b == 27) CHECK(p.npb == 1 && p.pre == 8, "b 27: <2, 3, %d, %d>", p.npb, p.pre);
            if (in_range(b, 28, 30)) CHECK(p.npb == 2 && p.pre == 9, "b %d: <2, 3, %d, %d>", b, p.npb, p.pre);
        }
        if (DC == 6 && p.lds_factor()) CHECK(p.back_sets == (b <= 10 ? 1 : b <= 21 ? 2 : 3), "b %d: %d task sets", b, p.back_sets);
        // ---- exactly one factorisation kind, and what belongs to it
        const int kinds = (p.factor == BAND_FACTOR_GLOBAL) + (p.factor == BAND_FACTOR_SQUARE) + (p.factor == BAND_FACTOR_PACKED3) + (p.factor == BAND_FACTOR_PACKED_T6);
        CHECK(kinds == 1, "DC %d b %d: %d kinds", DC, b, kinds);
        CHECK(p.lds_factor() == (p.factor != BAND_FACTOR_GLOBAL) && p.packed() == (p.factor == BAND_FACTOR_PACKED3 || p.factor == BAND_FACTOR_PACKED_T6), "DC %d b %d", DC, b);
        if (p.packed()) CHECK(DC == 6 && packed_on, "DC %d b %d packed %d", DC, b, packed_on);
        // ---- every dynamic-LDS request fits a compute unit
        CHECK(p.chol_lds <= LDS_MAX, "DC %d b %d: factorisation asks for %zu bytes", DC, b, p.chol_lds);
        CHECK(p.subst_lds(1) <= LDS_MAX && p.subst_lds(2) <= LDS_MAX, "DC %d b %d: substitution asks for %zu bytes", DC, b, p.subst_lds(2));
        if (p.factor == BAND_FACTOR_SQUARE) CHECK(p.chol_lds == chol2_lds_bytes(DC, b, 2) && p.chol_lds <= 140 * 1024, "DC %d b %d", DC, b);
        if (p.factor == BAND_FACTOR_PACKED3) CHECK(p.chol_lds == chol2p_lds_bytes(b, 2), "b %d", b);
        if (p.factor == BAND_FACTOR_PACKED_T6) CHECK(p.chol_lds == chol2p_lds_bytes(b, 2, true), "b %d", b);
        if (p.factor == BAND_FACTOR_GLOBAL) CHECK(p.chol_lds == band_chol_lds_bytes(DC, b, 2), "DC %d b %d", DC, b);
        if (p.substructured) {
            CHECK(p.Q == Q && p.apply_lds() <= LDS_MAX, "DC %d b %d: apply asks for %zu bytes", DC, b, p.apply_lds());
            // the planner cuts a component into a chain of segments only while a separator block fits the chain kernel (band_sub.h, sub_build: b DC <= 114);
            // wider substructured plans hold twisted components only and never launch the chain
            if (Q <= 114) CHECK(p.chain_lds <= LDS_MAX && p.chain_lds == chain_lds_bytes(Q, 2, p.chain_pp != 0), "DC %d b %d: chain asks for %zu bytes", DC, b, p.chain_lds);
            CHECK((p.chain_pp != 0) == (chain_lds_bytes(Q, 2, true) <= LDS_MAX), "DC %d b %d: ping-pong %d", DC, b, p.chain_pp);
            CHECK(p.ring_cr_threads == (Q > 48 ? 1024 : 512) && p.ring_back_threads % 256 == 0 && p.ring_back_threads >= 256 && p.ring_back_threads <= 1024, "DC %d b %d", DC, b);
        }
        // ---- launch bounds and header contracts of the kernels
        if (p.factor == BAND_FACTOR_SQUARE) {
            CHECK(p.chol_threads <= 768 && p.chol_threads == 64 * (2 + CHOL2_LOADERS + p.chol_ntw) && p.chol_ntw >= 1 && p.chol_heavy >= 1 && p.chol_heavy <= p.chol_ntw, "DC %d b %d", DC, b);
            // nine waves are remapped, every other shape keeps the identity; either way a permutation of the roles
            bool seen[16] = {false}; bool identity = true;
            for (int w = 0; w < 16; w++) { CHECK(p.chol_map.v[w] < 16 && !seen[p.chol_map.v[w]], "DC %d b %d: wave map", DC, b); seen[p.chol_map.v[w] & 15] = true; identity = identity && p.chol_map.v[w] == w; }
            CHECK(identity == (p.chol_threads != 9 * 64) && p.chol_map.v[0] == 0, "DC %d b %d: wave map of %d waves", DC, b, p.chol_threads / 64);
            CHECK(p.chol_mf == 0 && !p.chol_early, "DC %d b %d: lab variants in the shipped plan", DC, b);
        }
        if (p.packed()) {
            const bool t6 = p.factor == BAND_FACTOR_PACKED_T6;
            CHECK(p.chol_threads <= (t6 ? 768 : 1024), "b %d", b);
            CHECK(p.npb * p.chol_threads >= 36 * b, "b %d: NPB %d x %d threads < 36 b", b, p.npb, p.chol_threads);
            CHECK(p.pre * 128 >= 36 * (b + 1) + 12, "b %d: PRE %d", b, p.pre);
            const int ntw = p.chol_threads / 64 - 2 - 2;           // look-ahead, two loaders, writer
            if (t6) CHECK(64 * ntw >= b * (b + 1) / 2 - 1 + 6 * b, "b %d: one 6x6 block per lane", b);
            else CHECK(3 * 64 * ntw >= 4 * (b * (b + 1) / 2 - 1) + 6 * b, "b %d: three 3x3 tiles per lane", b);
        }
        // ---- back substitution: the single wave serves every LDS-resident factorisation (no band reaches a wider back substitution in LDS), with enough task sets
        CHECK((p.back_sets > 0) == p.lds_factor(), "DC %d b %d: %d task sets behind factor %d", DC, b, p.back_sets, (int)p.factor);
        if (p.back_sets > 0) CHECK(p.back_sets <= 3 && 64 * p.back_sets >= Q && (p.back_sets == 1 || 64 * (p.back_sets - 1) < Q), "DC %d b %d: %d task sets", DC, b, p.back_sets);
        // ---- the substructured path and the refactor rule
        CHECK(p.substructured == (sub && p.lds_factor()) && p.needs_refactor() == p.substructured, "DC %d b %d sub %d", DC, b, sub);
    }
    // ---- the rules that look at the plan's counts
    {
        const BandPath p = band_path(6, 10, true, true, 256);
        CHECK(p.chain_two_sided(128) && !p.chain_two_sided(129), "two-sided chains while 2 nchain <= compute units");
        CHECK(p.spike_cols(50) == 1 && p.spike_cols(51) == 2 && p.spike_cols(100) == 2 && p.spike_cols(101) == 3, "spike columns per wave at 3000 / 6000 waves");
        CHECK(p.ring_elim_roles(85) == 3 && p.ring_elim_roles(86) == 2 && p.ring_elim_roles(128) == 2 && p.ring_elim_roles(129) == 1, "ring roles at Q = 60");
        CHECK(band_path(6, 6, true, true, 256).ring_elim_roles(1) == 1, "ring roles below Q = 40");
        CHECK(!p.fused_factor(4, 2), "fused factorisation is a lab variant");
        BandPathLab lab; lab.chol_fuse = true; lab.spike_nc = 7; lab.ring_roles = 4; lab.chain_twist = false; lab.chain_pingpong = false; lab.band_mfma = 3; lab.chol_wave_map = false;
        const BandPath q = band_path(6, 10, true, true, 256, lab);
        CHECK(q.fused_factor(4, 2) && !q.fused_factor(255, 2) && !q.fused_factor(4, 0), "fused factorisation: resident workgroups only");
        CHECK(q.spike_cols(1) == 4 && q.ring_elim_roles(1000) == 4 && !q.chain_two_sided(1) && q.chain_pp == 0 && q.chain_lds == chain_lds_bytes(60, 2, false), "lab overrides");
        CHECK(q.chol_mf == 3 && q.chol_map.v[1] == 1 && q.chol_map.v[4] == 4, "lab overrides of the factorisation");
        CHECK(band_path(6, 22, false, true, 256, lab).chol_mf == 0, "the packed window has no matrix-core variant");
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("BAND_PATH_OK\n");
    return 0;
}
