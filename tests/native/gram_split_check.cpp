// csrc/gram_path.h, gram_share: the share [s_begin, s_end) of a Gram task's cnt points that wave w of W takes (k_schur_gram with the task split over a workgroup).
// Stand-alone, under UBSan (tests/test_gram_split_cpu.py).  For cnt in 1..200 and W in 1..4:
//   the shares are disjoint, in wave order, and cover [0, cnt);
//   every share is made of whole sub-chunks of 8 points, except that the task's last sub-chunk may be partial;
//   some share is empty exactly when W exceeds the number of sub-chunks; the longest share is ceil(sub-chunks / W).
#include <cstdio>
#include <vector>

#include "../../spherical_sfm_amd/csrc/gram_path.h"

int main() {
    constexpr int GRAM_SHARE_SUB = ssfm::GRAM_SUB_PTS; using ssfm::gram_share;
    int bad = 0, checked = 0;
    auto fail = [&](const char* what, int cnt, int W, int w, int b, int e) { if (bad++ < 20) std::printf("FAIL %s: cnt %d W %d w %d share [%d, %d)\n", what, cnt, W, w, b, e); };
    for (int cnt = 1; cnt <= 200; cnt++)
        for (int W = 1; W <= 4; W++) {
            const int nsub = (cnt + GRAM_SHARE_SUB - 1) / GRAM_SHARE_SUB;
            std::vector<int> owner(cnt, -1);
            int next = 0, empty = 0, longest = 0;
            for (int w = 0; w < W; w++) {
                int b = -1, e = -1; gram_share(cnt, W, w, b, e); checked++;
                if (b < 0 || e < b || e > cnt) { fail("range", cnt, W, w, b, e); continue; }
                if (b != next) fail("not contiguous with the share before it", cnt, W, w, b, e);
                next = e;
                for (int q = b; q < e; q++) { if (owner[q] != -1) fail("overlap", cnt, W, w, b, e); owner[q] = w; }
                if (e == b) { empty++; continue; }
                if (b % GRAM_SHARE_SUB != 0) fail("begins inside a sub-chunk", cnt, W, w, b, e);
                if (e % GRAM_SHARE_SUB != 0 && e != cnt) fail("ends inside a sub-chunk that is not the task's last", cnt, W, w, b, e);
                const int n = (e - b + GRAM_SHARE_SUB - 1) / GRAM_SHARE_SUB; if (n > longest) longest = n;
            }
            if (next != cnt) fail("does not reach the end", cnt, W, W - 1, next, cnt);
            for (int q = 0; q < cnt; q++) if (owner[q] == -1) { fail("point not covered", cnt, W, -1, q, q + 1); break; }
            if ((empty > 0) != (W > nsub)) fail("empty shares", cnt, W, -1, empty, nsub);
            if (longest != (nsub + W - 1) / W) fail("longest share", cnt, W, -1, longest, nsub);
        }
    // the shapes the GPU tests rely on (tests/test_gram_split_gpu.py)
    { int b, e; gram_share(8, 2, 1, b, e); if (b != e) fail("8 points on 2 waves: the second share is empty", 8, 2, 1, b, e); }
    { int b, e; gram_share(25, 4, 3, b, e); if (b != 24 || e != 25) fail("25 points on 4 waves: the last share is one point", 25, 4, 3, b, e); }
    { int b, e; gram_share(101, 2, 0, b, e); if (b != 0 || e != 56) fail("101 points on 2 waves: 7 + 6 sub-chunks", 101, 2, 0, b, e); }
    std::printf("%d shares checked, %d failures\n", checked, bad);
    if (bad == 0) std::printf("GRAM_SPLIT_OK\n");
    return bad == 0 ? 0 : 1;
}
