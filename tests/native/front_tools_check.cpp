// Host-side checks of the C++ mirror's find_largest_connected_component and read_features (spherical_sfm_amd/csrc/shim/tools.cpp) on hand-made cases.
// Stand-alone: built with the host compiler and -fsanitize=address,undefined together with shim/tools_host.cpp, the unit of the mirror that needs no library.
// Usage: front_tools_check <scratch directory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../spherical_sfm_amd/csrc/shim/tools.h"
using namespace sphericalsfm;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static Keyframe frame(int index, int nfeat) {
    Features f; f.points.resize(nfeat); f.descs.assign((size_t)nfeat * 128, 0.0f);
    for (int j = 0; j < nfeat; j++) { f.points[j].x = (float)(10 * index + j); f.points[j].y = (float)j; f.descs[(size_t)j * 128 + 5] = (float)(index + 1); }
    return Keyframe(index, "x", f);
}
static ImageMatch edge(int a, int b) { Matches m; m[(size_t)a] = (size_t)b; const Mat3 I = {1, 0, 0, 0, 1, 0, 0, 0, 1}; return ImageMatch(a, b, m, I); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: front_tools_check <dir>\n"); return 2; }
    {   // two components of equal size: {0, 2, 4} and {1, 3, 5}; the first (smallest vertex 0) wins; renumbering 0, 2, 4 -> 0, 1, 2
        std::vector<Keyframe> k; for (int i = 0; i < 6; i++) k.push_back(frame(i, 1));
        std::vector<ImageMatch> m = {edge(1, 3), edge(0, 2), edge(3, 5), edge(2, 4), edge(0, 4)};
        find_largest_connected_component(k, m);
        CHECK(k.size() == 3 && k[0].index == 0 && k[1].index == 2 && k[2].index == 4);
        CHECK(m.size() == 3 && m[0].index0 == 0 && m[0].index1 == 1 && m[1].index0 == 1 && m[1].index1 == 2 && m[2].index0 == 0 && m[2].index1 == 2);
        CHECK(m[0].matches.size() == 1 && m[0].matches.begin()->first == 0 && m[0].matches.begin()->second == 2);      // the feature matches travel untouched
    }
    {   // the larger component wins wherever it sits; an isolated trailing keyframe (6, named by no edge) and an isolated inner one (0) are dropped
        std::vector<Keyframe> k; for (int i = 0; i < 7; i++) k.push_back(frame(i, 1));
        std::vector<ImageMatch> m = {edge(1, 2), edge(3, 4), edge(4, 5)};
        find_largest_connected_component(k, m);
        CHECK(k.size() == 3 && k[0].index == 3 && k[1].index == 4 && k[2].index == 5);
        CHECK(m.size() == 2 && m[0].index0 == 0 && m[0].index1 == 1 && m[1].index0 == 1 && m[1].index1 == 2);
    }
    {   // an empty match list: nothing is connected, everything goes
        std::vector<Keyframe> k; for (int i = 0; i < 3; i++) k.push_back(frame(i, 1));
        std::vector<ImageMatch> m;
        find_largest_connected_component(k, m);
        CHECK(k.empty() && m.empty());
    }
    {   // an edge that names a vertex past the keyframes: the component is kept, no keyframe is read out of range
        std::vector<Keyframe> k; for (int i = 0; i < 2; i++) k.push_back(frame(i, 1));
        std::vector<ImageMatch> m = {edge(1, 3)};                        // vertices 0..3, component {1, 3}; only keyframe 1 of it exists
        find_largest_connected_component(k, m);
        CHECK(k.size() == 1 && k[0].index == 1 && m.empty());            // vertex 3 has no keyframe: its edge goes with it
    }
    {   // read_features: what write_feature_tracks wrote, without needing matches.dat
        const std::string dir = argv[1];
        std::vector<Keyframe> k = {frame(0, 3), frame(1, 0), frame(2, 2)};
        write_feature_tracks(dir, k, std::vector<ImageMatch>());
        std::remove((dir + "/matches.dat").c_str());
        std::vector<Keyframe> r;
        CHECK(read_features(dir, r));
        CHECK(r.size() == 3 && r[0].features.size() == 3 && r[1].features.size() == 0 && r[2].features.size() == 2 && r[2].index == 2);
        CHECK(r[2].features.points[1].x == 21.0f && r[2].features.descs[128 + 5] == 3.0f && r[0].features.descs.size() == 3 * 128);
        std::vector<Keyframe> r2; std::vector<ImageMatch> m2;
        CHECK(!read_feature_tracks(dir, r2, m2));                         // that one still needs matches.dat
        std::vector<Keyframe> r3;
        CHECK(!read_features(dir + "/nowhere", r3));
    }
    std::printf(fails ? "FRONT_TOOLS_CHECK failed=%d\n" : "FRONT_TOOLS_CHECK ok failed=%d\n", fails);
    return fails ? 1 : 0;
}
