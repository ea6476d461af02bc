// spherical_sfm_amd -- make_stereo_panoramas of the reference (examples/stereo_panorama_tools.cpp:404-637) over ssfm_pano_synthesize; the host steps are in
// stereo_panorama_tools_host.cpp.
#include "stereo_panorama_tools.h"
#include <cstdio>
#include <sys/stat.h>

namespace stereopanotools {

static std::string numbered(const std::string& dir, int index, const char* ext) {
    char name[32]; std::snprintf(name, sizeof name, "/%06d.%s", index, ext);
    return dir + name;
}
static bool is_dir(const std::string& p) { struct stat s; return stat(p.c_str(), &s) == 0 && S_ISDIR(s.st_mode); }

int make_stereo_panoramas(ssfm_ctx* ctx, const Intrinsics& intrinsics, const std::string& framespath, const std::string& outputpath, int panowidth, bool is_loop,
                          const ssfm_pano_options* options) {
    const std::string posespath = outputpath + "/poses.txt";
    std::vector<Keyframe> keyframes;
    std::printf("loading keyframes from %s...\n", posespath.c_str());
    if (!load_keyframes(posespath, keyframes)) { std::fprintf(stderr, "could not open %s\n", posespath.c_str()); return -1; }
    std::printf("loaded %zu keyframes\n", keyframes.size());
    if (keyframes.size() < 2) { std::fprintf(stderr, "need at least two keyframes\n"); return -1; }
    std::printf("estimating plane...\n");
    level_keyframes(keyframes);
    std::printf("computing thetas...\n");
    compute_thetas(keyframes);
    std::printf("re-ordering...\n");
    trim_loop(keyframes, is_loop);
    const int n = (int)keyframes.size();
    std::printf("%d keyframes after trimming\n", n);

    std::printf("loading images...\n");
    int width = 0, height = 0;
    for (int i = 0; i < n; i++) {
        int w = 0, h = 0;
        const std::string path = numbered(framespath, keyframes[i].index, "ppm");
        if (!read_ppm(path, w, h, keyframes[i].image)) { std::fprintf(stderr, "could not read %s\n", path.c_str()); return -1; }
        if (i == 0) { width = w; height = h; }
        if (w != width || h != height) { std::fprintf(stderr, "%s: %d x %d, the first frame is %d x %d\n", path.c_str(), w, h, width, height); return -1; }
    }
    ssfm_pano_options opt;
    if (options) opt = *options; else ssfm_pano_default_options(&opt);
    opt.is_loop = is_loop ? 1 : 0; opt.on_device = 0;
    const int pairs = is_loop ? n : n - 1;
    const std::string fwd_dir = outputpath + "/flow_fwd", bwd_dir = outputpath + "/flow_bwd";
    const bool have_fwd = is_dir(fwd_dir), have_bwd = is_dir(bwd_dir);
    if (have_fwd != have_bwd) { std::fprintf(stderr, "flow_fwd and flow_bwd must both be there, or neither\n"); return -1; }
    std::vector<std::vector<float>> fwd((size_t)n), bwd((size_t)n);
    if (have_fwd) {
        for (int k = 0; k < pairs; k++) {
            for (int dir = 0; dir < 2; dir++) {
                int w = 0, h = 0;
                const std::string path = numbered(dir == 0 ? fwd_dir : bwd_dir, keyframes[k].index, "flo");
                if (!read_flo(path, w, h, dir == 0 ? fwd[(size_t)k] : bwd[(size_t)k]) || w != width || h != height) {
                    std::fprintf(stderr, "could not read a %d x %d flow from %s\n", width, height, path.c_str()); return -1;
                }
            }
        }
    }
    std::vector<double> R(9 * (size_t)n), t(3 * (size_t)n);
    std::vector<const uint8_t*> frames((size_t)n); std::vector<const float*> pf((size_t)n, nullptr), pb((size_t)n, nullptr);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 9; k++) R[9 * (size_t)i + k] = keyframes[i].R[k];
        for (int k = 0; k < 3; k++) t[3 * (size_t)i + k] = keyframes[i].t[k];
        frames[(size_t)i] = keyframes[i].image.data();
        if (have_fwd && i < pairs) { pf[(size_t)i] = fwd[(size_t)i].data(); pb[(size_t)i] = bwd[(size_t)i].data(); }
    }
    {
        const std::string path = outputpath + "/levelled.txt";
        FILE* f = std::fopen(path.c_str(), "w");
        if (!f) { std::fprintf(stderr, "could not write %s\n", path.c_str()); return -1; }
        for (int i = 0; i < n; i++) {
            std::fprintf(f, "%d", keyframes[i].index);
            for (int k = 0; k < 9; k++) std::fprintf(f, " %.17g", keyframes[i].R[k]);
            for (int k = 0; k < 3; k++) std::fprintf(f, " %.17g", keyframes[i].t[k]);
            std::fprintf(f, "\n");
        }
        std::fclose(f);
    }
    std::printf("interpolating frames...\n");
    std::vector<uint8_t> panoramas((size_t)opt.num_phi * (size_t)height * (size_t)panowidth * 3);
    const int rc = ssfm_pano_synthesize(ctx, &opt, n, R.data(), t.data(), intrinsics.focal, intrinsics.centerx, intrinsics.centery, width, height, frames.data(),
                                        have_fwd ? pf.data() : nullptr, have_fwd ? pb.data() : nullptr, panowidth, panoramas.data(), nullptr);
    if (rc != SSFM_OK) { std::fprintf(stderr, "ssfm_pano_synthesize: %s\n", ssfm_last_error(ctx)); return rc; }
    double ms = 0; ssfm_pano_last_kernel_ms(ctx, &ms);
    std::printf("kernel time %.3f ms\n", ms);
    for (int phinum = 0; phinum < opt.num_phi; phinum++) {
        const std::string path = outputpath + "/cylindrical" + std::to_string(phinum) + ".ppm";
        if (!write_ppm(path, panowidth, height, panoramas.data() + (size_t)phinum * (size_t)height * (size_t)panowidth * 3)) { std::fprintf(stderr, "could not write %s\n", path.c_str()); return -1; }
    }
    return 0;
}

}  // namespace stereopanotools
