// spherical_sfm_amd -- drop-in for the reference's examples/make_stereo_panorama.cpp without gflags, OpenCV or a video decoder:
//   make_stereo_panorama --intrinsics <file: focal centerx centery> --frames <dir with %06d.ppm> --output <dir with poses.txt> [--width 8192] [--noloop]
//                        [--nphi 9] [--subpixel]
// Optional optical flow is read from <output>/flow_fwd/%06d.flo and <output>/flow_bwd/%06d.flo; the panoramas go to <output>/cylindrical<phinum>.ppm.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include "stereo_panorama_tools.h"

using namespace stereopanotools;

int main(int argc, char** argv) {
    std::string intrinsics_path, frames, output;
    int width = 8192, nphi = 9; bool loop = true, subpixel = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--intrinsics") intrinsics_path = value();
        else if (a == "--frames") frames = value();
        else if (a == "--output") output = value();
        else if (a == "--width") width = std::atoi(value());
        else if (a == "--nphi") nphi = std::atoi(value());
        else if (a == "--noloop") loop = false;
        else if (a == "--loop") loop = true;
        else if (a == "--subpixel") subpixel = true;
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (intrinsics_path.empty() || frames.empty() || output.empty()) { std::fprintf(stderr, "usage: make_stereo_panorama --intrinsics F --frames DIR --output DIR [--width N] [--noloop] [--nphi N] [--subpixel]\n"); return 2; }
    double focal = 0, centerx = 0, centery = 0;
    std::ifstream intrinsicsf(intrinsics_path);
    if (!(intrinsicsf >> focal >> centerx >> centery)) { std::fprintf(stderr, "could not read %s\n", intrinsics_path.c_str()); return 2; }
    std::cout << "intrinsics : " << focal << ", " << centerx << ", " << centery << "\n";
    ssfm_ctx* ctx = nullptr;
    if (ssfm_ctx_create(-1, nullptr, &ctx) != SSFM_OK) { std::fprintf(stderr, "ssfm_ctx_create: %s\n", ssfm_last_error(nullptr)); return 1; }
    ssfm_pano_options opt; ssfm_pano_default_options(&opt);
    opt.num_phi = nphi; opt.subpixel_bits = subpixel ? 5 : 0;
    const Intrinsics intrinsics{focal, centerx, centery};
    const int rc = make_stereo_panoramas(ctx, intrinsics, frames, output, width, loop, &opt);
    ssfm_ctx_destroy(ctx);
    return rc == 0 ? 0 : 1;
}
