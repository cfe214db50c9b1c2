// Drives aria::adapters::hip::HipRectifier and aria::io::AslSequence's calibration reader from tests/test_cpp_rectify.py:
//   rect_selftest <dataset> <frames.bin> <out.bin> <kp.bin> <kp_out.bin> <n_frames> <dst_w> <dst_h> <fx'> <fy'> <cx'> <cy'> <fill>
//       dataset: an ASL tree with mav0/cam0/sensor.yaml and mav0/cam1/sensor.yaml. Prints "cal <cam> <27 numbers>" as the
//       reader parsed them (intrinsics, distortion, T_BS, resolution), builds the two-camera rectifier from them, prints
//       "baseline <b>", "newK <4 numbers>" and "map <cam> <fnv of the map words>", remaps the 2 x n_frames raw images of
//       frames.bin (camera-major, tightly packed at the calibration's resolution) into out.bin, moves the keypoint records of
//       kp.bin through both cameras into kp_out.bin (camera-major), and prints DONE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "aria_hip/AslSequence.hpp"
#include "aria_hip/HipRectifier.hpp"

using namespace aria;

static unsigned long long fnv(const void* p, std::size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (std::size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

static std::vector<std::uint8_t> slurp(const char* path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<std::uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 14) { std::fprintf(stderr, "usage: rect_selftest <dataset> <frames> <out> <kp> <kp_out> <n> <dw> <dh> <fx> <fy> <cx> <cy> <fill>\n"); return 2; }
    try {
        io::AslSequence seq;
        if (!seq.load(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
        adapters::hip::RectifierConfig rc;
        rc.n_cameras = 2;
        for (int c = 0; c < 2; c++) {
            if (!seq.hasCalibration(c)) { std::fprintf(stderr, "no calibration for cam%d\n", c); return 2; }
            const io::AslCalibration& cal = seq.calibration(c);
            std::printf("cal %d", c);
            for (double v : cal.intrinsics) std::printf(" %.17g", v);
            for (double v : cal.distortion) std::printf(" %.17g", v);
            for (double v : cal.T_BS) std::printf(" %.17g", v);
            std::printf(" %d %d\n", cal.width, cal.height);
            rc.cam[c].K = adapters::hip::PoseIntrinsics{cal.intrinsics[0], cal.intrinsics[1], cal.intrinsics[2], cal.intrinsics[3]};
            std::memcpy(rc.cam[c].dist, cal.distortion, sizeof(cal.distortion));
            std::memcpy(rc.cam[c].T_BS, cal.T_BS, sizeof(cal.T_BS));
        }
        rc.src_width = seq.calibration(0).width;
        rc.src_height = seq.calibration(0).height;
        const int n = std::stoi(argv[6]);
        rc.dst_width = std::stoi(argv[7]);
        rc.dst_height = std::stoi(argv[8]);
        for (int k = 0; k < 4; k++) rc.new_K[k] = std::stod(argv[9 + k]);
        rc.fill = std::stoi(argv[13]);
        adapters::hip::HipRectifier rect(rc);
        std::printf("baseline %.17g\n", rect.baseline());
        const adapters::hip::PoseIntrinsics nk = rect.newK();
        std::printf("newK %.17g %.17g %.17g %.17g\n", nk.fx, nk.fy, nk.cx, nk.cy);
        for (int c = 0; c < 2; c++) {
            const std::vector<std::uint32_t> m = rect.map(c);
            std::printf("map %d %llu\n", c, fnv(m.data(), m.size() * 4));
        }
        const std::vector<std::uint8_t> frames = slurp(argv[2]);
        const std::size_t px = (std::size_t)rc.src_width * rc.src_height;
        if (frames.size() != 2 * (std::size_t)n * px) { std::fprintf(stderr, "frames.bin has the wrong size\n"); return 2; }
        std::ofstream out(argv[3], std::ios::binary);
        std::vector<std::uint8_t> dst;
        for (int c = 0; c < 2; c++)
            for (int f = 0; f < n; f++) {
                rect.remap(c, frames.data() + ((std::size_t)c * n + f) * px, dst);
                out.write(reinterpret_cast<const char*>(dst.data()), (std::streamsize)dst.size());
            }
        const std::vector<std::uint8_t> kp_bytes = slurp(argv[4]);
        std::ofstream kp_out(argv[5], std::ios::binary);
        for (int c = 0; c < 2; c++) {
            std::vector<core::KeyPoint> kps(kp_bytes.size() / sizeof(core::KeyPoint));
            std::memcpy(kps.data(), kp_bytes.data(), kps.size() * sizeof(core::KeyPoint));
            rect.points(c, kps);
            kp_out.write(reinterpret_cast<const char*>(kps.data()), (std::streamsize)(kps.size() * sizeof(core::KeyPoint)));
        }
        std::printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
