// Drives aria::adapters::hip::HipRectifier with a fisheye (KB4) camera from tests/test_cpp_fisheye.py:
//   rect_kb4_selftest <dataset> <map.bin> <kp.bin> <kp_out.bin> <dst_w> <dst_h> <fx'> <fy'> <cx'> <cy'>
//       dataset: an ASL tree with mav0/cam0/sensor.yaml. Prints "cal <27 numbers>" and "model <name> <rectModel()>" as the
//       reader parsed them, builds the one-camera rectifier with that model, writes the map words to map.bin, moves the
//       keypoint records of kp.bin into kp_out.bin, and prints DONE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "aria_hip/AslSequence.hpp"
#include "aria_hip/HipRectifier.hpp"

using namespace aria;

int main(int argc, char** argv) {
    if (argc < 11) { std::fprintf(stderr, "usage: rect_kb4_selftest <dataset> <map> <kp> <kp_out> <dw> <dh> <fx> <fy> <cx> <cy>\n"); return 2; }
    try {
        io::AslSequence seq;
        if (!seq.load(argv[1]) || !seq.hasCalibration(0)) { std::fprintf(stderr, "cannot load %s with a cam0 calibration\n", argv[1]); return 2; }
        const io::AslCalibration& cal = seq.calibration(0);
        std::printf("cal");
        for (double v : cal.intrinsics) std::printf(" %.17g", v);
        for (double v : cal.distortion) std::printf(" %.17g", v);
        for (double v : cal.T_BS) std::printf(" %.17g", v);
        std::printf(" %d %d\n", cal.width, cal.height);
        std::printf("model %s %d\n", cal.distortion_model.c_str(), cal.rectModel());
        adapters::hip::RectifierConfig rc;
        rc.model = cal.rectModel();
        rc.cam[0].K = adapters::hip::PoseIntrinsics{cal.intrinsics[0], cal.intrinsics[1], cal.intrinsics[2], cal.intrinsics[3]};
        std::memcpy(rc.cam[0].dist, cal.distortion, sizeof(cal.distortion));
        rc.src_width = cal.width;
        rc.src_height = cal.height;
        rc.dst_width = std::stoi(argv[5]);
        rc.dst_height = std::stoi(argv[6]);
        for (int k = 0; k < 4; k++) rc.new_K[k] = std::stod(argv[7 + k]);
        adapters::hip::HipRectifier rect(rc);
        if (rect.config().model != ARIA_RECT_MODEL_KB4) { std::fprintf(stderr, "the handle is not KB4\n"); return 2; }
        const std::vector<std::uint32_t> m = rect.map(0);
        std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char*>(m.data()), (std::streamsize)(m.size() * 4));
        std::ifstream in(argv[3], std::ios::binary);
        const std::vector<char> kp_bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::vector<core::KeyPoint> kps(kp_bytes.size() / sizeof(core::KeyPoint));
        std::memcpy(kps.data(), kp_bytes.data(), kps.size() * sizeof(core::KeyPoint));
        rect.points(0, kps);
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char*>(kps.data()), (std::streamsize)(kps.size() * sizeof(core::KeyPoint)));
        std::printf("DONE\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
