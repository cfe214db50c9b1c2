// Drives aria::adapters::hip::HipObjectDetector and the FrontEnd's injected detector from tests/test_gpu_detect.py and
// tests/test_detect_host.py:
//   det_selftest nogpu
//       constructs the adapter where no device is usable: it must throw, naming the status. Prints "OK nogpu".
//   det_selftest run <rawfile> <seed> <width> <height>
//       rawfile: rows of 6 floats [x1 y1 x2 y2 confidence class_id] -- the fixed table the inference hook writes as the
//       network's output for every frame. Frames are the synthetic pair of <seed>. Prints
//         "det <i> <x1> <y1> <x2> <y2> <confidence bits> <class_id>" per detection of frame A (detectGray),
//         "rgb_same", "async_same": detect() on the replicated RGB image / detectGrayAsync + getDetections give the same,
//         "nboxes <n>": the dynamic-class list deviceBoxes() left in HBM,
//         "fe <injected|byhand> <frame> <matches> <filtered> <fnv of the match bytes>" for three frames through two FrontEnds,
//         one with the detector injected, one fed setDetections() by hand with the same detector's output,
//       and DONE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "aria_hip/HipFactory.hpp"
#include "aria_hip/HipObjectDetector.hpp"

using namespace aria;

static unsigned long long fnv(const void* p, std::size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (std::size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

static bool same(const std::vector<core::Detection>& a, const std::vector<core::Detection>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(core::Detection)));
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "nogpu")) {
        try {
            adapters::hip::HipObjectDetector d([](const void*, void*, int, void*) {});
            std::printf("constructed: a device is present\n");
            return 1;
        } catch (const std::exception& e) {
            std::printf("%s\n", e.what());
            if (!std::strstr(e.what(), "no usable HIP device")) return 1;
        }
        std::printf("OK nogpu\n");
        return 0;
    }
    if (argc < 6 || std::strcmp(argv[1], "run")) { std::fprintf(stderr, "usage: det_selftest nogpu | run <rawfile> <seed> <w> <h>\n"); return 2; }
    try {
        std::vector<float> table;
        {
            std::ifstream in(argv[2]);
            float v;
            while (in >> v) table.push_back(v);
        }
        const int n_cand = (int)(table.size() / 6);
        const unsigned long long seed = std::stoull(argv[3]);
        const int W = std::stoi(argv[4]), H = std::stoi(argv[5]);
        std::vector<std::uint8_t> a((std::size_t)W * H), b(a.size());
        if (aria_synth_frame_pair(seed, W, H, a.data(), b.data()) != ARIA_OK) return 2;
        adapters::hip::ObjectDetectorConfig dc;
        dc.max_candidates = n_cand;
        auto hook = [&table, n_cand](const void*, void* d_output, int batch, void* stream) {
            for (int f = 0; f < batch; f++)
                aria_copy_h2d_async(0, stream, (float*)d_output + (std::size_t)f * n_cand * 6, table.data(), table.size() * sizeof(float));
        };
        adapters::hip::HipObjectDetector det(hook, dc);
        std::vector<core::Detection> d0, d1, d2;
        det.detectGray(a.data(), W, H, d0);
        for (std::size_t i = 0; i < d0.size(); i++) {
            unsigned bits;
            std::memcpy(&bits, &d0[i].confidence, 4);
            std::printf("det %zu %.9g %.9g %.9g %.9g %08x %d\n", i, d0[i].x1, d0[i].y1, d0[i].x2, d0[i].y2, bits, d0[i].class_id);
        }
        int nb = -1;
        aria_copy_d2h_async(0, det.stream(), &nb, det.deviceBoxes().n_boxes, sizeof(int));
        det.sync();
        std::printf("nboxes %d\n", nb);
        std::vector<std::uint8_t> rgb(a.size() * 3);
        for (std::size_t i = 0; i < a.size(); i++) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = a[i];
        det.detect(rgb.data(), W, H, d1);
        std::printf("rgb_same %d\n", (int)same(d0, d1));
        det.detectGrayAsync(a.data(), W, H);
        det.sync();
        det.getDetections(d2);
        std::printf("async_same %d\n", (int)same(d0, d2));
        std::printf("check %d\n", det.check());

        factory::HipFactoryConfig fc;
        fc.max_features = 1000;
        fc.enable_loop_closure = false;
        auto fe_injected = factory::createHip(fc, hook, dc);
        auto fe_byhand = factory::createHip(fc);
        const std::uint8_t* frames[3] = {a.data(), b.data(), a.data()};
        bool fe_same = true;
        for (int k = 0; k < 3; k++) {
            const pipeline::FrontEndResult& r1 = fe_injected->processFrame(frames[k], W, H, 0.05 * k);
            std::vector<core::Detection> dk;
            det.detectGray(frames[k], W, H, dk);
            fe_byhand->setDetections(dk);
            const pipeline::FrontEndResult& r2 = fe_byhand->processFrame(frames[k], W, H, 0.05 * k);
            const unsigned long long h1 = fnv(r1.matches.data(), r1.matches.size() * sizeof(core::Match));
            const unsigned long long h2 = fnv(r2.matches.data(), r2.matches.size() * sizeof(core::Match));
            std::printf("fe injected %d %zu %d %016llx\n", k, r1.matches.size(), r1.filtered_count, h1);
            std::printf("fe byhand %d %zu %d %016llx\n", k, r2.matches.size(), r2.filtered_count, h2);
            fe_same = fe_same && h1 == h2 && r1.matches.size() == r2.matches.size() && r1.filtered_count == r2.filtered_count;
        }
        std::printf("fe_same %d\n", (int)fe_same);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("DONE\n");
    return 0;
}
