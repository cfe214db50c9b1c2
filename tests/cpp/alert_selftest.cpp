// Drives aria_hip/HipObstacleAlerter.hpp with a RecordingAudioFeedback over a sequence read from a file (tests/test_cpp_alert.py):
//   alert_selftest host|device <in.bin>
// in.bin: int32 width, height, n_frames, n_names; n_names lines of 16 bytes (NUL-padded); per frame: int64 timestamp_ns, int32 n_dets,
// n_dets aria_detection records, width * height floats. Prints one line per event ("event frame source class_id direction priority
// distance flags") followed by the lines the mock recorded for it, and at the end "state <events_total>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "aria_hip/HipFactory.hpp"
#include "aria_hip/HipObstacleAlerter.hpp"

using namespace aria;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const bool device = !std::strcmp(argv[1], "device");
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::int32_t hdr[4];
    if (std::fread(hdr, 4, 4, f) != 4) return 2;
    const int W = hdr[0], H = hdr[1], n_frames = hdr[2], n_names = hdr[3];
    std::vector<std::string> names;
    for (int i = 0; i < n_names; i++) {
        char buf[17] = {0};
        if (std::fread(buf, 1, 16, f) != 16) return 2;
        names.emplace_back(buf);
    }
    try {
        adapters::hip::RecordingAudioFeedback audio;
        audio.initialize();
        adapters::hip::ObstacleAlerterConfig ac;
        ac.width = W;
        ac.height = H;
        ac.min_valid = 4;
        factory::HipFactoryConfig fc;
        std::unique_ptr<adapters::hip::HipObstacleAlerter> alerter = factory::createHipAlerter(fc, &audio, names, ac);
        void *d_depth = nullptr, *d_dets = nullptr, *d_n = nullptr;
        void* st = aria_alert_stream(alerter->handle());
        if (device && (aria_device_alloc(0, sizeof(float) * W * H, &d_depth) != ARIA_OK || aria_device_alloc(0, sizeof(aria_detection) * 64, &d_dets) != ARIA_OK ||
                       aria_device_alloc(0, sizeof(int), &d_n) != ARIA_OK))
            return 3;
        std::vector<float> depth((std::size_t)W * H);
        for (int i = 0; i < n_frames; i++) {
            std::int64_t ts;
            std::int32_t n_dets;
            if (std::fread(&ts, 8, 1, f) != 1 || std::fread(&n_dets, 4, 1, f) != 1 || n_dets < 0 || n_dets > 64) return 2;
            std::vector<core::Detection> dets((std::size_t)n_dets);
            if (n_dets && std::fread(dets.data(), sizeof(core::Detection), (std::size_t)n_dets, f) != (std::size_t)n_dets) return 2;
            if (std::fread(depth.data(), sizeof(float), depth.size(), f) != depth.size()) return 2;
            std::vector<aria_alert_event> ev;
            if (device) {
                if (aria_copy_h2d_async(0, st, d_depth, depth.data(), sizeof(float) * depth.size()) != ARIA_OK ||
                    aria_copy_h2d_async(0, st, d_dets, dets.data(), sizeof(core::Detection) * dets.size()) != ARIA_OK ||
                    aria_copy_h2d_async(0, st, d_n, &n_dets, sizeof(n_dets)) != ARIA_OK || aria_stream_synchronize(0, st) != ARIA_OK)
                    return 3;
                ev = alerter->processDevice(static_cast<const float*>(d_depth), W, static_cast<const aria_detection*>(d_dets),
                                            static_cast<const int*>(d_n), 64, ts);
            } else {
                ev = alerter->process(depth.data(), dets, ts);
            }
            std::size_t call = 0;
            for (const aria_alert_event& e : ev) {
                std::printf("event %d %d %d %d %d %.9g %d\n", i, e.source, e.class_id, e.direction, e.priority, (double)e.distance, e.flags);
                const std::size_t n_calls = 1 + ((e.flags & ARIA_ALERT_BEEP) ? 1 : 0) + ((e.flags & ARIA_ALERT_CRITICAL_ALERT) ? 1 : 0);
                for (std::size_t k = 0; k < n_calls && call < audio.log.size(); k++) std::printf("%s\n", audio.log[call++].c_str());
            }
            if (call != audio.log.size()) { std::printf("unexpected calls\n"); return 4; }
            audio.log.clear();
        }
        std::printf("state %lld spoken %zu beeps %zu critical %zu\n", (long long)alerter->state().events_total, audio.spoken.size(), audio.beeps.size(),
                    audio.critical_alerts.size());
        // a decreasing timestamp is refused before anything runs
        try {
            alerter->process(depth.data(), {}, -1);
            std::printf("decreasing timestamp accepted\n");
            return 5;
        } catch (const std::invalid_argument&) {
            std::printf("refused\n");
        }
        for (void* p : {d_depth, d_dets, d_n})
            if (p) aria_device_free(0, p);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::fclose(f);
    return 0;
}
