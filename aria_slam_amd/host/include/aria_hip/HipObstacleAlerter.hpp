// aria::adapters::hip::HipObstacleAlerter -- obstacle alerts over the C-ABI (include/aria_orb_hip.h, "obstacle alerts"): a frame's
// depth map and boxes turned into a short, prioritised, non-repeating list of warnings, spoken through the reference's port
// IAudioFeedback (include/interfaces/IAudioFeedback.hpp). It plays the role of the sketch's NavigationAudioEngine
// (docs/milestones/H16_AUDIO_FEEDBACK.md:421-493); the definition is the NumPy restatement aria_slam_amd/alert_ref.py, which the
// device equals bit for bit. The defaults for band, percentiles and zone_alert_m are assumptions: nobody has tuned them on a
// recording. RecordingAudioFeedback is the sketch's mock (H16:497-521): it keeps what was spoken and played.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct ObstacleAlerterConfig {
    int width = 752, height = 480;
    int zone_top = -1, zone_bottom = -1;         // -1 = [height / 4, height): [120, 480) at the default size
    int max_dets = 32, min_valid = 16;
    float min_depth = 0.1f, max_depth = 20.0f;
    int zone_pct_num = 5, zone_pct_den = 100, det_pct_num = 1, det_pct_den = 2;
    float zone_alert_m = 3.0f, default_depth = 5.0f, crit_m = 1.0f, high_m = 2.0f, medium_m = 3.0f, beep_m = 1.5f;
    bool obstacle_dangerous = true;
    std::vector<int> dangerous = {0, 1, 2, 3, 5, 7};     // H16:472
    int max_events_per_frame = 2;
    std::int64_t cooldown_ns[4] = {2000000000ll, 800000000ll, 500000000ll, 0};   // LOW..CRITICAL, H16:395-400
    int event_cap = 64;                          // events one process() call can return
    std::string obstacle_name = "obstacle";      // what a zone (class -1) is called
    void* stream = nullptr;
    int device = 0;
};

class RecordingAudioFeedback : public interfaces::IAudioFeedback {
public:
    struct Spoken { std::string text; interfaces::AudioPriority priority; bool interrupt; };
    struct Beep { interfaces::AudioDirection direction; int frequency_hz, duration_ms; float volume; };
    bool initialize() override { ready_ = true; return true; }
    void shutdown() override { ready_ = false; }
    bool isReady() const override { return ready_; }
    void speak(const std::string& text, interfaces::AudioPriority priority, bool interrupt) override;
    void playBeep(interfaces::AudioDirection direction, int frequency_hz, int duration_ms, float volume) override;
    void playCriticalAlert(interfaces::AudioDirection direction) override;
    void setVolume(float volume) override { volume_ = volume; }
    float getVolume() const override { return volume_; }
    void setMuted(bool muted) override { muted_ = muted; }
    bool isMuted() const override { return muted_; }
    void spinOnce() override {}

    std::vector<Spoken> spoken;
    std::vector<Beep> beeps;
    std::vector<interfaces::AudioDirection> critical_alerts;
    std::vector<std::string> log;                // every call in order, one line each: what euroc_frontend --alerts writes

private:
    bool ready_ = false, muted_ = false;
    float volume_ = 1.0f;
};

class HipObstacleAlerter {
public:
    // audio may be nullptr: the events are returned and nothing is played. class_names[class_id] is what a detection is called
    // ("object" beyond the list).
    explicit HipObstacleAlerter(const ObstacleAlerterConfig& cfg = {}, interfaces::IAudioFeedback* audio = nullptr,
                                std::vector<std::string> class_names = {});
    ~HipObstacleAlerter();

    // One frame: depth is width x height floats, tightly packed; timestamp_ns must not decrease (such a frame is refused with
    // std::invalid_argument before anything runs). A call that throws, for that or for any other reason, leaves the state and
    // the last accepted timestamp as they were. Returns the announced events in rule 4's order and plays them; blocks.
    std::vector<aria_alert_event> process(const float* depth, const std::vector<core::Detection>& detections, std::int64_t timestamp_ns);
    // The same from HBM without a copy: a depth map of `depth_pitch` elements a row (HipDenseStereo's, as
    // aria_dense_compute_batch_device writes it) and lists in HipObjectDetector::deviceBoxes()'s layout (d_detections may be
    // nullptr: zones only). The producers' streams must have been synchronised, or be this handle's. Blocks for the events.
    std::vector<aria_alert_event> processDevice(const float* d_depth, int depth_pitch, const aria_detection* d_detections,
                                                const int* d_n_detections, int det_cap, std::int64_t timestamp_ns);
    // name [+ ", " + distance with one decimal + " meters" when distance < 5.0f] (H16:480-487)
    std::string message(const aria_alert_event& e) const;
    void reset();                                // a cleared state: every cooldown forgotten
    const aria_alert_state& state() const { return state_; }
    const aria_alert_config& config() const { return cfg_; }
    aria_alert_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status);     // std::invalid_argument for ARIA_E_INVALID
    static void expect(const char* where, int rc) { if (rc != ARIA_OK) fail(where, rc); }
    std::vector<aria_alert_event> finish(int rc, int n_events, const aria_alert_state& after, std::int64_t timestamp_ns);
    void play(const aria_alert_event& e);
    void accept(std::int64_t timestamp_ns) const;
    void release();
    aria_alert_config cfg_{};
    detail::StageOwner<aria_alert_t, aria_alert_destroy> h_;
    interfaces::IAudioFeedback* audio_ = nullptr;
    std::vector<std::string> names_;
    std::string obstacle_name_;
    aria_alert_state state_{};
    std::int64_t last_ts_ = 0;
    bool have_ts_ = false;
    std::vector<aria_alert_event> events_;
    void *d_state_ = nullptr, *d_events_ = nullptr, *d_ints_ = nullptr, *d_ts_ = nullptr;   // device form: state, events, {0, 1, n}, timestamp
};

}  // namespace aria::adapters::hip
