// See aria_hip/HipObstacleAlerter.hpp.
#include "aria_hip/HipObstacleAlerter.hpp"

#include "aria_hip/HipFactory.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace aria::adapters::hip {

namespace {

const char* directionName(interfaces::AudioDirection d) {
    switch (d) {
        case interfaces::AudioDirection::LEFT: return "LEFT";
        case interfaces::AudioDirection::RIGHT: return "RIGHT";
        case interfaces::AudioDirection::BEHIND: return "BEHIND";
        default: return "CENTER";
    }
}

const char* priorityName(interfaces::AudioPriority p) {
    switch (p) {
        case interfaces::AudioPriority::LOW: return "LOW";
        case interfaces::AudioPriority::HIGH: return "HIGH";
        case interfaces::AudioPriority::CRITICAL: return "CRITICAL";
        default: return "MEDIUM";
    }
}

}  // namespace

void RecordingAudioFeedback::speak(const std::string& text, interfaces::AudioPriority priority, bool interrupt) {
    spoken.push_back({text, priority, interrupt});
    log.push_back(std::string("speak ") + priorityName(priority) + (interrupt ? " interrupt " : " - ") + text);
}

void RecordingAudioFeedback::playBeep(interfaces::AudioDirection direction, int frequency_hz, int duration_ms, float volume) {
    beeps.push_back({direction, frequency_hz, duration_ms, volume});
    char buf[96];
    std::snprintf(buf, sizeof(buf), "beep %s %d %d %.1f", directionName(direction), frequency_hz, duration_ms, (double)volume);
    log.push_back(buf);
}

void RecordingAudioFeedback::playCriticalAlert(interfaces::AudioDirection direction) {
    critical_alerts.push_back(direction);
    log.push_back(std::string("critical ") + directionName(direction));
}

// the one adapter whose ARIA_E_INVALID is a std::invalid_argument
void HipObstacleAlerter::fail(const char* where, int status) {
    if (status == ARIA_E_INVALID) throw std::invalid_argument(detail::message("HipObstacleAlerter", where, status));
    detail::fail("HipObstacleAlerter", where, status);
}

HipObstacleAlerter::HipObstacleAlerter(const ObstacleAlerterConfig& cfg, interfaces::IAudioFeedback* audio, std::vector<std::string> class_names)
    : audio_(audio), names_(std::move(class_names)), obstacle_name_(cfg.obstacle_name) {
    aria_alert_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.width = cfg.width; cfg_.height = cfg.height;
    cfg_.zone_top = cfg.zone_top >= 0 ? cfg.zone_top : cfg.height / 4;
    cfg_.zone_bottom = cfg.zone_bottom >= 0 ? cfg.zone_bottom : cfg.height;
    cfg_.max_dets = cfg.max_dets; cfg_.min_valid = cfg.min_valid; cfg_.min_depth = cfg.min_depth; cfg_.max_depth = cfg.max_depth;
    cfg_.zone_pct_num = cfg.zone_pct_num; cfg_.zone_pct_den = cfg.zone_pct_den; cfg_.det_pct_num = cfg.det_pct_num; cfg_.det_pct_den = cfg.det_pct_den;
    cfg_.zone_alert_m = cfg.zone_alert_m; cfg_.default_depth = cfg.default_depth; cfg_.crit_m = cfg.crit_m; cfg_.high_m = cfg.high_m;
    cfg_.medium_m = cfg.medium_m; cfg_.beep_m = cfg.beep_m;
    cfg_.obstacle_dangerous = cfg.obstacle_dangerous ? 1 : 0;
    if (cfg.dangerous.size() > 32 || cfg.event_cap < 1) fail("config", ARIA_E_INVALID);
    cfg_.n_dangerous = (int)cfg.dangerous.size();
    for (int i = 0; i < 32; i++) cfg_.dangerous[i] = i < cfg_.n_dangerous ? cfg.dangerous[(std::size_t)i] : 0;
    cfg_.max_events_per_frame = cfg.max_events_per_frame;
    for (int i = 0; i < 4; i++) cfg_.cooldown_ns[i] = cfg.cooldown_ns[i];
    events_.resize((std::size_t)cfg.event_cap);
    expect("aria_alert_create", aria_alert_create(&cfg_, h_.out()));
    // the buffers of the device form
    const std::int32_t ints[3] = {0, 1, 0};
    int rc;
    if ((rc = aria_device_alloc(cfg_.device, sizeof(aria_alert_state), &d_state_)) == ARIA_OK &&
        (rc = aria_device_alloc(cfg_.device, sizeof(aria_alert_event) * events_.size(), &d_events_)) == ARIA_OK &&
        (rc = aria_device_alloc(cfg_.device, sizeof(ints), &d_ints_)) == ARIA_OK &&
        (rc = aria_device_alloc(cfg_.device, sizeof(std::int64_t), &d_ts_)) == ARIA_OK)
        rc = aria_copy_h2d_async(cfg_.device, aria_alert_stream(h_.get()), d_ints_, ints, sizeof(ints));
    if (rc == ARIA_OK) rc = aria_stream_synchronize(cfg_.device, aria_alert_stream(h_.get()));   // `ints` leaves scope
    if (rc != ARIA_OK) {
        release();
        fail("device buffers", rc);
    }
}

HipObstacleAlerter::~HipObstacleAlerter() { release(); }

void HipObstacleAlerter::release() {
    h_.reset();
    for (void** p : {&d_state_, &d_events_, &d_ints_, &d_ts_}) {
        if (*p) aria_device_free(cfg_.device, *p);
        *p = nullptr;
    }
}

void HipObstacleAlerter::reset() {
    std::memset(&state_, 0, sizeof(state_));
    have_ts_ = false;
}

void HipObstacleAlerter::accept(std::int64_t timestamp_ns) const {
    if (have_ts_ && timestamp_ns < last_ts_) fail("a timestamp lower than its predecessor's", ARIA_E_INVALID);
}

std::string HipObstacleAlerter::message(const aria_alert_event& e) const {
    std::string s = e.class_id == -1 ? obstacle_name_
                    : e.class_id >= 0 && (std::size_t)e.class_id < names_.size() ? names_[(std::size_t)e.class_id] : std::string("object");
    if (e.distance < 5.0f) {
        char buf[48];
        std::snprintf(buf, sizeof(buf), ", %.1f meters", (double)e.distance);
        s += buf;
    }
    return s;
}

void HipObstacleAlerter::play(const aria_alert_event& e) {
    if (!audio_) return;
    const auto dir = static_cast<interfaces::AudioDirection>(e.direction);
    audio_->speak(message(e), static_cast<interfaces::AudioPriority>(e.priority), (e.flags & ARIA_ALERT_INTERRUPT) != 0);
    if (e.flags & ARIA_ALERT_BEEP) audio_->playBeep(dir, 800, 200, 0.8f);          // H16:453-455
    if (e.flags & ARIA_ALERT_CRITICAL_ALERT) audio_->playCriticalAlert(dir);      // H16:404-407
}

std::vector<aria_alert_event> HipObstacleAlerter::finish(int rc, int n_events, const aria_alert_state& after, std::int64_t timestamp_ns) {
    // a failed call leaves the state and the timestamp gate as they were. A frame's events beyond event_cap are counted, not
    // returned: the state has advanced past them.
    if (rc != ARIA_OK && rc != ARIA_E_OUTPUT_TOO_SMALL) fail("process", rc);
    state_ = after;
    last_ts_ = timestamp_ns;
    have_ts_ = true;
    std::vector<aria_alert_event> out(events_.begin(), events_.begin() + std::min<std::size_t>((std::size_t)std::max(n_events, 0), events_.size()));
    for (const aria_alert_event& e : out) play(e);
    return out;
}

std::vector<aria_alert_event> HipObstacleAlerter::process(const float* depth, const std::vector<core::Detection>& detections,
                                                          std::int64_t timestamp_ns) {
    static_assert(sizeof(core::Detection) == sizeof(aria_detection), "core::Detection is aria_detection");
    accept(timestamp_ns);
    const int track_offset[2] = {0, 1};
    const int n_dets = (int)detections.size();
    int n_events = 0;
    aria_alert_state after = state_;
    const bool have = n_dets > 0;
    const int rc = aria_alert_run(h_.get(), depth, (std::int64_t)cfg_.width * cfg_.height, cfg_.width, 1,
                                  have ? reinterpret_cast<const aria_detection*>(detections.data()) : nullptr, have ? &n_dets : nullptr,
                                  have ? n_dets : 0, track_offset, 1, &timestamp_ns, &after, events_.data(), (int)events_.size(), &n_events);
    return finish(rc, n_events, after, timestamp_ns);
}

std::vector<aria_alert_event> HipObstacleAlerter::processDevice(const float* d_depth, int depth_pitch, const aria_detection* d_detections,
                                                                const int* d_n_detections, int det_cap, std::int64_t timestamp_ns) {
    accept(timestamp_ns);
    void* st = aria_alert_stream(h_.get());
    const int dev = cfg_.device;
    std::int32_t* d_i = static_cast<std::int32_t*>(d_ints_);
    int rc = aria_copy_h2d_async(dev, st, d_state_, &state_, sizeof(state_));
    if (rc == ARIA_OK) rc = aria_copy_h2d_async(dev, st, d_ts_, &timestamp_ns, sizeof(timestamp_ns));
    if (rc == ARIA_OK)
        rc = aria_alert_run_batch_device(h_.get(), d_depth, 0, depth_pitch, 1, d_detections, d_n_detections, det_cap, d_i, 1,
                                         static_cast<const std::int64_t*>(d_ts_), static_cast<aria_alert_state*>(d_state_),
                                         static_cast<aria_alert_event*>(d_events_), (int)events_.size(), d_i + 2);
    expect("aria_alert_run_batch_device", rc);
    rc = aria_alert_check(h_.get());                                     // synchronises: the counts are there
    std::int32_t n_events = 0;
    int rc2 = aria_copy_d2h_async(dev, st, &n_events, d_i + 2, sizeof(n_events));
    aria_alert_state after;
    if (rc2 == ARIA_OK) rc2 = aria_copy_d2h_async(dev, st, &after, d_state_, sizeof(after));
    if (rc2 == ARIA_OK) rc2 = aria_copy_d2h_async(dev, st, events_.data(), d_events_, sizeof(aria_alert_event) * events_.size());
    if (rc2 == ARIA_OK) rc2 = aria_stream_synchronize(dev, st);
    expect("copy back", rc2);
    return finish(rc, n_events, after, timestamp_ns);
}

}  // namespace aria::adapters::hip

namespace aria::factory {

// Declared in aria_hip/HipFactory.hpp. Defined here and not in HipFactory.cpp: the reference-header build of the front end
// (tests/test_reference_headers.py) links HipFactory.cpp without the stage adapters and allows no undefined symbol.
std::unique_ptr<adapters::hip::HipObstacleAlerter> createHipAlerter(const HipFactoryConfig& cfg, interfaces::IAudioFeedback* audio,
                                                                    std::vector<std::string> class_names,
                                                                    adapters::hip::ObstacleAlerterConfig alert) {
    alert.device = cfg.hip_device;
    return std::make_unique<adapters::hip::HipObstacleAlerter>(alert, audio, std::move(class_names));
}

}  // namespace aria::factory
