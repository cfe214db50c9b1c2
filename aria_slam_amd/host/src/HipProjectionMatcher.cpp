// See aria_hip/HipProjectionMatcher.hpp.
#include "aria_hip/HipProjectionMatcher.hpp"

#include <cstring>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

HipProjectionMatcher::HipProjectionMatcher(const ProjectionConfig& cfg) {
    aria_proj_config c;
    aria_proj_default_config(&c);
    c.device = cfg.device;
    c.stream = cfg.stream;
    c.fx = cfg.K.fx; c.fy = cfg.K.fy; c.cx = cfg.K.cx; c.cy = cfg.K.cy;
    c.min_depth = cfg.min_depth;
    c.radius_px = cfg.radius_px;
    c.ratio = cfg.ratio;
    c.th_hamming = cfg.th_hamming;
    c.max_octave_diff = cfg.max_octave_diff;
    expect("aria_proj_create", aria_proj_create(&c, h_.out()));
}

HipProjectionMatcher::~HipProjectionMatcher() = default;

ProjectionMatches HipProjectionMatcher::search(const double T[16], const core::Frame& frame,
                                               const std::vector<aria_proj_landmark>& landmarks, std::size_t first, std::size_t count,
                                               int width, int height) {
    static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint), "layouts");
    if (first > landmarks.size() || count > landmarks.size() - first) throw std::out_of_range("HipProjectionMatcher::search: range");
    if (frame.descriptors.size() < frame.keypoints.size() * 32) throw std::invalid_argument("HipProjectionMatcher::search: descriptors");
    ProjectionMatches out;
    out.obs.resize(count);
    out.corr.resize(count);
    out.pairs.resize(count);
    int n = 0;
    expect("aria_proj_search",
           aria_proj_search(h_.get(), T, reinterpret_cast<const aria_keypoint*>(frame.keypoints.data()), frame.descriptors.data(),
                            (int)frame.keypoints.size(), width, height, landmarks.data() + first, (int)count, out.obs.data(),
                            out.corr.data(), out.pairs.data(), &n));   // the first 12 of T are [R|t] row-major
    out.corr.resize((std::size_t)n);
    out.pairs.resize((std::size_t)n);
    for (aria_proj_pair& p : out.pairs) p.landmark += (int)first;
    return out;
}

void HipProjectionMatcher::searchDevice(const double* d_pose, const aria_keypoint* d_kp, const std::uint8_t* d_desc, const int* d_n,
                                        std::int64_t kp_stride, int width, int height, const aria_proj_landmark* d_land, int n_landmarks,
                                        const int* d_range, int land_cap, int n_frames, aria_proj_obs* d_obs, aria_pnp_corr* d_corr,
                                        aria_proj_pair* d_pairs, int* d_ncorr) {
    expect("aria_proj_search_batch_device",
           aria_proj_search_batch_device(h_.get(), d_pose, d_kp, d_desc, d_n, kp_stride, width, height, d_land, n_landmarks, d_range,
                                         land_cap, n_frames, d_obs, d_corr, d_pairs, d_ncorr));
}

void HipProjectionMatcher::landmarksFromMapDevice(aria_map_t map, std::int64_t first, std::int64_t max_count, int pair_base, int view,
                                                  const aria_keypoint* d_kp, const std::uint8_t* d_desc, const int* d_n,
                                                  std::int64_t kp_stride, int n_slots, aria_proj_landmark* d_land, int* d_nland) {
    expect("aria_proj_landmarks_from_map_device",
           aria_proj_landmarks_from_map_device(h_.get(), map, first, max_count, pair_base, view, d_kp, d_desc, d_n, kp_stride, n_slots,
                                               d_land, d_nland));
}

void HipProjectionMatcher::check() {
    expect("aria_proj_check", aria_proj_check(h_.get()));
}

aria_proj_landmark landmarkFromPoint(const aria_map_point& point, const core::Frame& frame, int idx, int arena_position) {
    aria_proj_landmark lm;
    std::memset(&lm, 0, sizeof(lm));
    lm.octave = -1;
    lm.source = arena_position;
    if (idx < 0 || (std::size_t)idx >= frame.keypoints.size() || frame.descriptors.size() < ((std::size_t)idx + 1) * 32) return lm;
    for (int k = 0; k < 3; k++) lm.X[k] = point.X[k];
    std::memcpy(lm.desc, frame.descriptors.data() + (std::size_t)idx * 32, 32);
    lm.octave = frame.keypoints[(std::size_t)idx].octave;
    return lm;
}

}  // namespace aria::adapters::hip
