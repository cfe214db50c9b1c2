// See aria_hip/HipStereoMatcher.hpp.
#include "aria_hip/HipStereoMatcher.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");

float StereoObservations::medianDepth() const {
    std::vector<float> d;
    for (const aria_stereo_obs& o : obs)
        if (o.right_idx >= 0) d.push_back(o.depth);
    if (d.empty()) return 0.0f;
    std::sort(d.begin(), d.end());
    return d[d.size() / 2];
}

HipStereoMatcher::HipStereoMatcher(const StereoConfig& cfg) {
    aria_stereo_config c;
    aria_stereo_default_config(&c);
    c.device = cfg.device;
    c.stream = cfg.stream;
    c.fx = cfg.K.fx; c.fy = cfg.K.fy; c.cx = cfg.K.cx; c.cy = cfg.K.cy;
    c.baseline = cfg.baseline;
    c.min_disparity = cfg.min_disparity;
    c.max_disparity = cfg.max_disparity < 0 ? cfg.K.fx : cfg.max_disparity;
    c.th_hamming = cfg.th_hamming;
    c.sad_half_window = cfg.sad_half_window;
    c.sad_slide = cfg.sad_slide;
    c.max_octave_diff = cfg.max_octave_diff;
    c.min_scale_matches = cfg.min_scale_matches;
    c.band_factor = cfg.band_factor;
    c.median_factor = cfg.median_factor;
    expect("aria_stereo_create", aria_stereo_create(&c, h_.out()));
}

HipStereoMatcher::~HipStereoMatcher() = default;

StereoObservations HipStereoMatcher::match(const std::uint8_t* image_left, const std::uint8_t* image_right, int width, int height,
                                           const core::Frame& left, const core::Frame& right) {
    StereoObservations out;
    const int nl = (int)left.keypoints.size(), nr = (int)right.keypoints.size();
    out.obs.resize((size_t)nl);
    out.matches.resize((size_t)nl);
    int n = 0;
    expect("aria_stereo_match",
           aria_stereo_match(h_.get(), image_left, image_right, width, height, width,
                             reinterpret_cast<const aria_keypoint*>(left.keypoints.data()), left.descriptors.data(), nl,
                             reinterpret_cast<const aria_keypoint*>(right.keypoints.data()), right.descriptors.data(), nr,
                             out.obs.data(), reinterpret_cast<aria_match*>(out.matches.data()), &n));
    out.matches.resize((size_t)n);
    return out;
}

aria_stereo_scale HipStereoMatcher::scale(const TwoViewPose& pose, const std::vector<core::Match>& matches, bool query_is_first,
                                          const std::vector<aria_stereo_obs>& obs_query,
                                          const std::vector<aria_stereo_obs>& obs_train) {
    aria_pose_result r{};
    for (int k = 0; k < 9; k++) { r.R[k] = pose.R[(size_t)k]; r.E[k] = pose.E[(size_t)k]; }
    for (int k = 0; k < 3; k++) r.t[k] = pose.t[(size_t)k];
    r.n_matches = pose.n_matches;
    r.n_inliers = pose.n_inliers;
    r.n_pose_inliers = pose.n_pose_inliers;
    r.refined = pose.refined ? 1 : 0;
    r.valid = 1;
    aria_stereo_scale out{};
    const bool masked = !matches.empty() && pose.mask.size() == matches.size();
    expect("aria_stereo_scale_pose",
           aria_stereo_scale_pose(h_.get(), &r, masked ? pose.mask.data() : nullptr,
                                  reinterpret_cast<const aria_match*>(matches.data()), (int)matches.size(),
                                  query_is_first ? 1 : 0, obs_query.data(), (int)obs_query.size(), obs_train.data(),
                                  (int)obs_train.size(), &out));
    return out;
}

}  // namespace aria::adapters::hip
