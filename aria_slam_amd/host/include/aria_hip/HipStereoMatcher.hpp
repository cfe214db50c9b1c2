// aria::adapters::hip::HipStereoMatcher -- sparse stereo over the C-ABI (include/aria_orb_hip.h, "sparse stereo"): a depth per
// left keypoint of a RECTIFIED stereo pair and the metric scale of a relative pose. The reference has no stereo code (its
// roadmap item H19); the definition is the NumPy restatement aria_slam_amd/stereo_ref.py, which the device equals bit for bit.
// Rectification / undistortion is not part of the stage: the caller hands in row-aligned images -- see aria_rect_*
// (aria_hip/HipRectifier.hpp), which makes them from raw ones.
#pragma once
#include <cstdint>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct StereoConfig {
    PoseIntrinsics K{};                  // the rectified left camera (EuRoC cam0 by default)
    double baseline = 0.110;             // metres (EuRoC's nominal)
    double min_disparity = 0.0;
    double max_disparity = -1.0;         // < 0: fx, i.e. depth >= baseline
    int th_hamming = 75, sad_half_window = 5, sad_slide = 5, max_octave_diff = 1, min_scale_matches = 5;
    double band_factor = 2.0, median_factor = 2.1;
    void* stream = nullptr;
    int device = 0;
};

struct StereoObservations {
    std::vector<aria_stereo_obs> obs;    // one per left keypoint; right_idx = -1, depth = -1 when unmatched
    std::vector<core::Match> matches;    // (left index, right index, hamming) of the matched, ascending left index
    // the depth at index n / 2 of the ascending matched depths; 0 without a match
    float medianDepth() const;
};

class HipStereoMatcher {
public:
    explicit HipStereoMatcher(const StereoConfig& cfg = {});
    ~HipStereoMatcher();

    // One rectified pair: the two gray images (width x height bytes, tightly packed) and the frames extracted from them.
    StereoObservations match(const std::uint8_t* image_left, const std::uint8_t* image_right, int width, int height,
                             const core::Frame& left, const core::Frame& right);
    // Metric scale of `pose` (x2 ~ R x1 + t, |t| = 1) from the stereo observations of the two views; view 1 is the query side
    // of the matches when query_is_first. pose.mask selects the matches when it has one byte per match.
    aria_stereo_scale scale(const TwoViewPose& pose, const std::vector<core::Match>& matches, bool query_is_first,
                            const std::vector<aria_stereo_obs>& obs_query, const std::vector<aria_stereo_obs>& obs_train);
    aria_stereo_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipStereoMatcher", where, rc); }
    detail::StageOwner<aria_stereo_t, aria_stereo_destroy> h_;
};

}  // namespace aria::adapters::hip
