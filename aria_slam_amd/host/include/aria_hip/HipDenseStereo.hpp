// aria::adapters::hip::HipDenseStereo -- dense stereo over the C-ABI (include/aria_orb_hip.h, "dense stereo"): census +
// four-path semi-global matching over 64 disparities on a RECTIFIED pair, a disparity map in 1/16 px, an fp32 depth map, and
// the stereo observation at each keypoint in the sparse stage's record. The reference has no code for it (its roadmap item
// H19); the definition is the NumPy restatement aria_slam_amd/dense_ref.py, which the device equals bit for bit.
// Rectification is aria_rect_* (aria_hip/HipRectifier.hpp).
#pragma once
#include <cstdint>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct DenseStereoConfig {
    PoseIntrinsics K{};                  // the rectified left camera (EuRoC cam0 by default)
    double baseline = 0.110;             // metres
    int P1 = 8, P2 = 32, uniqueness = 10, lr_max_diff = 1;
    int max_width = 752, max_height = 480;
    std::int64_t scratch_bytes = std::int64_t(1) << 30;
    void* stream = nullptr;
    int device = 0;
};

struct DenseDepth {
    int width = 0, height = 0;
    std::vector<std::int16_t> disparity;   // width * height, 1/16 px, -16 = invalid
    std::vector<float> depth;              // width * height, metres, 0 where the disparity is not positive
    // share of the pixels with a positive disparity
    double validShare() const;
    // the depth at index n / 2 of the ascending depths of those pixels; 0 without one
    float medianDepth() const;
};

class HipDenseStereo {
public:
    explicit HipDenseStereo(const DenseStereoConfig& cfg = {});
    ~HipDenseStereo();

    // One rectified pair: the two gray images, width x height bytes, tightly packed.
    DenseDepth compute(const std::uint8_t* image_left, const std::uint8_t* image_right, int width, int height);
    // The stereo observations of `keypoints` on a map of compute(): unmatched where the rounded keypoint is outside the image
    // or on a pixel without a positive disparity.
    std::vector<aria_stereo_obs> sample(const DenseDepth& map, const std::vector<core::KeyPoint>& keypoints);
    int pairsInFlight() const { return aria_dense_pairs_in_flight(h_.get()); }
    aria_dense_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipDenseStereo", where, rc); }
    detail::StageOwner<aria_dense_t, aria_dense_destroy> h_;
};

}  // namespace aria::adapters::hip
