// aria::adapters::hip::HipRectifier -- undistortion and stereo rectification over the C-ABI (include/aria_orb_hip.h,
// "rectification"): the maps of one camera (plain undistortion) or of the two cameras of a rig (the rectifying rotations
// from their T_BS) built on the device, images warped into the frame the extractor and the stereo stage read, keypoints moved
// into it. The reference parses the distortion coefficients and never uses them; the definition is the NumPy restatement
// aria_slam_amd/rectify_ref.py, which the device equals bit for bit. RectifierConfig::model picks radtan or the fisheye model
// KB4 (OpenCV's "fisheye", Kalibr's "equidistant") for all cameras of the handle. Out of scope: Aria's FISHEYE624, KB3, rays at
// or beyond 90 degrees from the axis, cylindrical and equirectangular destinations; parity with OpenCV's fisheye:: functions
// is not pinned.
#pragma once
#include <cstdint>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct RectCalibration {                 // one camera as its sensor.yaml states it (EuRoC cam0 by default)
    PoseIntrinsics K{};
    double dist[5] = {-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0};   // radtan k1, k2, p1, p2, k3; KB4 k1..k4, 0
    double T_BS[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};             // sensor to body, row-major
};

struct RectifierConfig {
    int model = ARIA_RECT_MODEL_RADTAN;  // ARIA_RECT_MODEL_*, of every camera (AslCalibration::rectModel() of a sensor.yaml)
    int n_cameras = 1;                   // 1: plain undistortion of cam[0]; 2: stereo rectification of cam[0] (left), cam[1]
    RectCalibration cam[2];
    int src_width = 752, src_height = 480;
    int dst_width = 0, dst_height = 0;   // 0: the source size
    double new_K[4] = {0, 0, 0, 0};      // fx', fy', cx', cy'; a zero takes the default (one camera: its K; two: the header's)
    int fill = 0;
    void* stream = nullptr;
    int device = 0;
};

class HipRectifier {
public:
    explicit HipRectifier(const RectifierConfig& cfg = {});
    ~HipRectifier();

    // One gray image of camera cam (src_width x src_height bytes, tightly packed) -> dst_width x dst_height bytes.
    void remap(int cam, const std::uint8_t* src, std::vector<std::uint8_t>& dst);
    // The keypoints of a frame extracted from a RAW image of camera cam, moved into the undistorted / rectified frame.
    void points(int cam, std::vector<core::KeyPoint>& keypoints);
    std::vector<std::uint32_t> map(int cam);
    PoseIntrinsics newK() const { return PoseIntrinsics{cfg_.new_fx, cfg_.new_fy, cfg_.new_cx, cfg_.new_cy}; }
    double baseline() const { return baseline_; }        // 0 for one camera
    int dstWidth() const { return cfg_.dst_width; }
    int dstHeight() const { return cfg_.dst_height; }
    const aria_rect_config& config() const { return cfg_; }
    aria_rect_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipRectifier", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipRectifier", where, rc); }
    aria_rect_config cfg_{};
    double baseline_ = 0.0;
    detail::StageOwner<aria_rect_t, aria_rect_destroy> h_;
};

}  // namespace aria::adapters::hip
