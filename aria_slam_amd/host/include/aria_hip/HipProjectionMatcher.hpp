// aria::adapters::hip::HipProjectionMatcher -- guided matching over the C-ABI (include/aria_orb_hip.h, "guided matching"):
// landmarks projected into a frame by a predicted pose, the keypoints searched in a window around each projection, the matches
// as the 3D-2D correspondences HipPnPEstimator takes. The reference has no code for it; aria_slam_amd/proj_ref.py is the
// definition of every step. The defaults are ORB-SLAM's published tracking constants; nobody has tuned them on a recording here.
#pragma once
#include <cstdint>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct ProjectionConfig {
    PoseIntrinsics K{};
    double min_depth = 0.1, radius_px = 15.0;
    float ratio = 0.9f;
    int th_hamming = 100, max_octave_diff = 1;
    void* stream = nullptr;
    int device = 0;
};

struct ProjectionMatches {
    std::vector<aria_proj_obs> obs;      // one per landmark searched
    std::vector<aria_pnp_corr> corr;     // the matched landmarks in ascending index: X and the keypoint's pixel
    std::vector<aria_proj_pair> pairs;   // (landmark index, keypoint index) of each correspondence
};

class HipProjectionMatcher {
public:
    explicit HipProjectionMatcher(const ProjectionConfig& cfg = {});
    ~HipProjectionMatcher();

    // Host form: `count` landmarks from landmarks[first] on against the keypoints and descriptors of `frame`, under the predicted
    // world-to-camera pose T (4x4 row-major). pairs[].landmark indexes `landmarks`. Blocks; throws on a non-finite pose.
    ProjectionMatches search(const double T[16], const core::Frame& frame, const std::vector<aria_proj_landmark>& landmarks,
                             std::size_t first, std::size_t count, int width, int height);

    // Device forms: aria_proj_search_batch_device and aria_proj_landmarks_from_map_device on the handle's stream, as declared in
    // the header; nothing is synchronised. check() synchronises and throws on a deferred error.
    void searchDevice(const double* d_pose, const aria_keypoint* d_kp, const std::uint8_t* d_desc, const int* d_n, std::int64_t kp_stride,
                      int width, int height, const aria_proj_landmark* d_land, int n_landmarks, const int* d_range, int land_cap,
                      int n_frames, aria_proj_obs* d_obs, aria_pnp_corr* d_corr, aria_proj_pair* d_pairs, int* d_ncorr);
    void landmarksFromMapDevice(aria_map_t map, std::int64_t first, std::int64_t max_count, int pair_base, int view,
                                const aria_keypoint* d_kp, const std::uint8_t* d_desc, const int* d_n, std::int64_t kp_stride, int n_slots,
                                aria_proj_landmark* d_land, int* d_nland);
    void check();
    aria_proj_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipProjectionMatcher", where, rc); }
    detail::StageOwner<aria_proj_t, aria_proj_destroy> h_;
};

// The landmark of a map point seen in `frame` as keypoint idx: its X, the keypoint's descriptor row and octave, source = the
// arena position -- what aria_proj_landmarks_from_map_device makes on the device. A dead landmark when idx is out of range.
aria_proj_landmark landmarkFromPoint(const aria_map_point& point, const core::Frame& frame, int idx, int arena_position);

}  // namespace aria::adapters::hip
