// aria::adapters::hip::MapTracker -- the tracking loop that keeps a monocular trajectory and its map in one frame and one scale
// (euroc_frontend --track-map): the first accepted pair is bootstrapped by the two-view stage at unit baseline and triangulated;
// each later frame is placed by PnP (HipPnPEstimator::estimateAgainstMap) against the points of the previous pair, and the new
// pair is triangulated with the two extrinsics, so that every point and pose is in the first pair's frame. When PnP finds no
// pose, or one with n_inliers <= min_pose_inliers, the step falls back to the two-view delta (its scale is then arbitrary, as
// in --map); without either the pose is held and the next accepted pair starts from it.
//
// setLocalMap(K) (off by default) adds guided matching in front of that chain: every new map point is also kept as a landmark
// (its X, the descriptor and octave of its keypoint in the frame that was current when it was made), and a step first
// predicts the pose -- constant velocity when the last two steps were placed, else the last pose --, projects the landmarks of
// the last K pairs into the current frame, searches them (HipProjectionMatcher) and runs PnP on the result. A pose with
// n_inliers > min_pose_inliers is taken (TrackStep::LOCAL); otherwise the step goes down the path above unchanged. So a frame
// whose predecessor was blank, and which therefore has no matches to track through, is still placed in the map's frame.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "aria_hip/HipBundleAdjuster.hpp"
#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipPnPEstimator.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/HipProjectionMatcher.hpp"

namespace aria::adapters::hip {

struct TrackStep {
    enum Source { HELD = 0, BOOTSTRAP = 1, PNP = 2, FALLBACK = 3, LOCAL = 4 };
    Source source = HELD;
    int n_corr = 0;         // correspondences the join found (0 when there were no points to track against)
    int n_inliers = 0;      // of the PnP pose, when one was found
    int added = 0;          // map points the step's triangulation added
};

class MapTracker {
public:
    // pnp_solver: the minimal solver of the PnP step (ARIA_PNP_SOLVER_DLT6 or ARIA_PNP_SOLVER_P3P; HipPnPEstimator::setSolver).
    explicit MapTracker(const MapperConfig& map_cfg = {}, int min_pose_inliers = 10, int hypotheses = 1024,
                        int pnp_solver = ARIA_PNP_SOLVER_DLT6);

    // One step previous -> current. `matches` pair the two frames; previous_is_query: match.query_idx indexes `previous`.
    // two_view: the two-view stage's previous -> current pose, if it found one (accepted when n_pose_inliers >
    // min_pose_inliers). previous_image (optional): the previous frame's gray image, for the points' gray byte.
    TrackStep track(const core::Frame& previous, const core::Frame& current, const std::vector<core::Match>& matches,
                    bool previous_is_query, const std::optional<TwoViewPose>& two_view, const std::uint8_t* previous_image = nullptr,
                    int width = 0, int height = 0);
    const std::array<double, 16>& pose() const { return pose_; }   // world to camera of the last frame, 4x4 row-major
    // Pair id of the map points whose view 2 is the last frame (-1: it owns none). With pose(), read after a step, this is what
    // the loop alignment needs to know about a keyframe (aria_hip/HipSim3Aligner.hpp, KeyframeInMap).
    int anchorPair() const { return anchor_pair_; }
    HipMapper& mapper() { return mapper_; }
    // Every later step is also recorded in `builder` (nullptr: none): the frames, their poses, and which keypoint of the new
    // frame continues which point, for the windows of HipBundleAdjuster. The builder must outlive the tracking.
    void setWindowBuilder(WindowBuilder* builder) { builder_ = builder; }
    // Guided matching against the landmarks of the last `pairs` triangulated pairs (0 = off, the default: track() then does
    // what it did before the mode existed, call for call). radius_px: the search window at octave 0. The image size that bounds
    // a projection is track()'s width x height when given, else the stage's largest (4096 x 4096). Landmarks are collected from
    // the call on; the landmarks are made on the host from the points the step reads back (the device join
    // aria_proj_landmarks_from_map_device makes the same records).
    void setLocalMap(int pairs, float radius_px = 15.0f);

private:
    HipMapper mapper_;
    HipPnPEstimator pnp_;
    int min_pose_inliers_;
    std::array<double, 16> pose_;
    bool bootstrapped_ = false;
    int anchor_pair_ = -1;              // pair id of the points whose view 2 is the last frame; -1: none
    int steps_ = 0;
    WindowBuilder* builder_ = nullptr;
    // the local map (setLocalMap)
    int local_pairs_ = 0;
    std::unique_ptr<HipProjectionMatcher> proj_;
    std::vector<aria_proj_landmark> landmarks_;
    std::vector<std::size_t> pair_start_;           // where each triangulated pair's landmarks start
    std::array<double, 16> before_last_;            // the pose before the last step
    bool placed_last_ = false, placed_before_ = false;
    PoseIntrinsics K_;
    double min_depth_;
    int device_;
};

}  // namespace aria::adapters::hip
