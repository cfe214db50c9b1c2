// aria::adapters::hip::MapTracker -- the tracking loop that keeps a monocular trajectory and its map in one frame and one scale
// (euroc_frontend --track-map): the first accepted pair is bootstrapped by the two-view stage at unit baseline and triangulated;
// each later frame is placed by PnP (HipPnPEstimator::estimateAgainstMap) against the points of the previous pair, and the new
// pair is triangulated with the two extrinsics, so that every point and pose is in the first pair's frame. When PnP finds no
// pose, or one with n_inliers <= min_pose_inliers, the step falls back to the two-view delta (its scale is then arbitrary, as
// in --map); without either the pose is held and the next accepted pair starts from it.
#pragma once
#include <array>
#include <cstdint>
#include <optional>
#include <vector>

#include "aria_hip/HipBundleAdjuster.hpp"
#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipPnPEstimator.hpp"
#include "aria_hip/HipPoseEstimator.hpp"

namespace aria::adapters::hip {

struct TrackStep {
    enum Source { HELD = 0, BOOTSTRAP = 1, PNP = 2, FALLBACK = 3 };
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
    HipMapper& mapper() { return mapper_; }
    // Every later step is also recorded in `builder` (nullptr: none): the frames, their poses, and which keypoint of the new
    // frame continues which point, for the windows of HipBundleAdjuster. The builder must outlive the tracking.
    void setWindowBuilder(WindowBuilder* builder) { builder_ = builder; }

private:
    HipMapper mapper_;
    HipPnPEstimator pnp_;
    int min_pose_inliers_;
    std::array<double, 16> pose_;
    bool bootstrapped_ = false;
    int anchor_pair_ = -1;              // pair id of the points whose view 2 is the last frame; -1: none
    int steps_ = 0;
    WindowBuilder* builder_ = nullptr;
};

}  // namespace aria::adapters::hip
