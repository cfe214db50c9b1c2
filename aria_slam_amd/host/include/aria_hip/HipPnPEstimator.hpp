// aria::adapters::hip::HipPnPEstimator -- absolute pose from 3D-2D correspondences over the C-ABI (include/aria_orb_hip.h,
// "absolute pose from the point map"): PnP RANSAC on the device, the step that places a frame in the frame and the scale of the
// map HipMapper keeps. The reference has no PnP code; its notes name the method (docs/milestones/H04_POSE_ESTIMATION_AUDIT.md
// section 8, "PnP (con mapa)"). aria_slam_amd/pnp_ref.py is the definition of every step.
#pragma once
#include <array>
#include <cstdint>
#include <optional>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

// x_cam = R X + t, world to camera (the map stage's convention); R row-major
struct AbsolutePose {
    std::array<double, 9> R{};
    std::array<double, 3> t{};
    double rms_px = 0.0;
    int n_corr = 0, n_inliers = 0, iterations = 0;
    bool refined = false;
    std::vector<std::uint8_t> mask;     // per correspondence: inlier of the returned pose
};

class HipPnPEstimator {
public:
    explicit HipPnPEstimator(const PoseIntrinsics& K = {}, int hypotheses = 1024, double threshold_px = 2.0, int refine_iters = 5,
                             std::uint64_t seed = 0, void* stream = nullptr, int device = 0);
    ~HipPnPEstimator();

    // The minimal solver of the calls that follow: ARIA_PNP_SOLVER_DLT6 (the default; a planar scene yields no pose) or
    // ARIA_PNP_SOLVER_P3P (four correspondences are enough, planar scenes included). Throws on an unknown value.
    void setSolver(int solver);
    int solver() const { return aria_pnp_get_solver(h_.get()); }

    // std::nullopt when the stage finds no pose (fewer correspondences than the solver needs, 6 or 4; no valid hypothesis; with
    // the DLT a planar scene).
    std::optional<AbsolutePose> estimate(const std::vector<aria_pnp_corr>& corr, int pair_id = 0);

    // One tracked frame against the map, joined on the device (aria_pnp_associate_batch_device, then
    // aria_pnp_estimate_batch_device on the handle's stream; the map's host calls have synchronised before). The map points
    // used are those of pair `anchor_pair`; anchor_view (1 or 2) says whether their idx1 or idx2 indexes the anchor frame.
    // `matches` pair the anchor frame with `tracked`; anchor_is_query: match.query_idx indexes the anchor frame (the
    // reference's order: query = previous frame). n_corr (optional): the correspondences the join found; match_index
    // (optional): each correspondence's index in `matches`. std::nullopt when the stage finds no pose.
    std::optional<AbsolutePose> estimateAgainstMap(aria_map_t map, int anchor_pair, int anchor_view, const core::Frame& tracked,
                                                   const std::vector<core::Match>& matches, bool anchor_is_query, int pair_id = 0,
                                                   int* n_corr = nullptr, std::vector<int>* match_index = nullptr);
    aria_pnp_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipPnPEstimator", where, rc); }
    detail::DeviceScratch scratch_;     // staging of estimateAgainstMap; before h_ (see Stage.hpp, DECLARATION ORDER)
    detail::StageOwner<aria_pnp_t, aria_pnp_destroy> h_;
};

// 4x4 row-major [R t; 0 1] of a pose
std::array<double, 16> poseMatrix(const AbsolutePose& p);

}  // namespace aria::adapters::hip
