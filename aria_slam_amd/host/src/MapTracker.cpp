// See aria_hip/MapTracker.hpp.
#include "aria_hip/MapTracker.hpp"

#include <stdexcept>

namespace aria::adapters::hip {

MapTracker::MapTracker(const MapperConfig& map_cfg, int min_pose_inliers, int hypotheses, int pnp_solver)
    : mapper_(map_cfg), pnp_(map_cfg.K, hypotheses, map_cfg.max_reproj_px, 5, 0, nullptr, map_cfg.device),
      min_pose_inliers_(min_pose_inliers), pose_{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1} {
    if (pnp_solver != ARIA_PNP_SOLVER_DLT6) pnp_.setSolver(pnp_solver);
}

TrackStep MapTracker::track(const core::Frame& previous, const core::Frame& current, const std::vector<core::Match>& matches,
                            bool previous_is_query, const std::optional<TwoViewPose>& two_view, const std::uint8_t* previous_image,
                            int width, int height) {
    TrackStep step;
    const std::array<double, 16> before = pose_;
    std::array<double, 16> now = before;
    steps_++;
    if (anchor_pair_ >= 0) {                                       // the last pair's points index `previous` by idx2
        const std::optional<AbsolutePose> p = pnp_.estimateAgainstMap(mapper_.handle(), anchor_pair_, 2, current, matches,
                                                                      previous_is_query, steps_, &step.n_corr);
        if (p) step.n_inliers = p->n_inliers;
        if (p && p->n_inliers > min_pose_inliers_) {
            now = poseMatrix(*p);
            step.source = TrackStep::PNP;
        }
    }
    if (step.source == TrackStep::HELD && two_view && two_view->n_pose_inliers > min_pose_inliers_) {
        const std::array<double, 16> d = poseMatrix(*two_view);     // x_cur = R x_prev + t: world to camera composes on the left
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                double v = 0.0;
                for (int k = 0; k < 4; k++) v += d[(size_t)(a * 4 + k)] * before[(size_t)(k * 4 + b)];
                now[(size_t)(a * 4 + b)] = v;
            }
        step.source = bootstrapped_ ? TrackStep::FALLBACK : TrackStep::BOOTSTRAP;
    }
    anchor_pair_ = -1;
    std::vector<aria_map_point> appended;
    if (builder_ && builder_->frames() == 0) builder_->addFrame(previous, before.data());
    if (step.source != TrackStep::HELD) {
        bootstrapped_ = true;
        std::int64_t size0 = 0;
        int rc = aria_map_size(mapper_.handle(), &size0);
        if (rc != ARIA_OK) throw std::runtime_error("MapTracker: aria_map_size failed");
        step.added = mapper_.triangulateExtrinsics(previous, current, matches, before.data(), now.data(), previous_image, width, height,
                                                   previous_is_query);
        if (step.added > 0) {                                      // the pair id the mapper gave these points
            aria_map_point first{};
            if ((rc = aria_map_read(mapper_.handle(), size0, 1, &first)) != ARIA_OK) throw std::runtime_error("MapTracker: aria_map_read failed");
            anchor_pair_ = first.pair;
            if (builder_) {
                appended.resize((std::size_t)step.added);
                if ((rc = aria_map_read(mapper_.handle(), size0, step.added, appended.data())) != ARIA_OK)
                    throw std::runtime_error("MapTracker: aria_map_read failed");
            }
        }
    }
    if (builder_) builder_->addStep(current, now.data(), matches, previous_is_query, appended);
    pose_ = now;
    return step;
}

}  // namespace aria::adapters::hip
