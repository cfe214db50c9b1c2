// See aria_hip/MapTracker.hpp.
#include "aria_hip/MapTracker.hpp"

#include <stdexcept>

namespace aria::adapters::hip {

MapTracker::MapTracker(const MapperConfig& map_cfg, int min_pose_inliers, int hypotheses, int pnp_solver)
    : mapper_(map_cfg), pnp_(map_cfg.K, hypotheses, map_cfg.max_reproj_px, 5, 0, nullptr, map_cfg.device),
      min_pose_inliers_(min_pose_inliers), pose_{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, before_last_(pose_), K_(map_cfg.K),
      min_depth_(map_cfg.min_depth), device_(map_cfg.device) {
    if (pnp_solver != ARIA_PNP_SOLVER_DLT6) pnp_.setSolver(pnp_solver);
}

void MapTracker::setLocalMap(int pairs, float radius_px) {
    local_pairs_ = pairs > 0 ? pairs : 0;
    proj_.reset();
    if (!local_pairs_) return;
    ProjectionConfig c;
    c.K = K_;
    c.min_depth = min_depth_;
    c.radius_px = radius_px;
    c.device = device_;
    proj_ = std::make_unique<HipProjectionMatcher>(c);
}

namespace {

// a * b of 4x4 row-major matrices
std::array<double, 16> mul4(const std::array<double, 16>& a, const std::array<double, 16>& b) {
    std::array<double, 16> o{};
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double v = 0.0;
            for (int k = 0; k < 4; k++) v += a[(size_t)(r * 4 + k)] * b[(size_t)(k * 4 + c)];
            o[(size_t)(r * 4 + c)] = v;
        }
    return o;
}

// the inverse of a rigid [R t; 0 1]
std::array<double, 16> inverseRigid(const std::array<double, 16>& m) {
    std::array<double, 16> o{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[(size_t)(r * 4 + c)] = m[(size_t)(c * 4 + r)];
        o[(size_t)(r * 4 + 3)] = -(m[(size_t)r] * m[3] + m[(size_t)(4 + r)] * m[7] + m[(size_t)(8 + r)] * m[11]);
    }
    o[15] = 1.0;
    return o;
}

}  // namespace

TrackStep MapTracker::track(const core::Frame& previous, const core::Frame& current, const std::vector<core::Match>& matches,
                            bool previous_is_query, const std::optional<TwoViewPose>& two_view, const std::uint8_t* previous_image,
                            int width, int height) {
    TrackStep step;
    const std::array<double, 16> before = pose_;
    std::array<double, 16> now = before;
    steps_++;
    if (local_pairs_ && !pair_start_.empty()) {
        // predicted world-to-camera pose of `current`: the last step's motion once more, or the last pose
        const std::array<double, 16> predicted = placed_last_ && placed_before_ ? mul4(mul4(before, inverseRigid(before_last_)), before) : before;
        const std::size_t k0 = pair_start_.size() > (std::size_t)local_pairs_ ? pair_start_.size() - (std::size_t)local_pairs_ : 0;
        const std::size_t first = pair_start_[k0], count = landmarks_.size() - first;
        if (count && !current.keypoints.empty()) {
            const ProjectionMatches found = proj_->search(predicted.data(), current, landmarks_, first, count, width > 0 ? width : 4096,
                                                          height > 0 ? height : 4096);
            step.n_corr = (int)found.corr.size();
            const std::optional<AbsolutePose> p = pnp_.estimate(found.corr, steps_);
            if (p) step.n_inliers = p->n_inliers;
            if (p && p->n_inliers > min_pose_inliers_) {
                now = poseMatrix(*p);
                step.source = TrackStep::LOCAL;
            }
        }
    }
    if (step.source == TrackStep::HELD && anchor_pair_ >= 0) {     // the last pair's points index `previous` by idx2
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
    std::int64_t size0 = 0;                                         // the arena position of the step's first new point
    if (builder_ && builder_->frames() == 0) builder_->addFrame(previous, before.data());
    if (step.source != TrackStep::HELD) {
        bootstrapped_ = true;
        int rc = aria_map_size(mapper_.handle(), &size0);
        if (rc != ARIA_OK) throw std::runtime_error("MapTracker: aria_map_size failed");
        step.added = mapper_.triangulateExtrinsics(previous, current, matches, before.data(), now.data(), previous_image, width, height,
                                                   previous_is_query);
        if (step.added > 0) {                                      // the pair id the mapper gave these points
            aria_map_point first{};
            if ((rc = aria_map_read(mapper_.handle(), size0, 1, &first)) != ARIA_OK) throw std::runtime_error("MapTracker: aria_map_read failed");
            anchor_pair_ = first.pair;
            if (builder_ || local_pairs_) {
                appended.resize((std::size_t)step.added);
                if ((rc = aria_map_read(mapper_.handle(), size0, step.added, appended.data())) != ARIA_OK)
                    throw std::runtime_error("MapTracker: aria_map_read failed");
            }
        }
    }
    if (local_pairs_ && !appended.empty()) {                       // view 2 of the new points is `current`
        pair_start_.push_back(landmarks_.size());
        for (std::size_t j = 0; j < appended.size(); j++)
            landmarks_.push_back(landmarkFromPoint(appended[j], current, appended[j].idx2, (int)(size0 + (std::int64_t)j)));
    }
    if (builder_) builder_->addStep(current, now.data(), matches, previous_is_query, appended);
    before_last_ = before;
    placed_before_ = placed_last_;
    placed_last_ = step.source != TrackStep::HELD;
    pose_ = now;
    return step;
}

}  // namespace aria::adapters::hip
