// See aria_hip/HipFundamentalEstimator.hpp.
#include "aria_hip/HipFundamentalEstimator.hpp"

#include <utility>

namespace aria::adapters::hip {

namespace {
// LoopCandidate::relative_pose: Eigen::Matrix4d in the reference (core/Types.hpp:120), column-major double[16] in the
// stand-in (compat.hpp) -- as in HipPoseEstimator.cpp
template <typename M>
auto setPose(M& m, const std::array<double, 16>& T, int) -> decltype(m(0, 0) = 0.0, void()) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) m(r, c) = T[(size_t)(r * 4 + c)];
}
template <typename M>
void setPose(M& m, const std::array<double, 16>& T, long) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) m[c * 4 + r] = T[(size_t)(r * 4 + c)];
}
}  // namespace

HipLoopDetector::Verifier makeReferenceVerifier(HipFundamentalEstimator& fund, HipPoseEstimator& pose, int min_matches,
                                                KeyFrameLookup keyframes) {
    if (min_matches < 15)
        throw std::invalid_argument("makeReferenceVerifier: min_matches must be >= 15 (findFundamentalMat's RANSAC branch)");
    return [&fund, &pose, min_matches, keyframes](const core::KeyFrame& query, std::uint64_t match_id, core::LoopCandidate& cand) {
        const core::Frame* other = keyframes ? keyframes(match_id) : nullptr;
        if (!other) return false;
        if ((int)cand.matches.size() < min_matches) return false;                     // LoopClosure.cpp:132
        const std::optional<FundamentalResult> f = fund.estimate(query.frame, *other, cand.matches, true, 0);
        if (!f || f->n_inliers < min_matches) return false;                            // :145, :155
        std::vector<core::Match> inliers;
        inliers.reserve((size_t)f->n_inliers);
        for (std::size_t i = 0; i < cand.matches.size(); i++)
            if (f->mask[i]) inliers.push_back(cand.matches[i]);
        if (inliers.size() < 8) return false;                                          // :161
        const std::optional<TwoViewPose> p = pose.estimate(query.frame, *other, inliers, true, 0);
        if (!p || p->n_pose_inliers < min_matches) return false;                       // :177, :183
        setPose(cand.relative_pose, poseMatrix(*p), 0);
        cand.matches = std::move(inliers);
        return true;
    };
}

}  // namespace aria::adapters::hip
