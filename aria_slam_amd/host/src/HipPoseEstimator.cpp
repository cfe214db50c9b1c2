// See aria_hip/HipPoseEstimator.hpp.
#include "aria_hip/HipPoseEstimator.hpp"

namespace aria::adapters::hip {

namespace {
// LoopCandidate::relative_pose is an Eigen::Matrix4d in the reference (core/Types.hpp:120) and a double[16] in the stand-in
// (compat.hpp), stored column-major like Eigen's
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

std::array<double, 16> poseMatrix(const TwoViewPose& p) {
    std::array<double, 16> m{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[(size_t)(r * 4 + c)] = p.R[(size_t)(r * 3 + c)];
        m[(size_t)(r * 4 + 3)] = p.t[(size_t)r];
    }
    m[15] = 1.0;
    return m;
}

HipLoopDetector::Verifier makeGeometricVerifier(HipPoseEstimator& est, int min_inliers, KeyFrameLookup keyframes) {
    return [&est, min_inliers, keyframes](const core::KeyFrame& query, std::uint64_t match_id, core::LoopCandidate& cand) {
        const core::Frame* other = keyframes ? keyframes(match_id) : nullptr;
        if (!other) return false;
        // view 1 = the query keyframe (query side of the ratio-0.7 match list), view 2 = the matched keyframe
        const std::optional<TwoViewPose> p = est.estimate(query.frame, *other, cand.matches, true, 0);
        if (!p || p->n_pose_inliers < min_inliers) return false;                   // LoopClosure.cpp:181-183
        setPose(cand.relative_pose, poseMatrix(*p), 0);
        std::size_t kept = 0;
        for (std::size_t i = 0; i < cand.matches.size(); i++)
            if (p->mask[i]) cand.matches[kept++] = cand.matches[i];
        cand.matches.resize(kept);
        return true;
    };
}

}  // namespace aria::adapters::hip
