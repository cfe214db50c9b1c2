// aria::adapters::hip::HipFundamentalEstimator -- fundamental-matrix RANSAC over the C-ABI (include/aria_orb_hip.h,
// "fundamental-matrix RANSAC"): what the reference's loop verification computes with
// cv::findFundamentalMat(pts1, pts2, FM_RANSAC, 3.0, 0.99, mask) (src/legacy/LoopClosure.cpp:116-155), on the device.
//
// makeReferenceVerifier turns it and a HipPoseEstimator into a HipLoopDetector::Verifier that accepts exactly the loops
// LoopClosureDetector accepts: verifyGeometry (F-RANSAC, at least min_matches F inliers) then computeRelativePose on the F
// inliers (E-RANSAC + recoverPose with K = referenceLoopIntrinsics(), at least min_matches points), keeping the F inliers
// in candidate.matches. Opt-in: the detector's default stays the match-count test, makeGeometricVerifier stays as it is.
#pragma once
#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

// x2^T F x1 = 0 in pixel coordinates, F row-major
struct FundamentalResult {
    std::array<double, 9> F{};
    int n_matches = 0, n_inliers = 0, n_models = 0;
    std::vector<std::uint8_t> mask;     // per match: inlier of F
};

// The members are inline, like HipPoseEstimator's: they need nothing but the C-ABI.
class HipFundamentalEstimator {
public:
    explicit HipFundamentalEstimator(int hypotheses = 1024, double threshold_px = 3.0, std::uint64_t seed = 0,
                                     void* stream = nullptr, int device = 0) {
        aria_fund_config c;
        aria_fund_default_config(&c);
        c.device = device;
        c.stream = stream;
        c.hypotheses = hypotheses;
        c.threshold_px = threshold_px;
        c.seed = seed;
        expect("aria_fund_create", aria_fund_create(&c, h_.out()));
    }

    // view 1 = `first`, view 2 = `second`; query_is_first as in HipPoseEstimator::estimate. std::nullopt when the stage
    // finds no F (fewer than 15 matches, no model with 7 inliers).
    std::optional<FundamentalResult> estimate(const core::Frame& first, const core::Frame& second,
                                              const std::vector<core::Match>& matches, bool query_is_first = true,
                                              int pair_id = 0) {
        static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");
        const core::Frame& q = query_is_first ? first : second;
        const core::Frame& t = query_is_first ? second : first;
        aria_fund_result r{};
        FundamentalResult out;
        out.mask.assign(matches.size(), 0);
        expect("aria_fund_estimate",
               aria_fund_estimate(h_.get(), reinterpret_cast<const aria_keypoint*>(q.keypoints.data()), (int)q.keypoints.size(),
                                  reinterpret_cast<const aria_keypoint*>(t.keypoints.data()), (int)t.keypoints.size(),
                                  reinterpret_cast<const aria_match*>(matches.data()), (int)matches.size(),
                                  query_is_first ? 1 : 0, pair_id, &r, out.mask.data()));
        if (!r.valid) return std::nullopt;
        for (int k = 0; k < 9; k++) out.F[(size_t)k] = r.F[k];
        out.n_matches = r.n_matches;
        out.n_inliers = r.n_inliers;
        out.n_models = r.n_models;
        return out;
    }
    aria_fund_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipFundamentalEstimator", where, rc); }
    detail::StageOwner<aria_fund_t, aria_fund_destroy> h_;
};

// computeRelativePose's hard-coded camera (LoopClosure.cpp:171-174): build the HipPoseEstimator of makeReferenceVerifier
// with it (and the default threshold of 1 px) to verify as the reference does
inline PoseIntrinsics referenceLoopIntrinsics() { return PoseIntrinsics{700.0, 700.0, 320.0, 180.0}; }

// LoopClosure.cpp:116-195 over the device, view 1 = the query keyframe: reject when the ratio-0.7 list has fewer than
// min_matches entries, when F-RANSAC finds no F or fewer than min_matches inliers, when the F inliers are fewer than 8,
// when the pose stage on the F inliers finds no E or n_pose_inliers < min_matches; else fill candidate.relative_pose as
// makeGeometricVerifier does and leave the F inliers, in list order, in candidate.matches. Throws std::invalid_argument
// when min_matches < 15 (the stage restates only findFundamentalMat's RANSAC branch, n >= 15).
HipLoopDetector::Verifier makeReferenceVerifier(HipFundamentalEstimator& fund, HipPoseEstimator& pose, int min_matches,
                                                KeyFrameLookup keyframes);

}  // namespace aria::adapters::hip
