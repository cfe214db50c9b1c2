// aria::adapters::hip::HipPoseEstimator -- two-view relative pose over the C-ABI (include/aria_orb_hip.h, "two-view relative
// pose"): what the reference computes with cv::findEssentialMat(pts1, pts2, K, RANSAC, 0.999, 1.0) + cv::recoverPose after
// every match list (src/euroc_eval.cpp:178-201, src/legacy/LoopClosure.cpp:116-190), as essential-matrix RANSAC on the device.
//
// makeGeometricVerifier turns it into a HipLoopDetector::Verifier (opt-in; the detector's default stays the match-count
// test). Three differences from the reference's LoopClosureDetector: it verifies with E-RANSAC where verifyGeometry used
// F-RANSAC (cv::findFundamentalMat, LoopClosure.cpp:141-143), the caller passes K where computeRelativePose hard-codes its
// own (:171-174), and candidate.matches keeps the pose inliers where the reference keeps the F inliers (:58).
// makeReferenceVerifier (aria_hip/HipFundamentalEstimator.hpp) has none of them: it accepts the reference's loops.
#pragma once
#include <array>
#include <functional>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct PoseIntrinsics {          // EuRoC cam0 by default (src/legacy/EuRoCReader.cpp:11-17)
    double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;
};

// x2 ~ R x1 + t, |t| = 1 (recoverPose's convention); R row-major
struct TwoViewPose {
    std::array<double, 9> R{};
    std::array<double, 3> t{};
    std::array<double, 9> E{};
    int n_matches = 0, n_inliers = 0, n_pose_inliers = 0;
    bool refined = false;
    std::vector<std::uint8_t> mask;     // per match: RANSAC inlier AND in front of both cameras
};

// The members are inline: FrontEnd (estimate_pose) uses them, and they need nothing but the C-ABI.
class HipPoseEstimator {
public:
    explicit HipPoseEstimator(const PoseIntrinsics& K = {}, int hypotheses = 1024, double threshold_px = 1.0,
                              double distance_thresh = 50.0, std::uint64_t seed = 0, void* stream = nullptr, int device = 0) {
        aria_pose_config c;
        aria_pose_default_config(&c);
        c.device = device;
        c.stream = stream;
        c.hypotheses = hypotheses;
        c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy;
        c.threshold_px = threshold_px;
        c.distance_thresh = distance_thresh;
        c.seed = seed;
        expect("aria_pose_create", aria_pose_create(&c, h_.out()));
    }

    // view 1 = `first`, view 2 = `second`; query_is_first says which side of each match `first` is (true: match.query_idx
    // indexes first.keypoints). std::nullopt when the stage finds no pose (fewer than 8 matches, no valid hypothesis).
    std::optional<TwoViewPose> estimate(const core::Frame& first, const core::Frame& second, const std::vector<core::Match>& matches,
                                        bool query_is_first = true, int pair_id = 0) {
        static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");
        const core::Frame& q = query_is_first ? first : second;
        const core::Frame& t = query_is_first ? second : first;
        aria_pose_result r{};
        TwoViewPose out;
        out.mask.assign(matches.size(), 0);
        expect("aria_pose_estimate",
               aria_pose_estimate(h_.get(), reinterpret_cast<const aria_keypoint*>(q.keypoints.data()), (int)q.keypoints.size(),
                                  reinterpret_cast<const aria_keypoint*>(t.keypoints.data()), (int)t.keypoints.size(),
                                  reinterpret_cast<const aria_match*>(matches.data()), (int)matches.size(),
                                  query_is_first ? 1 : 0, pair_id, &r, out.mask.data()));
        if (!r.valid) return std::nullopt;
        for (int k = 0; k < 9; k++) { out.R[(size_t)k] = r.R[k]; out.E[(size_t)k] = r.E[k]; }
        for (int k = 0; k < 3; k++) out.t[(size_t)k] = r.t[k];
        out.n_matches = r.n_matches;
        out.n_inliers = r.n_inliers;
        out.n_pose_inliers = r.n_pose_inliers;
        out.refined = r.refined != 0;
        return out;
    }
    aria_pose_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipPoseEstimator", where, rc); }
    detail::StageOwner<aria_pose_t, aria_pose_destroy> h_;
};

// 4x4 row-major [R t; 0 1] of a pose
std::array<double, 16> poseMatrix(const TwoViewPose& p);

// LoopClosure.cpp:116-190 over the device: estimate the pose query -> match (view 1 = the query keyframe, whose keypoints
// candidate.matches index as query_idx); reject when n_pose_inliers < min_inliers (:181-183), else fill
// candidate.relative_pose ([R t; 0 1]; column-major storage in the stand-in's double[16], as Eigen::Matrix4d stores it) and
// keep only the pose inliers in candidate.matches (the reference keeps the F inliers; see makeReferenceVerifier for its
// exact acceptance). `keyframes` resolves a match id to the
// keyframe's frame (its keypoints): the detector's database keeps descriptors only, so the caller, who holds the keyframes,
// supplies them.
using KeyFrameLookup = std::function<const core::Frame*(std::uint64_t id)>;
HipLoopDetector::Verifier makeGeometricVerifier(HipPoseEstimator& est, int min_inliers, KeyFrameLookup keyframes);

}  // namespace aria::adapters::hip
