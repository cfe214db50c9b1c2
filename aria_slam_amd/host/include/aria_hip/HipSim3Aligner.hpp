// aria::adapters::hip::HipSim3Aligner -- loop alignment over the C-ABI (include/aria_orb_hip.h, "loop alignment"): the
// similarity X2 = s R X1 + t between the landmarks two keyframes of a loop own, by Sim(3) RANSAC on the device. It gives a loop
// edge its translation in map units and reports the scale drift s around the loop. The reference has no code for it (its H09
// and H10 audits name the loop edge's unknown scale as open); aria_slam_amd/sim3_ref.py is the definition of every step.
//
// makeSim3Verifier turns it into a HipLoopDetector::Verifier that runs AFTER another verifier (makeReferenceVerifier) has
// accepted a candidate: it joins the two keyframes' landmarks through the candidate's match list, aligns them, and when the
// result is valid with n_inliers >= min_inliers (default 20, ORB-SLAM's constant, untuned) overwrites candidate.relative_pose
// with [R t], in the convention makeReferenceVerifier fills (query keyframe -> matched keyframe). Otherwise the candidate is
// left as it was. It never rejects. s is only reported (Sim3Report): the SE(3) pose graph takes [R t].
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <optional>
#include <vector>

#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

// X2 = s R X1 + t; R row-major
struct Similarity {
    std::array<double, 9> R{};
    std::array<double, 3> t{};
    double s = 1.0;
    double rms_px = 0.0;
    int n_corr = 0, n_inliers = 0, iterations = 0;
    bool refined = false;
    std::vector<std::uint8_t> mask;     // per correspondence: inlier of the returned model
};

// What the caller knows about a keyframe's place in the map: the pair id whose points it owns (MapTracker::anchorPair() when
// the keyframe was the last frame), which view of that pair it is (MapTracker: 2), its world-to-camera pose (rows of [R t],
// MapTracker::pose()), and its frame (the keypoints).
struct KeyframeInMap {
    int anchor_pair = -1;
    int anchor_view = 2;
    std::array<double, 12> pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const core::Frame* frame = nullptr;
};

class HipSim3Aligner {
public:
    explicit HipSim3Aligner(const PoseIntrinsics& K = {}, int hypotheses = 1024, double threshold_px = 3.0, int refine_iters = 5,
                            bool fix_scale = false, std::uint64_t seed = 0, void* stream = nullptr, int device = 0,
                            double min_scale = 0.05, double max_scale = 20.0);   // a model with s outside them is invalid
    ~HipSim3Aligner();

    // std::nullopt when the stage finds no model (fewer than 3 correspondences, no valid hypothesis). A model is not a loop:
    // gate on n_inliers.
    std::optional<Similarity> estimate(const std::vector<aria_sim3_corr>& corr, int pair_id = 0);

    // Two keyframes against the map, joined on the device (aria_sim3_associate_batch_device, then
    // aria_sim3_estimate_batch_device on the handle's stream; the map's host calls have synchronised before). `matches` pair
    // kf1 (query_idx) with kf2 (train_idx). n_corr (optional): the correspondences the join found; match_index (optional):
    // each correspondence's index in `matches`. std::nullopt when the stage finds no model.
    std::optional<Similarity> estimateAgainstMap(aria_map_t map, const KeyframeInMap& kf1, const KeyframeInMap& kf2,
                                                 const std::vector<core::Match>& matches, int pair_id = 0, int* n_corr = nullptr,
                                                 std::vector<int>* match_index = nullptr);
    aria_sim3_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipSim3Aligner", where, rc); }
    detail::DeviceScratch scratch_;     // staging of estimateAgainstMap; before h_ (see Stage.hpp, DECLARATION ORDER)
    detail::StageOwner<aria_sim3_t, aria_sim3_destroy> h_;
};

// One line of what the verifier did with a candidate
struct Sim3Report {
    std::uint64_t query_id = 0, match_id = 0;
    double s = 1.0, rms_px = 0.0;
    int n_corr = 0, n_inliers = 0;
    bool replaced = false;
};

// id -> the keyframe's place in the map, or std::nullopt when the caller does not know it (the candidate is then left alone)
using KeyframeInMapLookup = std::function<std::optional<KeyframeInMap>(std::uint64_t id)>;

// See the top of this file. `inner` (optional) runs first and decides acceptance; `report` (optional) receives one record per
// candidate `inner` accepted. The aligner, the map and the lookup must outlive the detector's use of the verifier.
HipLoopDetector::Verifier makeSim3Verifier(HipSim3Aligner& aligner, aria_map_t map, KeyframeInMapLookup keyframes,
                                           HipLoopDetector::Verifier inner = nullptr, int min_inliers = 20,
                                           std::function<void(const Sim3Report&)> report = nullptr);

}  // namespace aria::adapters::hip
