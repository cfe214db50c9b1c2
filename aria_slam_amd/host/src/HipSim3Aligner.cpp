// See aria_hip/HipSim3Aligner.hpp.
#include "aria_hip/HipSim3Aligner.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "aria_hip/HipPoseGraphOptimizer.hpp"

namespace aria::adapters::hip {

HipSim3Aligner::HipSim3Aligner(const PoseIntrinsics& K, int hypotheses, double threshold_px, int refine_iters, bool fix_scale,
                               std::uint64_t seed, void* stream, int device, double min_scale, double max_scale)
    : scratch_("HipSim3Aligner", device) {
    aria_sim3_config c;
    aria_sim3_default_config(&c);
    c.device = device;
    c.stream = stream;
    c.hypotheses = hypotheses;
    c.refine_iters = refine_iters;
    c.fix_scale = fix_scale ? 1 : 0;
    c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy;
    c.threshold_px = threshold_px;
    c.seed = seed;
    c.min_scale = min_scale;
    c.max_scale = max_scale;
    expect("aria_sim3_create", aria_sim3_create(&c, h_.out()));
}

HipSim3Aligner::~HipSim3Aligner() = default;

namespace {
Similarity fromRecord(const aria_sim3_result& r) {
    Similarity out;
    for (int k = 0; k < 9; k++) out.R[(size_t)k] = r.R[k];
    for (int k = 0; k < 3; k++) out.t[(size_t)k] = r.t[k];
    out.s = r.s;
    out.rms_px = r.rms_px;
    out.n_corr = r.n_corr;
    out.n_inliers = r.n_inliers;
    out.iterations = r.iterations;
    out.refined = r.refined != 0;
    return out;
}
}  // namespace

std::optional<Similarity> HipSim3Aligner::estimate(const std::vector<aria_sim3_corr>& corr, int pair_id) {
    aria_sim3_result r{};
    std::vector<std::uint8_t> mask(corr.size(), 0);
    expect("aria_sim3_estimate", aria_sim3_estimate(h_.get(), corr.data(), (int)corr.size(), pair_id, &r, mask.data()));
    if (!r.valid) return std::nullopt;
    Similarity out = fromRecord(r);
    out.mask = std::move(mask);
    return out;
}

std::optional<Similarity> HipSim3Aligner::estimateAgainstMap(aria_map_t map, const KeyframeInMap& kf1, const KeyframeInMap& kf2,
                                                             const std::vector<core::Match>& matches, int pair_id, int* n_corr,
                                                             std::vector<int>* match_index) {
    static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");
    if (n_corr) *n_corr = 0;
    if (match_index) match_index->clear();
    if (!kf1.frame || !kf2.frame) return std::nullopt;
    const std::size_t n = matches.size(), n1 = kf1.frame->keypoints.size(), n2 = kf2.frame->keypoints.size();
    if (!n || !n1 || !n2) return std::nullopt;
    const std::size_t stride = std::max(n1, n2);
    detail::ScratchLayout lay;
    const std::size_t o_k1 = lay.take(stride * sizeof(aria_keypoint)), o_k2 = lay.take(stride * sizeof(aria_keypoint)),
                      o_m = lay.take(n * sizeof(aria_match)), o_cnt = lay.take(256), o_pose = lay.take(256),
                      o_corr = lay.take(n * sizeof(aria_sim3_corr)), o_back = lay.take(n * sizeof(int)), o_out = lay.take(256),
                      o_mask = lay.take(n);
    void* st = aria_sim3_stream(h_.get());
    const int dev = scratch_.device();
    scratch_.reserve(st, lay.total);
    char* d = scratch_.data();
    // counts: [0] n1, [1] n2, [2] n_matches, [3] the join's count, [4] anchor 1, [5] anchor 2
    const int counts[6] = {(int)n1, (int)n2, (int)n, 0, kf1.anchor_pair, kf2.anchor_pair};
    double poses[24];
    for (int k = 0; k < 12; k++) {
        poses[k] = kf1.pose[(size_t)k];
        poses[12 + k] = kf2.pose[(size_t)k];
    }
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_k1, kf1.frame->keypoints.data(), n1 * sizeof(aria_keypoint)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_k2, kf2.frame->keypoints.data(), n2 * sizeof(aria_keypoint)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_m, matches.data(), n * sizeof(aria_match)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_cnt, counts, sizeof(counts)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_pose, poses, sizeof(poses)));
    int* d_cnt = reinterpret_cast<int*>(d + o_cnt);
    const double* d_pose = reinterpret_cast<const double*>(d + o_pose);
    expect("aria_sim3_associate_batch_device",
           aria_sim3_associate_batch_device(h_.get(), map, d_cnt + 4, d_cnt + 5, kf1.anchor_view, kf2.anchor_view, d_pose, d_pose + 12,
                                            reinterpret_cast<const aria_keypoint*>(d + o_k1), d_cnt,
                                            reinterpret_cast<const aria_keypoint*>(d + o_k2), d_cnt + 1, (std::int64_t)stride,
                                            reinterpret_cast<const aria_match*>(d + o_m), d_cnt + 2, 1, (int)n,
                                            reinterpret_cast<aria_sim3_corr*>(d + o_corr), d_cnt + 3, reinterpret_cast<int*>(d + o_back)));
    expect("aria_sim3_estimate_batch_device",
           aria_sim3_estimate_batch_device(h_.get(), reinterpret_cast<const aria_sim3_corr*>(d + o_corr), d_cnt + 3, 1, (int)n, pair_id,
                                           reinterpret_cast<aria_sim3_result*>(d + o_out), reinterpret_cast<std::uint8_t*>(d + o_mask)));
    aria_sim3_result r{};
    int found = 0;
    std::vector<std::uint8_t> mask(n);
    std::vector<int> back(n);
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, &r, d + o_out, sizeof(r)));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, &found, d_cnt + 3, sizeof(int)));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, mask.data(), d + o_mask, n));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, back.data(), d + o_back, n * sizeof(int)));
    expect("aria_sim3_check", aria_sim3_check(h_.get()));   // synchronises the stream
    if (n_corr) *n_corr = found;
    if (match_index) match_index->assign(back.begin(), back.begin() + found);
    if (!r.valid) return std::nullopt;
    Similarity out = fromRecord(r);
    out.mask.assign(mask.begin(), mask.begin() + found);
    return out;
}

HipLoopDetector::Verifier makeSim3Verifier(HipSim3Aligner& aligner, aria_map_t map, KeyframeInMapLookup keyframes,
                                           HipLoopDetector::Verifier inner, int min_inliers,
                                           std::function<void(const Sim3Report&)> report) {
    return [&aligner, map, keyframes, inner, min_inliers, report](const core::KeyFrame& query, std::uint64_t match_id,
                                                                  core::LoopCandidate& cand) {
        if (inner && !inner(query, match_id, cand)) return false;
        Sim3Report rep;
        rep.query_id = query.id;
        rep.match_id = match_id;
        const auto kq = keyframes ? keyframes(query.id) : std::nullopt;
        const auto km = keyframes ? keyframes(match_id) : std::nullopt;
        if (kq && km && kq->anchor_pair >= 0 && km->anchor_pair >= 0) {
            // the match list's query side is the query keyframe: keyframe 1
            const auto sim = aligner.estimateAgainstMap(map, *kq, *km, cand.matches, (int)(query.id & 0x3FFFFFFF), &rep.n_corr);
            if (sim) {
                rep.s = sim->s;
                rep.rms_px = sim->rms_px;
                rep.n_inliers = sim->n_inliers;
                if (sim->n_inliers >= min_inliers) {
                    for (int r = 0; r < 3; r++) {
                        for (int c = 0; c < 3; c++) detail::setEntry(cand.relative_pose, r, c, sim->R[(size_t)(r * 3 + c)], 0);
                        detail::setEntry(cand.relative_pose, r, 3, sim->t[(size_t)r], 0);
                    }
                    for (int c = 0; c < 4; c++) detail::setEntry(cand.relative_pose, 3, c, c == 3 ? 1.0 : 0.0, 0);
                    rep.replaced = true;
                }
            }
        }
        if (report) report(rep);
        return true;
    };
}

}  // namespace aria::adapters::hip
