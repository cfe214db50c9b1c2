// See aria_hip/HipPnPEstimator.hpp.
#include "aria_hip/HipPnPEstimator.hpp"

#include <stdexcept>
#include <string>
#include <algorithm>

namespace aria::adapters::hip {

namespace {
AbsolutePose fromRecord(const aria_pnp_result& r) {
    AbsolutePose out;
    for (int k = 0; k < 9; k++) out.R[(size_t)k] = r.R[k];
    for (int k = 0; k < 3; k++) out.t[(size_t)k] = r.t[k];
    out.rms_px = r.rms_px;
    out.n_corr = r.n_corr;
    out.n_inliers = r.n_inliers;
    out.iterations = r.iterations;
    out.refined = r.refined != 0;
    return out;
}
}  // namespace

HipPnPEstimator::HipPnPEstimator(const PoseIntrinsics& K, int hypotheses, double threshold_px, int refine_iters, std::uint64_t seed,
                                 void* stream, int device)
    : scratch_("HipPnPEstimator", device) {
    aria_pnp_config c;
    aria_pnp_default_config(&c);
    c.device = device;
    c.stream = stream;
    c.hypotheses = hypotheses;
    c.refine_iters = refine_iters;
    c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy;
    c.threshold_px = threshold_px;
    c.seed = seed;
    expect("aria_pnp_create", aria_pnp_create(&c, h_.out()));
}

HipPnPEstimator::~HipPnPEstimator() = default;

void HipPnPEstimator::setSolver(int solver) { expect("aria_pnp_set_solver", aria_pnp_set_solver(h_.get(), solver)); }

std::optional<AbsolutePose> HipPnPEstimator::estimate(const std::vector<aria_pnp_corr>& corr, int pair_id) {
    aria_pnp_result r{};
    std::vector<std::uint8_t> mask(corr.size(), 0);
    expect("aria_pnp_estimate", aria_pnp_estimate(h_.get(), corr.data(), (int)corr.size(), pair_id, &r, mask.data()));
    if (!r.valid) return std::nullopt;
    AbsolutePose out = fromRecord(r);
    out.mask = std::move(mask);
    return out;
}

std::optional<AbsolutePose> HipPnPEstimator::estimateAgainstMap(aria_map_t map, int anchor_pair, int anchor_view,
                                                                const core::Frame& tracked, const std::vector<core::Match>& matches,
                                                                bool anchor_is_query, int pair_id, int* n_corr,
                                                                std::vector<int>* match_index) {
    static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");
    if (n_corr) *n_corr = 0;
    if (match_index) match_index->clear();
    const std::size_t n = matches.size(), nk = tracked.keypoints.size();
    if (!n || !nk) return std::nullopt;
    // the join takes the anchor frame on the train side
    std::vector<aria_match> m(n);
    std::size_t stride = nk;
    for (std::size_t i = 0; i < n; i++) {
        m[i].query_idx = anchor_is_query ? matches[i].train_idx : matches[i].query_idx;
        m[i].train_idx = anchor_is_query ? matches[i].query_idx : matches[i].train_idx;
        m[i].distance = matches[i].distance;
        if (m[i].train_idx >= 0) stride = std::max(stride, (std::size_t)m[i].train_idx + 1);
    }
    detail::ScratchLayout lay;
    const std::size_t o_kp = lay.take(stride * sizeof(aria_keypoint)), o_m = lay.take(n * sizeof(aria_match)), o_cnt = lay.take(256),
                      o_corr = lay.take(n * sizeof(aria_pnp_corr)), o_back = lay.take(n * sizeof(int)), o_out = lay.take(256),
                      o_mask = lay.take(n);
    void* st = aria_pnp_stream(h_.get());
    const int dev = scratch_.device();
    scratch_.reserve(st, lay.total);
    char* d = scratch_.data();
    const int counts[3] = {(int)nk, (int)n, 0};                  // nq, n_matches; [2] receives the join's count
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_kp, tracked.keypoints.data(), nk * sizeof(aria_keypoint)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_m, m.data(), n * sizeof(aria_match)));
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d + o_cnt, counts, sizeof(counts)));
    int* d_cnt = reinterpret_cast<int*>(d + o_cnt);
    expect("aria_pnp_associate_batch_device",
           aria_pnp_associate_batch_device(h_.get(), map, anchor_pair, anchor_view, reinterpret_cast<const aria_keypoint*>(d + o_kp), d_cnt,
                                           (std::int64_t)stride, reinterpret_cast<const aria_match*>(d + o_m), d_cnt + 1, 1, (int)n,
                                           reinterpret_cast<aria_pnp_corr*>(d + o_corr), d_cnt + 2, reinterpret_cast<int*>(d + o_back)));
    expect("aria_pnp_estimate_batch_device",
           aria_pnp_estimate_batch_device(h_.get(), reinterpret_cast<const aria_pnp_corr*>(d + o_corr), d_cnt + 2, 1, (int)n, pair_id,
                                          reinterpret_cast<aria_pnp_result*>(d + o_out), reinterpret_cast<std::uint8_t*>(d + o_mask)));
    aria_pnp_result r{};
    int found = 0;
    std::vector<std::uint8_t> mask(n);
    std::vector<int> back(n);
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, &r, d + o_out, sizeof(r)));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, &found, d_cnt + 2, sizeof(int)));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, mask.data(), d + o_mask, n));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, back.data(), d + o_back, n * sizeof(int)));
    expect("aria_pnp_check", aria_pnp_check(h_.get()));   // synchronises the stream
    if (n_corr) *n_corr = found;
    if (match_index) match_index->assign(back.begin(), back.begin() + found);
    if (!r.valid) return std::nullopt;
    AbsolutePose out = fromRecord(r);
    out.mask.assign(mask.begin(), mask.begin() + found);
    return out;
}

std::array<double, 16> poseMatrix(const AbsolutePose& p) {
    std::array<double, 16> m{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[(size_t)(r * 4 + c)] = p.R[(size_t)(r * 3 + c)];
        m[(size_t)(r * 4 + 3)] = p.t[(size_t)r];
    }
    m[15] = 1.0;
    return m;
}

}  // namespace aria::adapters::hip
