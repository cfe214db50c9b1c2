// See aria_hip/HipPnPEstimator.hpp.
#include "aria_hip/HipPnPEstimator.hpp"

#include <stdexcept>
#include <string>
#include <algorithm>

namespace aria::adapters::hip {

HipPnPEstimator::HipPnPEstimator(const PoseIntrinsics& K, int hypotheses, double threshold_px, int refine_iters, std::uint64_t seed,
                                 void* stream, int device) {
    aria_pnp_config c;
    aria_pnp_default_config(&c);
    c.device = device;
    c.stream = stream;
    c.hypotheses = hypotheses;
    c.refine_iters = refine_iters;
    c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy;
    c.threshold_px = threshold_px;
    c.seed = seed;
    device_ = device;
    const int rc = aria_pnp_create(&c, &h_);
    if (rc != ARIA_OK) fail("aria_pnp_create", rc);
}

HipPnPEstimator::~HipPnPEstimator() {
    aria_pnp_destroy(h_);                                          // drains the stream that reads d_buf_
    if (d_buf_) aria_device_free(device_, d_buf_);
}

void HipPnPEstimator::fail(const char* where, int status) {
    std::string msg = std::string("HipPnPEstimator: ") + where + ": " + aria_status_string(status);
    const char* hip = aria_last_hip_error();
    if (hip && hip[0]) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
}

void HipPnPEstimator::setSolver(int solver) {
    const int rc = aria_pnp_set_solver(h_, solver);
    if (rc != ARIA_OK) fail("aria_pnp_set_solver", rc);
}

std::optional<AbsolutePose> HipPnPEstimator::estimate(const std::vector<aria_pnp_corr>& corr, int pair_id) {
    aria_pnp_result r{};
    AbsolutePose out;
    out.mask.assign(corr.size(), 0);
    const int rc = aria_pnp_estimate(h_, corr.data(), (int)corr.size(), pair_id, &r, out.mask.data());
    if (rc != ARIA_OK) fail("aria_pnp_estimate", rc);
    if (!r.valid) return std::nullopt;
    for (int k = 0; k < 9; k++) out.R[(size_t)k] = r.R[k];
    for (int k = 0; k < 3; k++) out.t[(size_t)k] = r.t[k];
    out.rms_px = r.rms_px;
    out.n_corr = r.n_corr;
    out.n_inliers = r.n_inliers;
    out.iterations = r.iterations;
    out.refined = r.refined != 0;
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
    auto up = [](std::size_t b) { return (b + 255) / 256 * 256; };
    const std::size_t o_kp = 0, o_m = o_kp + up(stride * sizeof(aria_keypoint)), o_cnt = o_m + up(n * sizeof(aria_match)),
                      o_corr = o_cnt + 256, o_back = o_corr + up(n * sizeof(aria_pnp_corr)), o_out = o_back + up(n * sizeof(int)),
                      o_mask = o_out + 256, total = o_mask + up(n);
    int rc;
    void* st = aria_pnp_stream(h_);
    if (total > d_cap_) {
        if ((rc = aria_stream_synchronize(device_, st)) != ARIA_OK) fail("aria_stream_synchronize", rc);
        if (d_buf_) aria_device_free(device_, d_buf_);
        d_buf_ = nullptr;
        d_cap_ = 0;
        if ((rc = aria_device_alloc(device_, total, &d_buf_)) != ARIA_OK) fail("aria_device_alloc", rc);
        d_cap_ = total;
    }
    char* d = static_cast<char*>(d_buf_);
    const int counts[3] = {(int)nk, (int)n, 0};                  // nq, n_matches; [2] receives the join's count
    if ((rc = aria_copy_h2d_async(device_, st, d + o_kp, tracked.keypoints.data(), nk * sizeof(aria_keypoint))) != ARIA_OK ||
        (rc = aria_copy_h2d_async(device_, st, d + o_m, m.data(), n * sizeof(aria_match))) != ARIA_OK ||
        (rc = aria_copy_h2d_async(device_, st, d + o_cnt, counts, sizeof(counts))) != ARIA_OK)
        fail("aria_copy_h2d_async", rc);
    int* d_cnt = reinterpret_cast<int*>(d + o_cnt);
    rc = aria_pnp_associate_batch_device(h_, map, anchor_pair, anchor_view, reinterpret_cast<const aria_keypoint*>(d + o_kp), d_cnt,
                                         (std::int64_t)stride, reinterpret_cast<const aria_match*>(d + o_m), d_cnt + 1, 1, (int)n,
                                         reinterpret_cast<aria_pnp_corr*>(d + o_corr), d_cnt + 2, reinterpret_cast<int*>(d + o_back));
    if (rc != ARIA_OK) fail("aria_pnp_associate_batch_device", rc);
    rc = aria_pnp_estimate_batch_device(h_, reinterpret_cast<const aria_pnp_corr*>(d + o_corr), d_cnt + 2, 1, (int)n, pair_id,
                                        reinterpret_cast<aria_pnp_result*>(d + o_out), reinterpret_cast<std::uint8_t*>(d + o_mask));
    if (rc != ARIA_OK) fail("aria_pnp_estimate_batch_device", rc);
    aria_pnp_result r{};
    int found = 0;
    std::vector<std::uint8_t> mask(n);
    std::vector<int> back(n);
    if ((rc = aria_copy_d2h_async(device_, st, &r, d + o_out, sizeof(r))) != ARIA_OK ||
        (rc = aria_copy_d2h_async(device_, st, &found, d_cnt + 2, sizeof(int))) != ARIA_OK ||
        (rc = aria_copy_d2h_async(device_, st, mask.data(), d + o_mask, n)) != ARIA_OK ||
        (rc = aria_copy_d2h_async(device_, st, back.data(), d + o_back, n * sizeof(int))) != ARIA_OK)
        fail("aria_copy_d2h_async", rc);
    if ((rc = aria_pnp_check(h_)) != ARIA_OK) fail("aria_pnp_check", rc);   // synchronises the stream
    if (n_corr) *n_corr = found;
    if (match_index) match_index->assign(back.begin(), back.begin() + found);
    if (!r.valid) return std::nullopt;
    AbsolutePose out;
    for (int k = 0; k < 9; k++) out.R[(size_t)k] = r.R[k];
    for (int k = 0; k < 3; k++) out.t[(size_t)k] = r.t[k];
    out.rms_px = r.rms_px;
    out.n_corr = r.n_corr;
    out.n_inliers = r.n_inliers;
    out.iterations = r.iterations;
    out.refined = r.refined != 0;
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
