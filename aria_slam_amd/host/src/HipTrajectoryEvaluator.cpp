// See aria_hip/HipTrajectoryEvaluator.hpp.
#include "aria_hip/HipTrajectoryEvaluator.hpp"

#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

HipTrajectoryEvaluator::HipTrajectoryEvaluator(const aria_eval_config* cfg) {
    aria_eval_default_config(&cfg_);
    if (cfg) cfg_ = *cfg;
    expect("aria_eval_create", aria_eval_create(&cfg_, h_.out()));
}

HipTrajectoryEvaluator::~HipTrajectoryEvaluator() = default;

int HipTrajectoryEvaluator::sampleGroundTruth(const std::vector<aria_eval_truth>& gt, const std::vector<double>& timestamps,
                                              std::vector<aria_eval_truth>& out, std::vector<int>* valid) {
    out.assign(timestamps.size(), aria_eval_truth{});
    if (valid) valid->assign(timestamps.size(), 0);
    if (timestamps.empty()) return ARIA_OK;
    const int rc = aria_eval_sample_truth(h_.get(), gt.empty() ? nullptr : gt.data(), (int)gt.size(), timestamps.data(),
                                          (int)timestamps.size(), out.data(), valid ? valid->data() : nullptr);
    if (rc != ARIA_OK && rc != ARIA_E_INVALID) fail("aria_eval_sample_truth", rc);
    return rc;
}

aria_eval_result HipTrajectoryEvaluator::evaluate(const std::vector<double>& xyz, const std::vector<aria_eval_truth>& truth,
                                                  const std::vector<std::uint8_t>* mask, std::vector<double>* pose_err) {
    const int n = (int)(xyz.size() / 3);
    const int offset[2] = {0, n};
    aria_eval_result res{};
    if (pose_err) pose_err->assign((std::size_t)n, 0.0);
    evaluateBatch(xyz.data(), ARIA_EVAL_EST_XYZ, offset, n, 1, truth.empty() ? nullptr : truth.data(), (int)truth.size(), false,
                  mask ? mask->data() : nullptr, pose_err && n ? pose_err->data() : nullptr, &res);
    return res;
}

int HipTrajectoryEvaluator::evaluateBatch(const void* est, int est_kind, const int* offset, int n_poses_total, int n_traj,
                                          const aria_eval_truth* truth, int n_truth, bool truth_shared, const std::uint8_t* mask,
                                          double* pose_err, aria_eval_result* results) {
    const int rc = aria_eval_batch(h_.get(), est, est_kind, offset, n_poses_total, n_traj, truth, n_truth, truth_shared ? 1 : 0, mask,
                                   cfg_.align_mode, cfg_.rpe_delta, pose_err, results);
    if (rc != ARIA_OK && rc != ARIA_E_INVALID) fail("aria_eval_batch", rc);
    return rc;
}

void HipTrajectoryEvaluator::evaluateBatchDevice(const void* d_est, int est_kind, const int* d_offset, int n_poses_total, int n_traj,
                                                 const aria_eval_truth* d_truth, int n_truth, bool truth_shared,
                                                 const std::uint8_t* d_mask, double* d_pose_err, aria_eval_result* d_results) {
    expect("aria_eval_batch_device",
           aria_eval_batch_device(h_.get(), d_est, est_kind, d_offset, n_poses_total, n_traj, d_truth, n_truth, truth_shared ? 1 : 0,
                                  d_mask, cfg_.align_mode, cfg_.rpe_delta, d_pose_err, d_results));
}

int HipTrajectoryEvaluator::check() {
    const int rc = aria_eval_check(h_.get());
    if (rc != ARIA_OK && rc != ARIA_E_INVALID) fail("aria_eval_check", rc);
    return rc;
}

}  // namespace aria::adapters::hip
