// aria::adapters::hip::HipTrajectoryEvaluator -- trajectory evaluation over the C-ABI (include/aria_orb_hip.h, "trajectory
// evaluation"): the reference's ground-truth lookup (EuRoCReader::getGroundTruth, src/legacy/EuRoCReader.cpp:311-346), its
// computeATE / computeRPE (src/euroc_eval.cpp:28-61) and the Umeyama-aligned figures, on the device.
// aria_slam_amd/eval_ref.py is the definition of the stage; parity with an Eigen build of the reference is not pinned.
//
// The reference has no port for this step (it is two free functions in euroc_eval.cpp), so the class stands alone. The host
// forms block and throw std::runtime_error on an error status other than ARIA_E_INVALID, which they return: an invalid
// trajectory is a result (valid = 0), not a failure of the call. The device forms enqueue on the handle's stream.
#pragma once
#include <cstdint>
#include <vector>

#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

class HipTrajectoryEvaluator {
public:
    explicit HipTrajectoryEvaluator(const aria_eval_config* cfg = nullptr);     // nullptr: aria_eval_default_config
    ~HipTrajectoryEvaluator();

    const aria_eval_config& config() const { return cfg_; }
    void setAlignMode(int mode) { cfg_.align_mode = mode; }
    void setRpeDelta(int delta) { cfg_.rpe_delta = delta; }

    // getGroundTruth for every timestamp; out (and valid, when given) are resized. Returns ARIA_OK or ARIA_E_INVALID.
    int sampleGroundTruth(const std::vector<aria_eval_truth>& gt, const std::vector<double>& timestamps,
                          std::vector<aria_eval_truth>& out, std::vector<int>* valid = nullptr);
    // One trajectory of packed xyz positions against truth records of the same length, in the configured mode and delta.
    aria_eval_result evaluate(const std::vector<double>& xyz, const std::vector<aria_eval_truth>& truth,
                              const std::vector<std::uint8_t>* mask = nullptr, std::vector<double>* pose_err = nullptr);
    // The batch, host arrays (aria_eval_batch). Returns ARIA_OK or ARIA_E_INVALID.
    int evaluateBatch(const void* est, int est_kind, const int* offset, int n_poses_total, int n_traj, const aria_eval_truth* truth,
                      int n_truth, bool truth_shared, const std::uint8_t* mask, double* pose_err, aria_eval_result* results);
    // The batch over device arrays (aria_eval_batch_device); check() synchronises and returns the deferred status.
    void evaluateBatchDevice(const void* d_est, int est_kind, const int* d_offset, int n_poses_total, int n_traj,
                             const aria_eval_truth* d_truth, int n_truth, bool truth_shared, const std::uint8_t* d_mask,
                             double* d_pose_err, aria_eval_result* d_results);
    int check();
    void* stream() const { return aria_eval_stream(h_.get()); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipTrajectoryEvaluator", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipTrajectoryEvaluator", where, rc); }
    detail::StageOwner<aria_eval_t, aria_eval_destroy> h_;
    aria_eval_config cfg_{};
};

}  // namespace aria::adapters::hip
