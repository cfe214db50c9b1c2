// aria::adapters::hip::HipDenseTracker -- frame-to-model tracking over the C-ABI (include/aria_orb_hip.h, "frame-to-model
// tracking"): batched point-to-plane ICP of live fp32 depth maps against the depth maps and world-frame normals that a
// HipVolumeRenderer predicted from the volume. The reference has no code for it (KinectFusion's tracking step); the definition
// is the NumPy restatement aria_slam_amd/icp_ref.py, which the device equals bit for bit.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "aria_hip/HipVolumeRenderer.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct DenseTrackerConfig {
    PoseIntrinsics K{};                  // of the live and the model maps (EuRoC cam0 by default)
    float min_depth = 0.3f, max_depth = 10.0f;
    float dist_max = 0.1f, reach = 64.0f;
    int min_corr = 64;
    double min_pivot = 5e-6, eps = 1e-6;
    std::vector<int> strides{4, 2, 1}, iterations{4, 5, 10};
    void* stream = nullptr;
    int device = 0;
    // the intrinsics and device of a renderer
    static DenseTrackerConfig fromRenderer(const HipVolumeRenderer& renderer);
};

// What one frame's tracking leaves: the pose (12 doubles [R|t] row-major, world to camera; the guess when the frame is lost)
// and the stage's record.
struct DenseTrack {
    std::array<double, 12> extrinsics{};
    aria_icp_result result{};
};

class HipDenseTracker {
public:
    explicit HipDenseTracker(const DenseTrackerConfig& cfg = {});
    ~HipDenseTracker();

    // One frame from dense host buffers (aria_icp_track); blocks. The model view is what a renderer of these intrinsics cast at
    // model_extrinsics; guess = nullptr starts at the model's pose. A non-finite pose throws.
    DenseTrack track(const float* depth, const float* model_depth, const float* model_normal, int width, int height,
                     const double* model_extrinsics, const double* guess = nullptr);
    // A batch where it lies in HBM (aria_icp_track_batch_device); enqueued, check() synchronises.
    void trackBatchDevice(const float* d_depth, std::int64_t depth_stride, int depth_pitch, const float* d_model_depth,
                          std::int64_t model_depth_stride, int model_depth_pitch, const float* d_model_normal, std::int64_t normal_stride,
                          int normal_pitch, const double* d_model_extrinsics, const double* d_guess, const std::uint8_t* d_mask,
                          int n_frames, int width, int height, double* d_extrinsics_out, aria_icp_result* d_results);
    // A renderer that casts with other intrinsics than this tracker's is refused, as a volume of another geometry is elsewhere.
    void requireSameIntrinsics(const HipVolumeRenderer& renderer) const;
    int check() { return aria_icp_check(h_.get()); }
    const aria_icp_config& config() const { return cfg_; }
    aria_icp_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipDenseTracker", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipDenseTracker", where, rc); }
    aria_icp_config cfg_{};
    detail::StageOwner<aria_icp_t, aria_icp_destroy> h_;
};

}  // namespace aria::adapters::hip
