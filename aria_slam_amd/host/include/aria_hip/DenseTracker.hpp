// aria::adapters::hip::DenseTracker -- the sequential loop of dense frame-to-model tracking over the existing adapters, the
// analogue of MapTracker for the dense half: per frame (1) predict the pose from the pose chain's delta, (2) cast the volume at
// the prediction (HipVolumeRenderer), (3) track the frame's depth map against that view (HipDenseTracker), (4) on valid = 0
// fall back to the prediction, (5) integrate the frame at the resulting pose (HipTsdfVolume). It owns its volume, so a driver's
// other volume is not touched. The first frame, and every frame while the cast view is empty, is integrated at its prediction.
#pragma once
#include <array>
#include <cstdint>
#include <memory>

#include "aria_hip/HipDenseTracker.hpp"
#include "aria_hip/HipTsdfVolume.hpp"
#include "aria_hip/HipVolumeRenderer.hpp"

namespace aria::adapters::hip {

struct DenseTrackStep {
    bool tracked = false;                // a model view with hits existed and the tracker ran
    bool lost = false;                   // it ran and returned valid = 0: the pose is the prediction
    aria_icp_result result{};
};

class DenseTracker {
public:
    // near_z, far_z: the depth range the model views are cast over
    DenseTracker(const TsdfVolumeConfig& volume, DenseTrackerConfig tracker = {}, float near_z = 0.3f, float far_z = 10.0f);

    // One frame: depth width x height floats, image width x height bytes or null; chain_delta the 4x4 row-major step of the pose
    // chain since the last frame (pose = pose * delta, the driver's convention), null = none.
    DenseTrackStep step(const float* depth, int width, int height, const double* chain_delta, const std::uint8_t* image = nullptr);
    const std::array<double, 16>& pose() const { return pose_; }
    long long framesTracked() const { return tracked_; }
    long long framesLost() const { return lost_; }
    HipTsdfVolume& volume() { return *volume_; }

private:
    std::unique_ptr<HipTsdfVolume> volume_;
    std::unique_ptr<HipVolumeRenderer> renderer_;
    std::unique_ptr<HipDenseTracker> tracker_;
    std::array<double, 16> pose_{};
    long long integrated_ = 0, tracked_ = 0, lost_ = 0;
};

}  // namespace aria::adapters::hip
