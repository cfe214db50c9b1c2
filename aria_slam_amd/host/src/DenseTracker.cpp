// See aria_hip/DenseTracker.hpp.
#include "aria_hip/DenseTracker.hpp"

#include <algorithm>
#include <vector>

namespace aria::adapters::hip {

DenseTracker::DenseTracker(const TsdfVolumeConfig& volume, DenseTrackerConfig tracker, float near_z, float far_z) {
    volume_ = std::make_unique<HipTsdfVolume>(volume);
    VolumeRendererConfig rc = VolumeRendererConfig::fromVolume(*volume_);
    rc.near_z = near_z;
    rc.far_z = far_z;
    renderer_ = std::make_unique<HipVolumeRenderer>(rc);
    tracker.K = rc.K;
    tracker.device = rc.device;
    tracker_ = std::make_unique<HipDenseTracker>(tracker);
    tracker_->requireSameIntrinsics(*renderer_);
    pose_ = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
}

DenseTrackStep DenseTracker::step(const float* depth, int width, int height, const double* chain_delta, const std::uint8_t* image) {
    DenseTrackStep out;
    if (chain_delta) {                                                     // (1) pose = pose * delta
        std::array<double, 16> p{};
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                double v = 0.0;
                for (int k = 0; k < 4; k++) v += pose_[(std::size_t)(a * 4 + k)] * chain_delta[k * 4 + b];
                p[(std::size_t)(a * 4 + b)] = v;
            }
        pose_ = p;
    }
    if (integrated_ > 0) {
        std::array<double, 12> e;
        std::copy(pose_.begin(), pose_.begin() + 12, e.begin());
        renderer_->update(*volume_);                                       // (2) the volume changed since the last cast
        const RenderedViews view = renderer_->castBatch({e}, width, height, ARIA_RAY_DEPTH | ARIA_RAY_NORMAL);
        if (!view.invalid && view.hitPixels() > 0) {
            const DenseTrack t = tracker_->track(depth, view.depth.data(), view.normal.data(), width, height, e.data());   // (3)
            out.tracked = true;
            out.result = t.result;
            tracked_++;
            if (t.result.valid) std::copy(t.extrinsics.begin(), t.extrinsics.end(), pose_.begin());
            else { out.lost = true; lost_++; }                             // (4) the prediction stays
        }
    }
    if (volume_->integrate(depth, width, height, pose_.data(), image)) integrated_++;   // (5)
    return out;
}

}  // namespace aria::adapters::hip
