// See aria_hip/HipDenseTracker.hpp.
#include "aria_hip/HipDenseTracker.hpp"

#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

DenseTrackerConfig DenseTrackerConfig::fromRenderer(const HipVolumeRenderer& renderer) {
    const aria_ray_config& r = renderer.config();
    DenseTrackerConfig c;
    c.K.fx = r.fx; c.K.fy = r.fy; c.K.cx = r.cx; c.K.cy = r.cy;
    c.device = r.device;
    return c;
}

HipDenseTracker::HipDenseTracker(const DenseTrackerConfig& cfg) {
    aria_icp_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.fx = cfg.K.fx; cfg_.fy = cfg.K.fy; cfg_.cx = cfg.K.cx; cfg_.cy = cfg.K.cy;
    cfg_.min_depth = cfg.min_depth; cfg_.max_depth = cfg.max_depth;
    cfg_.dist_max = cfg.dist_max; cfg_.reach = cfg.reach;
    cfg_.min_corr = cfg.min_corr; cfg_.min_pivot = cfg.min_pivot; cfg_.eps = cfg.eps;
    if (cfg.strides.size() != cfg.iterations.size() || cfg.strides.empty() || cfg.strides.size() > ARIA_ICP_MAX_LEVELS)
        fail("one stride and one iteration count per level, 1..4 levels", ARIA_E_INVALID);
    cfg_.n_levels = (int)cfg.strides.size();
    for (int l = 0; l < ARIA_ICP_MAX_LEVELS; l++) {
        cfg_.stride[l] = l < cfg_.n_levels ? cfg.strides[(std::size_t)l] : 0;
        cfg_.iterations[l] = l < cfg_.n_levels ? cfg.iterations[(std::size_t)l] : 0;
    }
    expect("aria_icp_create", aria_icp_create(&cfg_, h_.out()));
}

HipDenseTracker::~HipDenseTracker() = default;

void HipDenseTracker::requireSameIntrinsics(const HipVolumeRenderer& renderer) const {
    const aria_ray_config& r = renderer.config();
    if (r.fx != cfg_.fx || r.fy != cfg_.fy || r.cx != cfg_.cx || r.cy != cfg_.cy)
        fail("the renderer casts with other intrinsics than the tracker's", ARIA_E_INVALID);
}

DenseTrack HipDenseTracker::track(const float* depth, const float* model_depth, const float* model_normal, int width, int height,
                                  const double* model_extrinsics, const double* guess) {
    DenseTrack out;
    expect("aria_icp_track",
           aria_icp_track(h_.get(), depth, model_depth, model_normal, model_extrinsics, guess ? guess : model_extrinsics, width, height,
                          out.extrinsics.data(), &out.result));
    return out;
}

void HipDenseTracker::trackBatchDevice(const float* d_depth, std::int64_t depth_stride, int depth_pitch, const float* d_model_depth,
                                       std::int64_t model_depth_stride, int model_depth_pitch, const float* d_model_normal,
                                       std::int64_t normal_stride, int normal_pitch, const double* d_model_extrinsics,
                                       const double* d_guess, const std::uint8_t* d_mask, int n_frames, int width, int height,
                                       double* d_extrinsics_out, aria_icp_result* d_results) {
    expect("aria_icp_track_batch_device",
           aria_icp_track_batch_device(h_.get(), d_depth, depth_stride, depth_pitch, d_model_depth, model_depth_stride, model_depth_pitch,
                                       d_model_normal, normal_stride, normal_pitch, d_model_extrinsics, d_guess, d_mask, n_frames,
                                       width, height, d_extrinsics_out, d_results));
}

}  // namespace aria::adapters::hip
