// aria::adapters::hip::HipVolumeRenderer -- ray casting of the volume over the C-ABI (include/aria_orb_hip.h, "ray casting of
// the volume"): predicted fp32 depth maps, world-frame normals, the fused gray and a head-light shade of a HipTsdfVolume at a
// batch of poses, the headless form of the reference's roadmap item H21 (a 3-D viewer). The reference has no code for it; the
// definition is the NumPy restatement aria_slam_amd/ray_ref.py, which the device equals bit for bit.
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "aria_hip/HipTsdfVolume.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct VolumeRendererConfig {
    PoseIntrinsics K{};                  // of the views (EuRoC cam0 by default)
    int nx = 256, ny = 256, nz = 128;    // the volume's geometry
    float voxel = 0.05f;
    float origin[3] = {-6.4f, -6.4f, 0.0f};
    int min_weight = 2;
    float near_z = 0.3f, far_z = 10.0f;  // metres of camera depth
    float step = 0.05f;
    int skip = 1;                        // 0: every sample loads its record; the same bytes either way
    void* stream = nullptr;
    int device = 0;
    // the geometry (dims, voxel, origin), min_weight, intrinsics and device of a volume; step = its voxel
    static VolumeRendererConfig fromVolume(const HipTsdfVolume& volume);
};

// The views of one castBatch, dense: view f at f * width * height (normals: three floats per pixel). A plane that was not
// asked for is empty.
struct RenderedViews {
    int width = 0, height = 0;
    std::vector<float> depth, normal;
    std::vector<std::uint8_t> gray, shade;
    std::vector<aria_ray_view> views;
    bool invalid = false;                // some view had a non-finite extrinsic: its planes are zero, its valid is 0
    long long hitPixels() const;
};

class HipVolumeRenderer {
public:
    explicit HipVolumeRenderer(const VolumeRendererConfig& cfg = {});
    ~HipVolumeRenderer();

    // Remembers the volume's records and rebuilds the skip words. A volume of other dims, voxel or origin than this renderer's
    // is refused (min_weight is the renderer's own: it may ask for more than the volume's extraction does). The volume's
    // stream is synchronised first through its check(); a deferred error of the volume is thrown here, not swallowed. Call it
    // again after the volume changed, and do not integrate between an update and the casts that follow it.
    void update(HipTsdfVolume& volume);
    // All views in one device batch (aria_ray_cast_batch_device), then one copy back per plane; blocks. extrinsics: 12 doubles
    // [R|t] row-major per view, world to camera (the first three rows of a 4x4 pose serve). planes: ARIA_RAY_* bits.
    RenderedViews castBatch(const std::vector<std::array<double, 12>>& extrinsics, int width, int height,
                            int planes = ARIA_RAY_DEPTH | ARIA_RAY_SHADE);
    // The same where the outputs lie in HBM; enqueued, check() synchronises.
    void castBatchDevice(const double* d_extrinsics, const std::uint8_t* d_view_mask, int n_views, int width, int height, float* d_depth,
                         std::int64_t depth_stride, int depth_pitch, float* d_normal, std::int64_t normal_stride, int normal_pitch,
                         std::uint8_t* d_gray, std::int64_t gray_stride, int gray_pitch, std::uint8_t* d_shade, std::int64_t shade_stride,
                         int shade_pitch, aria_ray_view* d_views);
    int check() { return aria_ray_check(h_.get()); }
    const aria_ray_config& config() const { return cfg_; }
    aria_ray_t handle() const { return h_.get(); }

    // Binary PGMs: depth as 16-bit millimetres, most significant byte first (0 = no hit, 65535 = 65.535 m or more); an 8-bit plane.
    static void writeDepthPGM(const std::string& filename, const float* depth, int width, int height);
    static void writeGrayPGM(const std::string& filename, const std::uint8_t* plane, int width, int height);

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipVolumeRenderer", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipVolumeRenderer", where, rc); }
    aria_ray_config cfg_{};
    detail::StageOwner<aria_ray_t, aria_ray_destroy> h_;
};

}  // namespace aria::adapters::hip
