// aria::adapters::hip::HipTsdfVolume -- dense depth fusion over the C-ABI (include/aria_orb_hip.h, "dense depth fusion"): the
// fp32 depth maps of HipDenseStereo integrated along the trajectory into one truncated signed distance volume kept in HBM, and
// the surface points read back out of it. The reference has no code for it (its roadmap items H17, H20, H22 sit on such a
// map); the definition is the NumPy restatement aria_slam_amd/tsdf_ref.py, which the device equals bit for bit.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct TsdfVolumeConfig {
    PoseIntrinsics K{};                  // of the depth maps (EuRoC cam0 by default)
    int nx = 256, ny = 256, nz = 128;    // each a multiple of 8 in 8..1024
    float voxel = 0.05f, trunc = 0.20f;  // metres
    float origin[3] = {-6.4f, -6.4f, 0.0f};   // the world corner of voxel (0, 0, 0)
    float min_depth = 0.3f, max_depth = 10.0f;
    int max_weight = 64, min_weight = 2;
    void* stream = nullptr;
    int device = 0;
    // origin such that the volume's centre is the world point (x, y, z)
    void centreOn(float x, float y, float z);
};

class HipTsdfVolume {
public:
    explicit HipTsdfVolume(const TsdfVolumeConfig& cfg = {});
    ~HipTsdfVolume();

    // One frame from host buffers: depth width x height floats, tightly packed; extrinsics 12 doubles [R|t] row-major, world to
    // camera (the first three rows of a 4x4 pose serve); image width x height bytes or null. False when an extrinsic is not
    // finite: the frame is refused and the volume untouched.
    bool integrate(const float* depth, int width, int height, const double* extrinsics, const std::uint8_t* image = nullptr);
    // A batch where it lies in HBM (aria_tsdf_integrate_batch_device); enqueued, check() synchronises.
    void integrateBatchDevice(const float* d_depth, std::int64_t depth_stride, int depth_pitch, int width, int height,
                              const double* d_extrinsics, const std::uint8_t* d_frame_mask, const std::uint8_t* d_image,
                              std::int64_t image_stride, int image_pitch, int n_frames);
    int check() { return aria_tsdf_check(h_.get()); }
    void clear();
    std::int64_t countPoints();
    // the surface points in canonical order
    std::vector<aria_tsdf_point> extractPoints();
    // voxels some frame has touched (weight > 0); reads the volume back
    std::int64_t observedVoxels();
    std::vector<aria_tsdf_voxel> readBox(int i0, int j0, int k0, int ni, int nj, int nk);
    // the surface points in HipMapper::exportPLY's header and vertex format (r = g = b = gray); returns their number
    std::size_t exportPLY(const std::string& filename);
    const aria_tsdf_config& config() const { return cfg_; }
    aria_tsdf_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipTsdfVolume", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipTsdfVolume", where, rc); }
    aria_tsdf_config cfg_{};
    detail::StageOwner<aria_tsdf_t, aria_tsdf_destroy> h_;
};

}  // namespace aria::adapters::hip
