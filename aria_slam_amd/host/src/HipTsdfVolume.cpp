// See aria_hip/HipTsdfVolume.hpp.
#include "aria_hip/HipTsdfVolume.hpp"

#include <fstream>
#include <stdexcept>

#include "aria_hip/ply.hpp"

namespace aria::adapters::hip {

void TsdfVolumeConfig::centreOn(float x, float y, float z) {
    origin[0] = x - 0.5f * (float)nx * voxel;
    origin[1] = y - 0.5f * (float)ny * voxel;
    origin[2] = z - 0.5f * (float)nz * voxel;
}

HipTsdfVolume::HipTsdfVolume(const TsdfVolumeConfig& cfg) {
    aria_tsdf_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.nx = cfg.nx; cfg_.ny = cfg.ny; cfg_.nz = cfg.nz;
    cfg_.voxel = cfg.voxel; cfg_.trunc = cfg.trunc;
    for (int a = 0; a < 3; a++) cfg_.origin[a] = cfg.origin[a];
    cfg_.min_depth = cfg.min_depth; cfg_.max_depth = cfg.max_depth;
    cfg_.max_weight = cfg.max_weight; cfg_.min_weight = cfg.min_weight;
    cfg_.fx = cfg.K.fx; cfg_.fy = cfg.K.fy; cfg_.cx = cfg.K.cx; cfg_.cy = cfg.K.cy;
    expect("aria_tsdf_create", aria_tsdf_create(&cfg_, h_.out()));
}

HipTsdfVolume::~HipTsdfVolume() = default;

bool HipTsdfVolume::integrate(const float* depth, int width, int height, const double* extrinsics, const std::uint8_t* image) {
    const int rc = aria_tsdf_integrate(h_.get(), depth, width, height, width, extrinsics, image, width);
    if (rc == ARIA_E_INVALID && depth && extrinsics) {
        for (int k = 0; k < 12; k++)
            if (!(extrinsics[k] - extrinsics[k] == 0.0)) return false;          // NaN or Inf: the frame was refused
    }
    expect("aria_tsdf_integrate", rc);
    return true;
}

void HipTsdfVolume::integrateBatchDevice(const float* d_depth, std::int64_t depth_stride, int depth_pitch, int width, int height,
                                         const double* d_extrinsics, const std::uint8_t* d_frame_mask, const std::uint8_t* d_image,
                                         std::int64_t image_stride, int image_pitch, int n_frames) {
    expect("aria_tsdf_integrate_batch_device",
           aria_tsdf_integrate_batch_device(h_.get(), d_depth, depth_stride, depth_pitch, width, height, d_extrinsics, d_frame_mask,
                                            d_image, image_stride, image_pitch, n_frames));
}

void HipTsdfVolume::clear() {
    expect("aria_tsdf_clear", aria_tsdf_clear(h_.get()));
}

std::int64_t HipTsdfVolume::countPoints() {
    std::int64_t total = 0;
    const int rc = aria_tsdf_extract_points(h_.get(), nullptr, 0, &total);
    if (rc != ARIA_OK && rc != ARIA_E_OUTPUT_TOO_SMALL) fail("aria_tsdf_extract_points", rc);
    return total;
}

std::vector<aria_tsdf_point> HipTsdfVolume::extractPoints() {
    std::vector<aria_tsdf_point> pts((std::size_t)countPoints());
    if (pts.empty()) return pts;
    std::int64_t total = 0;
    expect("aria_tsdf_extract_points", aria_tsdf_extract_points(h_.get(), pts.data(), (std::int64_t)pts.size(), &total));
    return pts;
}

std::vector<aria_tsdf_voxel> HipTsdfVolume::readBox(int i0, int j0, int k0, int ni, int nj, int nk) {
    if (ni < 1 || nj < 1 || nk < 1) fail("aria_tsdf_read_box", ARIA_E_INVALID);
    std::vector<aria_tsdf_voxel> out((std::size_t)ni * (std::size_t)nj * (std::size_t)nk);
    expect("aria_tsdf_read_box", aria_tsdf_read_box(h_.get(), i0, j0, k0, ni, nj, nk, out.data()));
    return out;
}

std::int64_t HipTsdfVolume::observedVoxels() {
    std::int64_t n = 0;
    for (int k = 0; k < cfg_.nz; k += 8)                                         // slabs of eight layers: 4 MiB at the default size
        for (const aria_tsdf_voxel& v : readBox(0, 0, k, cfg_.nx, cfg_.ny, 8)) n += v.weight > 0;
    return n;
}

std::size_t HipTsdfVolume::exportPLY(const std::string& filename) {
    const std::vector<aria_tsdf_point> pts = extractPoints();
    std::ofstream file(filename);
    if (!file.is_open()) throw std::runtime_error("HipTsdfVolume: failed to open " + filename);
    writePLY(file, pts);
    return pts.size();
}

}  // namespace aria::adapters::hip
