// See aria_hip/HipVolumeRenderer.hpp.
#include "aria_hip/HipVolumeRenderer.hpp"

#include <cmath>
#include <fstream>
#include <stdexcept>

namespace aria::adapters::hip {

VolumeRendererConfig VolumeRendererConfig::fromVolume(const HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    VolumeRendererConfig c;
    c.K.fx = v.fx; c.K.fy = v.fy; c.K.cx = v.cx; c.K.cy = v.cy;
    c.nx = v.nx; c.ny = v.ny; c.nz = v.nz;
    c.voxel = v.voxel;
    c.step = v.voxel;
    for (int a = 0; a < 3; a++) c.origin[a] = v.origin[a];
    c.min_weight = v.min_weight;
    c.device = v.device;
    return c;
}

long long RenderedViews::hitPixels() const {
    long long n = 0;
    for (const aria_ray_view& v : views) n += v.n_hit;
    return n;
}

HipVolumeRenderer::HipVolumeRenderer(const VolumeRendererConfig& cfg) {
    aria_ray_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.nx = cfg.nx; cfg_.ny = cfg.ny; cfg_.nz = cfg.nz;
    cfg_.min_weight = cfg.min_weight;
    cfg_.skip = cfg.skip;
    cfg_.voxel = cfg.voxel;
    for (int a = 0; a < 3; a++) cfg_.origin[a] = cfg.origin[a];
    cfg_.near = cfg.near_z; cfg_.far = cfg.far_z; cfg_.step = cfg.step;
    cfg_.fx = cfg.K.fx; cfg_.fy = cfg.K.fy; cfg_.cx = cfg.K.cx; cfg_.cy = cfg.K.cy;
    expect("aria_ray_create", aria_ray_create(&cfg_, h_.out()));
}

HipVolumeRenderer::~HipVolumeRenderer() = default;

void HipVolumeRenderer::update(HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    bool same = v.nx == cfg_.nx && v.ny == cfg_.ny && v.nz == cfg_.nz && v.voxel == cfg_.voxel;
    for (int a = 0; a < 3; a++) same = same && v.origin[a] == cfg_.origin[a];
    if (!same) fail("update: the volume has another geometry (dims, voxel or origin)", ARIA_E_INVALID);
    // its stream is not this handle's: drain it. The check reports the volume's deferred error once, so it must not be dropped.
    expect("update: the volume reports a deferred error", volume.check());
    expect("aria_ray_update_from_volume_device",
           aria_ray_update_from_volume_device(h_.get(), aria_tsdf_device_voxels(volume.handle())));
}

void HipVolumeRenderer::castBatchDevice(const double* d_extrinsics, const std::uint8_t* d_view_mask, int n_views, int width, int height,
                                        float* d_depth, std::int64_t depth_stride, int depth_pitch, float* d_normal,
                                        std::int64_t normal_stride, int normal_pitch, std::uint8_t* d_gray, std::int64_t gray_stride,
                                        int gray_pitch, std::uint8_t* d_shade, std::int64_t shade_stride, int shade_pitch,
                                        aria_ray_view* d_views) {
    expect("aria_ray_cast_batch_device",
           aria_ray_cast_batch_device(h_.get(), d_extrinsics, d_view_mask, n_views, width, height, d_depth, depth_stride, depth_pitch,
                                      d_normal, normal_stride, normal_pitch, d_gray, gray_stride, gray_pitch, d_shade, shade_stride,
                                      shade_pitch, d_views));
}

namespace {

// One device block for the life of a castBatch.
struct DeviceBlock {
    int device;
    void* p = nullptr;
    DeviceBlock(int dev, std::size_t bytes) : device(dev) {
        if (bytes && aria_device_alloc(dev, bytes, &p) != ARIA_OK) throw std::runtime_error("HipVolumeRenderer: aria_device_alloc failed");
    }
    ~DeviceBlock() {
        if (p) aria_device_free(device, p);
    }
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
};

}  // namespace

RenderedViews HipVolumeRenderer::castBatch(const std::vector<std::array<double, 12>>& extrinsics, int width, int height, int planes) {
    RenderedViews out;
    out.width = width;
    out.height = height;
    const int n = (int)extrinsics.size();
    if (n == 0) return out;
    if (width < 1 || height < 1) fail("castBatch", ARIA_E_INVALID);
    const std::size_t px = (std::size_t)width * height, all = px * n;
    void* const st = aria_ray_stream(h_.get());
    const int dev = cfg_.device;
    DeviceBlock d_ext(dev, sizeof(double) * 12 * n), d_views(dev, sizeof(aria_ray_view) * n);
    DeviceBlock d_depth(dev, (planes & ARIA_RAY_DEPTH) ? all * 4 : 0), d_normal(dev, (planes & ARIA_RAY_NORMAL) ? all * 12 : 0);
    DeviceBlock d_gray(dev, (planes & ARIA_RAY_GRAY) ? all : 0), d_shade(dev, (planes & ARIA_RAY_SHADE) ? all : 0);
    expect("aria_copy_h2d_async", aria_copy_h2d_async(dev, st, d_ext.p, extrinsics.data(), sizeof(double) * 12 * n));
    castBatchDevice((const double*)d_ext.p, nullptr, n, width, height, (float*)d_depth.p, (std::int64_t)px, width, (float*)d_normal.p,
                    (std::int64_t)(3 * px), width, (std::uint8_t*)d_gray.p, (std::int64_t)px, width, (std::uint8_t*)d_shade.p, (std::int64_t)px,
                    width, (aria_ray_view*)d_views.p);
    auto back = [&](auto& v, const DeviceBlock& d, std::size_t count) {
        if (!d.p) return;
        v.resize(count);
        expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, v.data(), d.p, count * sizeof(v[0])));
    };
    back(out.depth, d_depth, all);
    back(out.normal, d_normal, 3 * all);
    back(out.gray, d_gray, all);
    back(out.shade, d_shade, all);
    back(out.views, d_views, (std::size_t)n);
    const int rc = check();                                                    // synchronises: the copies have landed
    if (rc == ARIA_E_INVALID) out.invalid = true;
    else if (rc != ARIA_OK) fail("aria_ray_check", rc);
    return out;
}

void HipVolumeRenderer::writeDepthPGM(const std::string& filename, const float* depth, int width, int height) {
    std::ofstream f(filename, std::ios::binary);
    f << "P5\n" << width << ' ' << height << "\n65535\n";
    std::vector<unsigned char> row((std::size_t)width * 2);
    for (int v = 0; v < height; v++) {
        for (int u = 0; u < width; u++) {
            const double mm = std::nearbyint((double)depth[(std::size_t)v * width + u] * 1000.0);
            const unsigned q = mm >= 65535.0 ? 65535u : mm > 0.0 ? (unsigned)mm : 0u;   // a NaN is 0
            row[(std::size_t)2 * u] = (unsigned char)(q >> 8);
            row[(std::size_t)2 * u + 1] = (unsigned char)(q & 255u);
        }
        f.write((const char*)row.data(), (std::streamsize)row.size());
    }
    if (!f) throw std::runtime_error("HipVolumeRenderer: cannot write " + filename);
}

void HipVolumeRenderer::writeGrayPGM(const std::string& filename, const std::uint8_t* plane, int width, int height) {
    std::ofstream f(filename, std::ios::binary);
    f << "P5\n" << width << ' ' << height << "\n255\n";
    f.write((const char*)plane, (std::streamsize)((std::size_t)width * height));
    if (!f) throw std::runtime_error("HipVolumeRenderer: cannot write " + filename);
}

}  // namespace aria::adapters::hip
