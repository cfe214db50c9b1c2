// See aria_hip/HipDenseStereo.hpp.
#include "aria_hip/HipDenseStereo.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint), "layouts");

double DenseDepth::validShare() const {
    if (disparity.empty()) return 0.0;
    size_t n = 0;
    for (const std::int16_t d : disparity) n += d > 0;
    return (double)n / (double)disparity.size();
}

float DenseDepth::medianDepth() const {
    std::vector<float> d;
    for (size_t i = 0; i < disparity.size(); i++)
        if (disparity[i] > 0) d.push_back(depth[i]);
    if (d.empty()) return 0.0f;
    std::nth_element(d.begin(), d.begin() + (std::ptrdiff_t)(d.size() / 2), d.end());
    return d[d.size() / 2];
}

HipDenseStereo::HipDenseStereo(const DenseStereoConfig& cfg) {
    aria_dense_config c;
    aria_dense_default_config(&c);
    c.device = cfg.device;
    c.stream = cfg.stream;
    c.fx = cfg.K.fx; c.fy = cfg.K.fy; c.cx = cfg.K.cx; c.cy = cfg.K.cy;
    c.baseline = cfg.baseline;
    c.P1 = cfg.P1; c.P2 = cfg.P2; c.uniqueness = cfg.uniqueness; c.lr_max_diff = cfg.lr_max_diff;
    c.max_width = cfg.max_width; c.max_height = cfg.max_height;
    c.scratch_bytes = cfg.scratch_bytes;
    expect("aria_dense_create", aria_dense_create(&c, h_.out()));
}

HipDenseStereo::~HipDenseStereo() = default;

DenseDepth HipDenseStereo::compute(const std::uint8_t* image_left, const std::uint8_t* image_right, int width, int height) {
    DenseDepth out;
    out.width = width;
    out.height = height;
    out.disparity.resize((size_t)width * (size_t)height);
    out.depth.resize(out.disparity.size());
    expect("aria_dense_compute",
           aria_dense_compute(h_.get(), image_left, image_right, width, height, width, out.disparity.data(), out.depth.data()));
    return out;
}

std::vector<aria_stereo_obs> HipDenseStereo::sample(const DenseDepth& map, const std::vector<core::KeyPoint>& keypoints) {
    std::vector<aria_stereo_obs> obs(keypoints.size());
    if (keypoints.empty()) return obs;
    expect("aria_dense_sample",
           aria_dense_sample(h_.get(), map.disparity.data(), map.width, map.height, map.width,
                             reinterpret_cast<const aria_keypoint*>(keypoints.data()), (int)keypoints.size(), obs.data()));
    return obs;
}

}  // namespace aria::adapters::hip
