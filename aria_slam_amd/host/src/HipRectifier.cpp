// See aria_hip/HipRectifier.hpp.
#include "aria_hip/HipRectifier.hpp"

#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint), "layouts");

HipRectifier::HipRectifier(const RectifierConfig& cfg) {
    aria_rect_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.src_width = cfg.src_width;
    cfg_.src_height = cfg.src_height;
    cfg_.dst_width = cfg.dst_width > 0 ? cfg.dst_width : cfg.src_width;
    cfg_.dst_height = cfg.dst_height > 0 ? cfg.dst_height : cfg.src_height;
    cfg_.n_cameras = cfg.n_cameras;
    cfg_.fill = cfg.fill;
    cfg_.model = cfg.model;
    if (cfg.n_cameras < 1 || cfg.n_cameras > 2) fail("HipRectifier", ARIA_E_INVALID);
    for (int k = 0; k < cfg.n_cameras; k++) {
        aria_rect_camera& c = cfg_.cam[k];
        c.fx = cfg.cam[k].K.fx; c.fy = cfg.cam[k].K.fy; c.cx = cfg.cam[k].K.cx; c.cy = cfg.cam[k].K.cy;
        for (int j = 0; j < 5; j++) c.dist[j] = cfg.cam[k].dist[j];
    }
    cfg_.new_fx = cfg.new_K[0]; cfg_.new_fy = cfg.new_K[1]; cfg_.new_cx = cfg.new_K[2]; cfg_.new_cy = cfg.new_K[3];
    if (cfg.n_cameras == 2) {
        const double kl[4] = {cfg.cam[0].K.fx, cfg.cam[0].K.fy, cfg.cam[0].K.cx, cfg.cam[0].K.cy};
        const double kr[4] = {cfg.cam[1].K.fx, cfg.cam[1].K.fy, cfg.cam[1].K.cx, cfg.cam[1].K.cy};
        expect("aria_rect_stereo_geometry", aria_rect_stereo_geometry(kl, kr, cfg.cam[0].T_BS, cfg.cam[1].T_BS, &cfg_, &baseline_));
    } else {                                               // plain undistortion: R = I (the default), new K = K where zero
        if (cfg_.new_fx == 0.0) cfg_.new_fx = cfg_.cam[0].fx;
        if (cfg_.new_fy == 0.0) cfg_.new_fy = cfg_.cam[0].fy;
        if (cfg_.new_cx == 0.0) cfg_.new_cx = cfg_.cam[0].cx;
        if (cfg_.new_cy == 0.0) cfg_.new_cy = cfg_.cam[0].cy;
    }
    expect("aria_rect_create", aria_rect_create(&cfg_, h_.out()));
}

HipRectifier::~HipRectifier() = default;

void HipRectifier::remap(int cam, const std::uint8_t* src, std::vector<std::uint8_t>& dst) {
    dst.resize((std::size_t)cfg_.dst_width * cfg_.dst_height);
    expect("aria_rect_remap", aria_rect_remap(h_.get(), cam, src, cfg_.src_width, dst.data(), cfg_.dst_width));
}

void HipRectifier::points(int cam, std::vector<core::KeyPoint>& keypoints) {
    if (keypoints.empty()) return;
    aria_keypoint* k = reinterpret_cast<aria_keypoint*>(keypoints.data());
    expect("aria_rect_points", aria_rect_points(h_.get(), cam, k, (int)keypoints.size(), k));
}

std::vector<std::uint32_t> HipRectifier::map(int cam) {
    std::vector<std::uint32_t> m((std::size_t)cfg_.dst_width * cfg_.dst_height);
    const int rc = aria_rect_get_map(h_.get(), cam, m.data(), (int)m.size());
    if (rc < 0) fail("aria_rect_get_map", rc);
    return m;
}

}  // namespace aria::adapters::hip
