// See aria_hip/HipPathPlanner.hpp.
#include "aria_hip/HipPathPlanner.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

PathPlannerConfig PathPlannerConfig::fromVolume(const HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    PathPlannerConfig c;
    c.nx = v.nx; c.ny = v.ny; c.nz = v.nz;
    c.voxel = v.voxel;
    for (int a = 0; a < 3; a++) c.origin[a] = v.origin[a];
    c.min_weight = v.min_weight;
    c.device = v.device;
    return c;
}

HipPathPlanner::HipPathPlanner(const PathPlannerConfig& cfg) {
    aria_nav_default_config(&cfg_);
    cfg_.device = cfg.device;
    cfg_.stream = cfg.stream;
    cfg_.nx = cfg.nx; cfg_.ny = cfg.ny; cfg_.nz = cfg.nz;
    cfg_.up_axis = cfg.up_axis;
    const int dims[3] = {cfg.nx, cfg.ny, cfg.nz};
    const int n_up = dims[cfg.up_axis >= 0 && cfg.up_axis <= 2 ? cfg.up_axis : 1];
    cfg_.band0 = cfg.band0 >= 0 ? cfg.band0 : std::max(n_up / 2 - 8, 0);
    cfg_.band1 = cfg.band1 >= 0 ? cfg.band1 : std::min(n_up / 2 + 16, n_up);
    cfg_.min_weight = cfg.min_weight; cfg_.occ_tsdf = cfg.occ_tsdf; cfg_.occ_count = cfg.occ_count; cfg_.free_count = cfg.free_count;
    cfg_.clear_radius = cfg.clear_radius; cfg_.block_d2 = cfg.block_d2; cfg_.soft_d2 = cfg.soft_d2; cfg_.penalty = cfg.penalty;
    cfg_.unknown_penalty = cfg.unknown_penalty; cfg_.allow_unknown = cfg.allow_unknown; cfg_.max_goals = cfg.max_goals;
    cfg_.voxel = cfg.voxel;
    for (int a = 0; a < 3; a++) cfg_.origin[a] = cfg.origin[a];
    expect("aria_nav_create", aria_nav_create(&cfg_, h_.out()));
    axis_u_ = cfg_.up_axis == 0 ? 1 : 0;
    axis_v_ = cfg_.up_axis == 2 ? 1 : 2;
    nu_ = dims[axis_u_];
    nv_ = dims[axis_v_];
}

HipPathPlanner::~HipPathPlanner() = default;

void HipPathPlanner::update(HipTsdfVolume& volume) {
    const aria_tsdf_config& v = volume.config();
    if (v.nx != cfg_.nx || v.ny != cfg_.ny || v.nz != cfg_.nz) fail("update: the volume has another geometry", ARIA_E_INVALID);
    // its stream is not this handle's: drain it. The check reports the volume's deferred error once, so it must not be dropped.
    expect("update: the volume reports a deferred error", volume.check());
    expect("aria_nav_update_from_volume_device",
           aria_nav_update_from_volume_device(h_.get(), aria_tsdf_device_voxels(volume.handle())));
}

bool HipPathPlanner::setCells(const std::uint8_t* cells) {
    const int rc = aria_nav_set_cells(h_.get(), cells);
    if (rc == ARIA_E_INVALID && cells) return false;
    expect("aria_nav_set_cells", rc);
    return true;
}

std::vector<std::uint8_t> HipPathPlanner::cells() {
    std::vector<std::uint8_t> out((std::size_t)nu_ * (std::size_t)nv_);
    expect("aria_nav_read_cells", aria_nav_read_cells(h_.get(), out.data()));
    return out;
}

std::vector<std::uint16_t> HipPathPlanner::clearance() {
    std::vector<std::uint16_t> out((std::size_t)nu_ * (std::size_t)nv_);
    expect("aria_nav_read_clearance", aria_nav_read_clearance(h_.get(), out.data()));
    return out;
}

std::vector<std::uint16_t> HipPathPlanner::costs() {
    std::vector<std::uint16_t> out((std::size_t)nu_ * (std::size_t)nv_);
    expect("aria_nav_read_costs", aria_nav_read_costs(h_.get(), out.data()));
    return out;
}

PlanResult HipPathPlanner::plan(const std::vector<std::array<std::int32_t, 2>>& goals,
                                const std::vector<std::array<std::int32_t, 3>>& queries, int path_cap) {
    if (path_cap < 0) fail("aria_nav_plan", ARIA_E_INVALID);
    PlanResult r;
    r.path_cap = path_cap;
    r.records.resize(queries.size());
    r.paths.assign(queries.size() * (std::size_t)path_cap, 0);
    const int rc = aria_nav_plan(h_.get(), goals.empty() ? nullptr : goals[0].data(), (int)goals.size(), queries.empty() ? nullptr : queries[0].data(),
                                 (int)queries.size(), r.records.data(), r.paths.empty() ? nullptr : r.paths.data(), path_cap);
    if (rc != ARIA_OK && rc != ARIA_E_OUTPUT_TOO_SMALL) fail("aria_nav_plan", rc);
    r.truncated = rc == ARIA_E_OUTPUT_TOO_SMALL;
    return r;
}

std::vector<std::int32_t> HipPathPlanner::field(int goal) {
    std::vector<std::int32_t> out((std::size_t)nu_ * (std::size_t)nv_);
    expect("aria_nav_read_field", aria_nav_read_field(h_.get(), goal, out.data()));
    return out;
}

std::array<std::int32_t, 2> HipPathPlanner::cellOf(float x, float y, float z) const {
    const float X[3] = {x, y, z};
    return {(std::int32_t)std::floor((X[axis_u_] - cfg_.origin[axis_u_]) / cfg_.voxel),
            (std::int32_t)std::floor((X[axis_v_] - cfg_.origin[axis_v_]) / cfg_.voxel)};
}

std::array<float, 3> HipPathPlanner::centreOf(std::int32_t u, std::int32_t v) const {
    std::array<float, 3> X{};
    X[(std::size_t)axis_u_] = cfg_.origin[axis_u_] + ((float)u + 0.5f) * cfg_.voxel;
    X[(std::size_t)axis_v_] = cfg_.origin[axis_v_] + ((float)v + 0.5f) * cfg_.voxel;
    X[(std::size_t)cfg_.up_axis] = cfg_.origin[cfg_.up_axis] + ((float)(cfg_.band0 + cfg_.band1) * 0.5f) * cfg_.voxel;
    return X;
}

}  // namespace aria::adapters::hip
