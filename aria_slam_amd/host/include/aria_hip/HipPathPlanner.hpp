// aria::adapters::hip::HipPathPlanner -- path planning over the C-ABI (include/aria_orb_hip.h, "path planning"): a 2-D
// traversability grid collapsed out of a height band of a HipTsdfVolume, an exact clearance field and an integer cost map, exact
// cost-to-go fields for a batch of goals and paths traced for a batch of queries. The reference has no code for it (its roadmap
// items H20, H22 sit on such a map); the definition is the NumPy restatement aria_slam_amd/nav_ref.py, which the device equals
// bit for bit. The default band and radii are assumptions: nobody has tuned them on a recording.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "aria_hip/HipTsdfVolume.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct PathPlannerConfig {
    int nx = 256, ny = 256, nz = 128;    // the volume's geometry
    int up_axis = 1;                     // the first camera's y is the world's vertical in this chain
    int band0 = -1, band1 = -1;          // [band0, band1) on up_axis; -1 = [n/2 - 8, n/2 + 16) cut to the axis
    int min_weight = 2;
    float occ_tsdf = 0.0f;
    int occ_count = 1, free_count = 1;
    int clear_radius = 8, block_d2 = 16, soft_d2 = 64, penalty = 20, unknown_penalty = 10, allow_unknown = 1;
    int max_goals = 256;
    float voxel = 0.05f;
    float origin[3] = {-6.4f, -6.4f, 0.0f};
    void* stream = nullptr;
    int device = 0;
    // the geometry (dims, voxel, origin), min_weight and device of a volume
    static PathPlannerConfig fromVolume(const HipTsdfVolume& volume);
};

struct PlanResult {
    std::vector<aria_nav_record> records;    // one per query
    std::vector<std::int32_t> paths;         // query q at q * path_cap: linear cell indices v*nu + u
    int path_cap = 0;
    bool truncated = false;                  // some query has status ARIA_NAV_TRUNCATED
};

class HipPathPlanner {
public:
    explicit HipPathPlanner(const PathPlannerConfig& cfg = {});
    ~HipPathPlanner();

    int nu() const { return nu_; }
    int nv() const { return nv_; }
    // Rules 2-4 from a volume of this geometry. The volume's stream is synchronised first through its check(); a deferred error
    // of the volume (a skipped frame, a cut extraction) is thrown here, not swallowed. The update is then enqueued on THIS
    // handle's stream: an integrate on the volume's own stream before check() or a blocking call of this class races the
    // band walk, so do not integrate in between.
    void update(HipTsdfVolume& volume);
    // Rules 3-4 on nu*nv given cells (0 FREE, 1 OCCUPIED, 2 UNKNOWN); blocks. False for a value above 2: nothing changes.
    bool setCells(const std::uint8_t* cells);
    std::vector<std::uint8_t> cells();
    std::vector<std::uint16_t> clearance();
    std::vector<std::uint16_t> costs();
    // goals: (u, v) pairs; queries: (su, sv, goal_index) triples; blocks.
    PlanResult plan(const std::vector<std::array<std::int32_t, 2>>& goals, const std::vector<std::array<std::int32_t, 3>>& queries,
                    int path_cap);
    std::vector<std::int32_t> field(int goal);
    int check() { return aria_nav_check(h_.get()); }
    // world helpers, on the host: floor((x - origin) / voxel) in fp32 on the two plane axes, and back to the voxel centre with
    // the up coordinate at the middle of the band
    std::array<std::int32_t, 2> cellOf(float x, float y, float z) const;
    std::array<float, 3> centreOf(std::int32_t u, std::int32_t v) const;
    const aria_nav_config& config() const { return cfg_; }
    aria_nav_t handle() const { return h_.get(); }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipPathPlanner", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipPathPlanner", where, rc); }
    aria_nav_config cfg_{};
    detail::StageOwner<aria_nav_t, aria_nav_destroy> h_;
    int nu_ = 0, nv_ = 0, axis_u_ = 0, axis_v_ = 2;
};

}  // namespace aria::adapters::hip
