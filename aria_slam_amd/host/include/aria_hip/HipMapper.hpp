// aria::adapters::hip::HipMapper -- the reference's IMapper port (include/interfaces/IMapper.hpp) over the C-ABI
// (include/aria_orb_hip.h, "two-view triangulation and point map"): Mapper::triangulate's DLT and tests on the device, the
// map kept in HBM, filterOutliers / filterByDistance and the reference's PLY / PCD exports.
//
// triangulate() takes pose.toMatrix() of each view as world-to-camera extrinsics [R | t], as Mapper::triangulate uses its
// Matrix4d arguments (src/legacy/Mapper.cpp:16-32), and the matches' query side as view 1. The handle's intrinsics are fixed
// at construction: a K argument that differs from them is an error. Every map point gets two observations (frame id,
// keypoint index) and view 1's descriptor row.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

#ifdef ARIA_HIP_USE_REFERENCE_HEADERS
using MapperK = Eigen::Matrix3d;
#else
using MapperK = core::Matrix3;
#endif

struct MapperConfig {            // include/legacy/Mapper.hpp:67-70
    PoseIntrinsics K{};
    double min_depth = 0.1, max_depth = 50.0, min_parallax_deg = 1.0, max_reproj_px = 2.0;
    std::int64_t capacity = 1 << 16;
    void* stream = nullptr;
    int device = 0;
};

class HipMapper : public interfaces::IMapper {
public:
    explicit HipMapper(const MapperConfig& cfg = {});
    ~HipMapper() override;

    // IMapper
    void triangulate(const core::Frame& frame1, const core::Frame& frame2, const core::Pose& pose1, const core::Pose& pose2,
                     const std::vector<core::Match>& matches, const MapperK& K, std::vector<core::MapPoint>& new_points) override;
    const std::vector<core::MapPoint>& getMapPoints() const override;
    void exportPLY(const std::string& filename) const override;
    void exportPCD(const std::string& filename) const override;
    void clear() override;
    std::size_t size() const override;

    // Mapper::triangulate's own form: T1 / T2 world-to-camera, 4x4 row-major; image1 (optional) = view 1's gray image,
    // width x height bytes. query_is_first: match.query_idx indexes `first` (the reference's order). Returns the points added.
    int triangulateExtrinsics(const core::Frame& first, const core::Frame& second, const std::vector<core::Match>& matches,
                              const double T1[16], const double T2[16], const std::uint8_t* image1 = nullptr, int width = 0,
                              int height = 0, bool query_is_first = true, std::vector<core::MapPoint>* new_points = nullptr);
    void filterOutliers();                                // Mapper::filterOutliers
    void filterByDistance(double max_distance = 100.0);   // Mapper::filterByDistance
    std::vector<aria_map_point> records() const;          // the device records, in map order
    aria_map_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipMapper", where, rc); }
    detail::StageOwner<aria_map_t, aria_map_destroy> h_;
    MapperConfig cfg_;
    int next_pair_ = 0;
    std::vector<core::MapPoint> made_;                    // every point made since clear(), indexed by id
    mutable std::vector<core::MapPoint> cache_;
};

}  // namespace aria::adapters::hip
