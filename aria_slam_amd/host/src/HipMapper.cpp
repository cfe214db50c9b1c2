// See aria_hip/HipMapper.hpp.
#include "aria_hip/HipMapper.hpp"

#include <algorithm>
#include <fstream>
#include <stdexcept>

#include "aria_hip/ply.hpp"

namespace aria::adapters::hip {

namespace {
std::ofstream open_out(const std::string& filename) {
    std::ofstream f(filename);
    if (!f.is_open()) throw std::runtime_error("HipMapper: failed to open " + filename);
    return f;
}
}  // namespace

HipMapper::HipMapper(const MapperConfig& cfg) : cfg_(cfg) {
    aria_map_config c;
    aria_map_default_config(&c);
    c.device = cfg.device;
    c.stream = cfg.stream;
    c.fx = cfg.K.fx; c.fy = cfg.K.fy; c.cx = cfg.K.cx; c.cy = cfg.K.cy;
    c.min_depth = cfg.min_depth;
    c.max_depth = cfg.max_depth;
    c.min_parallax_deg = cfg.min_parallax_deg;
    c.max_reproj_px = cfg.max_reproj_px;
    c.capacity = cfg.capacity;
    expect("aria_map_create", aria_map_create(&c, h_.out()));
}

HipMapper::~HipMapper() = default;

int HipMapper::triangulateExtrinsics(const core::Frame& first, const core::Frame& second, const std::vector<core::Match>& matches,
                                     const double T1[16], const double T2[16], const std::uint8_t* image1, int width, int height,
                                     bool query_is_first, std::vector<core::MapPoint>* new_points) {
    static_assert(sizeof(core::KeyPoint) == sizeof(aria_keypoint) && sizeof(core::Match) == sizeof(aria_match), "layouts");
    const core::Frame& q = query_is_first ? first : second;
    const core::Frame& t = query_is_first ? second : first;
    std::int64_t before = 0;
    expect("aria_map_size", aria_map_size(h_.get(), &before));
    int added = 0;
    expect("aria_map_triangulate",
           aria_map_triangulate(h_.get(), reinterpret_cast<const aria_keypoint*>(q.keypoints.data()), (int)q.keypoints.size(),
                                reinterpret_cast<const aria_keypoint*>(t.keypoints.data()), (int)t.keypoints.size(),
                                reinterpret_cast<const aria_match*>(matches.data()), (int)matches.size(), query_is_first ? 1 : 0,
                                T1, T2, image1, width, height, width, nullptr, next_pair_, &added));
    next_pair_ = (next_pair_ + 1) & 0x7fffffff;
    std::vector<aria_map_point> recs((std::size_t)added);
    if (added) expect("aria_map_read", aria_map_read(h_.get(), before, added, recs.data()));
    for (const aria_map_point& r : recs) {
        core::MapPoint mp;
        mp.id = r.id;
        for (int k = 0; k < 3; k++) mp.position(k) = r.X[k];
        mp.observations = {{first.id, r.idx1}, {second.id, r.idx2}};
        mp.num_observations = 2;
        const std::size_t d = (std::size_t)r.idx1 * 32;
        if (first.descriptors.size() >= d + 32)
            mp.descriptor.assign(first.descriptors.begin() + (std::ptrdiff_t)d, first.descriptors.begin() + (std::ptrdiff_t)(d + 32));
        if (made_.size() <= r.id) made_.resize((std::size_t)r.id + 1);
        made_[(std::size_t)r.id] = mp;
        if (new_points) new_points->push_back(std::move(mp));
    }
    return added;
}

void HipMapper::triangulate(const core::Frame& frame1, const core::Frame& frame2, const core::Pose& pose1, const core::Pose& pose2,
                            const std::vector<core::Match>& matches, const MapperK& K, std::vector<core::MapPoint>& new_points) {
    if (K(0, 0) != cfg_.K.fx || K(1, 1) != cfg_.K.fy || K(0, 2) != cfg_.K.cx || K(1, 2) != cfg_.K.cy)
        throw std::invalid_argument("HipMapper::triangulate: K differs from the intrinsics the mapper was created with");
    const auto M1 = pose1.toMatrix();
    const auto M2 = pose2.toMatrix();
    double T1[16], T2[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            T1[r * 4 + c] = M1(r, c);
            T2[r * 4 + c] = M2(r, c);
        }
    new_points.clear();
    triangulateExtrinsics(frame1, frame2, matches, T1, T2, nullptr, 0, 0, true, &new_points);
}

std::vector<aria_map_point> HipMapper::records() const {
    std::int64_t n = 0;
    expect("aria_map_size", aria_map_size(h_.get(), &n));
    std::vector<aria_map_point> recs((std::size_t)n);
    if (n) expect("aria_map_read", aria_map_read(h_.get(), 0, n, recs.data()));
    return recs;
}

const std::vector<core::MapPoint>& HipMapper::getMapPoints() const {
    const std::vector<aria_map_point> recs = records();
    cache_.clear();
    cache_.reserve(recs.size());
    for (const aria_map_point& r : recs) cache_.push_back(made_[(std::size_t)r.id]);
    return cache_;
}

// Mapper::exportPLY / exportPCD (src/legacy/Mapper.cpp:170-235): r = g = b = the gray byte, ostream's default format
void HipMapper::exportPLY(const std::string& filename) const {
    const std::vector<aria_map_point> recs = records();
    std::ofstream file = open_out(filename);
    writePLY(file, recs);
}

void HipMapper::exportPCD(const std::string& filename) const {
    const std::vector<aria_map_point> recs = records();
    std::ofstream file = open_out(filename);
    file << "# .PCD v0.7 - Point Cloud Data\n";
    file << "VERSION 0.7\n";
    file << "FIELDS x y z rgb\n";
    file << "SIZE 4 4 4 4\n";
    file << "TYPE F F F U\n";
    file << "COUNT 1 1 1 1\n";
    file << "WIDTH " << recs.size() << "\n";
    file << "HEIGHT 1\n";
    file << "VIEWPOINT 0 0 0 1 0 0 0\n";
    file << "POINTS " << recs.size() << "\n";
    file << "DATA ascii\n";
    for (const aria_map_point& p : recs) {
        const std::uint32_t g = p.gray, rgb = (g << 16) | (g << 8) | g;
        file << p.X[0] << " " << p.X[1] << " " << p.X[2] << " " << rgb << "\n";
    }
}

void HipMapper::clear() {
    expect("aria_map_clear", aria_map_clear(h_.get()));
    made_.clear();
    cache_.clear();
}

std::size_t HipMapper::size() const {
    std::int64_t n = 0;
    expect("aria_map_size", aria_map_size(h_.get(), &n));
    return (std::size_t)n;
}

void HipMapper::filterOutliers() {
    int rc = aria_map_filter_outliers(h_.get());
    if (rc == ARIA_OK) rc = aria_map_check(h_.get());
    expect("aria_map_filter_outliers", rc);
}

void HipMapper::filterByDistance(double max_distance) {
    int rc = aria_map_filter_distance(h_.get(), max_distance);
    if (rc == ARIA_OK) rc = aria_map_check(h_.get());
    expect("aria_map_filter_distance", rc);
}

}  // namespace aria::adapters::hip
