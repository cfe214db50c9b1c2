// See aria_hip/HipBundleAdjuster.hpp.
#include "aria_hip/HipBundleAdjuster.hpp"

#include <stdexcept>
#include <string>
#include <unordered_map>

namespace aria::adapters::hip {

HipBundleAdjuster::HipBundleAdjuster(const PoseIntrinsics& K, double huber_px, double min_depth, int max_iterations, int max_windows,
                                     void* stream, int device) {
    aria_ba_config c;
    aria_ba_default_config(&c);
    c.device = device;
    c.stream = stream;
    c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy;
    if (huber_px >= 0) c.huber_px = huber_px;
    c.min_depth = min_depth;
    c.max_iterations = max_iterations;
    c.max_windows = max_windows;
    expect("aria_ba_create", aria_ba_create(&c, h_.out()));
}

HipBundleAdjuster::~HipBundleAdjuster() = default;

BundleResult HipBundleAdjuster::optimize(BundleWindow& w, int iterations) {
    BundleResult out;
    out.used.assign(w.obs.size(), 0);
    expect("aria_ba_optimize",
           aria_ba_optimize(h_.get(), w.poses.data(), w.pose_fixed.data(), w.nPoses(), w.points.data(), w.point_fixed.data(),
                            w.nPoints(), w.obs.data(), (int)w.obs.size(), iterations, &out.record, out.used.data()));
    return out;
}

void HipBundleAdjuster::optimizeBatchDevice(double* d_poses, const std::uint8_t* d_pose_fixed, double* d_points,
                                            const std::uint8_t* d_point_fixed, const aria_ba_obs* d_obs, const int* d_n_poses,
                                            const int* d_n_points, const int* d_n_obs, int n_windows, int pose_cap, int point_cap,
                                            int obs_cap, int iterations, aria_ba_result* d_out, std::uint8_t* d_used) {
    expect("aria_ba_optimize_batch_device",
           aria_ba_optimize_batch_device(h_.get(), d_poses, d_pose_fixed, d_points, d_point_fixed, d_obs, d_n_poses, d_n_points,
                                         d_n_obs, n_windows, pose_cap, point_cap, obs_cap, iterations, d_out, d_used));
}

void HipBundleAdjuster::check() {
    expect("aria_ba_check", aria_ba_check(h_.get()));
}

// ---- WindowBuilder ------------------------------------------------------------------------------------------------------------
namespace {
std::array<double, 12> rows34(const double pose[16]) {
    std::array<double, 12> p{};
    for (int k = 0; k < 12; k++) p[(std::size_t)k] = pose[k];
    return p;
}
}  // namespace

void WindowBuilder::addFrame(const core::Frame& frame, const double pose[16]) {
    poses_.assign(1, rows34(pose));
    tracks_.clear();
    live_.clear();
    last_px_.clear();
    for (const core::KeyPoint& k : frame.keypoints) last_px_.push_back({k.x, k.y});
}

void WindowBuilder::addStep(const core::Frame& current, const double pose[16], const std::vector<core::Match>& matches,
                            bool previous_is_query, const std::vector<aria_map_point>& new_points) {
    if (poses_.empty()) throw std::logic_error("WindowBuilder: addStep before addFrame");
    const int frame = (int)poses_.size();
    poses_.push_back(rows34(pose));
    // previous-frame index -> the current-frame index of its lowest match
    std::unordered_map<int, int> next;
    for (const core::Match& m : matches) {
        const int a = previous_is_query ? m.query_idx : m.train_idx, b = previous_is_query ? m.train_idx : m.query_idx;
        if (a < 0 || b < 0 || (std::size_t)b >= current.keypoints.size()) continue;
        next.emplace(a, b);                                           // the first (lowest index) wins
    }
    std::vector<std::size_t> live;
    for (std::size_t t : live_) {
        Track& tr = tracks_[t];
        const auto it = next.find(tr.carried);
        if (it == next.end()) continue;                               // the track ends here
        tr.carried = it->second;
        const core::KeyPoint& k = current.keypoints[(std::size_t)tr.carried];
        tr.seen.push_back(Seen{frame, k.x, k.y});
        live.push_back(t);
    }
    for (const aria_map_point& p : new_points) {
        if (p.idx1 < 0 || (std::size_t)p.idx1 >= last_px_.size() || p.idx2 < 0 || (std::size_t)p.idx2 >= current.keypoints.size())
            continue;
        Track tr{};
        for (int a = 0; a < 3; a++) tr.X[a] = p.X[a];
        tr.first_frame = frame - 1;
        tr.seen.push_back(Seen{frame - 1, last_px_[(std::size_t)p.idx1][0], last_px_[(std::size_t)p.idx1][1]});
        const core::KeyPoint& k2 = current.keypoints[(std::size_t)p.idx2];
        tr.seen.push_back(Seen{frame, k2.x, k2.y});
        tr.carried = p.idx2;
        tracks_.push_back(tr);
        live.push_back(tracks_.size() - 1);
    }
    live_.swap(live);
    last_px_.clear();
    for (const core::KeyPoint& k : current.keypoints) last_px_.push_back({k.x, k.y});
}

BundleWindow WindowBuilder::window(int first_frame, int n_frames, int n_fixed) const {
    BundleWindow w;
    w.first_frame = first_frame;
    if (first_frame < 0 || n_frames < 2 || n_frames > ARIA_BA_MAX_POSES || first_frame + n_frames > frames())
        throw std::out_of_range("WindowBuilder::window");
    for (int f = 0; f < n_frames; f++) {
        const std::array<double, 12>& p = poses_[(std::size_t)(first_frame + f)];
        w.poses.insert(w.poses.end(), p.begin(), p.end());
        w.pose_fixed.push_back(f < n_fixed ? 1 : 0);
    }
    for (std::size_t t = 0; t < tracks_.size(); t++) {
        const Track& tr = tracks_[t];
        if (tr.first_frame < first_frame || tr.first_frame + 1 >= first_frame + n_frames) continue;
        const int j = w.nPoints();
        w.points.insert(w.points.end(), tr.X, tr.X + 3);
        w.point_fixed.push_back(0);
        w.point_src.push_back((int)t);
        for (const Seen& s : tr.seen)
            if (s.frame < first_frame + n_frames) w.obs.push_back(aria_ba_obs{j, s.frame - first_frame, s.u, s.v});
    }
    return w;
}

void WindowBuilder::store(const BundleWindow& w) {
    for (int f = 0; f < w.nPoses(); f++)
        for (int k = 0; k < 12; k++) poses_[(std::size_t)(w.first_frame + f)][(std::size_t)k] = w.poses[(std::size_t)(12 * f + k)];
    for (int j = 0; j < w.nPoints(); j++)
        for (int a = 0; a < 3; a++) tracks_[(std::size_t)w.point_src[(std::size_t)j]].X[a] = w.points[(std::size_t)(3 * j + a)];
}

}  // namespace aria::adapters::hip
