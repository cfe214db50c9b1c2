// aria::adapters::hip::HipBundleAdjuster -- local bundle adjustment over the C-ABI (include/aria_orb_hip.h, "local bundle
// adjustment"): the poses and points of a sliding window refined together on the device, and WindowBuilder, the host
// bookkeeping that turns what MapTracker does step by step into such windows with the rule of the device's track builder.
// The reference has no bundle adjustment; its notes name the step (README.md:1162). aria_slam_amd/ba_ref.py is the definition.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

// One window as the C-ABI takes it: world-to-camera poses [R t] (12 doubles each), points, observations sorted by (point, pose)
struct BundleWindow {
    std::vector<double> poses;
    std::vector<std::uint8_t> pose_fixed;
    std::vector<double> points;
    std::vector<std::uint8_t> point_fixed;
    std::vector<aria_ba_obs> obs;
    std::vector<int> point_src;         // WindowBuilder: the track each point came from
    int first_frame = 0;
    int nPoses() const { return (int)pose_fixed.size(); }
    int nPoints() const { return (int)point_fixed.size(); }
};

struct BundleResult {
    aria_ba_result record{};
    std::vector<std::uint8_t> used;     // per observation
};

class HipBundleAdjuster {
public:
    explicit HipBundleAdjuster(const PoseIntrinsics& K = {}, double huber_px = -1.0, double min_depth = 1e-6, int max_iterations = 10,
                               int max_windows = 256, void* stream = nullptr, int device = 0);   // huber_px < 0: the default
    ~HipBundleAdjuster();

    // One window, updated in place; blocks. iterations = 0: the handle's. Throws on an invalid window.
    BundleResult optimize(BundleWindow& window, int iterations = 0);
    // aria_ba_optimize_batch_device, device pointers; enqueued on the handle's stream
    void optimizeBatchDevice(double* d_poses, const std::uint8_t* d_pose_fixed, double* d_points, const std::uint8_t* d_point_fixed,
                             const aria_ba_obs* d_obs, const int* d_n_poses, const int* d_n_points, const int* d_n_obs, int n_windows,
                             int pose_cap, int point_cap, int obs_cap, int iterations, aria_ba_result* d_out,
                             std::uint8_t* d_used = nullptr);
    void check();
    aria_ba_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipBundleAdjuster", where, rc); }
    detail::StageOwner<aria_ba_t, aria_ba_destroy> h_;
};

// The tracks of a sequence, kept on the host as MapTracker goes: a point the mapper triangulated from frames (f, f + 1) is
// seen at its view-1 and view-2 keypoints, and at every later frame a match carries it to -- the match whose previous-frame
// index equals the index carried so far, the lowest match index of several; the first step without one ends the track
// (aria_ba_window_from_chain_device's rule). Points keep the order the mapper appended them in.
class WindowBuilder {
public:
    // The first frame of the sequence, with its world-to-camera pose (4x4 row-major).
    void addFrame(const core::Frame& frame, const double pose[16]);
    // One step previous -> current: the new frame and its pose, the step's matches, and the points its triangulation appended
    // (idx1 indexes the previous frame, idx2 the current one). A held step passes no points.
    void addStep(const core::Frame& current, const double pose[16], const std::vector<core::Match>& matches, bool previous_is_query,
                 const std::vector<aria_map_point>& new_points);
    int frames() const { return (int)poses_.size(); }
    std::size_t tracks() const { return tracks_.size(); }
    // The window of n_frames frames from first_frame: its poses (the first n_fixed fixed), the points whose pair lies in it and
    // their observations up to its last frame.
    BundleWindow window(int first_frame, int n_frames, int n_fixed = 2) const;
    // The refined poses and points of a window back into the builder (they seed the windows that follow).
    void store(const BundleWindow& window);
    const std::array<double, 12>& pose(int frame) const { return poses_[(std::size_t)frame]; }

private:
    struct Seen { int frame; float u, v; };
    struct Track { double X[3]; int first_frame; std::vector<Seen> seen; int carried; };   // carried: its index in the last frame
    std::vector<std::array<double, 12>> poses_;
    std::vector<Track> tracks_;
    std::vector<std::size_t> live_;     // tracks that reach the last frame
    std::vector<std::array<float, 2>> last_px_;   // the last frame's keypoint pixels
};

}  // namespace aria::adapters::hip
