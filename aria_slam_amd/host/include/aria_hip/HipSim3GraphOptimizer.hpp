// aria::adapters::hip::HipSim3GraphOptimizer -- the Sim(3) pose graph and the map correction after a loop (the roles of
// ORB-SLAM's OptimizeEssentialGraph and CorrectLoop; the reference has neither) over the C-ABI (include/aria_orb_hip.h,
// "Sim(3) pose-graph optimisation"; aria_slam_amd/sgraph_ref.py is the definition of the stage).
//
// The surface and the bookkeeping are HipPoseGraphOptimizer's: ids map to dense vertex indices in the order they were first
// added, the first one added is the fixed vertex, setInitialPose on a known id overwrites the estimate (and puts its scale
// back to 1), an edge that names an unknown id is dropped silently, loop edges carry 10x the information. In addition a loop
// edge carries the scale of its alignment (aria_sim3_result::s with keyframe 1 = `to` and keyframe 2 = `from`),
// getOptimizedScale returns what the graph made of it, and correctMap moves a point map by each pair's anchor keyframe:
// X' = S_new S_old^-1 X with S_old the vertices as they entered the last optimize() and S_new as they left it.
//
// Poses are camera-to-world GraphPose (HipPoseGraphOptimizer.hpp); a caller that holds world-to-camera poses inverts them on
// the host in fp64 (cameraToWorld below). After the correction a keyframe's pose is [R_new t_new] with s dropped: a point at
// camera coordinates x_c is now at s_new x_c -- the local structure is rescaled, the camera is not.
#pragma once
#include <map>
#include <vector>

#include "aria_hip/HipPoseGraphOptimizer.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

// the inverse of a rigid [R t; 0 1] in fp64: [R^T, -R^T t]
GraphPose cameraToWorld(const GraphPose& world_to_camera);

class HipSim3GraphOptimizer {
public:
    explicit HipSim3GraphOptimizer(bool fix_scale = false, int pcg_max_iters = 1000, double pcg_rel_tol = 1e-8, void* stream = nullptr,
                                   int device = 0);
    ~HipSim3GraphOptimizer();

    // HipPoseGraphOptimizer's surface
    void addOdometryEdge(int from_id, int to_id, const GraphPose& relative_pose, double info_scale = 1.0);
    void addLoopEdge(int from_id, int to_id, const GraphPose& relative_pose, double scale = 1.0, double info_scale = 1.0);
    void setInitialPose(int id, const GraphPose& pose);
    void optimize(int iterations = 10);
    GraphPose getOptimizedPose(int id) const;
    double getOptimizedScale(int id) const;                  // 1 for an unknown id
    std::vector<GraphPose> getAllPoses() const;
    void clear();

    // Moves the arena of `map` (aria_sgraph_correct_map_device; blocks): a point of pair p with pair_base <= p < pair_base +
    // pair_anchor_id.size() moves with the keyframe id pair_anchor_id[p - pair_base]; an id the graph does not know, or -1,
    // leaves its points alone. Returns the counts. Nothing else may use the map while this runs.
    // Precondition: optimize() has run on the graph as it stands -- a vertex added by setInitialPose since then, or no
    // optimize() at all, makes the call throw std::runtime_error (S_old and S_new must name the same vertices); so does clear().
    // Afterwards the host copies a HipMapper keeps of the points it made (getMapPoints) are stale: records(), exportPLY and
    // exportPCD read the corrected arena.
    aria_sgraph_correct_stats correctMap(aria_map_t map, const std::vector<int>& pair_anchor_id, int pair_base = 0);

    const aria_sgraph_result& lastResult() const { return last_; }
    std::size_t numVertices() const { return verts_.size(); }
    std::size_t numEdges() const { return edges_.size(); }
    const std::vector<aria_sgraph_vertex>& vertices() const { return verts_; }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipSim3GraphOptimizer", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipSim3GraphOptimizer", where, rc); }
    void addEdge(int from_id, int to_id, const GraphPose& rel, double scale, double info_scale);
    void ensureHandle(int nv, int ne);
    detail::StageOwner<aria_sgraph_t, aria_sgraph_destroy> h_;
    aria_sgraph_config cfg_{};
    std::map<int, int> index_;               // id -> vertex index, in order of first setInitialPose
    std::vector<aria_sgraph_vertex> verts_;  // the estimates
    std::vector<aria_sgraph_vertex> before_; // the vertices as they entered the last optimize()
    std::vector<aria_sgraph_edge> edges_;
    aria_sgraph_result last_{};
};

}  // namespace aria::adapters::hip
