// See aria_hip/HipPoseGraphOptimizer.hpp.
#include "aria_hip/HipPoseGraphOptimizer.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

namespace {
constexpr double kLoopWeight = 10.0;         // LoopClosure.cpp: loop edges at 10x the information

void rowsOf(const GraphPose& T, double rows[12]) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) rows[r * 4 + c] = T(r, c);
}
}  // namespace

HipPoseGraphOptimizer::HipPoseGraphOptimizer(int pcg_max_iters, double pcg_rel_tol, void* stream, int device) {
    aria_graph_default_config(&cfg_);
    cfg_.device = device;
    cfg_.stream = stream;
    cfg_.pcg_max_iters = pcg_max_iters;
    cfg_.pcg_rel_tol = pcg_rel_tol;
    cfg_.max_graphs = 1;
    cfg_.max_vertices = 0;                   // no handle yet: created at the first optimize()
    cfg_.max_edges = 0;
}

HipPoseGraphOptimizer::~HipPoseGraphOptimizer() = default;

void HipPoseGraphOptimizer::setInitialPose(int id, const GraphPose& pose) {
    double rows[12];
    rowsOf(pose, rows);
    auto it = index_.find(id);
    if (it == index_.end()) {
        index_[id] = (int)(poses_.size() / 12);
        poses_.insert(poses_.end(), rows, rows + 12);
    } else {
        std::copy(rows, rows + 12, poses_.begin() + 12 * (std::size_t)it->second);
    }
}

void HipPoseGraphOptimizer::addEdge(int from_id, int to_id, const double rows[12], double info_scale) {
    const auto a = index_.find(from_id), b = index_.find(to_id);
    if (a == index_.end() || b == index_.end()) return;                 // LoopClosure.cpp:258-261
    if (a->second == b->second) return;                                 // an edge from a vertex to itself is invalid input of the stage
    aria_graph_edge e{};
    e.from = a->second;
    e.to = b->second;
    e.info_scale = info_scale;
    std::copy(rows, rows + 12, e.Z);
    edges_.push_back(e);
}

void HipPoseGraphOptimizer::addOdometryEdge(int from_id, int to_id, const GraphPose& relative_pose, double info_scale) {
    double rows[12];
    rowsOf(relative_pose, rows);
    addEdge(from_id, to_id, rows, info_scale);
}

void HipPoseGraphOptimizer::addLoopEdge(int from_id, int to_id, const GraphPose& relative_pose, double info_scale) {
    double rows[12];
    rowsOf(relative_pose, rows);
    addEdge(from_id, to_id, rows, info_scale * kLoopWeight);
}

void HipPoseGraphOptimizer::optimize(int iterations) {
    const int nv = (int)(poses_.size() / 12), ne = (int)edges_.size();
    if (nv == 0) return;
    if (!h_.get() || nv > cfg_.max_vertices || ne > cfg_.max_edges) {
        h_.reset();
        cfg_.max_vertices = std::max(std::max(nv, 2 * cfg_.max_vertices), 256);
        cfg_.max_edges = std::max(std::max(ne, 2 * cfg_.max_edges), 256);
        expect("aria_graph_create", aria_graph_create(&cfg_, h_.out()));
    }
    expect("aria_graph_optimize", aria_graph_optimize(h_.get(), poses_.data(), nv, 0, edges_.data(), ne, iterations, &last_));
}

GraphPose HipPoseGraphOptimizer::getOptimizedPose(int id) const {
    GraphPose T = GraphPose::Identity();
    const auto it = index_.find(id);
    if (it == index_.end()) return T;
    const double* rows = poses_.data() + 12 * (std::size_t)it->second;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) T(r, c) = rows[r * 4 + c];
    return T;
}

std::vector<GraphPose> HipPoseGraphOptimizer::getAllPoses() const {
    std::vector<GraphPose> out;
    out.reserve(index_.size());
    for (const auto& kv : index_) out.push_back(getOptimizedPose(kv.first));     // std::map: ascending id
    return out;
}

void HipPoseGraphOptimizer::clear() {
    index_.clear();
    poses_.clear();
    edges_.clear();
}

}  // namespace aria::adapters::hip
