// See aria_hip/HipSim3GraphOptimizer.hpp.
#include "aria_hip/HipSim3GraphOptimizer.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

namespace {
constexpr double kLoopWeight = 10.0;         // as HipPoseGraphOptimizer: loop edges at 10x the information

aria_sgraph_vertex vertexOf(const GraphPose& T) {
    aria_sgraph_vertex v{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) v.R[3 * r + c] = T(r, c);
        v.t[r] = T(r, 3);
    }
    v.s = 1.0;
    return v;
}

// device memory of one correctMap call, freed on every path
struct DeviceBlock {
    int device;
    void* p = nullptr;
    DeviceBlock(int dev, std::size_t bytes) : device(dev) {
        if (aria_device_alloc(dev, std::max<std::size_t>(bytes, 8), &p) != ARIA_OK) p = nullptr;
    }
    ~DeviceBlock() {
        if (p) aria_device_free(device, p);
    }
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
};
}  // namespace

GraphPose cameraToWorld(const GraphPose& T) {
    GraphPose X = GraphPose::Identity();
    for (int r = 0; r < 3; r++) {
        double t = 0.0;
        for (int c = 0; c < 3; c++) {
            X(r, c) = T(c, r);
            t -= T(c, r) * T(c, 3);
        }
        X(r, 3) = t;
    }
    return X;
}

HipSim3GraphOptimizer::HipSim3GraphOptimizer(bool fix_scale, int pcg_max_iters, double pcg_rel_tol, void* stream, int device) {
    aria_sgraph_default_config(&cfg_);
    cfg_.device = device;
    cfg_.stream = stream;
    cfg_.pcg_max_iters = pcg_max_iters;
    cfg_.pcg_rel_tol = pcg_rel_tol;
    cfg_.fix_scale = fix_scale ? 1 : 0;
    cfg_.max_graphs = 1;
    cfg_.max_vertices = 0;                   // no handle yet: created at the first optimize() or correctMap()
    cfg_.max_edges = 0;
}

HipSim3GraphOptimizer::~HipSim3GraphOptimizer() = default;

void HipSim3GraphOptimizer::setInitialPose(int id, const GraphPose& pose) {
    const aria_sgraph_vertex v = vertexOf(pose);
    auto it = index_.find(id);
    if (it == index_.end()) {
        index_[id] = (int)verts_.size();
        verts_.push_back(v);
    } else {
        verts_[(std::size_t)it->second] = v;
    }
}

void HipSim3GraphOptimizer::addEdge(int from_id, int to_id, const GraphPose& rel, double scale, double info_scale) {
    const auto a = index_.find(from_id), b = index_.find(to_id);
    if (a == index_.end() || b == index_.end()) return;                 // an unknown id: dropped silently
    if (a->second == b->second) return;                                 // an edge from a vertex to itself is invalid input of the stage
    aria_sgraph_edge e{};
    e.from = a->second;
    e.to = b->second;
    e.info_scale = info_scale;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) e.Z[r * 4 + c] = rel(r, c);
    e.s = scale;
    edges_.push_back(e);
}

void HipSim3GraphOptimizer::addOdometryEdge(int from_id, int to_id, const GraphPose& relative_pose, double info_scale) {
    addEdge(from_id, to_id, relative_pose, 1.0, info_scale);
}

void HipSim3GraphOptimizer::addLoopEdge(int from_id, int to_id, const GraphPose& relative_pose, double scale, double info_scale) {
    addEdge(from_id, to_id, relative_pose, scale, info_scale * kLoopWeight);
}

void HipSim3GraphOptimizer::ensureHandle(int nv, int ne) {
    if (h_.get() && nv <= cfg_.max_vertices && ne <= cfg_.max_edges) return;
    h_.reset();
    cfg_.max_vertices = std::max(std::max(nv, 2 * cfg_.max_vertices), 256);
    cfg_.max_edges = std::max(std::max(ne, 2 * cfg_.max_edges), 256);
    expect("aria_sgraph_create", aria_sgraph_create(&cfg_, h_.out()));
}

void HipSim3GraphOptimizer::optimize(int iterations) {
    const int nv = (int)verts_.size(), ne = (int)edges_.size();
    if (nv == 0) return;
    ensureHandle(nv, ne);
    before_ = verts_;
    expect("aria_sgraph_optimize", aria_sgraph_optimize(h_.get(), verts_.data(), nv, 0, edges_.data(), ne, iterations, &last_));
}

GraphPose HipSim3GraphOptimizer::getOptimizedPose(int id) const {
    GraphPose T = GraphPose::Identity();
    const auto it = index_.find(id);
    if (it == index_.end()) return T;
    const aria_sgraph_vertex& v = verts_[(std::size_t)it->second];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T(r, c) = v.R[3 * r + c];
        T(r, 3) = v.t[r];
    }
    return T;
}

double HipSim3GraphOptimizer::getOptimizedScale(int id) const {
    const auto it = index_.find(id);
    return it == index_.end() ? 1.0 : verts_[(std::size_t)it->second].s;
}

std::vector<GraphPose> HipSim3GraphOptimizer::getAllPoses() const {
    std::vector<GraphPose> out;
    out.reserve(index_.size());
    for (const auto& kv : index_) out.push_back(getOptimizedPose(kv.first));     // std::map: ascending id
    return out;
}

void HipSim3GraphOptimizer::clear() {
    index_.clear();
    verts_.clear();
    before_.clear();
    edges_.clear();
}

aria_sgraph_correct_stats HipSim3GraphOptimizer::correctMap(aria_map_t map, const std::vector<int>& pair_anchor_id, int pair_base) {
    aria_sgraph_correct_stats stats{};
    const int nv = (int)verts_.size(), nt = (int)pair_anchor_id.size();
    if (before_.size() != verts_.size()) throw std::runtime_error("HipSim3GraphOptimizer: correctMap needs an optimize() of this graph first");
    ensureHandle(std::max(nv, 1), (int)edges_.size());
    std::vector<int> table((std::size_t)nt, -1);
    for (int k = 0; k < nt; k++) {
        const auto it = index_.find(pair_anchor_id[(std::size_t)k]);
        if (pair_anchor_id[(std::size_t)k] >= 0 && it != index_.end()) table[(std::size_t)k] = it->second;
    }
    const int dev = cfg_.device;
    void* st = aria_sgraph_stream(h_.get());
    const std::size_t vbytes = sizeof(aria_sgraph_vertex) * (std::size_t)nv;
    DeviceBlock d_table(dev, sizeof(int) * (std::size_t)nt), d_old(dev, vbytes), d_new(dev, vbytes), d_stats(dev, sizeof(stats));
    if (!d_table.p || !d_old.p || !d_new.p || !d_stats.p) fail("aria_device_alloc", ARIA_E_OOM);
    int rc = ARIA_OK;
    if (nt) rc = aria_copy_h2d_async(dev, st, d_table.p, table.data(), sizeof(int) * (std::size_t)nt);
    if (rc == ARIA_OK && nv) rc = aria_copy_h2d_async(dev, st, d_old.p, before_.data(), vbytes);
    if (rc == ARIA_OK && nv) rc = aria_copy_h2d_async(dev, st, d_new.p, verts_.data(), vbytes);
    expect("aria_copy_h2d_async", rc);
    expect("aria_sgraph_correct_map_device",
           aria_sgraph_correct_map_device(h_.get(), map, (const int*)d_table.p, nt, pair_base, (const aria_sgraph_vertex*)d_old.p,
                                          (const aria_sgraph_vertex*)d_new.p, nv, (aria_sgraph_correct_stats*)d_stats.p));
    expect("aria_copy_d2h_async", aria_copy_d2h_async(dev, st, &stats, d_stats.p, sizeof(stats)));
    expect("aria_sgraph_correct_map_device", aria_sgraph_check(h_.get()));   // synchronises: the copies and the kernel have run
    return stats;
}

}  // namespace aria::adapters::hip
