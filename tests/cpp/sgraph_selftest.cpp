// Drives aria_hip/HipSim3GraphOptimizer.hpp on the GPU.
//   sgraph_selftest            the closed walk of tests/cpp/sim3_selftest.cpp (tools/sim3_walk.py's scene, formula for formula: 16
//                              keyframes that return to their start with trajectory and map drifted in scale by 1.5) carried on:
//                              the first and the last pair triangulated (HipMapper), the loop aligned against the map
//                              (HipSim3Aligner), then the Sim(3) graph with the edge (R, t, s) beside the SE(3) graph with the same
//                              [R t], 20 iterations each, and the map corrected by the two pairs' anchor keyframes 0 and L - 1.
//                              Prints "key values..." lines that tests/test_cpp_sgraph.py checks.
//   sgraph_selftest IN OUT     one graph from IN through the adapter's surface, optimised, its vertices to OUT as raw doubles (13
//                              per vertex): what tests/test_cpp_sgraph.py compares bit for bit with the Python adapter. IN is
//                              int32 K, n_odometry, n_loop, iterations; K poses (16 doubles, camera-to-world, row-major);
//                              n_odometry x (int32 from, to; 16 doubles); n_loop x (int32 from, to; 16 doubles; double s).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipPoseGraphOptimizer.hpp"
#include "aria_hip/HipSim3Aligner.hpp"
#include "aria_hip/HipSim3GraphOptimizer.hpp"
#include "aria_orb_hip.h"

using namespace aria;

namespace {
const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;
const int K_FRAMES = 16, N_POINTS = 300;
const double DRIFT = 1.5, RADIUS = 1.0, CLOSE = 0.95;

double u01(long long k) { return (double)((unsigned long long)(k * 2654435761LL + 12345LL) % (1ULL << 32)) / 4294967296.0; }

using Mat4 = std::array<double, 16>;       // row-major

Mat4 rigid(const double R[9], const double c[3]) {      // world-to-camera [R | -R c]
    Mat4 T{};
    for (int r = 0; r < 3; r++) {
        for (int q = 0; q < 3; q++) T[(size_t)(r * 4 + q)] = R[r * 3 + q];
        T[(size_t)(r * 4 + 3)] = -(R[r * 3] * c[0] + R[r * 3 + 1] * c[1] + R[r * 3 + 2] * c[2]);
    }
    T[15] = 1.0;
    return T;
}

Mat4 inverse(const Mat4& T) {
    Mat4 I{};
    for (int r = 0; r < 3; r++) {
        for (int q = 0; q < 3; q++) I[(size_t)(r * 4 + q)] = T[(size_t)(q * 4 + r)];
        I[(size_t)(r * 4 + 3)] = -(T[(size_t)r] * T[3] + T[(size_t)(4 + r)] * T[7] + T[(size_t)(8 + r)] * T[11]);
    }
    I[15] = 1.0;
    return I;
}

Mat4 mul(const Mat4& A, const Mat4& B) {
    Mat4 C{};
    for (int r = 0; r < 4; r++)
        for (int q = 0; q < 4; q++)
            for (int k = 0; k < 4; k++) C[(size_t)(r * 4 + q)] += A[(size_t)(r * 4 + k)] * B[(size_t)(k * 4 + q)];
    return C;
}

adapters::hip::GraphPose graphPose(const Mat4& T) {
    adapters::hip::GraphPose m = adapters::hip::GraphPose::Identity();
    for (int r = 0; r < 4; r++)
        for (int q = 0; q < 4; q++) m(r, q) = T[(size_t)(r * 4 + q)];
    return m;
}

// (rms, max) distance of the optimised camera centres from the scene's, nothing aligned
template <class G>
std::array<double, 2> ate(const G& g, const std::vector<std::array<double, 3>>& centre) {
    double sum = 0.0, mx = 0.0;
    for (int i = 0; i < K_FRAMES; i++) {
        const adapters::hip::GraphPose X = g.getOptimizedPose(i);
        double d2 = 0.0;
        for (int k = 0; k < 3; k++) d2 += (X(k, 3) - centre[(size_t)i][(size_t)k]) * (X(k, 3) - centre[(size_t)i][(size_t)k]);
        sum += d2;
        mx = std::max(mx, std::sqrt(d2));
    }
    return {std::sqrt(sum / K_FRAMES), mx};
}

int walk() {
    const int L = K_FRAMES - 1;
    std::vector<Mat4> truth((size_t)K_FRAMES), drifted((size_t)K_FRAMES);
    std::vector<std::array<double, 3>> centre((size_t)K_FRAMES);
    double cd[3] = {0, 0, 0};
    for (int i = 0; i < K_FRAMES; i++) {
        const double th = i * (2.0 * M_PI * CLOSE) / (K_FRAMES - 1);
        centre[(size_t)i] = {RADIUS * std::sin(th), 0.1 * RADIUS * std::sin(2.0 * th), RADIUS * (std::cos(th) - 1.0)};
        const double a = (3.0 * M_PI / 180.0) * std::sin(th);
        const double R[9] = {std::cos(a), 0.0, std::sin(a), 0.0, 1.0, 0.0, -std::sin(a), 0.0, std::cos(a)};
        truth[(size_t)i] = rigid(R, centre[(size_t)i].data());
        if (i == 0) for (int k = 0; k < 3; k++) cd[k] = centre[0][(size_t)k];
        else {
            const double g = std::pow(DRIFT, i / (K_FRAMES - 1.0));
            for (int k = 0; k < 3; k++) cd[k] += g * (centre[(size_t)i][(size_t)k] - centre[(size_t)i - 1][(size_t)k]);
        }
        drifted[(size_t)i] = rigid(R, cd);
    }
    std::vector<core::Frame> f((size_t)K_FRAMES);
    for (int i = 0; i < K_FRAMES; i++) {
        f[(size_t)i].id = (std::uint64_t)i;
        for (int j = 0; j < N_POINTS; j++) {
            const double u = 100.0 + 550.0 * u01(3 * j), v = 80.0 + 320.0 * u01(3 * j + 1), z = 4.0 + 8.0 * u01(3 * j + 2);
            const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
            const Mat4& T = truth[(size_t)i];
            double Y[3];
            for (int r = 0; r < 3; r++) Y[r] = T[(size_t)(r * 4)] * X[0] + T[(size_t)(r * 4 + 1)] * X[1] + T[(size_t)(r * 4 + 2)] * X[2] + T[(size_t)(r * 4 + 3)];
            const long long k = 2LL * ((long long)i * N_POINTS + j);
            const double nx = 0.6 * (u01(1000003 + k) - 0.5), ny = 0.6 * (u01(1000004 + k) - 0.5);
            f[(size_t)i].keypoints.push_back({(float)(fx * Y[0] / Y[2] + cx + nx), (float)(fy * Y[1] / Y[2] + cy + ny), 31.f, 0.f, 1.f, 0});
        }
        f[(size_t)i].descriptors.assign((size_t)N_POINTS * 32, 0);
    }
    std::vector<core::Match> ident, loop;
    for (int j = 0; j < N_POINTS; j++) {
        ident.push_back({j, j, 10.f});
        loop.push_back({j, j % 7 == 3 ? (j + 1) % N_POINTS : j, 10.f});     // query = keyframe L, train = keyframe 0
    }
    // the map: the first pair in the start's scale (pair id 0), the last pair in the drifted scale (pair id 1)
    adapters::hip::HipMapper mapper;
    const int added0 = mapper.triangulateExtrinsics(f[0], f[1], ident, drifted[0].data(), drifted[1].data());
    const int added1 = mapper.triangulateExtrinsics(f[(size_t)L - 1], f[(size_t)L], ident, drifted[(size_t)L - 1].data(), drifted[(size_t)L].data());
    adapters::hip::KeyframeInMap kL, k0;
    kL.anchor_pair = 1; kL.anchor_view = 2; kL.frame = &f[(size_t)L];
    k0.anchor_pair = 0; k0.anchor_view = 1; k0.frame = &f[0];
    for (int k = 0; k < 12; k++) { kL.pose[(size_t)k] = drifted[(size_t)L][(size_t)k]; k0.pose[(size_t)k] = drifted[0][(size_t)k]; }
    adapters::hip::HipSim3Aligner aligner;
    const auto sim = aligner.estimateAgainstMap(mapper.handle(), kL, k0, loop, L);     // keyframe 1 = L = `to`, keyframe 2 = 0 = `from`
    std::printf("walk_map %d %d\n", added0, added1);
    if (!sim) { std::printf("walk_sim 0\n"); return 1; }
    std::printf("walk_sim 1 %.6f %d\n", sim->s, sim->n_inliers);
    adapters::hip::GraphPose edge = adapters::hip::GraphPose::Identity();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) edge(r, c) = sim->R[(size_t)(r * 3 + c)];
        edge(r, 3) = sim->t[(size_t)r];
    }
    adapters::hip::HipPoseGraphOptimizer g6;
    adapters::hip::HipSim3GraphOptimizer g7;
    for (int i = 0; i < K_FRAMES; i++) {                                   // vertices are camera-to-world; Z_ij = X_i^-1 X_j
        const adapters::hip::GraphPose X = adapters::hip::cameraToWorld(graphPose(drifted[(size_t)i]));
        g6.setInitialPose(i, X);
        g7.setInitialPose(i, X);
        if (i) {
            const adapters::hip::GraphPose Z = graphPose(mul(drifted[(size_t)i - 1], inverse(drifted[(size_t)i])));
            g6.addOdometryEdge(i - 1, i, Z);
            g7.addOdometryEdge(i - 1, i, Z);
        }
    }
    std::vector<std::array<double, 3>> before_c((size_t)K_FRAMES);
    for (int i = 0; i < K_FRAMES; i++)
        for (int k = 0; k < 3; k++) before_c[(size_t)i][(size_t)k] = g7.getOptimizedPose(i)(k, 3);
    const std::array<double, 2> a0 = ate(g7, centre);
    g6.addLoopEdge(0, L, edge);
    g7.addLoopEdge(0, L, edge, sim->s);
    g6.optimize(20);
    g7.optimize(20);
    const std::array<double, 2> a6 = ate(g6, centre), a7 = ate(g7, centre);
    std::printf("walk_ate %.6f %.6f %.6f %.6f %.6f %.6f\n", a0[0], a0[1], a6[0], a6[1], a7[0], a7[1]);
    std::printf("walk_scale %.6f %.6f %.6f\n", g7.getOptimizedScale(0), g7.getOptimizedScale(L - 1), g7.getOptimizedScale(L));
    // the map after the loop: pair 0 hangs on keyframe 0 (the fixed vertex: nothing moves), pair 1 on keyframe L - 1
    const std::vector<aria_map_point> before = mapper.records();
    const aria_sgraph_correct_stats st = g7.correctMap(mapper.handle(), {0, L - 1}, 0);
    const std::vector<aria_map_point> after = mapper.records();
    int same0 = 0, moved1 = 0, other = 0;
    double shrink = 0.0;
    const adapters::hip::GraphPose XL1 = g7.getOptimizedPose(L - 1);
    const adapters::hip::GraphPose XL1_old = adapters::hip::cameraToWorld(graphPose(drifted[(size_t)L - 1]));
    for (std::size_t i = 0; i < before.size(); i++) {
        const bool same = before[i].X[0] == after[i].X[0] && before[i].X[1] == after[i].X[1] && before[i].X[2] == after[i].X[2];
        if (before[i].pair == 0) same0 += same ? 1 : 0;
        else moved1 += same ? 0 : 1;
        if (before[i].id != after[i].id || before[i].pair != after[i].pair || before[i].idx1 != after[i].idx1 || before[i].quality != after[i].quality) other++;
        if (before[i].pair == 1) {       // distance from the anchor's centre, after over before: the anchor's new scale
            double d0 = 0, d1 = 0;
            for (int k = 0; k < 3; k++) {
                d0 += std::pow(before[i].X[k] - XL1_old(k, 3), 2);
                d1 += std::pow(after[i].X[k] - XL1(k, 3), 2);
            }
            shrink += std::sqrt(d1 / d0);
        }
    }
    std::printf("walk_correct %d %d %d %zu %d %d %d %d %.6f\n", st.moved, st.left_alone, st.refused, before.size(), added0, same0, moved1, other,
                added1 ? shrink / added1 : 0.0);
    return 0;
}

int fromFile(const char* in, const char* out) {
    std::FILE* fi = std::fopen(in, "rb");
    if (!fi) return 2;
    std::int32_t head[4];
    if (std::fread(head, sizeof(head), 1, fi) != 1) return 2;
    adapters::hip::HipSim3GraphOptimizer g;
    Mat4 T;
    for (int i = 0; i < head[0]; i++) {
        if (std::fread(T.data(), sizeof(double), 16, fi) != 16) return 2;
        g.setInitialPose(i, graphPose(T));
    }
    for (int k = 0; k < head[1] + head[2]; k++) {
        std::int32_t ft[2];
        double s = 1.0;
        if (std::fread(ft, sizeof(ft), 1, fi) != 1 || std::fread(T.data(), sizeof(double), 16, fi) != 16) return 2;
        if (k >= head[1] && std::fread(&s, sizeof(double), 1, fi) != 1) return 2;
        if (k < head[1]) g.addOdometryEdge(ft[0], ft[1], graphPose(T));
        else g.addLoopEdge(ft[0], ft[1], graphPose(T), s);
    }
    std::fclose(fi);
    g.optimize(head[3]);
    std::FILE* fo = std::fopen(out, "wb");
    if (!fo) return 2;
    std::fwrite(g.vertices().data(), sizeof(aria_sgraph_vertex), g.vertices().size(), fo);
    std::fclose(fo);
    const aria_sgraph_result& r = g.lastResult();
    std::printf("graph %zu %zu %d %d %d\n", g.numVertices(), g.numEdges(), r.iterations_done, r.trials, r.valid);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const int rc = argc == 3 ? fromFile(argv[1], argv[2]) : walk();
    if (rc == 0) std::printf("DONE\n");
    return rc;
}
