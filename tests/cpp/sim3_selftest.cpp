// Drives the loop-alignment adapters on the GPU: HipSim3Aligner::estimate on a synthetic pair of landmark clouds whose maps
// differ by a scale of 2; estimateAgainstMap on the map a MapTracker bootstraps (keyframe 1 = the pair's second view, keyframe
// 2 = its first: one scale, s = 1, and the similarity is the inverse of the tracker's pose, whose translation is one map unit
// long); and makeSim3Verifier, which overwrites a candidate's unit-length relative pose with that edge and leaves it alone
// when the inlier gate is not met or the keyframe is unknown; and the closed walk of tools/sim3_walk.py: 16 keyframes that
// return to their start with the map's scale drifted by 1.5, the first and last pair triangulated, the loop edge made by the
// verifier behind a two-view stand-in, and the pose graph optimised with that edge and with the unit-length one. Prints
// "key values..." lines that tests/test_cpp_sim3.py checks.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipPoseGraphOptimizer.hpp"
#include "aria_hip/HipSim3Aligner.hpp"
#include "aria_hip/MapTracker.hpp"
#include "aria_orb_hip.h"

using namespace aria;

namespace {
const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;

struct View {
    double R[9], t[3];
};

View yaw(double deg, double tx, double ty, double tz) {
    const double th = deg * M_PI / 180.0;
    return View{{std::cos(th), 0, std::sin(th), 0, 1, 0, -std::sin(th), 0, std::cos(th)}, {tx, ty, tz}};
}

void apply(const View& v, double s, const double X[3], double Y[3]) {
    for (int r = 0; r < 3; r++) Y[r] = s * (v.R[r * 3] * X[0] + v.R[r * 3 + 1] * X[1] + v.R[r * 3 + 2] * X[2]) + v.t[r];
}

bool pixel(const double Y[3], double& u, double& w) {
    if (Y[2] < 0.5) return false;
    u = fx * Y[0] / Y[2] + cx;
    w = fy * Y[1] / Y[2] + cy;
    return u >= 0 && u < 752 && w >= 0 && w < 480;
}

double rot_err_deg(const double* A, const double* B) {
    double tr = 0;
    for (int k = 0; k < 9; k++) tr += A[k] * B[k];
    return std::acos(std::max(-1.0, std::min(1.0, (tr - 1) / 2))) * 180.0 / M_PI;
}

double dist(const double* a, const double* b) { return std::sqrt(std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2)); }
}  // namespace

// ---- 4. the closed walk of tools/sim3_walk.py, formula for formula --------------------------------------------------------------
namespace {
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

void walk() {
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
    auto lookup = [&](std::uint64_t id) -> std::optional<adapters::hip::KeyframeInMap> {
        if (id == (std::uint64_t)L) return kL;
        if (id == 0) return k0;
        return std::nullopt;
    };
    const Mat4 T_true = mul(truth[0], inverse(truth[(size_t)L]));          // camera L's coordinates -> camera 0's
    const double tl = std::sqrt(T_true[3] * T_true[3] + T_true[7] * T_true[7] + T_true[11] * T_true[11]);
    // the verifier in front: what a two-view verification hands over -- the true rotation, the true direction, length 1
    auto two_view = [&](const core::KeyFrame&, std::uint64_t, core::LoopCandidate& c) {
        for (int r = 0; r < 3; r++) {
            for (int q = 0; q < 3; q++) adapters::hip::detail::setEntry(c.relative_pose, r, q, T_true[(size_t)(r * 4 + q)], 0);
            adapters::hip::detail::setEntry(c.relative_pose, r, 3, T_true[(size_t)(r * 4 + 3)] / tl, 0);
        }
        return true;
    };
    core::KeyFrame q;
    q.id = (std::uint64_t)L;
    q.frame = f[(size_t)L];
    adapters::hip::HipSim3Aligner aligner;
    adapters::hip::Sim3Report rep;
    core::LoopCandidate with, without;
    with.query_id = without.query_id = (std::uint64_t)L;
    with.matches = without.matches = loop;
    const bool ok = adapters::hip::makeSim3Verifier(aligner, mapper.handle(), lookup, two_view, 20,
                                                    [&](const adapters::hip::Sim3Report& r) { rep = r; })(q, 0, with);
    two_view(q, 0, without);
    const adapters::hip::GraphPose edge = adapters::hip::loopRelativePose(with);
    const double et[3] = {edge(0, 3), edge(1, 3), edge(2, 3)}, tt[3] = {T_true[3], T_true[7], T_true[11]}, zero[3] = {0, 0, 0};
    std::printf("walk_map %d %d\n", added0, added1);
    std::printf("walk_edge %d %d %.6f %d %d %.4f %.6f %.6f %.6f\n", ok ? 1 : 0, rep.replaced ? 1 : 0, rep.s, rep.n_corr, rep.n_inliers, rep.rms_px,
                dist(et, zero), tl, dist(et, tt));
    const core::LoopCandidate* cands[2] = {&with, &without};
    const char* names[2] = {"walk_aligned", "walk_unit"};
    for (int v = 0; v < 2; v++) {
        adapters::hip::HipPoseGraphOptimizer g;
        for (int i = 0; i < K_FRAMES; i++) {                                   // vertices are camera-to-world; Z_ij = X_i^-1 X_j
            g.setInitialPose(i, graphPose(inverse(drifted[(size_t)i])));
            if (i) g.addOdometryEdge(i - 1, i, graphPose(mul(drifted[(size_t)i - 1], inverse(drifted[(size_t)i]))));
        }
        g.addLoopEdge(0, L, adapters::hip::loopRelativePose(*cands[v]));       // X_0^-1 X_L: camera L's coordinates -> camera 0's
        g.optimize(20);
        const adapters::hip::GraphPose X0 = g.getOptimizedPose(0), XL = g.getOptimizedPose(L);
        Mat4 A{}, B{};
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) { A[(size_t)(r * 4 + c)] = X0(r, c); B[(size_t)(r * 4 + c)] = XL(r, c); }
        const Mat4 E = mul(inverse(A), B);
        double Re[9], Rt[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) { Re[r * 3 + c] = E[(size_t)(r * 4 + c)]; Rt[r * 3 + c] = T_true[(size_t)(r * 4 + c)]; }
        const double te[3] = {E[3], E[7], E[11]};
        std::printf("%s %.6f %.6f\n", names[v], rot_err_deg(Re, Rt), dist(te, tt));
    }
}
}  // namespace

int main() {
    std::mt19937 g(11);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(3, 12);
    std::normal_distribution<double> N(0, 0.3);

    // 1. two clouds: X2 = 2 R X1 + t, 0.3 px on the four pixels, every fifth correspondence paired with its neighbour's side 2
    const View rel = yaw(6, 1.6, 0.2, 0.6);
    std::vector<aria_sim3_corr> direct;
    while (direct.size() < 400) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X1[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double X2[3], u2, v2;
        apply(rel, 2.0, X1, X2);
        if (!pixel(X2, u2, v2)) continue;
        aria_sim3_corr c{{X1[0], X1[1], X1[2]}, {X2[0], X2[1], X2[2]}, (float)(u + N(g)), (float)(v + N(g)), (float)(u2 + N(g)), (float)(v2 + N(g))};
        direct.push_back(c);
    }
    for (std::size_t i = 5; i < direct.size(); i += 5) {
        const aria_sim3_corr& o = direct[i - 1];
        for (int k = 0; k < 3; k++) direct[i].X2[k] = o.X2[k];
        direct[i].u2 = o.u2;
        direct[i].v2 = o.v2;
    }
    adapters::hip::HipSim3Aligner aligner;
    const auto d = aligner.estimate(direct);
    std::printf("estimate %d %.6f %.6f %.6f %d %.4f\n", d ? 1 : 0, d ? rot_err_deg(d->R.data(), rel.R) : 99.0,
                d ? dist(d->t.data(), rel.t) / 2.0 : 99.0, d ? std::fabs(d->s / 2.0 - 1.0) : 99.0, d ? d->n_inliers : 0, d ? d->rms_px : 0.0);
    std::vector<aria_sim3_corr> few(direct.begin(), direct.begin() + 2);
    std::printf("too_few %d\n", aligner.estimate(few) ? 1 : 0);

    // 2. the map a tracker bootstraps from two views half a unit apart (the two-view stage's |t| = 1: the map is twice the scene)
    const View v0 = yaw(0, 0, 0, 0), v1 = yaw(4, 0.5, 0.0, 0.0);
    core::Frame f[2];
    std::vector<core::Match> m01, loop;
    f[0].id = 0;
    f[1].id = 1;
    while (m01.size() < 400) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double Y[3], p[2][2];
        apply(v0, 1.0, X, Y);
        if (!pixel(Y, p[0][0], p[0][1])) continue;
        apply(v1, 1.0, X, Y);
        if (!pixel(Y, p[1][0], p[1][1])) continue;
        const int i = (int)m01.size();
        for (int k = 0; k < 2; k++) f[k].keypoints.push_back({(float)(p[k][0] + N(g)), (float)(p[k][1] + N(g)), 31.f, 0.f, 1.f, 0});
        m01.push_back({i, i, 10.f});                                          // query = the earlier frame, the reference's order
        loop.push_back({i, i, 10.f});                                         // query = keyframe 1 = frame 1, train = frame 0
    }
    for (int k = 0; k < 2; k++) f[k].descriptors.assign(f[k].keypoints.size() * 32, 0);
    adapters::hip::HipPoseEstimator two_view;
    const auto e01 = two_view.estimate(f[0], f[1], m01, true, 1);
    adapters::hip::MapTracker tracker;
    const adapters::hip::TrackStep s1 = tracker.track(f[0], f[1], m01, true, e01);
    const std::array<double, 16> T1 = tracker.pose();
    std::printf("bootstrap %d %d %d\n", (int)s1.source, s1.added, tracker.anchorPair());
    adapters::hip::KeyframeInMap k1, k0;
    k1.anchor_pair = k0.anchor_pair = tracker.anchorPair();
    k1.anchor_view = 2;
    k0.anchor_view = 1;
    for (int k = 0; k < 12; k++) k1.pose[(size_t)k] = T1[(size_t)k];           // rows of [R t]; frame 0 is the map's frame
    k1.frame = &f[1];
    k0.frame = &f[0];
    // truth: X2 = X = R1^T (X1 - t1)
    double Rt[9], tt[3], R1[9], t1[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R1[r * 3 + c] = T1[(size_t)(r * 4 + c)];
        t1[r] = T1[(size_t)(r * 4 + 3)];
    }
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rt[r * 3 + c] = R1[c * 3 + r];
        tt[r] = -(R1[r] * t1[0] + R1[3 + r] * t1[1] + R1[6 + r] * t1[2]);
    }
    int n_corr = 0;
    std::vector<int> back;
    const auto a = aligner.estimateAgainstMap(tracker.mapper().handle(), k1, k0, loop, 7, &n_corr, &back);
    const double zero[3] = {0, 0, 0};
    std::printf("against_map %d %.6f %.6f %.6f %d %d %.6f %zu\n", a ? 1 : 0, a ? rot_err_deg(a->R.data(), Rt) : 99.0,
                a ? dist(a->t.data(), tt) : 99.0, a ? std::fabs(a->s - 1.0) : 99.0, n_corr, a ? a->n_inliers : 0,
                a ? dist(a->t.data(), zero) : 0.0, back.size());

    // 3. the verifier: a candidate that carries a unit-length edge pointing elsewhere
    auto lookup = [&](std::uint64_t id) -> std::optional<adapters::hip::KeyframeInMap> {
        if (id == 1) return k1;
        if (id == 0) return k0;
        return std::nullopt;
    };
    auto candidate = [&]() {
        core::LoopCandidate c;
        c.query_id = 1;
        c.match_id = 0;
        c.matches = loop;
        adapters::hip::detail::setEntry(c.relative_pose, 2, 3, 1.0, 0);      // t = (0, 0, 1), R = I
        return c;
    };
    core::KeyFrame q;
    q.id = 1;
    q.frame = f[1];
    std::vector<adapters::hip::Sim3Report> reports;
    auto note = [&](const adapters::hip::Sim3Report& r) { reports.push_back(r); };
    {
        core::LoopCandidate c = candidate();
        const bool ok = adapters::hip::makeSim3Verifier(aligner, tracker.mapper().handle(), lookup, nullptr, 20, note)(q, 0, c);
        const adapters::hip::GraphPose T = adapters::hip::loopRelativePose(c);
        const double t[3] = {T(0, 3), T(1, 3), T(2, 3)};
        double R[9];
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) R[r * 3 + cc] = T(r, cc);
        std::printf("verifier %d %d %.6f %.6f %.6f %d %d\n", ok ? 1 : 0, reports.back().replaced ? 1 : 0, rot_err_deg(R, Rt), dist(t, tt),
                    reports.back().s, reports.back().n_corr, reports.back().n_inliers);
    }
    {   // the gate is not met: the candidate stays as it was, and is still accepted
        core::LoopCandidate c = candidate();
        const bool ok = adapters::hip::makeSim3Verifier(aligner, tracker.mapper().handle(), lookup, nullptr, 100000, note)(q, 0, c);
        const adapters::hip::GraphPose T = adapters::hip::loopRelativePose(c);
        std::printf("gate %d %d %.1f %.1f %.1f %.1f\n", ok ? 1 : 0, reports.back().replaced ? 1 : 0, T(0, 3), T(1, 3), T(2, 3), T(0, 0));
    }
    {   // an unknown keyframe: left alone; an inner verifier that rejects: rejected, no report
        core::LoopCandidate c = candidate();
        const std::size_t before = reports.size();
        const bool ok = adapters::hip::makeSim3Verifier(aligner, tracker.mapper().handle(), lookup, nullptr, 20, note)(q, 5, c);
        const adapters::hip::GraphPose T = adapters::hip::loopRelativePose(c);
        auto reject = [](const core::KeyFrame&, std::uint64_t, core::LoopCandidate&) { return false; };
        const bool inner = adapters::hip::makeSim3Verifier(aligner, tracker.mapper().handle(), lookup, reject, 20, note)(q, 0, c);
        std::printf("unknown %d %d %.1f %d %zu\n", ok ? 1 : 0, reports[before].replaced ? 1 : 0, T(2, 3), inner ? 1 : 0, reports.size() - before);
    }
    walk();
    std::printf("DONE\n");
    return 0;
}
