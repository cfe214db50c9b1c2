// Drives the absolute-pose adapters on the GPU: HipPnPEstimator on a synthetic scene, and MapTracker -- the loop behind
// euroc_frontend --track-map -- on a three-frame sequence: frames 0 and 1 bootstrapped by the two-view stage at unit baseline
// and triangulated into the map, frame 2 placed by PnP against those points, whose two step lengths must have the scene's
// ratio; then the fallback and the held step. Prints "key values..." lines that tests/test_gpu_pnp.py checks.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "aria_hip/HipMapper.hpp"
#include "aria_hip/HipPnPEstimator.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
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

bool project(const View& v, const double X[3], double& u, double& w) {
    double Y[3];
    for (int r = 0; r < 3; r++) Y[r] = v.R[r * 3] * X[0] + v.R[r * 3 + 1] * X[1] + v.R[r * 3 + 2] * X[2] + v.t[r];
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

// camera centre -R^T t
void centre(const double* R, const double* t, double c[3]) {
    for (int a = 0; a < 3; a++) c[a] = -(R[a] * t[0] + R[3 + a] * t[1] + R[6 + a] * t[2]);
}
}  // namespace

int main() {
    // the scene: points at 3-12 units seen by three views; the true first baseline is 0.5, the second step 0.9 long
    const View v0 = yaw(0, 0, 0, 0), v1 = yaw(4, 0.5, 0.0, 0.0), v2 = yaw(7, 1.3, 0.1, 0.4);
    std::mt19937 g(11);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(3, 12);
    std::normal_distribution<double> N(0, 0.3);
    core::Frame f[3];
    std::vector<core::Match> m01, m12;
    std::vector<aria_pnp_corr> direct;                                        // true points against view 2, 20 % outliers
    for (int k = 0; k < 3; k++) f[k].id = (std::uint64_t)k;
    while (m01.size() < 400) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double p[3][2];
        if (!project(v0, X, p[0][0], p[0][1]) || !project(v1, X, p[1][0], p[1][1]) || !project(v2, X, p[2][0], p[2][1])) continue;
        const int i = (int)m01.size();
        for (int k = 0; k < 3; k++) f[k].keypoints.push_back({(float)(p[k][0] + N(g)), (float)(p[k][1] + N(g)), 31.f, 0.f, 1.f, 0});
        m01.push_back({i, i, 10.f});                                          // query = the earlier frame, the reference's order
        m12.push_back({i, i, 10.f});
        aria_pnp_corr c{{X[0], X[1], X[2]}, f[2].keypoints.back().x, f[2].keypoints.back().y};
        if (i % 5 == 0) { c.u = (float)U(g); c.v = (float)V(g); }
        direct.push_back(c);
    }
    for (int k = 0; k < 3; k++) f[k].descriptors.assign(f[k].keypoints.size() * 32, 0);

    adapters::hip::HipPnPEstimator pnp;
    auto d = pnp.estimate(direct);
    double dt = 99.0;
    if (d) dt = std::sqrt(std::pow(d->t[0] - v2.t[0], 2) + std::pow(d->t[1] - v2.t[1], 2) + std::pow(d->t[2] - v2.t[2], 2));
    std::printf("estimate %d %.6f %.6f %d %.4f\n", d ? 1 : 0, d ? rot_err_deg(d->R.data(), v2.R) : 99.0, dt, d ? d->n_inliers : 0,
                d ? d->rms_px : 0.0);
    std::vector<aria_pnp_corr> few(direct.begin(), direct.begin() + 5);
    std::printf("too_few %d\n", pnp.estimate(few) ? 1 : 0);

    // the track (aria_hip/MapTracker.hpp, what euroc_frontend --track-map runs): 0 -> 1 bootstrapped by the two-view stage
    // (|t| = 1) and triangulated, frame 2 placed by PnP against the pair's points, joined on the device
    adapters::hip::HipPoseEstimator two_view;
    const auto e01 = two_view.estimate(f[0], f[1], m01, true, 1), e12 = two_view.estimate(f[1], f[2], m12, true, 2);
    adapters::hip::MapTracker tracker;
    const adapters::hip::TrackStep s1 = tracker.track(f[0], f[1], m01, true, e01);
    const std::array<double, 16> T1 = tracker.pose();
    std::printf("bootstrap %d %d %d\n", (int)s1.source, s1.added, s1.n_corr);
    const adapters::hip::TrackStep s2 = tracker.track(f[1], f[2], m12, true, e12);
    const std::array<double, 16> T2 = tracker.pose();
    auto Rt = [](const std::array<double, 16>& T, double R[9], double t[3]) {
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R[r * 3 + c] = T[(size_t)(r * 4 + c)];
            t[r] = T[(size_t)(r * 4 + 3)];
        }
    };
    double R1[9], t1[3], R2[9], t2[3], c0[3] = {0, 0, 0}, c1[3], c2[3], g1[3], g2[3];
    Rt(T1, R1, t1);
    Rt(T2, R2, t2);
    centre(R1, t1, c1);
    centre(R2, t2, c2);
    centre(v1.R, v1.t, g1);
    centre(v2.R, v2.t, g2);
    auto dist = [](const double* a, const double* b) { return std::sqrt(std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2)); };
    const double ratio = dist(c2, c1) / dist(c1, c0), truth = dist(g2, g1) / dist(g1, c0);
    // the map's scale is 1 / 0.5: the placed pose in the scene's units
    const double sc = dist(g1, c0) / dist(c1, c0);
    const double t2s[3] = {t2[0] * sc, t2[1] * sc, t2[2] * sc};
    std::printf("track %d %.6f %.6f %.6f %.6f %d %d %d %.6f\n", (int)s2.source, ratio, truth, rot_err_deg(R2, v2.R), dist(t2s, v2.t), s2.n_inliers,
                s2.n_corr, s2.added, dist(c1, c0));
    std::printf("map %zu\n", tracker.mapper().size());

    // the fallback rule: the second step's matches hit no mapped keypoint, so PnP has nothing and the two-view delta is taken
    {
        std::vector<core::Match> lo(m01.begin(), m01.begin() + 200), hi(m12.begin() + 200, m12.end());
        adapters::hip::MapTracker t;
        const adapters::hip::TrackStep a = t.track(f[0], f[1], lo, true, e01);
        const adapters::hip::TrackStep b2 = t.track(f[1], f[2], hi, true, e12);
        double Rf[9], tf[3];
        Rt(t.pose(), Rf, tf);
        std::printf("fallback %d %d %d %.6f %d\n", (int)a.source, (int)b2.source, b2.n_corr, rot_err_deg(Rf, v2.R), b2.added);
    }
    {   // neither points to track against nor a two-view pose: the pose is held, nothing is triangulated
        adapters::hip::MapTracker t;
        const std::array<double, 16> held = t.pose();
        const adapters::hip::TrackStep c = t.track(f[0], f[1], m01, true, std::nullopt);
        std::printf("held %d %d %d\n", (int)c.source, c.added, held == t.pose() ? 1 : 0);
    }
    std::printf("DONE\n");
    return 0;
}
