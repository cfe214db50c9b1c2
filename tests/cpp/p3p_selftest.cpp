// Drives the absolute-pose adapters with the P3P minimal solver on the GPU: HipPnPEstimator::setSolver on a planar scene (where
// the default solver finds no pose), MapTracker with the P3P option on the three-frame sequence of pnp_selftest.cpp, and a
// third frame whose matches are restricted to the mapped points of one wall. Prints "key values..." lines that
// tests/test_gpu_p3p.py checks.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

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

void centre(const double* R, const double* t, double c[3]) {
    for (int a = 0; a < 3; a++) c[a] = -(R[a] * t[0] + R[3 + a] * t[1] + R[6 + a] * t[2]);
}

double dist(const double* a, const double* b) {
    return std::sqrt(std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2));
}

void split(const std::array<double, 16>& T, double R[9], double t[3]) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r * 3 + c] = T[(size_t)(r * 4 + c)];
        t[r] = T[(size_t)(r * 4 + 3)];
    }
}

struct Sequence {
    core::Frame f[3];
    std::vector<core::Match> m01, m12;
    std::vector<int> wall;               // the points on the wall
};

// 400 points seen by three views, 0.3 px of noise; wall_share of them on the plane z = 6 / (1 - 0.3 x - 0.2 y) (x, y the
// normalised pixel of view 0: pnp_ref.synth_pnp's plane), the others at 3-12 units
Sequence make_sequence(unsigned seed, const View* v, double wall_share) {
    Sequence s;
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(3, 12), S(0, 1);
    std::normal_distribution<double> N(0, 0.3);
    for (int k = 0; k < 3; k++) s.f[k].id = (std::uint64_t)k;
    while (s.m01.size() < 400) {
        const double u = U(g), w = V(g);
        double z = Z(g);
        const bool on_wall = S(g) < wall_share;
        const double xn = (u - cx) / fx, yn = (w - cy) / fy;
        if (on_wall) z = 6.0 / (1.0 - 0.3 * xn - 0.2 * yn);
        const double X[3] = {xn * z, yn * z, z};
        double p[3][2];
        if (!project(v[0], X, p[0][0], p[0][1]) || !project(v[1], X, p[1][0], p[1][1]) || !project(v[2], X, p[2][0], p[2][1])) continue;
        const int i = (int)s.m01.size();
        for (int k = 0; k < 3; k++) s.f[k].keypoints.push_back({(float)(p[k][0] + N(g)), (float)(p[k][1] + N(g)), 31.f, 0.f, 1.f, 0});
        s.m01.push_back({i, i, 10.f});
        s.m12.push_back({i, i, 10.f});
        if (on_wall) s.wall.push_back(i);
    }
    for (int k = 0; k < 3; k++) s.f[k].descriptors.assign(s.f[k].keypoints.size() * 32, 0);
    return s;
}

// bootstrap on frames 0 -> 1, then frame 2 against `m12`: prints "<key> source ratio truth rot_err t_err n_inliers n_corr first_step"
void track(const char* key, int solver, const Sequence& s, const std::vector<core::Match>& m12, const View* v,
           const std::optional<adapters::hip::TwoViewPose>& e01, const std::optional<adapters::hip::TwoViewPose>& e12) {
    adapters::hip::MapTracker tracker(adapters::hip::MapperConfig{}, 10, 1024, solver);
    const adapters::hip::TrackStep s1 = tracker.track(s.f[0], s.f[1], s.m01, true, e01);
    const std::array<double, 16> T1 = tracker.pose();
    const adapters::hip::TrackStep s2 = tracker.track(s.f[1], s.f[2], m12, true, e12);
    double R1[9], t1[3], R2[9], t2[3], c0[3] = {0, 0, 0}, c1[3], c2[3], g1[3], g2[3];
    split(T1, R1, t1);
    split(tracker.pose(), R2, t2);
    centre(R1, t1, c1);
    centre(R2, t2, c2);
    centre(v[1].R, v[1].t, g1);
    centre(v[2].R, v[2].t, g2);
    const double ratio = dist(c2, c1) / dist(c1, c0), truth = dist(g2, g1) / dist(g1, c0);
    const double sc = dist(g1, c0) / dist(c1, c0);
    const double t2s[3] = {t2[0] * sc, t2[1] * sc, t2[2] * sc};
    std::printf("%s %d %.6f %.6f %.6f %.6f %d %d %.6f %d\n", key, (int)s2.source, ratio, truth, rot_err_deg(R2, v[2].R), dist(t2s, v[2].t),
                s2.n_inliers, s2.n_corr, dist(c1, c0), (int)s1.source);
}
}  // namespace

int main() {
    // a planar scene (pnp_ref.synth_pnp's plane) seen by view 2, 400 correspondences at 0.3 px, every fifth an outlier
    const View v[3] = {yaw(0, 0, 0, 0), yaw(4, 0.5, 0.0, 0.0), yaw(7, 1.3, 0.1, 0.4)};
    {
        std::mt19937 g(12);
        std::uniform_real_distribution<double> U(0, 752), V(0, 480);
        std::normal_distribution<double> N(0, 0.3);
        std::vector<aria_pnp_corr> planar;
        while (planar.size() < 400) {
            const double u = U(g), w = V(g), xn = (u - cx) / fx, yn = (w - cy) / fy, z = 6.0 / (1.0 - 0.3 * xn - 0.2 * yn);
            const double X[3] = {xn * z, yn * z, z};
            double pu, pw;
            if (!project(v[2], X, pu, pw)) continue;
            aria_pnp_corr c{{X[0], X[1], X[2]}, (float)(pu + N(g)), (float)(pw + N(g))};
            if (planar.size() % 5 == 0) { c.u = (float)U(g); c.v = (float)V(g); }
            planar.push_back(c);
        }
        adapters::hip::HipPnPEstimator pnp;
        const auto dlt = pnp.estimate(planar);
        pnp.setSolver(ARIA_PNP_SOLVER_P3P);
        const auto d = pnp.estimate(planar);
        double dt = 99.0;
        if (d) dt = dist(d->t.data(), v[2].t);
        std::printf("planar %d %.6f %.6f %d %.4f %d %d\n", d ? 1 : 0, d ? rot_err_deg(d->R.data(), v[2].R) : 99.0, dt, d ? d->n_inliers : 0,
                    d ? d->rms_px : 0.0, dlt ? 1 : 0, pnp.solver());
        std::vector<aria_pnp_corr> four(planar.begin() + 1, planar.begin() + 5), three(planar.begin() + 1, planar.begin() + 4);
        std::printf("few %d %d\n", pnp.estimate(four) ? 1 : 0, pnp.estimate(three) ? 1 : 0);
        bool refused = false;
        try {
            pnp.setSolver(7);
        } catch (const std::exception&) {
            refused = true;
        }
        std::printf("unknown %d %d\n", refused ? 1 : 0, pnp.solver());
    }
    adapters::hip::HipPoseEstimator two_view;
    {   // the three-frame 3-D sequence of pnp_selftest.cpp (its generator and seed), tracked with the P3P option
        const Sequence s = make_sequence(11, v, 0.0);
        const auto e01 = two_view.estimate(s.f[0], s.f[1], s.m01, true, 1), e12 = two_view.estimate(s.f[1], s.f[2], s.m12, true, 2);
        track("track", ARIA_PNP_SOLVER_P3P, s, s.m12, v, e01, e12);
    }
    {   // a scene with a wall: the third frame's matches are restricted to the mapped points on it; no two-view pose is
        // offered for that step, so the frame is placed by PnP or held
        const Sequence s = make_sequence(13, v, 0.5);
        const auto e01 = two_view.estimate(s.f[0], s.f[1], s.m01, true, 1);
        std::vector<core::Match> wall;
        for (int i : s.wall) wall.push_back(s.m12[(size_t)i]);
        std::printf("wall_points %zu\n", wall.size());
        track("wall_p3p", ARIA_PNP_SOLVER_P3P, s, wall, v, e01, std::nullopt);
        track("wall_dlt", ARIA_PNP_SOLVER_DLT6, s, wall, v, e01, std::nullopt);
    }
    std::printf("DONE\n");
    return 0;
}
