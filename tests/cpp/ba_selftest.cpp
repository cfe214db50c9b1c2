// Drives the bundle-adjustment adapters on the GPU: MapTracker -- the loop behind euroc_frontend --track-map -- over a
// six-frame synthetic 3-D scene with a WindowBuilder attached, then HipBundleAdjuster on the window of all six frames with the
// first two poses fixed, and on two overlapping windows of four frames whose first seeds the second. Prints "key values..."
// lines that tests/test_cpp_ba.py checks.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "aria_hip/HipBundleAdjuster.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_hip/MapTracker.hpp"
#include "aria_orb_hip.h"

using namespace aria;

namespace {
const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;
const int F = 6;

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

// camera centre -R^T t of the 12 doubles [R t]
void centre(const double* P, double c[3]) {
    for (int a = 0; a < 3; a++) c[a] = -(P[a] * P[3] + P[4 + a] * P[7] + P[8 + a] * P[11]);
}

double dist(const double* a, const double* b) {
    return std::sqrt(std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2));
}
}  // namespace

int main() {
    // the scene: points at 3-12 units seen by six views 0.5 apart with a little yaw; pixel noise 0.3
    View v[F];
    for (int k = 0; k < F; k++) v[k] = yaw(1.5 * k, 0.5 * k, 0.02 * (k % 2), 0.05 * k);
    std::mt19937 g(17);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(3, 12);
    std::normal_distribution<double> N(0, 0.3);
    core::Frame f[F];
    for (int k = 0; k < F; k++) f[k].id = (std::uint64_t)k;
    std::vector<core::Match> m;                                   // the same list for every step: keypoint i is point i in every frame
    while (m.size() < 400) {
        const double u = U(g), w = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (w - cy) / fy * z, z};
        double p[F][2];
        bool seen = true;
        for (int k = 0; k < F && seen; k++) seen = project(v[k], X, p[k][0], p[k][1]);
        if (!seen) continue;
        const int i = (int)m.size();
        for (int k = 0; k < F; k++) f[k].keypoints.push_back({(float)(p[k][0] + N(g)), (float)(p[k][1] + N(g)), 31.f, 0.f, 1.f, 0});
        m.push_back({i, i, 10.f});
    }
    for (int k = 0; k < F; k++) f[k].descriptors.assign(f[k].keypoints.size() * 32, 0);
    std::vector<core::Match> cut(m.begin(), m.begin() + 300);     // step 3 loses a quarter of the tracks

    adapters::hip::HipPoseEstimator two_view;
    adapters::hip::MapTracker tracker;
    adapters::hip::WindowBuilder builder;
    tracker.setWindowBuilder(&builder);
    int pnp_steps = 0;
    for (int k = 1; k < F; k++) {
        const std::vector<core::Match>& mk = k == 3 ? cut : m;
        const auto e = two_view.estimate(f[k - 1], f[k], mk, true, k);
        const adapters::hip::TrackStep s = tracker.track(f[k - 1], f[k], mk, true, e);
        pnp_steps += s.source == adapters::hip::TrackStep::PNP;
        std::printf("step %d %d %d %d\n", k, (int)s.source, s.n_inliers, s.added);
    }
    std::printf("builder %d %zu %d\n", builder.frames(), builder.tracks(), pnp_steps);

    // the map's unit is the first step's length
    double c0[3], c1[3], g0[3] = {0, 0, 0}, g1[3];
    centre(builder.pose(0).data(), c0);
    centre(builder.pose(1).data(), c1);
    double P1[12];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) P1[4 * r + c] = v[1].R[3 * r + c];  P1[4 * r + 3] = v[1].t[r]; }
    centre(P1, g1);
    const double sc = dist(c1, c0) / dist(g1, g0);
    auto pose_error = [&](const std::vector<double>& poses, int first) {   // mean centre error of the window's free frames
        double sum = 0;
        int n = 0;
        for (int k = 2; k * 12 < (int)poses.size(); k++, n++) {
            double Pk[12], gk[3], ck[3];
            const View& t = v[first + k];
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Pk[4 * r + c] = t.R[3 * r + c];  Pk[4 * r + 3] = t.t[r]; }
            centre(Pk, gk);
            for (int a = 0; a < 3; a++) gk[a] *= sc;
            centre(poses.data() + 12 * k, ck);
            sum += dist(ck, gk);
        }
        return n ? sum / n : 0.0;
    };

    adapters::hip::HipBundleAdjuster ba;
    adapters::hip::BundleWindow w = builder.window(0, F);
    std::vector<int> views((std::size_t)w.nPoints(), 0);
    bool sorted = true;
    for (std::size_t o = 0; o < w.obs.size(); o++) {
        views[(std::size_t)w.obs[o].point]++;
        if (o && !(w.obs[o - 1].point < w.obs[o].point || (w.obs[o - 1].point == w.obs[o].point && w.obs[o - 1].pose < w.obs[o].pose)))
            sorted = false;
    }
    int full = 0, two = 0;
    for (int n : views) { full += n == F;  two += n == 2; }
    std::printf("window %d %d %zu %d %d %d\n", w.nPoses(), w.nPoints(), w.obs.size(), full, two, sorted ? 1 : 0);
    const double before = pose_error(w.poses, 0);
    const std::vector<double> fixed_before(w.poses.begin(), w.poses.begin() + 24);
    const adapters::hip::BundleResult r = ba.optimize(w, 10);
    const bool fixed_same = std::equal(fixed_before.begin(), fixed_before.end(), w.poses.begin());
    std::printf("adjust %d %d %.6f %.6f %.6f %d %d %.6f %.6f %d\n", r.record.valid, r.record.stop_reason, r.record.chi2_initial,
                r.record.chi2_final, r.record.rms_px, r.record.iterations_done, r.record.n_obs_used, before, pose_error(w.poses, 0),
                fixed_same ? 1 : 0);

    // sliding windows of four frames with stride two: the first window's refined poses and points seed the second
    adapters::hip::BundleWindow a = builder.window(0, 4);
    const adapters::hip::BundleResult ra = ba.optimize(a, 10);
    builder.store(a);
    adapters::hip::BundleWindow b = builder.window(2, 4);
    const bool seeded = std::equal(a.poses.begin() + 24, a.poses.end(), b.poses.begin());
    const adapters::hip::BundleResult rb = ba.optimize(b, 10);
    builder.store(b);
    std::printf("slide %d %d %.6f %.6f %.6f %.6f %d %d %d\n", ra.record.valid, rb.record.valid, ra.record.chi2_initial,
                ra.record.chi2_final, rb.record.chi2_initial, rb.record.chi2_final, a.nPoints(), b.nPoints(), seeded ? 1 : 0);

    // an invalid window is refused
    adapters::hip::BundleWindow bad = builder.window(0, 3);
    bad.obs[1].pose = 7;
    int threw = 0;
    try {
        ba.optimize(bad, 2);
    } catch (const std::exception&) {
        threw = 1;
    }
    std::printf("invalid %d\n", threw);
    std::printf("DONE\n");
    return 0;
}
