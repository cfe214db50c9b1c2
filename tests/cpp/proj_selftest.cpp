// Drives guided matching through the C++ adapters on the GPU: HipProjectionMatcher's host form on a generated 3-D scene, and
// MapTracker's local-map mode on a seven-frame sequence of keypoint and descriptor lists (no images): the mode off equals a
// tracker that never heard of it; with frame 4 emptied the chain breaks without the mode and holds with it. Prints
// "key values..." lines that tests/test_cpp_proj.py checks.
#include <cmath>
#include <cstdio>
#include <optional>
#include <random>
#include <vector>

#include "aria_hip/HipProjectionMatcher.hpp"
#include "aria_hip/MapTracker.hpp"
#include "aria_orb_hip.h"

using namespace aria;

namespace {
const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;
const int W = 752, H = 480, FRAMES = 7, GAP = 4, POINTS = 500;

struct View {
    double R[9], t[3];
};

// the camera of frame k: a steady motion of 0.1 units and 0.3 degrees of yaw per frame
View view(int k) {
    const double th = 0.3 * k * M_PI / 180.0;
    return View{{std::cos(th), 0, std::sin(th), 0, 1, 0, -std::sin(th), 0, std::cos(th)}, {0.1 * k, 0.01 * k, 0.02 * k}};
}

bool project(const View& v, const double X[3], double& u, double& w) {
    double Y[3];
    for (int r = 0; r < 3; r++) Y[r] = v.R[r * 3] * X[0] + v.R[r * 3 + 1] * X[1] + v.R[r * 3 + 2] * X[2] + v.t[r];
    if (Y[2] < 0.5) return false;
    u = fx * Y[0] / Y[2] + cx;
    w = fy * Y[1] / Y[2] + cy;
    return u >= 8 && u < W - 8 && w >= 8 && w < H - 8;
}

void centre(const double* R, const double* t, double c[3]) {
    for (int a = 0; a < 3; a++) c[a] = -(R[a] * t[0] + R[3 + a] * t[1] + R[6 + a] * t[2]);
}

void centreOf(const std::array<double, 16>& T, double c[3]) {
    double R[9], t[3];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) R[r * 3 + k] = T[(size_t)(r * 4 + k)];
        t[r] = T[(size_t)(r * 4 + 3)];
    }
    centre(R, t, c);
}

double dist(const double* a, const double* b) { return std::sqrt(std::pow(a[0] - b[0], 2) + std::pow(a[1] - b[1], 2) + std::pow(a[2] - b[2], 2)); }

// the two-view stage's answer for a -> b, from the truth: x_b = R x_a + t with |t| = 1
adapters::hip::TwoViewPose relative(const View& a, const View& b) {
    adapters::hip::TwoViewPose p;
    double t[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double v = 0;
            for (int k = 0; k < 3; k++) v += b.R[r * 3 + k] * a.R[c * 3 + k];
            p.R[(size_t)(r * 3 + c)] = v;
        }
    for (int r = 0; r < 3; r++) t[r] = b.t[r] - (p.R[(size_t)(r * 3)] * a.t[0] + p.R[(size_t)(r * 3 + 1)] * a.t[1] + p.R[(size_t)(r * 3 + 2)] * a.t[2]);
    const double n = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int r = 0; r < 3; r++) p.t[(size_t)r] = t[r] / n;
    p.n_matches = p.n_inliers = p.n_pose_inliers = POINTS;
    return p;
}

struct Run {
    std::vector<int> source, n_corr, n_inliers;
    std::vector<std::array<double, 16>> pose;
};

// local < 0: a tracker that is never told about the mode
Run track(const core::Frame* f, const std::vector<std::vector<core::Match>>& m, const std::vector<std::optional<adapters::hip::TwoViewPose>>& e,
          int local, float radius) {
    adapters::hip::MapperConfig mc;
    mc.min_parallax_deg = 0.25;                                               // a step is 0.1 units against depths of 3 to 12,
    mc.max_depth = 200.0;                                                     // which are 30 to 120 of the map's units (the bootstrap step)
    adapters::hip::MapTracker t(mc);
    if (local >= 0) t.setLocalMap(local, radius);
    Run r;
    for (int k = 1; k < FRAMES; k++) {
        const adapters::hip::TrackStep s = t.track(f[k - 1], f[k], m[(size_t)k], true, e[(size_t)k], nullptr, W, H);
        r.source.push_back((int)s.source);
        r.n_corr.push_back(s.n_corr);
        r.n_inliers.push_back(s.n_inliers);
        r.pose.push_back(t.pose());
    }
    return r;
}
}  // namespace

int main() {
    std::mt19937 g(21);
    std::uniform_real_distribution<double> U(0, W), V(0, H), Z(3, 12);
    std::normal_distribution<double> N(0, 0.3);
    std::uniform_int_distribution<int> B(0, 255), BIT(0, 255);
    core::Frame f[FRAMES], gap[FRAMES];
    std::vector<std::vector<core::Match>> m((size_t)FRAMES), mg((size_t)FRAMES);
    std::vector<std::optional<adapters::hip::TwoViewPose>> e((size_t)FRAMES), eg((size_t)FRAMES);
    std::vector<aria_proj_landmark> truth;
    for (int k = 0; k < FRAMES; k++) f[k].id = (std::uint64_t)k;
    while ((int)truth.size() < POINTS) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double p[FRAMES][2];
        bool ok = true;
        for (int k = 0; k < FRAMES && ok; k++) ok = project(view(k), X, p[k][0], p[k][1]);
        if (!ok) continue;
        aria_proj_landmark lm{};
        for (int a = 0; a < 3; a++) lm.X[a] = X[a];
        for (int b = 0; b < 32; b++) lm.desc[b] = (std::uint8_t)B(g);
        lm.octave = 0;
        lm.source = (int)truth.size();
        truth.push_back(lm);
        for (int k = 0; k < FRAMES; k++) {
            f[k].keypoints.push_back({(float)(p[k][0] + N(g)), (float)(p[k][1] + N(g)), 31.f, 0.f, 1.f, 0});
            std::uint8_t d[32];
            for (int b = 0; b < 32; b++) d[b] = lm.desc[b];
            for (int flips = 0; flips < 4; flips++) {                         // a few bits of descriptor noise per view
                const int bit = BIT(g);
                d[bit >> 3] ^= (std::uint8_t)(1 << (bit & 7));
            }
            f[k].descriptors.insert(f[k].descriptors.end(), d, d + 32);
        }
    }
    for (int k = 1; k < FRAMES; k++) {
        for (int i = 0; i < POINTS; i++) m[(size_t)k].push_back({i, i, 10.f});   // query = the earlier frame
        e[(size_t)k] = relative(view(k - 1), view(k));
    }
    // the same sequence with frame GAP blank: no keypoints, so no matches into or out of it and no two-view pose
    for (int k = 0; k < FRAMES; k++) {
        gap[k] = f[k];
        mg[(size_t)k] = m[(size_t)k];
        eg[(size_t)k] = e[(size_t)k];
    }
    gap[GAP].keypoints.clear();
    gap[GAP].descriptors.clear();
    mg[(size_t)GAP].clear(); mg[(size_t)GAP + 1].clear();
    eg[(size_t)GAP].reset(); eg[(size_t)GAP + 1].reset();

    // the adapter's host form: the true points searched in frame 3 from frame 2's true pose
    {
        adapters::hip::HipProjectionMatcher pm;
        const View p = view(2);
        const double T[16] = {p.R[0], p.R[1], p.R[2], p.t[0], p.R[3], p.R[4], p.R[5], p.t[1], p.R[6], p.R[7], p.R[8], p.t[2], 0, 0, 0, 1};
        const adapters::hip::ProjectionMatches r = pm.search(T, f[3], truth, 0, truth.size(), W, H);
        int right = 0;
        for (const aria_proj_pair& q : r.pairs) right += q.landmark == q.keypoint;
        const adapters::hip::ProjectionMatches part = pm.search(T, f[3], truth, 100, 50, W, H);
        int part_ok = part.obs.size() == 50;
        for (const aria_proj_pair& q : part.pairs) part_ok = part_ok && q.landmark >= 100 && q.landmark < 150 && q.landmark == q.keypoint;
        std::printf("adapter %zu %zu %d %zu %d\n", r.obs.size(), r.corr.size(), right, part.corr.size(), part_ok);
    }

    const Run plain = track(f, m, e, -1, 0.f), off = track(f, m, e, 0, 15.f);
    std::printf("off_equal %d", plain.source == off.source && plain.pose == off.pose && plain.n_corr == off.n_corr ? 1 : 0);
    for (int s : plain.source) std::printf(" %d", s);
    std::printf("\n");

    // scale of the map: the bootstrap's step is one map unit, the scene's is |c1|
    double g1[3], zero[3] = {0, 0, 0};
    const View v1 = view(1);
    centre(v1.R, v1.t, g1);
    const double sc = dist(g1, zero);
    auto error = [&](const Run& r, int frame) {                              // position error of `frame` in scene units
        double c[3], gt[3];
        centreOf(r.pose[(size_t)frame - 1], c);
        for (double& x : c) x *= sc;
        const View v = view(frame);
        centre(v.R, v.t, gt);
        return dist(c, gt);
    };
    const Run broken = track(gap, mg, eg, 0, 15.f), held = track(gap, mg, eg, 4, 30.f);
    std::printf("gap_off");
    for (int s : broken.source) std::printf(" %d", s);
    std::printf("\n");
    std::printf("gap_on");
    for (int s : held.source) std::printf(" %d", s);
    std::printf("\n");
    double worst_pnp = 0.0;                                                   // today's path before the gap: frames 2 .. GAP - 1 of the mode-off run
    for (int k = 2; k < GAP; k++) worst_pnp = std::max(worst_pnp, error(broken, k));
    std::printf("errors %.6f %.6f %.6f %.6f %d %d %d\n", worst_pnp, error(held, GAP + 1), error(held, GAP + 2), error(broken, GAP + 1),
                held.n_corr[(size_t)GAP], held.n_inliers[(size_t)GAP], broken.source[1] == 2 && broken.source[2] == 2 ? 1 : 0);
    std::printf("DONE\n");
    return 0;
}
