// Drives the two-view pose adapters on the GPU: HipPoseEstimator on a synthetic scene, the geometric verifier through
// HipLoopDetector, and FrontEnd with estimate_pose. Prints "key values..." lines that tests/test_gpu_pose.py checks.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "aria_hip/FrontEnd.hpp"
#include "aria_hip/HipFactory.hpp"
#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPoseEstimator.hpp"
#include "aria_orb_hip.h"

using namespace aria;

namespace {
// yaw of 10 degrees and a unit baseline; points at 2-20 m seen by both cameras (EuRoC cam0 intrinsics), sigma 0.5 px
void scene(int n, std::uint32_t seed, core::Frame& a, core::Frame& b, std::vector<core::Match>& m, double R[9], double t[3]) {
    const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375, th = 10.0 * M_PI / 180.0;
    const double Rv[9] = {std::cos(th), 0, std::sin(th), 0, 1, 0, -std::sin(th), 0, std::cos(th)};
    const double tv[3] = {0.6, 0.0, 0.8};
    for (int k = 0; k < 9; k++) R[k] = Rv[k];
    for (int k = 0; k < 3; k++) t[k] = tv[k];
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(2, 20);
    std::normal_distribution<double> N(0, 0.5);
    while ((int)m.size() < n) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double Y[3];
        for (int r = 0; r < 3; r++) Y[r] = Rv[r * 3] * X[0] + Rv[r * 3 + 1] * X[1] + Rv[r * 3 + 2] * X[2] + tv[r];
        if (Y[2] < 0.5) continue;
        const double u2 = fx * Y[0] / Y[2] + cx, v2 = fy * Y[1] / Y[2] + cy;
        if (u2 < 0 || u2 >= 752 || v2 < 0 || v2 >= 480) continue;
        const int i = (int)a.keypoints.size();
        a.keypoints.push_back({(float)(u + N(g)), (float)(v + N(g)), 31.f, 0.f, 1.f, 0});
        b.keypoints.push_back({(float)(u2 + N(g)), (float)(v2 + N(g)), 31.f, 0.f, 1.f, 0});
        m.push_back({i, i, 10.f});
    }
    a.descriptors.assign(a.keypoints.size() * 32, 0);
    b.descriptors.assign(b.keypoints.size() * 32, 0);
}

double rot_err_deg(const double* A, const double* B) {
    double tr = 0;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) tr += A[k * 3 + r] * B[k * 3 + r];
    return std::acos(std::max(-1.0, std::min(1.0, (tr - 1) / 2))) * 180.0 / M_PI;
}
}  // namespace

int main() {
    core::Frame a, b;
    std::vector<core::Match> m;
    double R[9], t[3];
    scene(300, 5, a, b, m, R, t);
    adapters::hip::HipPoseEstimator est;
    auto p = est.estimate(a, b, m);
    std::printf("estimate %d %.6f %d\n", p ? 1 : 0, p ? rot_err_deg(p->R.data(), R) : 99.0, p ? p->n_pose_inliers : 0);

    // verifier through the loop detector: keyframe 0 = a, query keyframe 100 = a again with b's keypoints (the matches of
    // the detector are ratio-test matches of identical descriptors -- i -> i -- so the scene's correspondences come back)
    std::vector<std::uint8_t> desc(m.size() * 32);
    std::mt19937 g(7);
    for (auto& x : desc) x = (std::uint8_t)g();
    core::KeyFrame k0, kq;
    k0.id = 0; k0.frame = b; k0.frame.descriptors = desc;
    kq.id = 100; kq.frame = a; kq.frame.descriptors = desc;
    auto lookup = [&](std::uint64_t id) -> const core::Frame* { return id == 0 ? &k0.frame : nullptr; };
    for (int pass = 0; pass < 2; pass++) {
        adapters::hip::HipLoopDetector ld(1, 0.3, 30, 512, 10);
        ld.addKeyFrame(k0);
        ld.setVerifier(adapters::hip::makeGeometricVerifier(est, pass == 0 ? 100000 : 30, lookup));
        auto c = ld.detect(kq);
        if (pass == 0) {
            std::printf("verifier_reject %d\n", c ? 1 : 0);
        } else {
            double Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            if (c)
                for (int r = 0; r < 3; r++)
                    for (int k = 0; k < 3; k++) Rl[r * 3 + k] = c->relative_pose[k * 4 + r];   // column-major, as Eigen stores it
            auto p2 = est.estimate(a, b, m);
            std::printf("verifier_accept %d %zu %d %.6f\n", c ? 1 : 0, c ? c->matches.size() : 0, p2 ? p2->n_pose_inliers : -1,
                        c ? rot_err_deg(Rl, R) : 99.0);
        }
    }

    // FrontEnd with estimate_pose: two synthetic frames (a 2-D shift: degenerate for E, so only presence is checked)
    std::vector<std::uint8_t> fa(640 * 480), fb(640 * 480);
    aria_synth_frame_pair(1, 640, 480, fa.data(), fb.data());
    int have[2] = {0, 0}, off_default = 0;
    {
        factory::HipFactoryConfig fc;
        fc.frontend.estimate_pose = true;
        fc.frontend.legacy_order = true;
        auto fe = factory::createHip(fc);
        have[0] = fe->processFrame(fa.data(), 640, 480, 0.0).pose.has_value() ? 1 : 0;
        const auto& r1 = fe->processFrame(fb.data(), 640, 480, 0.05);
        // the same as the estimator called directly on previous -> current (legacy order: query = previous, pair id = frame id)
        auto d = est.estimate(*r1.previous, *r1.frame, r1.matches, true, 1);
        const bool same = r1.matches.size() >= 8 && r1.pose.has_value() == d.has_value() &&
                          (!d || (r1.pose->R == d->R && r1.pose->t == d->t && r1.pose->n_pose_inliers == d->n_pose_inliers));
        have[1] = same ? 1 : 0;
    }
    {
        factory::HipFactoryConfig fc;
        auto fe = factory::createHip(fc);
        fe->processFrame(fa.data(), 640, 480, 0.0);
        off_default = fe->processFrame(fb.data(), 640, 480, 0.05).pose.has_value() ? 1 : 0;
    }
    std::printf("frontend %d %d %d\n", have[1], 1 - have[0], off_default);
    std::printf("DONE\n");
    return 0;
}
