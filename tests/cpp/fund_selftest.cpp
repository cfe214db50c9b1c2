// Drives the reference loop verifier on the GPU through HipLoopDetector: a revisit with the scene's geometry and one whose
// keypoints are shuffled against their descriptors (a long ratio-0.7 list, random geometry). Prints "key values..." lines
// that tests/test_gpu_fund.py checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "aria_hip/HipFundamentalEstimator.hpp"
#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPoseEstimator.hpp"

using namespace aria;

namespace {
// computeRelativePose's camera (700 / 700 / 320 / 180) at 640x360; yaw of 10 degrees and a unit baseline; points at 2-20 m
// seen by both cameras, sigma 0.5 px
void scene(int n, std::uint32_t seed, core::Frame& a, core::Frame& b, std::vector<core::Match>& m, double R[9]) {
    const double fx = 700, fy = 700, cx = 320, cy = 180, th = 10.0 * M_PI / 180.0;
    const double Rv[9] = {std::cos(th), 0, std::sin(th), 0, 1, 0, -std::sin(th), 0, std::cos(th)};
    const double tv[3] = {0.6, 0.0, 0.8};
    for (int k = 0; k < 9; k++) R[k] = Rv[k];
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> U(0, 640), V(0, 360), Z(2, 20);
    std::normal_distribution<double> N(0, 0.5);
    while ((int)m.size() < n) {
        const double u = U(g), v = V(g), z = Z(g);
        const double X[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double Y[3];
        for (int r = 0; r < 3; r++) Y[r] = Rv[r * 3] * X[0] + Rv[r * 3 + 1] * X[1] + Rv[r * 3 + 2] * X[2] + tv[r];
        if (Y[2] < 0.5) continue;
        const double u2 = fx * Y[0] / Y[2] + cx, v2 = fy * Y[1] / Y[2] + cy;
        if (u2 < 0 || u2 >= 640 || v2 < 0 || v2 >= 360) continue;
        const int i = (int)a.keypoints.size();
        a.keypoints.push_back({(float)(u + N(g)), (float)(v + N(g)), 31.f, 0.f, 1.f, 0});
        b.keypoints.push_back({(float)(u2 + N(g)), (float)(v2 + N(g)), 31.f, 0.f, 1.f, 0});
        m.push_back({i, i, 10.f});
    }
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
    double R[9];
    scene(300, 5, a, b, m, R);
    // keyframe 0 = b (the revisited place), query keyframe 100 = a; identical descriptors i -> i, so the detector's
    // ratio-0.7 list is the scene's correspondences. The shuffled keyframe carries b's keypoints in a random order.
    std::vector<std::uint8_t> desc(m.size() * 32);
    std::mt19937 g(7);
    for (auto& x : desc) x = (std::uint8_t)g();
    core::KeyFrame k0, ks, kq;
    k0.id = 0; k0.frame = b; k0.frame.descriptors = desc;
    ks.id = 0; ks.frame = b; ks.frame.descriptors = desc;
    std::shuffle(ks.frame.keypoints.begin(), ks.frame.keypoints.end(), g);
    kq.id = 100; kq.frame = a; kq.frame.descriptors = desc;
    adapters::hip::HipFundamentalEstimator fund;
    adapters::hip::HipPoseEstimator pose(adapters::hip::referenceLoopIntrinsics());
    int threw = 0;
    try {
        adapters::hip::makeReferenceVerifier(fund, pose, 14, nullptr);
    } catch (const std::invalid_argument&) {
        threw = 1;
    }
    std::printf("min_matches_guard %d\n", threw);
    for (int pass = 0; pass < 3; pass++) {
        const core::KeyFrame& db = pass == 2 ? k0 : ks;
        auto lookup = [&](std::uint64_t id) -> const core::Frame* { return id == 0 ? &db.frame : nullptr; };
        adapters::hip::HipLoopDetector ld(1, 0.3, 30, 512, 10);
        ld.addKeyFrame(db);
        if (pass > 0) ld.setVerifier(adapters::hip::makeReferenceVerifier(fund, pose, 30, lookup));
        auto c = ld.detect(kq);
        if (pass == 0) std::printf("default_shuffled %d %zu\n", c ? 1 : 0, c ? c->matches.size() : 0);
        if (pass == 1) std::printf("reference_shuffled %d\n", c ? 1 : 0);
        if (pass == 2) {
            // the F inliers of the same call, directly
            auto f = fund.estimate(kq.frame, k0.frame, m, true, 0);
            std::size_t same = 0, n_in = 0;
            if (f && c) {
                std::vector<core::Match> inl;
                for (std::size_t i = 0; i < m.size(); i++)
                    if (f->mask[i]) inl.push_back(m[i]);
                n_in = inl.size();
                same = inl.size() == c->matches.size() &&
                       std::equal(inl.begin(), inl.end(), c->matches.begin(), [](const core::Match& x, const core::Match& y) {
                           return x.query_idx == y.query_idx && x.train_idx == y.train_idx;   // distances: the detector's
                       });
            }
            double Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            if (c)
                for (int r = 0; r < 3; r++)
                    for (int k = 0; k < 3; k++) Rl[r * 3 + k] = c->relative_pose[k * 4 + r];   // column-major, as Eigen stores it
            std::printf("reference_true %d %zu %zu %d %.6f\n", c ? 1 : 0, c ? c->matches.size() : 0, n_in, (int)same,
                        c ? rot_err_deg(Rl, R) : 99.0);
        }
    }
    std::printf("DONE\n");
    return 0;
}
