// Drives the IMapper adapter on the GPU: HipMapper::triangulate through the port (core::Pose extrinsics, K) on a synthetic
// scene with a few planted far points, then filterOutliers and exportPLY. Prints "key values..." lines that
// tests/test_gpu_map.py checks. Usage: map_selftest OUT.ply
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "aria_hip/HipMapper.hpp"

using namespace aria;

namespace {
constexpr double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375;

// view 1 = identity, view 2 = yaw 10 degrees, t = (-0.6, 0, 0.2); n points at 2-5 m plus 5 at 15-18 m (parallax above
// 1 degree, beyond 3 sigma of the map), noise-free
void scene(int n, core::Frame& a, core::Frame& b, std::vector<core::Match>& m, std::vector<std::array<double, 3>>& X,
           core::Pose& p2) {
    const double th = 10.0 * M_PI / 180.0;
    const double R[9] = {std::cos(th), 0, std::sin(th), 0, 1, 0, -std::sin(th), 0, std::cos(th)};
    const double t[3] = {-0.6, 0.0, 0.2};
    p2.orientation.w = std::cos(th / 2);
    p2.orientation.y = std::sin(th / 2);
    for (int k = 0; k < 3; k++) p2.position(k) = t[k];
    std::mt19937 g(7);
    std::uniform_real_distribution<double> U(0, 752), V(0, 480), Z(2, 5), F(15, 18);
    while ((int)m.size() < n + 5) {
        const bool far = (int)m.size() >= n;
        const double u = U(g), v = V(g), z = far ? F(g) : Z(g);
        const double P[3] = {(u - cx) / fx * z, (v - cy) / fy * z, z};
        double Y[3];
        for (int r = 0; r < 3; r++) Y[r] = R[r * 3] * P[0] + R[r * 3 + 1] * P[1] + R[r * 3 + 2] * P[2] + t[r];
        const double u2 = fx * Y[0] / Y[2] + cx, v2 = fy * Y[1] / Y[2] + cy;
        if (Y[2] < 0.5 || u2 < 0 || u2 >= 752 || v2 < 0 || v2 >= 480) continue;
        const int i = (int)a.keypoints.size();
        a.keypoints.push_back({(float)u, (float)v, 31.f, 0.f, 1.f, 0});
        b.keypoints.push_back({(float)u2, (float)v2, 31.f, 0.f, 1.f, 0});
        m.push_back({i, i, 10.f});
        X.push_back({P[0], P[1], P[2]});
    }
    a.descriptors.resize(a.keypoints.size() * 32);
    for (std::size_t k = 0; k < a.descriptors.size(); k++) a.descriptors[k] = (std::uint8_t)(k * 7 + 3);
    b.descriptors.assign(b.keypoints.size() * 32, 0);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    core::Frame a, b;
    a.id = 1;
    b.id = 2;
    std::vector<core::Match> m;
    std::vector<std::array<double, 3>> X;
    core::Pose p1, p2;
    scene(200, a, b, m, X, p2);
    core::Matrix3 K;
    K(0, 0) = fx; K(1, 1) = fy; K(0, 2) = cx; K(1, 2) = cy; K(2, 2) = 1.0;
    adapters::hip::HipMapper mapper;
    interfaces::IMapper& port = mapper;
    std::vector<core::MapPoint> pts;
    port.triangulate(a, b, p1, p2, m, K, pts);
    double worst = 0.0;
    bool desc_ok = !pts.empty();
    for (const core::MapPoint& p : pts) {
        const int i = p.observations[0].second;
        double d2 = 0, n2 = 0;
        for (int k = 0; k < 3; k++) {
            d2 += (p.position(k) - X[(std::size_t)i][(std::size_t)k]) * (p.position(k) - X[(std::size_t)i][(std::size_t)k]);
            n2 += X[(std::size_t)i][(std::size_t)k] * X[(std::size_t)i][(std::size_t)k];
        }
        worst = std::max(worst, std::sqrt(d2 / n2));
        for (int k = 0; k < 32; k++) desc_ok = desc_ok && p.descriptor.size() == 32 && p.descriptor[(std::size_t)k] == a.descriptors[(std::size_t)(i * 32 + k)];
    }
    std::printf("triangulate %zu %.3g\n", pts.size(), worst);
    if (!pts.empty())
        std::printf("observations %llu %llu %d\n", (unsigned long long)pts[0].observations[0].first,
                    (unsigned long long)pts[0].observations[1].first, pts[0].num_observations);
    std::printf("descriptor %d\n", desc_ok ? 1 : 0);
    port.triangulate(a, b, p1, p2, m, K, pts);
    std::printf("size %zu\n", port.size());
    mapper.filterOutliers();
    std::printf("filtered %zu %zu\n", port.size(), port.getMapPoints().size());
    port.exportPLY(argv[1]);
    std::ifstream f(argv[1]);
    std::string line;
    std::size_t lines = 0;
    while (std::getline(f, line)) lines++;
    std::printf("ply %zu\n", lines - 10);
    std::printf("DONE\n");
    return 0;
}
