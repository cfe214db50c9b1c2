// Drives aria_hip/DenseTracker.hpp and HipDenseTracker.hpp on a generated 3-D scene (three mutually orthogonal planes and a
// sphere, rendered analytically): six frames along a small arc, each handed to DenseTracker with no chain delta, so the
// prediction is the previous estimate and everything the camera moved is the tracker's to find. Prints one line per frame
//   frame <k> <tracked> <lost> <valid> <n_corr> <rms> <rot error> <centre error> <prediction's centre error>
// then "final <rot error> <centre error> <total rotation> <total motion> <lost>", "refused <0|1>" and DONE. Run by
// tests/test_cpp_icp.py.
#include <array>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "aria_hip/DenseTracker.hpp"

using namespace aria::adapters::hip;

namespace {

constexpr int W = 96, H = 72;
constexpr double FX = 60.0, FY = 60.0, CX = 47.3, CY = 35.3;

struct Pose { double R[9], t[3]; };                                     // world to camera

Pose makePose(double yaw, double x, double y) {                            // camera centre (x, y, 0), turned about y
    Pose p{};
    const double c = std::cos(yaw), s = std::sin(yaw);
    const double R[9] = {c, 0, -s, 0, 1, 0, s, 0, c};
    const double o[3] = {x, y, 0};
    for (int i = 0; i < 9; i++) p.R[i] = R[i];
    for (int i = 0; i < 3; i++) p.t[i] = -(R[3 * i] * o[0] + R[3 * i + 1] * o[1] + R[3 * i + 2] * o[2]);
    return p;
}

// camera depth per pixel: the walls z = 1.7, x = -1.2, y = -1.0 and a sphere of 0.35 m at (0.3, 0.2, 1.2)
std::vector<float> render(const Pose& p) {
    std::vector<float> depth((std::size_t)W * H, 0.0f);
    double o[3];
    for (int a = 0; a < 3; a++) o[a] = -(p.R[a] * p.t[0] + p.R[3 + a] * p.t[1] + p.R[6 + a] * p.t[2]);
    const double n[3][3] = {{0, 0, -1}, {1, 0, 0}, {0, 1, 0}}, d[3] = {-1.7, -1.2, -1.0}, c[3] = {0.3, 0.2, 1.2}, rad = 0.35;
    for (int v = 0; v < H; v++)
        for (int u = 0; u < W; u++) {
            const double dc[3] = {(u - CX) / FX, (v - CY) / FY, 1.0};
            double dw[3];
            for (int a = 0; a < 3; a++) dw[a] = p.R[a] * dc[0] + p.R[3 + a] * dc[1] + p.R[6 + a] * dc[2];
            double best = 1e30;
            for (int k = 0; k < 3; k++) {
                const double den = dw[0] * n[k][0] + dw[1] * n[k][1] + dw[2] * n[k][2];
                const double num = d[k] - (o[0] * n[k][0] + o[1] * n[k][1] + o[2] * n[k][2]);
                if (den != 0 && num / den > 0 && num / den < best) best = num / den;
            }
            const double oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
            const double A = dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2], B = 2 * (dw[0] * oc[0] + dw[1] * oc[1] + dw[2] * oc[2]);
            const double C = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - rad * rad, disc = B * B - 4 * A * C;
            if (disc > 0) {
                const double s = (-B - std::sqrt(disc)) / (2 * A);
                if (s > 0 && s < best) best = s;
            }
            depth[(std::size_t)v * W + u] = best < 1e29 ? (float)best : 0.0f;
        }
    return depth;
}

// (rotation angle, distance of the camera centres) between a 4x4 row-major estimate and a true pose
void errors(const std::array<double, 16>& T, const Pose& p, double& rot, double& centre) {
    double tr = 0, ce[3], ct[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) tr += T[(std::size_t)(4 * i + j)] * p.R[3 * i + j];
    rot = std::acos(std::fmin(1.0, std::fmax(-1.0, (tr - 1) / 2)));
    for (int a = 0; a < 3; a++) {
        ce[a] = -(T[(std::size_t)a] * T[3] + T[(std::size_t)(4 + a)] * T[7] + T[(std::size_t)(8 + a)] * T[11]);
        ct[a] = -(p.R[a] * p.t[0] + p.R[3 + a] * p.t[1] + p.R[6 + a] * p.t[2]);
    }
    centre = std::sqrt((ce[0] - ct[0]) * (ce[0] - ct[0]) + (ce[1] - ct[1]) * (ce[1] - ct[1]) + (ce[2] - ct[2]) * (ce[2] - ct[2]));
}

}  // namespace

int main() {
    try {
        TsdfVolumeConfig vc;
        vc.K.fx = FX; vc.K.fy = FY; vc.K.cx = CX; vc.K.cy = CY;
        vc.nx = 64; vc.ny = 64; vc.nz = 32;
        vc.voxel = 0.05f; vc.trunc = 0.2f;
        vc.origin[0] = -1.6f; vc.origin[1] = -1.6f; vc.origin[2] = 0.4f;
        vc.min_weight = 1;                                                 // the first frame alone is a model
        DenseTracker dt(vc, DenseTrackerConfig{}, 0.3f, 3.0f);
        const int frames = 6;
        const double yaw_step = 0.02, x_step = 0.03;
        double rot = 0, centre = 0;
        for (int k = 0; k < frames; k++) {
            const Pose truth = makePose(yaw_step * k, x_step * k, 0.01 * k);
            double prot, pcentre;
            errors(dt.pose(), truth, prot, pcentre);                       // no delta: the prediction is the previous estimate
            const std::vector<float> depth = render(truth);
            const DenseTrackStep s = dt.step(depth.data(), W, H, nullptr);
            errors(dt.pose(), truth, rot, centre);
            std::printf("frame %d %d %d %d %d %.6f %.6f %.6f %.6f\n", k, (int)s.tracked, (int)s.lost, s.result.valid, s.result.n_corr,
                        s.result.rms, rot, centre, pcentre);
        }
        std::printf("final %.6f %.6f %.6f %.6f %lld\n", rot, centre, yaw_step * (frames - 1),
                    std::sqrt(x_step * x_step + 0.01 * 0.01) * (frames - 1), dt.framesLost());
        int refused = 0;
        try {
            DenseTrackerConfig bad;
            bad.dist_max = 2.0f;
            HipDenseTracker t(bad);
        } catch (const std::runtime_error&) {
            refused = 1;
        }
        std::printf("refused %d\nDONE\n", refused);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "icp_selftest: %s\n", e.what());
        return 1;
    }
    return 0;
}
