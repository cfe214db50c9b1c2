// Absolute pose from 3D-2D correspondences on the device: PnP RANSAC (6-point DLT or P3P minimal solver, fp32 reprojection scoring,
// Gauss-Newton refinement over the winner's inliers), batched over pairs, and the join of a match list with the point map
// that feeds it. Semantics in include/aria_orb_hip.h ("absolute pose from the point map"); aria_slam_amd/pnp_ref.py restates
// every step in NumPy and is the definition.
//
// Four launches on the handle's stream:
//   k_pnp_stage   one workgroup per pair: the count check BEFORE any correspondence is read, then the scoring values --
//                 d = X - X0 and the normalised pixel in fp32, (dx, dy, dz, x) as one float4 and y beside it
//   k_pnp_hyp     16 lanes per hypothesis, one row of the 11x12 fp64 system per lane (a lane per hypothesis would hold the
//                 system in 264 VGPRs): the pivot search and the pivot-row broadcast are cross-lane moves inside the 16-lane
//                 row, the back substitution broadcasts one unknown per step; then every lane of the row holds P and lane
//                 0 writes (R, t0) in fp32 or "invalid". No scratch (tests/test_pnp_host.py)
//   k_pnp_hyp_p3p the other solver (aria_pnp_set_solver), in k_pnp_hyp's place: a lane per hypothesis, 256 hypotheses of one
//                 pair per workgroup -- the three-point system is a few dozen live fp64 values, all 3x3 code is written out
//                 with constant indices, "the largest of three" and "the best of four" are selects. No LDS, no scratch
//                 (tests/test_p3p_host.py)
//   k_pnp_score   one lane per hypothesis, the pair's points staged in LDS tiles (20 B per point) and read as a broadcast:
//                 inlier count per hypothesis (the hot loop: 27 fp32 ops per evaluation, no scratch)
//   k_pnp_finish  one workgroup per pair: argmax over (count, -h), Gauss-Newton on the winner's inliers (21 + 6 sums in
//                 fp64, strided per-thread sums + fixed butterfly, 6x6 Cholesky in one lane), rescoring, mask, rms_px
// The association is two launches: a scatter over the arena (integer atomicMin of the arena position into an
// n_pairs x kp_stride table) and a lane per match with the wave-ordered compaction of ransac_device.h.
// No float atomics anywhere: counts are integers, every floating-point sum has a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "ransac_device.h"
#include "solver_device.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int PNP_TILE = 2048;             // points per LDS tile of k_pnp_score (32 KB + 8 KB)
constexpr int PNP_SCORE_BLOCK = 256;
constexpr int PNP_FINISH_BLOCK = 256;
constexpr int PNP_HYP_BLOCK = 256;         // 16 hypotheses of one pair
constexpr int PNP_ROW = 16;                // lanes per hypothesis in k_pnp_hyp
constexpr int PNP_MAX_RETRY = 256;
constexpr int PNP_MIN = 6;                 // correspondences of a DLT sample, and the least a refinement needs
constexpr int PNP_MIN_P3P = 4;             // correspondences of a P3P sample: three for the solver, one to pick its root
constexpr int PNP_P3P_BLOCK = 256;         // hypotheses of one pair per workgroup of k_pnp_hyp_p3p
constexpr double P3P_AREA_TOL = 1e-12;     // |(X1 - X2) x (X1 - X3)|^2 <= tol * max(a_ij)^2: collinear or coincident sample
constexpr int P3P_CUBIC_STEPS = 30;
constexpr int P3P_POLISH_STEPS = 5;
constexpr double PNP_PIVOT_TOL = 1e-9;     // |pivot| <= tol * max|A_ij|: degenerate sample
constexpr double PNP_RANK_TOL = 1e-9;      // sigma3 <= tol * sigma1: M is no scaled rotation
constexpr double PNP_RANGE = 1e15;         // scoring values and |t0| beyond this never score (header, "Points")
constexpr double PNP_STEP_TOL = 1e-12;
constexpr int PNP_EMPTY = 0x7F7F7F7F;      // association table: no map point (the fill byte 0x7F)
constexpr int ERRBIT_PNP_INPUT = 1;        // a pair's counts or match indices were out of range (pair skipped)

// The reprojection test, division-free, every sum left to right: Xc = R d + t0; z > 0 and
// (Xc.x - x z)^2 + (Xc.y - y z)^2 <= thr2 z^2. a = (dx, dy, dz, x).
__device__ __forceinline__ int pnp_inlier(const float r[9], const float t[3], float4 a, float y, float thr2) {
    const float X = ((r[0] * a.x + r[1] * a.y) + r[2] * a.z) + t[0];
    const float Y = ((r[3] * a.x + r[4] * a.y) + r[5] * a.z) + t[1];
    const float Z = ((r[6] * a.x + r[7] * a.y) + r[8] * a.z) + t[2];
    const float ex = X - a.w * Z, ey = Y - y * Z;
    return (Z > 0.0f && ex * ex + ey * ey <= thr2 * (Z * Z)) ? 1 : 0;
}

// R = U V^T of M = U S V^T (row-major), sig = the singular values, descending: V from the eigenvectors of M^T M,
// u_i = M v_i / sigma_i, third columns as cross products. False when sigma3 <= PNP_RANK_TOL * sigma1.
__device__ __forceinline__ bool pnp_rotation(const double M[9], double R[9], double sig[3]) {
    double G[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) G[r * 3 + c] = M[r] * M[c] + M[3 + r] * M[3 + c] + M[6 + r] * M[6 + c];
    jacobi3(G, V);
    double l0 = G[0], l1 = G[4], l2 = G[8];
    double a0 = V[0], a1 = V[3], a2 = V[6];   // columns as (x, y, z)
    double b0 = V[1], b1 = V[4], b2 = V[7];
    double c0 = V[2], c1 = V[5], c2 = V[8];
    bool s = l1 > l0;
    swap_if(s, l0, l1); swap_if(s, a0, b0); swap_if(s, a1, b1); swap_if(s, a2, b2);
    s = l2 > l1;
    swap_if(s, l1, l2); swap_if(s, b0, c0); swap_if(s, b1, c1); swap_if(s, b2, c2);
    s = l1 > l0;
    swap_if(s, l0, l1); swap_if(s, a0, b0); swap_if(s, a1, b1); swap_if(s, a2, b2);
    sig[0] = sqrt(fmax(l0, 0.0));
    sig[1] = sqrt(fmax(l1, 0.0));
    sig[2] = sqrt(fmax(l2, 0.0));
    if (!(sig[2] > PNP_RANK_TOL * sig[0])) return false;
    const double v1[3] = {a0, a1, a2}, v2[3] = {b0, b1, b2};
    double u1[3], u2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        u1[r] = (M[3 * r] * v1[0] + M[3 * r + 1] * v1[1] + M[3 * r + 2] * v1[2]) / sig[0];
        u2[r] = (M[3 * r] * v2[0] + M[3 * r + 1] * v2[1] + M[3 * r + 2] * v2[2]) / sig[1];
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r * 3 + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
    return true;
}

__device__ __forceinline__ bool finite9(const double* v, int n) {
    bool ok = true;
    for (int k = 0; k < n; k++) ok &= isfinite(v[k]);
    return ok;
}

// The hand-over of both hypothesis kernels, component k: t0[k] = (R X0)[k] + t; false when t is not finite or |t0[k]| is
// beyond PNP_RANGE. The caller adds finite9(R, 9).
__device__ __forceinline__ bool pnp_hand_over(const double R[9], double t, const double X0[3], int k, double t0[3]) {
    t0[k] = ((R[3 * k] * X0[0] + R[3 * k + 1] * X0[1]) + R[3 * k + 2] * X0[2]) + t;
    return isfinite(t) && fabs(t0[k]) <= PNP_RANGE;
}

// (R, t0) in fp32, structure-of-arrays per pair: Ps[(p * 12 + k) * H + h], k = 0..8 R, 9..11 t0; cnt[p * H + h] = 0 (valid,
// to be scored) or -1.
__device__ __forceinline__ void pnp_store_model(float* Ps, int* cnt, int p, int H, int h, bool ok,
                                                const double R[9], const double t0[3]) {
    float* Pp = Ps + (int64_t)p * 12 * H;
#pragma unroll
    for (int k = 0; k < 9; k++) Pp[(int64_t)k * H + h] = ok ? (float)R[k] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) Pp[(int64_t)(9 + k) * H + h] = ok ? (float)t0[k] : 0.0f;
    cnt[(int64_t)p * H + h] = ok ? 0 : -1;
}

// ---- stage: count check, normalisation, centring on X0 ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pnp_stage(const aria_pnp_corr* __restrict__ corr, const int* __restrict__ ncorr,
                                                   int corr_cap, double fx, double fy, double cx, double cy,
                                                   float4* __restrict__ pa, float* __restrict__ pb, int* __restrict__ npts,
                                                   int* __restrict__ err) {
    const int p = blockIdx.x;
    const int n = ncorr[p];
    if (n < 0 || n > corr_cap) {             // uniform over the workgroup
        if (threadIdx.x == 0) {
            npts[p] = 0;
            atomicOr(err, ERRBIT_PNP_INPUT);
        }
        return;
    }
    if (threadIdx.x == 0) npts[p] = n;
    if (n == 0) return;
    const aria_pnp_corr* cp = corr + (int64_t)p * corr_cap;
    const double X0 = cp[0].X[0], Y0 = cp[0].X[1], Z0 = cp[0].X[2];
    float4* oa = pa + (int64_t)p * corr_cap;
    float* ob = pb + (int64_t)p * corr_cap;
    const float lim = (float)PNP_RANGE;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const aria_pnp_corr c = cp[i];
        float4 a = make_float4((float)(c.X[0] - X0), (float)(c.X[1] - Y0), (float)(c.X[2] - Z0),
                               (float)(((double)c.u - cx) / fx));
        float y = (float)(((double)c.v - cy) / fy);
        const bool ok = fabsf(a.x) <= lim && fabsf(a.y) <= lim && fabsf(a.z) <= lim && fabsf(a.w) <= lim && fabsf(y) <= lim;
        if (!ok) {
            const float q = __builtin_nanf("");
            a = make_float4(q, q, q, q);
            y = q;
        }
        oa[i] = a;
        ob[i] = y;
    }
}

// ---- hypotheses: sample + 6-point DLT, a row of the system per lane -------------------------------------------------------
__device__ __forceinline__ double nanmax(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(PNP_HYP_BLOCK) void k_pnp_hyp(const aria_pnp_corr* __restrict__ corr, const int* __restrict__ npts,
                                                           int corr_cap, int H, uint64_t seed, int pair_base, double fx,
                                                           double fy, double cx, double cy, float* __restrict__ Ps,
                                                           int* __restrict__ cnt, int* __restrict__ dbg_idx) {
    const int p = blockIdx.x;
    const int row = threadIdx.x & (PNP_ROW - 1);
    const int h = blockIdx.y * (PNP_HYP_BLOCK / PNP_ROW) + (threadIdx.x / PNP_ROW);
    const int n = npts[p];
    bool ok = n >= PNP_MIN;                  // uniform over the 16 lanes of a hypothesis, as is everything that decides below
    int idx[6];
#pragma unroll
    for (int j = 0; j < 6; j++) idx[j] = -1;
    if (ok) ok = draw_sample<6, PNP_MAX_RETRY>(seed, (uint32_t)(pair_base + p), h, n, idx);
    if (dbg_idx && row == 0) {
#pragma unroll
        for (int j = 0; j < 6; j++) dbg_idx[h * 6 + j] = idx[j];
    }
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t0[3] = {0, 0, 0};
    if (ok) {
        const aria_pnp_corr* cp = corr + (int64_t)p * corr_cap;
        // conditioning, in sample order, by every lane of the row
        double X[6][3];
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) X[j][k] = cp[idx[j]].X[k];
        double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = c[k] + X[j][k];
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = c[k] / 6.0;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double d0 = X[j][0] - c[0], d1 = X[j][1] - c[1], d2 = X[j][2] - c[2];
            s = s + sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        }
        s = s / 6.0;
        ok = s > 0.0 && isfinite(s);
        const double sd = ok ? s : 1.0;
        // this lane's row: point row / 2, the x-row (even) or the y-row (odd); rows 11..15 do not exist
        const int mj = min(row >> 1, 5);
        const bool second = (row & 1) != 0, real = row < 11;
        double xm[3] = {X[0][0], X[0][1], X[0][2]};
        int im = idx[0];
#pragma unroll
        for (int j = 1; j < 6; j++) {
            const bool sel = mj == j;
#pragma unroll
            for (int k = 0; k < 3; k++) xm[k] = sel ? X[j][k] : xm[k];
            im = sel ? idx[j] : im;
        }
        const double xn = second ? ((double)cp[im].v - cy) / fy : ((double)cp[im].u - cx) / fx;
        double Xh[4];
#pragma unroll
        for (int k = 0; k < 3; k++) Xh[k] = (xm[k] - c[k]) / sd;
        Xh[3] = 1.0;
        double a[12];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = (real && !second) ? Xh[k] : 0.0;
            a[4 + k] = (real && second) ? Xh[k] : 0.0;
            a[8 + k] = real ? (-xn) * Xh[k] : 0.0;
        }
        double amax = 0.0;
#pragma unroll
        for (int k = 0; k < 12; k++) amax = nanmax(amax, fabs(a[k]));
#pragma unroll
        for (int off = PNP_ROW / 2; off > 0; off >>= 1) amax = nanmax(amax, __shfl_xor(amax, off, PNP_ROW));
        // Gaussian elimination with partial pivoting: first row of largest |a[r][col]|, r >= col
#pragma unroll
        for (int col = 0; col < 11; col++) {
            double v = (row >= col && real) ? fabs(a[col]) : -1.0;
            v = (v != v) ? -1.0 : v;
            int pl = row;
#pragma unroll
            for (int off = PNP_ROW / 2; off > 0; off >>= 1) {
                const double ov = __shfl_xor(v, off, PNP_ROW);
                const int ol = __shfl_xor(pl, off, PNP_ROW);
                const bool take = ov > v || (ov == v && ol < pl);
                v = take ? ov : v;
                pl = take ? ol : pl;
            }
            ok &= v > PNP_PIVOT_TOL * amax;
            double pr[12];
#pragma unroll
            for (int k = col; k < 12; k++) {
                const double prow = __shfl(a[k], pl, PNP_ROW);
                const double rowc = __shfl(a[k], col, PNP_ROW);
                a[k] = (row == col) ? prow : (row == pl) ? rowc : a[k];
                pr[k] = prow;
            }
            const double inv = 1.0 / (ok ? pr[col] : 1.0);
            const bool below = row > col && real;
            const double f = a[col] * inv;
#pragma unroll
            for (int k = col + 1; k < 12; k++) a[k] = below ? a[k] - f * pr[k] : a[k];
        }
        // back substitution with p11 = 1: row `col` lies in lane `col`
        double P[12];
        P[11] = 1.0;
#pragma unroll
        for (int col = 10; col >= 0; col--) {
            double acc = 0.0;
#pragma unroll
            for (int k = col + 1; k < 12; k++) acc = acc + a[k] * P[k];
            const double mine = -acc / (ok ? a[col] : 1.0);
            P[col] = __shfl(mine, col, PNP_ROW);
        }
        ok &= finite9(P, 12);
        const double M[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
        const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
        ok &= det > 0.0;
        double sig[3];
        if (ok) ok = pnp_rotation(M, R, sig);
        if (ok) {
            const double lam = (sig[0] + sig[1] + sig[2]) / 3.0;
            const double X0[3] = {cp[0].X[0], cp[0].X[1], cp[0].X[2]};
            const double m[3] = {P[3], P[7], P[11]};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double t = sd * (m[k] / lam) - ((R[3 * k] * c[0] + R[3 * k + 1] * c[1]) + R[3 * k + 2] * c[2]);
                ok &= pnp_hand_over(R, t, X0, k, t0);
            }
            ok &= finite9(R, 9);
        }
    }
    if (row == 0) pnp_store_model(Ps, cnt, p, H, h, ok, R, t0);
}

// ---- hypotheses, the other solver: sample of 4 + P3P, a lane per hypothesis ---------------------------------------------------
// pnp_ref.solve_p3p line by line (the header's "Minimal solver, P3P"): every sum in its order, no contraction.
struct P3 {
    double x, y, z;
};
__device__ __forceinline__ P3 p3_sub(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3 p3_cross(P3 a, P3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double p3_dot(P3 a, P3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double p3_det(P3 a, P3 b, P3 c) { return p3_dot(a, p3_cross(b, c)); }
__device__ __forceinline__ P3 p3_sel(bool c, P3 a, P3 b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }

// unit null vector of D0 - lam I, D0 symmetric with entries d00 d01 d02 d11 d12 d22: the largest row cross product, ties to
// the earliest
__device__ __forceinline__ P3 p3_rank2_vector(double d00, double d01, double d02, double d11, double d12, double d22, double lam) {
    const P3 r0 = {d00 - lam, d01, d02}, r1 = {d01, d11 - lam, d12}, r2 = {d02, d12, d22 - lam};
    P3 v = p3_cross(r0, r1);
    double n = p3_dot(v, v);
    const P3 c1 = p3_cross(r0, r2);
    const double n1 = p3_dot(c1, c1);
    bool take = n1 > n;
    v = p3_sel(take, c1, v);
    n = take ? n1 : n;
    const P3 c2 = p3_cross(r1, r2);
    const double n2 = p3_dot(c2, c2);
    take = n2 > n;
    v = p3_sel(take, c2, v);
    n = take ? n2 : n;
    const double nn = sqrt(n);
    return {v.x / nn, v.y / nn, v.z / nn};
}

__global__ __launch_bounds__(PNP_P3P_BLOCK) void k_pnp_hyp_p3p(const aria_pnp_corr* __restrict__ corr, const int* __restrict__ npts,
                                                               int corr_cap, int H, uint64_t seed, int pair_base, double fx,
                                                               double fy, double cx, double cy, float* __restrict__ Ps,
                                                               int* __restrict__ cnt, int* __restrict__ dbg_idx) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * PNP_P3P_BLOCK + threadIdx.x;
    if (h >= H) return;
    const int n = npts[p];
    bool ok = n >= PNP_MIN_P3P;
    int idx[4] = {-1, -1, -1, -1};
    if (ok) ok = draw_sample<4, PNP_MAX_RETRY>(seed, (uint32_t)(pair_base + p), h, n, idx);
    if (dbg_idx) {
#pragma unroll
        for (int j = 0; j < 4; j++) dbg_idx[h * 6 + j] = idx[j];
        dbg_idx[h * 6 + 4] = -1;
        dbg_idx[h * 6 + 5] = -1;
    }
    double Rb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tb[3] = {0, 0, 0}, t0[3] = {0, 0, 0};
    int slot = -1;
    if (ok) {
        const aria_pnp_corr* cp = corr + (int64_t)p * corr_cap;
        const aria_pnp_corr q0 = cp[idx[0]], q1 = cp[idx[1]], q2 = cp[idx[2]], q3 = cp[idx[3]];
        const P3 X1 = {q0.X[0], q0.X[1], q0.X[2]}, X2 = {q1.X[0], q1.X[1], q1.X[2]}, X3 = {q2.X[0], q2.X[1], q2.X[2]};
        const P3 X4 = {q3.X[0], q3.X[1], q3.X[2]};
        // 1. unit bearings, squared distances from differences, cosines
        P3 y1, y2, y3;
        {
            double x = ((double)q0.u - cx) / fx, y = ((double)q0.v - cy) / fy, nr = sqrt((x * x + y * y) + 1.0);
            y1 = {x / nr, y / nr, 1.0 / nr};
            x = ((double)q1.u - cx) / fx; y = ((double)q1.v - cy) / fy; nr = sqrt((x * x + y * y) + 1.0);
            y2 = {x / nr, y / nr, 1.0 / nr};
            x = ((double)q2.u - cx) / fx; y = ((double)q2.v - cy) / fy; nr = sqrt((x * x + y * y) + 1.0);
            y3 = {x / nr, y / nr, 1.0 / nr};
        }
        const double x4 = ((double)q3.u - cx) / fx, y4 = ((double)q3.v - cy) / fy;
        const P3 v1 = p3_sub(X1, X2), v2 = p3_sub(X1, X3), d23 = p3_sub(X2, X3);
        const double a12 = p3_dot(v1, v1), a13 = p3_dot(v2, v2), a23 = p3_dot(d23, d23);
        const double b12 = p3_dot(y1, y2), b13 = p3_dot(y1, y3), b23 = p3_dot(y2, y3);
        const P3 v3 = p3_cross(v1, v2);
        const double area2 = p3_dot(v3, v3);
        const double amax = fmax(fmax(a12, a13), a23);
        ok = area2 > P3P_AREA_TOL * (amax * amax);
        // 2. the cubic det(D1 + g D2) = 0, D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23 (columns; both symmetric)
        const P3 D1a = {a23, -(a23 * b12), 0.0}, D1b = {-(a23 * b12), a23 - a12, a12 * b23}, D1c = {0.0, a12 * b23, -a12};
        const P3 D2a = {a23, 0.0, -(a23 * b13)}, D2b = {0.0, -a13, a13 * b23}, D2c = {-(a23 * b13), a13 * b23, a23 - a13};
        const double c3 = p3_det(D2a, D2b, D2c);
        const double c2 = (p3_det(D1a, D2b, D2c) + p3_det(D2a, D1b, D2c)) + p3_det(D2a, D2b, D1c);
        const double c1 = (p3_det(D2a, D1b, D1c) + p3_det(D1a, D2b, D1c)) + p3_det(D1a, D1b, D2c);
        const double c0 = p3_det(D1a, D1b, D1c);
        ok &= c3 != 0.0;
        const double ca = c2 / c3, cb = c1 / c3, cc = c0 / c3;
        const double xi = -ca / 3.0;
        const double disc = ca * ca - 3.0 * cb;
        const double fi = ((xi + ca) * xi + cb) * xi + cc;
        const double rr = 2.0 * sqrt(disc > 0.0 ? disc : 0.0) / 3.0;
        double g = disc > 0.0 ? (fi > 0.0 ? xi - rr : xi + rr) : xi;
#pragma unroll 1
        for (int it = 0; it < P3P_CUBIC_STEPS; it++) {
            const double f = ((g + ca) * g + cb) * g + cc;
            const double fp = (3.0 * g + 2.0 * ca) * g + cb;
            g = fp != 0.0 ? g - f / fp : g;
        }
        // 3. the rank-2 form D0 = D1 + g D2 and its two eigenpairs
        const double d00 = D1a.x + g * D2a.x, d01 = D1a.y + g * D2a.y, d02 = D1a.z + g * D2a.z;
        const double d11 = D1b.y + g * D2b.y, d12 = D1b.z + g * D2b.z, d22 = D1c.z + g * D2c.z;
        const double tr = (d00 + d11) + d22;
        const double mm = ((d00 * d11 - d01 * d01) + (d00 * d22 - d02 * d02)) + (d11 * d22 - d12 * d12);
        const double dq = tr * tr - 4.0 * mm;
        const double sq = sqrt(dq > 0.0 ? dq : 0.0);
        const double la = (tr + (tr >= 0.0 ? sq : -sq)) / 2.0;
        const double lb = mm / la;
        const bool pos = la > 0.0;
        ok &= (pos && lb < 0.0) || (la < 0.0 && lb > 0.0);
        if (ok) {
            const P3 ea = p3_rank2_vector(d00, d01, d02, d11, d12, d22, la), eb = p3_rank2_vector(d00, d01, d02, d11, d12, d22, lb);
            const P3 e1 = p3_sel(pos, ea, eb), e2 = p3_sel(pos, eb, ea);
            const double lpos = pos ? la : lb, lneg = pos ? lb : la;
            const double s = sqrt(-lneg / lpos);
            const double iw = 1.0 / area2;
            const P3 wa = p3_cross(v2, v3), wb = p3_cross(v3, v1);
            const P3 w1v = {wa.x * iw, wa.y * iw, wa.z * iw}, w2v = {wb.x * iw, wb.y * iw, wb.z * iw}, w3v = {v3.x * iw, v3.y * iw, v3.z * iw};
            double best = __builtin_inf();
            // 4. - 7. the four candidate slots in their order: (+s, -s) x (q / A, C / q); a fixed trip count, predicated
#pragma unroll 1
            for (int sign = 0; sign < 2; sign++) {
                const double ss = sign ? -s : s;
                const double p0 = e1.x - ss * e2.x, p1 = e1.y - ss * e2.y, p2 = e1.z - ss * e2.z;
                const double w0 = -p1 / p0, w1 = -p2 / p0;
                const double A = a23 * (w1 * w1) - a12;
                const double B = a23 * (2.0 * (w0 * w1) - 2.0 * (b12 * w1)) + 2.0 * (a12 * b23);
                const double C = a23 * ((w0 * w0 + 1.0) - 2.0 * (b12 * w0)) - a12;
                const double qd = B * B - 4.0 * (A * C);
                const double sqd = sqrt(qd >= 0.0 ? qd : 0.0);
                const double q = -(B + (B >= 0.0 ? sqd : -sqd)) / 2.0;
#pragma unroll 1
                for (int root = 0; root < 2; root++) {
                    const double tau = root ? C / q : q / A;
                    const double den = (1.0 + tau * tau) - (2.0 * b23) * tau;
                    double l2 = sqrt(a23 / (den > 0.0 ? den : 1.0));
                    double l3 = tau * l2;
                    double l1 = w0 * l2 + w1 * l3;
                    const bool alive = qd >= 0.0 && tau > 0.0 && den > 0.0 && l1 > 0.0;
                    // 5. polish: Newton on the three distance equations, the 3x3 solve by the adjugate
#pragma unroll 1
                    for (int it = 0; it < P3P_POLISH_STEPS; it++) {
                        const double r1 = ((l1 * l1 + l2 * l2) - (2.0 * b12) * (l1 * l2)) - a12;
                        const double r2 = ((l1 * l1 + l3 * l3) - (2.0 * b13) * (l1 * l3)) - a13;
                        const double r3 = ((l2 * l2 + l3 * l3) - (2.0 * b23) * (l2 * l3)) - a23;
                        const double j00 = 2.0 * (l1 - b12 * l2), j01 = 2.0 * (l2 - b12 * l1);
                        const double j10 = 2.0 * (l1 - b13 * l3), j12 = 2.0 * (l3 - b13 * l1);
                        const double j21 = 2.0 * (l2 - b23 * l3), j22 = 2.0 * (l3 - b23 * l2);
                        const double dj = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
                        const bool go = dj != 0.0;
                        const double g1 = (-(j12 * j21) * r1 - (j01 * j22) * r2) + (j01 * j12) * r3;
                        const double g2 = (-(j10 * j22) * r1 + (j00 * j22) * r2) - (j00 * j12) * r3;
                        const double g3 = ((j10 * j21) * r1 - (j00 * j21) * r2) - (j01 * j10) * r3;
                        l1 = go ? l1 - g1 / dj : l1;
                        l2 = go ? l2 - g2 / dj : l2;
                        l3 = go ? l3 - g3 / dj : l3;
                    }
                    // 6. pose from the two triangles
                    const P3 Y1 = {l1 * y1.x, l1 * y1.y, l1 * y1.z}, Y2 = {l2 * y2.x, l2 * y2.y, l2 * y2.z}, Y3 = {l3 * y3.x, l3 * y3.y, l3 * y3.z};
                    const P3 u1 = p3_sub(Y1, Y2), u2 = p3_sub(Y1, Y3);
                    const P3 u3 = p3_cross(u1, u2);
                    double R[9], t[3];
                    R[0] = (u1.x * w1v.x + u2.x * w2v.x) + u3.x * w3v.x;
                    R[1] = (u1.x * w1v.y + u2.x * w2v.y) + u3.x * w3v.y;
                    R[2] = (u1.x * w1v.z + u2.x * w2v.z) + u3.x * w3v.z;
                    R[3] = (u1.y * w1v.x + u2.y * w2v.x) + u3.y * w3v.x;
                    R[4] = (u1.y * w1v.y + u2.y * w2v.y) + u3.y * w3v.y;
                    R[5] = (u1.y * w1v.z + u2.y * w2v.z) + u3.y * w3v.z;
                    R[6] = (u1.z * w1v.x + u2.z * w2v.x) + u3.z * w3v.x;
                    R[7] = (u1.z * w1v.y + u2.z * w2v.y) + u3.z * w3v.y;
                    R[8] = (u1.z * w1v.z + u2.z * w2v.z) + u3.z * w3v.z;
                    t[0] = Y1.x - ((R[0] * X1.x + R[1] * X1.y) + R[2] * X1.z);
                    t[1] = Y1.y - ((R[3] * X1.x + R[4] * X1.y) + R[5] * X1.z);
                    t[2] = Y1.z - ((R[6] * X1.x + R[7] * X1.y) + R[8] * X1.z);
                    // 7. the fourth point picks: least error, ties to the earliest slot
                    const double cx4 = ((R[0] * X4.x + R[1] * X4.y) + R[2] * X4.z) + t[0];
                    const double cy4 = ((R[3] * X4.x + R[4] * X4.y) + R[5] * X4.z) + t[1];
                    const double cz4 = ((R[6] * X4.x + R[7] * X4.y) + R[8] * X4.z) + t[2];
                    const double zz = cz4 > 0.0 ? cz4 : 1.0;
                    const double ex = cx4 / zz - x4, ey = cy4 / zz - y4;
                    const double err = ex * ex + ey * ey;
                    const bool fin = isfinite(err) && finite9(R, 9) && finite9(t, 3);
                    const bool take = alive && fin && cz4 > 0.0 && err < best;
                    best = take ? err : best;
                    slot = take ? 2 * sign + root : slot;
#pragma unroll
                    for (int k = 0; k < 9; k++) Rb[k] = take ? R[k] : Rb[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) tb[k] = take ? t[k] : tb[k];
                }
            }
        }
        ok = slot >= 0;
        // 8. hand-over
        if (ok) {
            const double X0[3] = {cp[0].X[0], cp[0].X[1], cp[0].X[2]};
#pragma unroll
            for (int k = 0; k < 3; k++) ok &= pnp_hand_over(Rb, tb[k], X0, k, t0);
            ok &= finite9(Rb, 9);
        }
    }
    pnp_store_model(Ps, cnt, p, H, h, ok, Rb, t0);
}

// ---- scoring: the hot loop ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNP_SCORE_BLOCK) void k_pnp_score(const float4* __restrict__ pa, const float* __restrict__ pb,
                                                               const int* __restrict__ npts, int corr_cap, int H,
                                                               const float* __restrict__ Ps, int* __restrict__ cnt, float thr2) {
    __shared__ float4 ta[PNP_TILE];
    __shared__ float tb[PNP_TILE];
    const int p = blockIdx.x;
    const int h = blockIdx.y * PNP_SCORE_BLOCK + threadIdx.x;
    const int n = npts[p];
    const bool live = h < H && cnt[(int64_t)p * H + h] == 0;
    float r[9], t[3];
    const float* Pp = Ps + (int64_t)p * 12 * H;
#pragma unroll
    for (int k = 0; k < 9; k++) r[k] = live ? Pp[(int64_t)k * H + h] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = live ? Pp[(int64_t)(9 + k) * H + h] : 0.0f;
    const float4* qa = pa + (int64_t)p * corr_cap;
    const float* qb = pb + (int64_t)p * corr_cap;
    int count = 0;
    for (int base = 0; base < n; base += PNP_TILE) {
        const int m = min(PNP_TILE, n - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += PNP_SCORE_BLOCK) {
            ta[i] = qa[base + i];
            tb[i] = qb[base + i];
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < m; i++) count += pnp_inlier(r, t, ta[i], tb[i], thr2);
        }
    }
    if (live) cnt[(int64_t)p * H + h] = count;
}

// ---- finish: winner, Gauss-Newton, rescoring, outputs ---------------------------------------------------------------------
struct PnpPoint {
    double d[3], x, y;
};

__device__ __forceinline__ PnpPoint pnp_point(const aria_pnp_corr& c, const double* X0, double fx, double fy, double cx, double cy) {
    PnpPoint q;
    q.d[0] = c.X[0] - X0[0];
    q.d[1] = c.X[1] - X0[1];
    q.d[2] = c.X[2] - X0[2];
    q.x = ((double)c.u - cx) / fx;
    q.y = ((double)c.v - cy) / fy;
    return q;
}

__device__ __forceinline__ void pnp_camera(const double* R, const double* t, const PnpPoint& q, double Xc[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) Xc[k] = ((R[3 * k] * q.d[0] + R[3 * k + 1] * q.d[1]) + R[3 * k + 2] * q.d[2]) + t[k];
}

// sum over the workgroup in a fixed order: xor butterfly inside each wave, then the waves in wave order; result in out[k]
template <int N>
__device__ __forceinline__ void block_sum(double (&acc)[N], double (*wave)[N], double* out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
        if ((tid & 63) == 0) wave[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < N) {
        double v = 0.0;
        for (int w = 0; w < PNP_FINISH_BLOCK / 64; w++) v = v + wave[w][tid];
        out[tid] = v;
    }
    __syncthreads();
}

// One Gauss-Newton step from the summed normal equations S (21 upper entries row by row, then the 6 of J^T r), by one lane:
// Cholesky, the left update of (R, t). Returns 0 = no step (the refinement ends), 1 = step taken, 2 = step taken and small.
__device__ int pnp_gn_step(const double* S, double* L, double* R, double* t) {
    int k = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) L[c * 6 + r] = S[k++];      // lower triangle of A
    for (int j = 0; j < 6; j++) {
        double d = L[j * 6 + j];
        for (int q = 0; q < j; q++) d = d - L[j * 6 + q] * L[j * 6 + q];
        if (!(d > 0.0) || !isfinite(d)) return 0;
        const double dj = sqrt(d);
        L[j * 6 + j] = dj;
        for (int i = j + 1; i < 6; i++) {
            double v = L[i * 6 + j];
            for (int q = 0; q < j; q++) v = v - L[i * 6 + q] * L[j * 6 + q];
            L[i * 6 + j] = v / dj;
        }
    }
    double y[6], x[6];
    for (int i = 0; i < 6; i++) {
        double v = -S[21 + i];
        for (int q = 0; q < i; q++) v = v - L[i * 6 + q] * y[q];
        y[i] = v / L[i * 6 + i];
    }
    for (int i = 5; i >= 0; i--) {
        double v = y[i];
        for (int q = i + 1; q < 6; q++) v = v - L[q * 6 + i] * x[q];
        x[i] = v / L[i * 6 + i];
    }
    double nrm = 0.0;
    for (int i = 0; i < 6; i++) nrm = nrm + x[i] * x[i];
    if (!isfinite(nrm)) return 0;
    double E[9];
    exp_so3(x, E);
    double Rn[9], tn[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rn[r * 3 + c] = E[r * 3] * R[c] + E[r * 3 + 1] * R[3 + c] + E[r * 3 + 2] * R[6 + c];
        tn[r] = (E[r * 3] * t[0] + E[r * 3 + 1] * t[1] + E[r * 3 + 2] * t[2]) + x[3 + r];
    }
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    for (int i = 0; i < 3; i++) t[i] = tn[i];
    return sqrt(nrm) <= PNP_STEP_TOL ? 2 : 1;
}

__device__ __forceinline__ void pnp_write_invalid(aria_pnp_result* o, int n) {
    for (int k = 0; k < 9; k++) o->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 3; k++) o->t[k] = 0.0;
    o->rms_px = 0.0;
    o->n_corr = n; o->n_inliers = 0; o->best_hypothesis = -1; o->iterations = 0; o->refined = 0; o->valid = 0;
}

__global__ __launch_bounds__(PNP_FINISH_BLOCK) void k_pnp_finish(const aria_pnp_corr* __restrict__ corr, const float4* __restrict__ pa,
                                                                 const float* __restrict__ pb, const int* __restrict__ npts,
                                                                 int corr_cap, int H, const float* __restrict__ Ps,
                                                                 const int* __restrict__ cnt, float thr2, double fx, double fy,
                                                                 double cx, double cy, int refine_iters, int min_corr,
                                                                 uint8_t* __restrict__ ws, uint8_t* __restrict__ mask,
                                                                 aria_pnp_result* __restrict__ out) {
    __shared__ int red_c[PNP_FINISH_BLOCK], red_h[PNP_FINISH_BLOCK];
    __shared__ double Sw[PNP_FINISH_BLOCK / 64][27], S[27], L[36];
    __shared__ double Rc[9], tc[3], X0[3];
    __shared__ float Pw[12], Pf[12];
    __shared__ int n_in, n_ref, stop, iters, have_ref, out_ok;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = npts[p];
    const aria_pnp_corr* cp = corr + (int64_t)p * corr_cap;
    const float4* qa = pa + (int64_t)p * corr_cap;
    const float* qb = pb + (int64_t)p * corr_cap;
    uint8_t* w = ws + (int64_t)p * corr_cap;

    // argmax over (count, -h): ascending scan per lane, then a fixed tree
    int bc = -1, bh = -1;
    for (int h = tid; h < H; h += PNP_FINISH_BLOCK) {
        const int c = cnt[(int64_t)p * H + h];
        if (c > bc) { bc = c; bh = h; }
    }
    red_c[tid] = bc;
    red_h[tid] = bh;
    __syncthreads();
    for (int s = PNP_FINISH_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int c2 = red_c[tid + s], h2 = red_h[tid + s];
            if (c2 > red_c[tid] || (c2 == red_c[tid] && c2 >= 0 && h2 < red_h[tid])) { red_c[tid] = c2; red_h[tid] = h2; }
        }
        __syncthreads();
    }
    const int win_c = red_c[0], win_h = red_h[0];
    aria_pnp_result* o = out + p;
    uint8_t* mk = mask ? mask + (int64_t)p * corr_cap : nullptr;
    if (n < min_corr || win_c < 0) {             // min_corr: the solver's sample size
        if (mk)
            for (int i = tid; i < corr_cap; i += PNP_FINISH_BLOCK) mk[i] = 0;
        if (tid == 0) pnp_write_invalid(o, n);
        return;
    }
    if (tid < 12) Pw[tid] = Ps[((int64_t)p * 12 + tid) * H + win_h];
    if (tid < 3) X0[tid] = cp[0].X[tid];
    if (tid == 0) { n_in = 0; n_ref = 0; stop = 1; iters = 0; have_ref = 0; out_ok = 0; }
    __syncthreads();
    {   // the winner's inliers (the same test, on the same fp32 pose, as its score)
        float r[9], t[3];
        for (int k = 0; k < 9; k++) r[k] = Pw[k];
        for (int k = 0; k < 3; k++) t[k] = Pw[9 + k];
        int c = 0;
        for (int i = tid; i < n; i += PNP_FINISH_BLOCK) {
            const int in = pnp_inlier(r, t, qa[i], qb[i], thr2);
            w[i] = (uint8_t)in;
            c += in;
        }
        atomicAdd(&n_in, c);
    }
    __syncthreads();
    const int win_in = n_in;
    if (win_in >= PNP_MIN && refine_iters > 0) {
        if (tid == 0) {   // the start: the winner as scored, R replaced by the nearest rotation
            double M[9], R[9], sig[3];
            for (int k = 0; k < 9; k++) M[k] = (double)Pw[k];
            const bool ok = pnp_rotation(M, R, sig);
            for (int k = 0; k < 9; k++) Rc[k] = ok ? R[k] : M[k];
            for (int k = 0; k < 3; k++) tc[k] = (double)Pw[9 + k];
            stop = ok ? 0 : 1;
        }
        __syncthreads();
        for (int it = 0; it < refine_iters; it++) {
            if (stop) break;                 // read between two barriers that no write to `stop` lies between
            double R[9], t[3], x0[3];
            for (int k = 0; k < 9; k++) R[k] = Rc[k];
            for (int k = 0; k < 3; k++) { t[k] = tc[k]; x0[k] = X0[k]; }
            double acc[27];
#pragma unroll
            for (int k = 0; k < 27; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += PNP_FINISH_BLOCK) {
                if (!w[i]) continue;
                const PnpPoint q = pnp_point(cp[i], x0, fx, fy, cx, cy);
                double Xc[3];
                pnp_camera(R, t, q, Xc);
                const double iz = 1.0 / Xc[2];
                const double px = Xc[0] * iz, py = Xc[1] * iz;
                const double rx = px - q.x, ry = py - q.y;
                const double Jx[6] = {-(px * py), 1.0 + px * px, -py, iz, 0.0, -(px * iz)};
                const double Jy[6] = {-(1.0 + py * py), px * py, px, 0.0, iz, -(py * iz)};
                int k = 0;
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int c = r; c < 6; c++) acc[k++] += Jx[r] * Jx[c] + Jy[r] * Jy[c];
#pragma unroll
                for (int r = 0; r < 6; r++) acc[21 + r] += Jx[r] * rx + Jy[r] * ry;
            }
            block_sum<27>(acc, Sw, S);
            if (tid == 0) {
                const int step = finite9(S, 27) ? pnp_gn_step(S, L, Rc, tc) : 0;
                if (step) iters = iters + 1;
                if (step != 1) stop = 1;
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) {
            bool ok = iters > 0;
            for (int k = 0; k < 9; k++) { Pf[k] = (float)Rc[k]; ok &= isfinite(Pf[k]); }
            for (int k = 0; k < 3; k++) { Pf[9 + k] = (float)tc[k]; ok &= fabsf(Pf[9 + k]) <= (float)PNP_RANGE; }
            have_ref = ok ? 1 : 0;
        }
        __syncthreads();
        if (have_ref) {
            float r[9], t[3];
            for (int k = 0; k < 9; k++) r[k] = Pf[k];
            for (int k = 0; k < 3; k++) t[k] = Pf[9 + k];
            int c = 0;
            for (int i = tid; i < n; i += PNP_FINISH_BLOCK) c += pnp_inlier(r, t, qa[i], qb[i], thr2);
            atomicAdd(&n_ref, c);
        }
        __syncthreads();
    }
    const bool refined = have_ref && n_ref >= win_in;
    const int n_it = iters;
    __syncthreads();
    if (refined) {
        float r[9], t[3];
        for (int k = 0; k < 9; k++) r[k] = Pf[k];
        for (int k = 0; k < 3; k++) t[k] = Pf[9 + k];
        for (int i = tid; i < n; i += PNP_FINISH_BLOCK) w[i] = (uint8_t)pnp_inlier(r, t, qa[i], qb[i], thr2);
    } else if (tid < 12) {                   // the winner as scored
        if (tid < 9) Rc[tid] = (double)Pw[tid];
        else tc[tid - 9] = (double)Pw[tid];
    }
    __syncthreads();
    const int final_in = refined ? n_ref : win_in;
    {   // rms over the kept inliers
        double R[9], t[3], x0[3];
        for (int k = 0; k < 9; k++) R[k] = Rc[k];
        for (int k = 0; k < 3; k++) { t[k] = tc[k]; x0[k] = X0[k]; }
        double acc[1] = {0.0};
        for (int i = tid; i < n; i += PNP_FINISH_BLOCK) {
            if (!w[i]) continue;
            const PnpPoint q = pnp_point(cp[i], x0, fx, fy, cx, cy);
            double Xc[3];
            pnp_camera(R, t, q, Xc);
            const double rx = Xc[0] / Xc[2] - q.x, ry = Xc[1] / Xc[2] - q.y;
            acc[0] += rx * rx + ry * ry;
        }
        block_sum<1>(acc, (double(*)[1])Sw, S);
    }
    if (tid == 0) {
        double tt[3];
        for (int k = 0; k < 3; k++) tt[k] = tc[k] - ((Rc[3 * k] * X0[0] + Rc[3 * k + 1] * X0[1]) + Rc[3 * k + 2] * X0[2]);
        const double rms = final_in > 0 ? sqrt(S[0] / (double)final_in) * ((fx + fy) * 0.5) : 0.0;
        const bool ok = finite9(Rc, 9) && finite9(tt, 3) && isfinite(rms);
        if (ok) {
            for (int k = 0; k < 9; k++) o->R[k] = Rc[k];
            for (int k = 0; k < 3; k++) o->t[k] = tt[k];
            o->rms_px = rms;
            o->n_corr = n; o->n_inliers = final_in; o->best_hypothesis = win_h; o->iterations = n_it;
            o->refined = refined ? 1 : 0; o->valid = 1;
        } else {
            pnp_write_invalid(o, n);
        }
        out_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (mk) {
        const bool ok = out_ok != 0;
        for (int i = tid; i < corr_cap; i += PNP_FINISH_BLOCK) mk[i] = (ok && i < n) ? w[i] : (uint8_t)0;
    }
}

// ---- association: match list x point map -> correspondences ---------------------------------------------------------------
// table[p * kp_stride + k] = the lowest arena position of a point of pair anchor_base + p whose anchor-frame index is k
__global__ __launch_bounds__(256) void k_pnp_assoc_scatter(const aria_map_point* __restrict__ arena, const long long* __restrict__ d_size,
                                                           long long capacity, int anchor_base, int anchor_view, int n_pairs,
                                                           int64_t kp_stride, int* __restrict__ table) {
    long long size = *d_size;
    size = size < 0 ? 0 : (size > capacity ? capacity : size);
    if (size > (long long)PNP_EMPTY) size = PNP_EMPTY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += (long long)gridDim.x * blockDim.x) {
        const int pair = arena[i].pair;
        const int key = anchor_view == 1 ? arena[i].idx1 : arena[i].idx2;
        const long long rel = (long long)pair - (long long)anchor_base;
        if (rel < 0 || rel >= n_pairs || key < 0 || key >= kp_stride) continue;
        atomicMin(&table[rel * kp_stride + key], (int)i);
    }
}

__global__ __launch_bounds__(256) void k_pnp_assoc_gather(const aria_map_point* __restrict__ arena, const int* __restrict__ table,
                                                          const aria_keypoint* __restrict__ kq, const int* __restrict__ nq,
                                                          int64_t kp_stride, const aria_match* __restrict__ matches,
                                                          const int* __restrict__ nmatches, int match_cap,
                                                          aria_pnp_corr* __restrict__ corr, int* __restrict__ ncorr,
                                                          int* __restrict__ corr_match, int* __restrict__ err) {
    __shared__ int bad_count, bad_index;       // written before / read after a barrier each: no thread reads one while another writes it
    __shared__ int wsum[4];
    const int p = blockIdx.x;
    const int n = nmatches[p], nqp = nq[p];
    if (threadIdx.x == 0) {
        bad_count = (n < 0 || n > match_cap || nqp < 0 || nqp > kp_stride) ? 1 : 0;
        bad_index = 0;
    }
    __syncthreads();
    const aria_match* m = matches + (int64_t)p * match_cap;
    if (!bad_count) {
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const aria_match a = m[i];
            mine |= (a.query_idx < 0 || a.query_idx >= nqp || a.train_idx < 0 || a.train_idx >= kp_stride);
        }
        if (mine) atomicOr(&bad_index, 1);
    }
    __syncthreads();
    if (bad_count | bad_index) {
        if (threadIdx.x == 0) {
            ncorr[p] = 0;
            atomicOr(err, ERRBIT_PNP_INPUT);
        }
        return;
    }
    const aria_keypoint* q = kq + (int64_t)p * kp_stride;
    const int* tb = table + (int64_t)p * kp_stride;
    aria_pnp_corr* oc = corr + (int64_t)p * match_cap;
    int* om = corr_match ? corr_match + (int64_t)p * match_cap : nullptr;
    int o = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        aria_match a{};
        int pos = PNP_EMPTY;
        if (i < n) {
            a = m[i];
            pos = tb[a.train_idx];
        }
        const bool keep = pos != PNP_EMPTY;
        int total;
        const int slot = block_compact<256>(keep, wsum, total);
        if (keep) {
            aria_pnp_corr c;
            c.X[0] = arena[pos].X[0];
            c.X[1] = arena[pos].X[1];
            c.X[2] = arena[pos].X[2];
            c.u = q[a.query_idx].x;
            c.v = q[a.query_idx].y;
            oc[o + slot] = c;
            if (om) om[o + slot] = i;
        }
        o += total;
    }
    if (threadIdx.x == 0) ncorr[p] = o;
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_pnp_s : StageHandle {
    aria_pnp_config cfg{};
    int solver = ARIA_PNP_SOLVER_DLT6;    // a launch parameter: read when a call is issued (aria_pnp_set_solver)
    // grow-only workspace of the batch path
    DeviceBuffer<float4> d_pa;            // [n_pairs][corr_cap] (dx, dy, dz, x)
    DeviceBuffer<float> d_pb;             // [n_pairs][corr_cap] y
    DeviceBuffer<int> d_npts;             // [n_pairs]
    DeviceBuffer<float> d_P;              // [n_pairs][12][H]
    DeviceBuffer<int> d_cnt;              // [n_pairs][H]
    DeviceBuffer<uint8_t> d_ws;           // [n_pairs][corr_cap] inlier flags
    DeviceBuffer<int> d_table;            // [n_pairs][kp_stride] association table
    // single-pair staging of the host forms
    CorrStaging<aria_pnp_corr> one;
    DeviceBuffer<aria_pnp_result> d_res;
    DeviceBuffer<int> d_dbg;
};

namespace {

float pnp_thr2(const aria_pnp_config& c) { return normalized_thr2(c.threshold_px, c.fx, c.fy); }

int enqueue(aria_pnp_t h, const aria_pnp_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap, int pair_base,
            aria_pnp_result* d_out, uint8_t* d_mask, int* d_dbg, bool finish) {
    const int H = h->cfg.hypotheses;
    int rc;
    if ((rc = h->d_pa.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_pb.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_ws.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_npts.reserve(h->stream, (size_t)n_pairs)) != ARIA_OK) return rc;
    if ((rc = h->d_P.reserve(h->stream, (size_t)n_pairs * H * 12)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, (size_t)n_pairs * H)) != ARIA_OK) return rc;
    const aria_pnp_config& c = h->cfg;
    hipLaunchKernelGGL(k_pnp_stage, dim3(n_pairs), dim3(256), 0, h->stream, d_corr, d_ncorr, corr_cap, c.fx, c.fy, c.cx, c.cy,
                       h->d_pa, h->d_pb, h->d_npts, h->d_err);
    const bool p3p = h->solver == ARIA_PNP_SOLVER_P3P;
    if (p3p)
        hipLaunchKernelGGL(k_pnp_hyp_p3p, dim3(n_pairs, (H + PNP_P3P_BLOCK - 1) / PNP_P3P_BLOCK), dim3(PNP_P3P_BLOCK), 0, h->stream,
                           d_corr, h->d_npts, corr_cap, H, (uint64_t)c.seed, pair_base, c.fx, c.fy, c.cx, c.cy, h->d_P, h->d_cnt, d_dbg);
    else
        hipLaunchKernelGGL(k_pnp_hyp, dim3(n_pairs, H / (PNP_HYP_BLOCK / PNP_ROW)), dim3(PNP_HYP_BLOCK), 0, h->stream, d_corr, h->d_npts,
                           corr_cap, H, (uint64_t)c.seed, pair_base, c.fx, c.fy, c.cx, c.cy, h->d_P, h->d_cnt, d_dbg);
    hipLaunchKernelGGL(k_pnp_score, dim3(n_pairs, (H + PNP_SCORE_BLOCK - 1) / PNP_SCORE_BLOCK), dim3(PNP_SCORE_BLOCK), 0, h->stream,
                       h->d_pa, h->d_pb, h->d_npts, corr_cap, H, h->d_P, h->d_cnt, pnp_thr2(c));
    if (finish)
        hipLaunchKernelGGL(k_pnp_finish, dim3(n_pairs), dim3(PNP_FINISH_BLOCK), 0, h->stream, d_corr, h->d_pa, h->d_pb, h->d_npts,
                           corr_cap, H, h->d_P, h->d_cnt, pnp_thr2(c), c.fx, c.fy, c.cx, c.cy, c.refine_iters,
                           p3p ? PNP_MIN_P3P : PNP_MIN, h->d_ws, d_mask, d_out);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // namespace

extern "C" {

void aria_pnp_default_config(aria_pnp_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_pnp_config);
    c->device = 0;
    c->stream = nullptr;
    c->hypotheses = 1024;
    c->refine_iters = 5;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0, as aria_pose_default_config
    c->threshold_px = 2.0;
    c->seed = 0;
}

int aria_pnp_create(const aria_pnp_config* c, aria_pnp_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_pnp_config)) return ARIA_E_INVALID;
    if (c->hypotheses < 64 || c->hypotheses > 16384 || (c->hypotheses % 64)) return ARIA_E_INVALID;
    if (c->refine_iters < 0 || c->refine_iters > 16) return ARIA_E_INVALID;
    if (bad_pinhole(c->fx, c->fy, c->cx, c->cy) || !(c->threshold_px > 0) || !std::isfinite(c->threshold_px)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_pnp_create", [](aria_pnp_s* h) {
        const int rc = h->d_res.reserve(h->stream, 1, "aria_pnp_create");
        return rc != ARIA_OK ? rc : h->one.create(h->stream, "aria_pnp_create");
    });
}

void aria_pnp_destroy(aria_pnp_t h) { stage_destroy(h); }

void* aria_pnp_stream(aria_pnp_t h) { return stage_stream(h); }

int aria_pnp_set_solver(aria_pnp_t h, int solver) {
    if (!h || (solver != ARIA_PNP_SOLVER_DLT6 && solver != ARIA_PNP_SOLVER_P3P)) return ARIA_E_INVALID;
    h->solver = solver;
    return ARIA_OK;
}

int aria_pnp_get_solver(aria_pnp_t h) { return h ? h->solver : ARIA_E_INVALID; }

int aria_pnp_check(aria_pnp_t h) { return stage_check(h, {{ERRBIT_PNP_INPUT, ARIA_E_INVALID}}); }

int aria_pnp_estimate_batch_device(aria_pnp_t h, const aria_pnp_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap,
                                   int pair_base, aria_pnp_result* d_out, uint8_t* d_mask) {
    if (!h || !d_corr || !d_ncorr || !d_out || n_pairs < 0 || corr_cap < 1 || corr_cap > (1 << 20) || pair_base < 0)
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return enqueue(h, d_corr, d_ncorr, n_pairs, corr_cap, pair_base, d_out, d_mask, nullptr, true);
}

int aria_pnp_estimate(aria_pnp_t h, const aria_pnp_corr* corr, int n, int pair_base, aria_pnp_result* out, uint8_t* mask) {
    if (!h || !out || pair_base < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    CorrStaging<aria_pnp_corr>& s = h->one;
    int rc = s.upload(h->stream, corr, n);
    if (rc != ARIA_OK) return rc;
    if ((rc = enqueue(h, s.d_corr, s.d_n, 1, s.cap, pair_base, h->d_res, s.d_mask, nullptr, true)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(out, h->d_res, sizeof(aria_pnp_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && n) ARIA_HIP(hipMemcpyAsync(mask, s.d_mask, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_pnp_check(h);
}

int aria_pnp_debug_hypotheses(aria_pnp_t h, const aria_pnp_corr* corr, int n, int pair_base, int* sample_idx, float* R, float* t0,
                              int* counts) {
    if (!h || !sample_idx || !R || !t0 || !counts || pair_base < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->one.upload(h->stream, corr, n);
    if (rc != ARIA_OK) return rc;
    const int H = h->cfg.hypotheses;
    if ((rc = h->d_dbg.reserve(h->stream, (size_t)H * 6)) != ARIA_OK) return rc;
    if ((rc = enqueue(h, h->one.d_corr, h->one.d_n, 1, h->one.cap, pair_base, nullptr, nullptr, h->d_dbg, false)) != ARIA_OK) return rc;
    std::vector<float> soa((size_t)12 * H);
    ARIA_HIP(hipMemcpyAsync(sample_idx, h->d_dbg, sizeof(int) * 6 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(soa.data(), h->d_P, sizeof(float) * 12 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(counts, h->d_cnt, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    unpack_models(soa.data(), H, 0, 9, R);
    unpack_models(soa.data(), H, 9, 3, t0);
    return aria_pnp_check(h);
}

int aria_pnp_associate_batch_device(aria_pnp_t h, aria_map_t map, int anchor_base, int anchor_view, const aria_keypoint* d_kp_query,
                                    const int* d_nq, int64_t kp_stride, const aria_match* d_matches, const int* d_nmatches,
                                    int n_pairs, int match_cap, aria_pnp_corr* d_corr, int* d_ncorr, int* d_corr_match) {
    if (!h || !map || !d_kp_query || !d_nq || !d_matches || !d_nmatches || !d_corr || !d_ncorr || n_pairs < 0 || match_cap < 1 ||
        match_cap > (1 << 20) || kp_stride < 1 || kp_stride > (1 << 24) || anchor_base < 0 || (anchor_view != 1 && anchor_view != 2))
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t cells = (size_t)n_pairs * (size_t)kp_stride;
    int rc;
    if ((rc = h->d_table.reserve(h->stream, cells)) != ARIA_OK) return rc;
    const aria_map_point* arena = nullptr;
    const long long* d_size = nullptr;
    int64_t capacity = 0;
    int map_device = -1;
    map_device_view(map, &arena, &d_size, &capacity, &map_device);
    if (map_device != h->device) return ARIA_E_INVALID;          // the join reads the map's arena where it lies
    ARIA_HIP(hipMemsetAsync(h->d_table, 0x7F, cells * sizeof(int), h->stream));
    if (arena && capacity > 0) {
        const int blocks = (int)std::min<int64_t>((capacity + 255) / 256, 2048);
        hipLaunchKernelGGL(k_pnp_assoc_scatter, dim3(blocks), dim3(256), 0, h->stream, arena, d_size, (long long)capacity, anchor_base,
                           anchor_view, n_pairs, kp_stride, h->d_table);
    }
    hipLaunchKernelGGL(k_pnp_assoc_gather, dim3(n_pairs), dim3(256), 0, h->stream, arena, h->d_table, d_kp_query, d_nq, kp_stride,
                       d_matches, d_nmatches, match_cap, d_corr, d_ncorr, d_corr_match, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // extern "C"
