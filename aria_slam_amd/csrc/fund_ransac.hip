// Fundamental-matrix RANSAC on the device: the 7-point minimal solver (run7Point), OpenCV's symmetric epipolar error
// (computeError) and the winner's inliers, batched over pairs. Semantics in include/aria_orb_hip.h ("fundamental-matrix
// RANSAC"); aria_slam_amd/fund_ref.py restates every step in NumPy.
//
// Four launches on the handle's stream:
//   k_fund_stage   one workgroup per pair: validates every match index against the pair's keypoint counts BEFORE any
//                  keypoint is read, writes the pixel points (x1, y1, x2, y2) as one float4 per match, sums centroid and
//                  RMS distance of each view in fp64 (fixed order) and writes the conditioned points (x - c) / d as float4
//   k_fund_hyp     one lane per hypothesis: 7 sample indices from the pose stage's hash, collinearity check, fp64 7-point
//                  solve (elimination with partial pivoting, closed-form cubic), up to 3 models in pixel coordinates (fp64)
//                  and their conditioned form G (fp32, max|G_ij| = 1) for the scorer
//   k_fund_score   one lane per hypothesis with its 3 model slots in registers; the pair's conditioned points in LDS tiles
//                  read as a broadcast, so one point load serves three models (the hot loop; no scratch --
//                  tests/test_fund_host.py)
//   k_fund_finish  one workgroup per pair: argmax tree over (count, -(3 h + k)), the mask and the ordered compaction of the
//                  winner's inlier match records (ballot + popcount per wave, waves in order), result record
// No float atomics anywhere: counts are integers, every floating-point sum has a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "ransac_device.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int FUND_TILE = 2048;            // points per LDS tile of k_fund_score (32 KB)
constexpr int FUND_STAGE_BLOCK = 256;
constexpr int FUND_SCORE_BLOCK = 256;
constexpr int FUND_FINISH_BLOCK = 256;
constexpr int FUND_MIN_MATCHES = 15;       // header "Small inputs": the RANSAC branch of findFundamentalMat
constexpr int FUND_MIN_INLIERS = 7;        // OpenCV's count > max(best, 6)
constexpr int FUND_MAX_RETRY = 256;        // redraws per sample slot (the pose stage's)
constexpr double FUND_PIVOT_TOL = 1e-9;    // |pivot| <= tol * max|A_ij|: rank-deficient sample
constexpr double FUND_CUBIC_TOL = 1e-12;   // |c0| <= tol * max|c_i|: no cubic
constexpr double FUND_2PI_3 = 2.0 * 3.14159265358979323846 / 3.0;
constexpr int ERRBIT_FUND_INPUT = 1;       // a pair's counts or match indices were out of range (pair skipped)
constexpr int FUND_COND = 8;               // per-pair conditioning record: c1x, c1y, d1, c2x, c2y, d2, -, -

// computeError in conditioned coordinates, division-free: q = (u1x, u1y, u2x, u2y), g = G (fp32), t1 / t2 = (thr / d_i)^2
__device__ __forceinline__ int fund_inlier(const float* g, float4 q, float t1, float t2) {
    const float l0 = g[0] * q.x + g[1] * q.y + g[2];
    const float l1 = g[3] * q.x + g[4] * q.y + g[5];
    const float l2 = g[6] * q.x + g[7] * q.y + g[8];
    const float m0 = g[0] * q.z + g[3] * q.w + g[6];
    const float m1 = g[1] * q.z + g[4] * q.w + g[7];
    const float r = q.z * l0 + q.w * l1 + l2;
    const float d2 = l0 * l0 + l1 * l1, d1 = m0 * m0 + m1 * m1, rr = r * r;
    return (d2 > 0.0f && d1 > 0.0f && rr <= t2 * d2 && rr <= t1 * d1) ? 1 : 0;
}

__device__ __forceinline__ float fund_thr(double thr, double d) {
    const double t = thr / d;
    return (float)(t * t);
}

// haveCollinearPoints: slot 6 against every pair of slots 0..5
__device__ __forceinline__ bool collinear7(const double* x, const double* y) {
    bool col = false;
#pragma unroll
    for (int j = 1; j < 6; j++) {
        const double dx1 = x[j] - x[6], dy1 = y[j] - y[6];
#pragma unroll
        for (int k = 0; k < j; k++) {
            const double dx2 = x[k] - x[6], dy2 = y[k] - y[6];
            col |= fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
        }
    }
    return col;
}

// run7Point on the 7 pixel correspondences (fp64): models out[k*9 + e] for k < return value (0, 1 or 3), zero beyond
__device__ __forceinline__ int fund_solve7(const double* x1, const double* y1, const double* x2, const double* y2, double* out) {
#pragma unroll
    for (int e = 0; e < 27; e++) out[e] = 0.0;
    bool ok = !collinear7(x1, y1) && !collinear7(x2, y2);
    double m1x = 0.0, m1y = 0.0, m2x = 0.0, m2y = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) { m1x = m1x + x1[i]; m1y = m1y + y1[i]; m2x = m2x + x2[i]; m2y = m2y + y2[i]; }
    const double t = 1.0 / 7.0;
    m1x = m1x * t; m1y = m1y * t; m2x = m2x * t; m2y = m2y * t;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const double a = x1[i] - m1x, b = y1[i] - m1y, c = x2[i] - m2x, d = y2[i] - m2y;
        s1 = s1 + sqrt(a * a + b * b);
        s2 = s2 + sqrt(c * c + d * d);
    }
    s1 = s1 * t; s2 = s2 * t;
    ok &= s1 >= (double)FLT_EPSILON && s2 >= (double)FLT_EPSILON;
    if (!ok) return 0;
    s1 = sqrt(2.0) / s1;
    s2 = sqrt(2.0) / s2;
    double a[7][9];
    double amax = 0.0;
#pragma unroll
    for (int r = 0; r < 7; r++) {
        const double X0 = (x1[r] - m1x) * s1, Y0 = (y1[r] - m1y) * s1, X1 = (x2[r] - m2x) * s2, Y1 = (y2[r] - m2y) * s2;
        a[r][0] = X1 * X0; a[r][1] = X1 * Y0; a[r][2] = X1;
        a[r][3] = Y1 * X0; a[r][4] = Y1 * Y0; a[r][5] = Y1;
        a[r][6] = X0;      a[r][7] = Y0;      a[r][8] = 1.0;
#pragma unroll
        for (int k = 0; k < 9; k++) amax = fmax(amax, fabs(a[r][k]));
    }
    // Gaussian elimination over columns 0..6 with partial pivoting (first row of largest |a[r][c]|); row swaps as selects
#pragma unroll
    for (int c = 0; c < 7; c++) {
        int piv = c;
        double best = fabs(a[c][c]);
#pragma unroll
        for (int r = c + 1; r < 7; r++) {
            const double v = fabs(a[r][c]);
            if (v > best) { best = v; piv = r; }
        }
        ok &= best > FUND_PIVOT_TOL * amax;
#pragma unroll
        for (int r = c + 1; r < 7; r++)
#pragma unroll
            for (int k = c; k < 9; k++) swap_if(piv == r, a[c][k], a[r][k]);
        const double inv = 1.0 / (ok ? a[c][c] : 1.0);
#pragma unroll
        for (int r = c + 1; r < 7; r++) {
            const double f = a[r][c] * inv;
#pragma unroll
            for (int k = c + 1; k < 9; k++) a[r][k] = a[r][k] - f * a[c][k];
        }
    }
    if (!ok) return 0;
    // null-space basis: g1 (f7 = 1, f8 = 0), g2 (f7 = 0, f8 = 1); f1 = g1 - g2, f2 = g2
    double g1[9], g2[9];
    g1[7] = 1.0; g1[8] = 0.0; g2[7] = 0.0; g2[8] = 1.0;
#pragma unroll
    for (int c = 6; c >= 0; c--) {
        double u = 0.0, v = 0.0;
#pragma unroll
        for (int k = c + 1; k < 9; k++) { u = u + a[c][k] * g1[k]; v = v + a[c][k] * g2[k]; }
        g1[c] = -u / a[c][c];
        g2[c] = -v / a[c][c];
    }
    double f1[9], f2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { f1[i] = g1[i] - g2[i]; f2[i] = g2[i]; }
    // det(l f1 + f2) = c0 l^3 + c1 l^2 + c2 l + c3 (run7Point's expansion)
    double t0 = f2[4] * f2[8] - f2[5] * f2[7];
    double t1 = f2[3] * f2[8] - f2[5] * f2[6];
    double t2 = f2[3] * f2[7] - f2[4] * f2[6];
    const double c3 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    const double c2 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
                      f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
                      f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
                      f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    const double c1 = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
                      f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
                      f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
                      f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    const double c0 = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    const double cmax = fmax(fmax(fabs(c0), fabs(c1)), fmax(fabs(c2), fabs(c3)));
    if (!(fabs(c0) > FUND_CUBIC_TOL * cmax)) return 0;
    // real roots in closed form (solveCubic's Q, R and discriminant Q^3 - R^2)
    const double a1 = c1 / c0, a2 = c2 / c0, a3 = c3 / c0;
    const double Q = (a1 * a1 - 3.0 * a2) * (1.0 / 9.0);
    const double R = (a1 * (2.0 * a1 * a1 - 9.0 * a2) + 27.0 * a3) * (1.0 / 54.0);
    const double disc = (a1 * a1 * (a2 * a2 - 4.0 * a1 * a3) + 2.0 * a2 * (9.0 * a1 * a3 - 2.0 * a2 * a2) - 27.0 * a3 * a3) *
                        (1.0 / 108.0);
    double r0, r1 = 0.0, r2 = 0.0;
    int nr;
    if (disc > 0.0) {
        const double theta = acos(fmin(1.0, fmax(-1.0, R / sqrt(Q * Q * Q))));
        const double sq = -2.0 * sqrt(Q), th = theta * (1.0 / 3.0), sh = a1 * (1.0 / 3.0);
        r0 = sq * cos(th) - sh;
        r1 = sq * cos(th + FUND_2PI_3) - sh;
        r2 = sq * cos(th - FUND_2PI_3) - sh;
        swap_if(r1 < r0, r0, r1);            // ascending: a three-element network of selects
        swap_if(r2 < r1, r1, r2);
        swap_if(r1 < r0, r0, r1);
        nr = 3;
    } else {
        double e = cbrt(sqrt(-disc) + fabs(R));
        if (R > 0.0) e = -e;
        r0 = (e + Q / e) - a1 * (1.0 / 3.0);
        nr = 1;
    }
    const double T1x = -s1 * m1x, T1y = -s1 * m1y, T2x = -s2 * m2x, T2y = -s2 * m2y;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k >= nr) break;
        double lam = k == 0 ? r0 : (k == 1 ? r1 : r2), mu = 1.0;
        const double s = f1[8] * lam + f2[8];
        double Fn[9];
        Fn[8] = 0.0;
        if (fabs(s) > DBL_EPSILON) {
            mu = 1.0 / s;
            lam = lam * mu;
            Fn[8] = 1.0;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) Fn[i] = f1[i] * lam + f2[i] * mu;
        // F = T2^T Fn T1, T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]
        double M[9], F[9];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            M[j] = s2 * Fn[j];
            M[3 + j] = s2 * Fn[3 + j];
            M[6 + j] = (T2x * Fn[j] + T2y * Fn[3 + j]) + Fn[6 + j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            F[i * 3 + 0] = M[i * 3 + 0] * s1;
            F[i * 3 + 1] = M[i * 3 + 1] * s1;
            F[i * 3 + 2] = (M[i * 3 + 0] * T1x + M[i * 3 + 1] * T1y) + M[i * 3 + 2];
        }
        if (fabs(F[8]) > (double)FLT_EPSILON) {
            const double inv = 1.0 / F[8];
#pragma unroll
            for (int i = 0; i < 9; i++) F[i] = F[i] * inv;
        }
#pragma unroll
        for (int i = 0; i < 9; i++) {
            fin &= isfinite(F[i]);
            out[k * 9 + i] = F[i];
        }
    }
    if (!fin) {
#pragma unroll
        for (int e = 0; e < 27; e++) out[e] = 0.0;
        return 0;
    }
    return nr;
}

// G = A2^T F A1 (A = [[d, 0, cx], [0, d, cy], [0, 0, 1]]), scaled to max|G_ij| = 1, rounded to fp32
__device__ __forceinline__ void fund_condition(const double* F, const double* cd, float* G) {
    const double c1x = cd[0], c1y = cd[1], d1 = cd[2], c2x = cd[3], c2y = cd[4], d2 = cd[5];
    double M[9], g[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        M[j] = d2 * F[j];
        M[3 + j] = d2 * F[3 + j];
        M[6 + j] = (c2x * F[j] + c2y * F[3 + j]) + F[6 + j];
    }
    double gmax = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        g[i * 3 + 0] = M[i * 3 + 0] * d1;
        g[i * 3 + 1] = M[i * 3 + 1] * d1;
        g[i * 3 + 2] = (M[i * 3 + 0] * c1x + M[i * 3 + 1] * c1y) + M[i * 3 + 2];
        gmax = fmax(gmax, fmax(fabs(g[i * 3]), fmax(fabs(g[i * 3 + 1]), fabs(g[i * 3 + 2]))));
    }
    const double inv = (gmax > 0.0 && isfinite(gmax)) ? 1.0 / gmax : 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) G[i] = (float)(g[i] * inv);
}

// ---- stage: validate, pixel points, per-pair conditioning ---------------------------------------------------------------
__global__ __launch_bounds__(FUND_STAGE_BLOCK) void k_fund_stage(const aria_keypoint* __restrict__ kq, const int* __restrict__ nq,
                                                                 const aria_keypoint* __restrict__ kt, const int* __restrict__ nt,
                                                                 int64_t kp_stride, const aria_match* __restrict__ matches,
                                                                 const int* __restrict__ nmatches, int match_cap, int query_is_first,
                                                                 float4* __restrict__ pix, float4* __restrict__ pts,
                                                                 double* __restrict__ cond, int* __restrict__ npts,
                                                                 int* __restrict__ err) {
    __shared__ int bad;
    __shared__ double red[6][FUND_STAGE_BLOCK];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = nmatches[p], nqp = nq[p], ntp = nt[p];
    if (tid == 0) bad = (n < 0 || n > match_cap || nqp < 0 || nqp > kp_stride || ntp < 0 || ntp > kp_stride) ? 1 : 0;
    __syncthreads();
    const aria_match* m = matches + (int64_t)p * match_cap;
    if (!bad) {
        int mine = 0;
        for (int i = tid; i < n; i += FUND_STAGE_BLOCK) {
            const aria_match a = m[i];
            mine |= (a.query_idx < 0 || a.query_idx >= nqp || a.train_idx < 0 || a.train_idx >= ntp);
        }
        if (mine) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) {
            npts[p] = 0;
            atomicOr(err, ERRBIT_FUND_INPUT);
        }
        return;
    }
    if (tid == 0) npts[p] = n;
    if (n < FUND_MIN_MATCHES) return;
    const aria_keypoint* q = kq + (int64_t)p * kp_stride;
    const aria_keypoint* t = kt + (int64_t)p * kp_stride;
    float4* px = pix + (int64_t)p * match_cap;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += FUND_STAGE_BLOCK) {
        const aria_match a = m[i];
        const aria_keypoint k1 = query_is_first ? q[a.query_idx] : t[a.train_idx];
        const aria_keypoint k2 = query_is_first ? t[a.train_idx] : q[a.query_idx];
        const double x1 = k1.x, y1 = k1.y, x2 = k2.x, y2 = k2.y;
        s[0] = s[0] + x1; s[1] = s[1] + y1; s[2] = s[2] + (x1 * x1 + y1 * y1);
        s[3] = s[3] + x2; s[4] = s[4] + y2; s[5] = s[5] + (x2 * x2 + y2 * y2);
        px[i] = make_float4(k1.x, k1.y, k2.x, k2.y);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) red[k][tid] = s[k];
    __syncthreads();
    for (int w = FUND_STAGE_BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 6; k++) red[k][tid] = red[k][tid] + red[k][tid + w];
        }
        __syncthreads();
    }
    const double inv = 1.0 / (double)n;
    double cd[6];
#pragma unroll
    for (int v = 0; v < 2; v++) {
        const double cx = red[3 * v][0] * inv, cy = red[3 * v + 1][0] * inv;
        double d = sqrt(fmax(red[3 * v + 2][0] * inv - (cx * cx + cy * cy), 0.0));
        if (!(d >= 1.0)) d = 1.0;
        cd[3 * v] = cx; cd[3 * v + 1] = cy; cd[3 * v + 2] = d;
    }
    if (tid < 6) cond[(int64_t)p * FUND_COND + tid] = cd[tid];
    float4* o = pts + (int64_t)p * match_cap;
    for (int i = tid; i < n; i += FUND_STAGE_BLOCK) {
        const float4 a = px[i];              // written by this thread above
        o[i] = make_float4((float)(((double)a.x - cd[0]) / cd[2]), (float)(((double)a.y - cd[1]) / cd[2]),
                           (float)(((double)a.z - cd[3]) / cd[5]), (float)(((double)a.w - cd[4]) / cd[5]));
    }
}

// ---- hypotheses: sample + 7-point solve ---------------------------------------------------------------------------------
// F (fp64) and G (fp32) are structure-of-arrays per pair: X[(p * 27 + k * 9 + e) * H + h]; nmod[p * H + h] = 0, 1 or 3.
__global__ __launch_bounds__(64) void k_fund_hyp(const float4* __restrict__ pix, const int* __restrict__ npts,
                                                 const double* __restrict__ cond, int match_cap, int H, uint64_t seed, int pair_base,
                                                 double* __restrict__ Fo, float* __restrict__ Go, int* __restrict__ nmod,
                                                 int* __restrict__ dbg_idx) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int n = npts[p];
    bool ok = n >= FUND_MIN_MATCHES;
    int idx[7];
#pragma unroll
    for (int j = 0; j < 7; j++) idx[j] = -1;
    if (ok) ok = draw_sample<7, FUND_MAX_RETRY>(seed, (uint32_t)(pair_base + p), h, n, idx);
    if (dbg_idx) {
#pragma unroll
        for (int j = 0; j < 7; j++) dbg_idx[h * 7 + j] = idx[j];
    }
    double F[27];
    int nm = 0;
    if (ok) {
        const float4* pp = pix + (int64_t)p * match_cap;
        double x1[7], y1[7], x2[7], y2[7];
#pragma unroll
        for (int r = 0; r < 7; r++) {
            const float4 q = pp[idx[r]];
            x1[r] = q.x; y1[r] = q.y; x2[r] = q.z; y2[r] = q.w;
        }
        nm = fund_solve7(x1, y1, x2, y2, F);
    } else {
#pragma unroll
        for (int e = 0; e < 27; e++) F[e] = 0.0;
    }
    double cd[6];
#pragma unroll
    for (int k = 0; k < 6; k++) cd[k] = nm ? cond[(int64_t)p * FUND_COND + k] : 1.0;
    const int64_t base = (int64_t)p * 27 * H + h;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float G[9];
        fund_condition(F + k * 9, cd, G);
#pragma unroll
        for (int e = 0; e < 9; e++) {
            Fo[base + (int64_t)(k * 9 + e) * H] = F[k * 9 + e];
            Go[base + (int64_t)(k * 9 + e) * H] = k < nm ? G[e] : 0.0f;
        }
    }
    nmod[(int64_t)p * H + h] = nm;
}

// ---- scoring: the hot loop ----------------------------------------------------------------------------------------------
// cnt[(p * H + h) * 3 + k]: inliers of model k, -1 for k >= nmod
__global__ __launch_bounds__(FUND_SCORE_BLOCK) void k_fund_score(const float4* __restrict__ pts, const int* __restrict__ npts,
                                                                 const double* __restrict__ cond, int match_cap, int H,
                                                                 const float* __restrict__ G, const int* __restrict__ nmod,
                                                                 int* __restrict__ cnt, double thr) {
    __shared__ float4 tile[FUND_TILE];
    const int p = blockIdx.x;
    const int h = blockIdx.y * FUND_SCORE_BLOCK + threadIdx.x;
    const int n = npts[p];
    const int nn = n >= FUND_MIN_MATCHES ? n : 0;
    const int nm = (h < H && nn) ? nmod[(int64_t)p * H + h] : 0;
    float g[27];
    const float* Gp = G + (int64_t)p * 27 * H + h;
#pragma unroll
    for (int e = 0; e < 27; e++) g[e] = nm ? Gp[(int64_t)e * H] : 0.0f;
    float t1 = 0.0f, t2 = 0.0f;
    if (nn) {
        t1 = fund_thr(thr, cond[(int64_t)p * FUND_COND + 2]);
        t2 = fund_thr(thr, cond[(int64_t)p * FUND_COND + 5]);
    }
    const float4* pp = pts + (int64_t)p * match_cap;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int base = 0; base < nn; base += FUND_TILE) {
        const int m = min(FUND_TILE, nn - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += FUND_SCORE_BLOCK) tile[i] = pp[base + i];
        __syncthreads();
        if (nm) {
            for (int i = 0; i < m; i++) {
                const float4 q = tile[i];
                c0 += fund_inlier(g, q, t1, t2);
                c1 += fund_inlier(g + 9, q, t1, t2);
                c2 += fund_inlier(g + 18, q, t1, t2);
            }
        }
    }
    if (h < H) {
        int* o = cnt + ((int64_t)p * H + h) * 3;
        o[0] = nm > 0 ? c0 : -1;
        o[1] = nm > 1 ? c1 : -1;
        o[2] = nm > 2 ? c2 : -1;
    }
}

// ---- finish: winner, mask, compaction -----------------------------------------------------------------------------------
__global__ __launch_bounds__(FUND_FINISH_BLOCK) void k_fund_finish(const float4* __restrict__ pts, const int* __restrict__ npts,
                                                                   const double* __restrict__ cond, int match_cap, int H,
                                                                   const double* __restrict__ F, const float* __restrict__ G,
                                                                   const int* __restrict__ nmod, const int* __restrict__ cnt,
                                                                   double thr, const aria_match* __restrict__ matches,
                                                                   uint8_t* __restrict__ mask, aria_match* __restrict__ inl,
                                                                   int* __restrict__ ninl, aria_fund_result* __restrict__ out) {
    constexpr int NW = FUND_FINISH_BLOCK / 64;
    __shared__ int red_c[FUND_FINISH_BLOCK], red_i[FUND_FINISH_BLOCK];
    __shared__ int n_models, wave_n[NW];
    __shared__ float Gw[9];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = npts[p];
    if (tid == 0) n_models = 0;
    // argmax over (count, -(3 h + k)): ascending scan per lane, then a fixed tree
    int bc = -1, bi = -1, nms = 0;
    if (n >= FUND_MIN_MATCHES) {
        for (int h = tid; h < H; h += FUND_FINISH_BLOCK) {
            nms += nmod[(int64_t)p * H + h];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int c = cnt[((int64_t)p * H + h) * 3 + k];
                if (c > bc) { bc = c; bi = h * 3 + k; }
            }
        }
    }
    red_c[tid] = bc;
    red_i[tid] = bi;
    __syncthreads();
    atomicAdd(&n_models, nms);
    for (int s = FUND_FINISH_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int c2 = red_c[tid + s], i2 = red_i[tid + s];
            if (c2 > red_c[tid] || (c2 == red_c[tid] && c2 >= 0 && i2 < red_i[tid])) { red_c[tid] = c2; red_i[tid] = i2; }
        }
        __syncthreads();
    }
    const int win_c = red_c[0], win_i = red_i[0];
    const bool valid = n >= FUND_MIN_MATCHES && win_c >= FUND_MIN_INLIERS;
    aria_fund_result* o = out + p;
    uint8_t* mk = mask ? mask + (int64_t)p * match_cap : nullptr;
    aria_match* il = inl ? inl + (int64_t)p * match_cap : nullptr;
    if (!valid) {
        for (int i = tid; i < match_cap; i += FUND_FINISH_BLOCK) {
            if (mk) mk[i] = 0;
            if (il) il[i] = aria_match{0, 0, 0.0f};
        }
        if (tid == 0) {
            for (int k = 0; k < 9; k++) o->F[k] = 0.0;
            o->n_matches = n; o->n_inliers = 0; o->n_models = 0; o->best_hypothesis = -1; o->best_root = -1; o->valid = 0;
            if (ninl) ninl[p] = 0;
        }
        return;
    }
    const int win_h = win_i / 3, win_k = win_i % 3;
    const int64_t wbase = (int64_t)p * 27 * H + (int64_t)(win_k * 9) * H + win_h;
    if (tid < 9) Gw[tid] = G[wbase + (int64_t)tid * H];
    __syncthreads();
    float g[9];
#pragma unroll
    for (int e = 0; e < 9; e++) g[e] = Gw[e];
    const float t1 = fund_thr(thr, cond[(int64_t)p * FUND_COND + 2]);
    const float t2 = fund_thr(thr, cond[(int64_t)p * FUND_COND + 5]);
    const float4* pp = pts + (int64_t)p * match_cap;
    const aria_match* m = matches + (int64_t)p * match_cap;
    // the winner's inliers (the same test, on the same fp32 G, as its score), compacted in match order
    int run = 0;
    for (int c0 = 0; c0 < match_cap; c0 += FUND_FINISH_BLOCK) {
        const int i = c0 + tid;
        const int in = i < n ? fund_inlier(g, pp[i], t1, t2) : 0;
        if (mk && i < match_cap) mk[i] = (uint8_t)in;
        const uint64_t b = __ballot(in);
        const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (lane == 0) wave_n[wv] = __popcll(b);
        __syncthreads();
        int off = run, tot = 0;
        for (int w = 0; w < NW; w++) {
            off += w < wv ? wave_n[w] : 0;
            tot += wave_n[w];
        }
        if (il && in) il[off + __popcll(b & below)] = m[i];
        __syncthreads();
        run += tot;
    }
    if (il)
        for (int i = run + tid; i < match_cap; i += FUND_FINISH_BLOCK) il[i] = aria_match{0, 0, 0.0f};
    if (tid == 0) {
        for (int k = 0; k < 9; k++) o->F[k] = F[wbase + (int64_t)k * H];
        o->n_matches = n; o->n_inliers = run; o->n_models = n_models; o->best_hypothesis = win_h; o->best_root = win_k;
        o->valid = 1;
        if (ninl) ninl[p] = run;
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_fund_s : StageHandle {
    aria_fund_config cfg{};
    // grow-only workspace of the batch path
    DeviceBuffer<float4> d_pix;           // [n_pairs][match_cap] pixel points
    DeviceBuffer<float4> d_pts;           // [n_pairs][match_cap] conditioned points
    DeviceBuffer<double> d_cond;          // [n_pairs][8]
    DeviceBuffer<int> d_npts;             // [n_pairs]
    DeviceBuffer<double> d_F;             // [n_pairs][27][H]
    DeviceBuffer<float> d_G;              // [n_pairs][27][H]
    DeviceBuffer<int> d_nmod;             // [n_pairs][H]
    DeviceBuffer<int> d_cnt;              // [n_pairs][H][3]
    PairStaging pair;                     // aria_fund_estimate, aria_fund_debug_hypotheses
    DeviceBuffer<aria_fund_result> d_res;
    DeviceBuffer<int> d_dbg;
};

namespace {

int fund_enqueue(aria_fund_t h, const aria_keypoint* d_kq, const int* d_nq, const aria_keypoint* d_kt, const int* d_nt,
                 int64_t kp_stride, const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                 int query_is_first, int pair_base, aria_fund_result* d_out, uint8_t* d_mask, aria_match* d_inl, int* d_ninl,
                 int* d_dbg, bool finish) {
    const int H = h->cfg.hypotheses;
    const size_t P = (size_t)n_pairs;
    int rc;
    if ((rc = h->d_pix.reserve(h->stream, P * match_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_pts.reserve(h->stream, P * match_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_cond.reserve(h->stream, P * FUND_COND)) != ARIA_OK) return rc;
    if ((rc = h->d_npts.reserve(h->stream, P)) != ARIA_OK) return rc;
    if ((rc = h->d_F.reserve(h->stream, P * H * 27)) != ARIA_OK) return rc;
    if ((rc = h->d_G.reserve(h->stream, P * H * 27)) != ARIA_OK) return rc;
    if ((rc = h->d_nmod.reserve(h->stream, P * H)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, P * H * 3)) != ARIA_OK) return rc;
    const aria_fund_config& c = h->cfg;
    hipLaunchKernelGGL(k_fund_stage, dim3(n_pairs), dim3(FUND_STAGE_BLOCK), 0, h->stream, d_kq, d_nq, d_kt, d_nt, kp_stride,
                       d_matches, d_nmatches, match_cap, query_is_first ? 1 : 0, h->d_pix, h->d_pts, h->d_cond, h->d_npts,
                       h->d_err);
    hipLaunchKernelGGL(k_fund_hyp, dim3(n_pairs, H / 64), dim3(64), 0, h->stream, h->d_pix, h->d_npts, h->d_cond, match_cap, H,
                       (uint64_t)c.seed, pair_base, h->d_F, h->d_G, h->d_nmod, d_dbg);
    hipLaunchKernelGGL(k_fund_score, dim3(n_pairs, (H + FUND_SCORE_BLOCK - 1) / FUND_SCORE_BLOCK), dim3(FUND_SCORE_BLOCK), 0,
                       h->stream, h->d_pts, h->d_npts, h->d_cond, match_cap, H, h->d_G, h->d_nmod, h->d_cnt, c.threshold_px);
    if (finish)
        hipLaunchKernelGGL(k_fund_finish, dim3(n_pairs), dim3(FUND_FINISH_BLOCK), 0, h->stream, h->d_pts, h->d_npts, h->d_cond,
                           match_cap, H, h->d_F, h->d_G, h->d_nmod, h->d_cnt, c.threshold_px, d_matches, d_mask, d_inl, d_ninl,
                           d_out);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

// the batch form over the one staged pair
int fund_enqueue_staged(aria_fund_t h, int query_is_first, int pair_base, int* d_dbg, bool finish) {
    const PairStaging& s = h->pair;
    return fund_enqueue(h, s.d_kq, s.d_counts, s.d_kt, s.d_counts + 1, s.kp_stride, s.d_m, s.d_counts + 2, 1, s.match_cap,
                        query_is_first, pair_base, finish ? h->d_res.p : nullptr, finish ? s.d_mask.p : nullptr, nullptr, nullptr,
                        d_dbg, finish);
}

}  // namespace

extern "C" {

void aria_fund_default_config(aria_fund_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_fund_config);
    c->device = 0;
    c->stream = nullptr;
    c->hypotheses = 1024;
    c->threshold_px = 3.0;                 // findFundamentalMat(..., FM_RANSAC, 3.0, 0.99), LoopClosure.cpp:143
    c->seed = 0;
}

int aria_fund_create(const aria_fund_config* c, aria_fund_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_fund_config)) return ARIA_E_INVALID;
    if (c->hypotheses < 64 || c->hypotheses > 16384 || (c->hypotheses % 64)) return ARIA_E_INVALID;
    if (!(c->threshold_px > 0) || !std::isfinite(c->threshold_px)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_fund_create", [](aria_fund_s* h) {
        const int rc = h->pair.create(h->stream);
        return rc != ARIA_OK ? rc : h->d_res.reserve(h->stream, 1, "aria_fund_create");
    });
}

void aria_fund_destroy(aria_fund_t h) { stage_destroy(h); }

void* aria_fund_stream(aria_fund_t h) { return stage_stream(h); }

int aria_fund_check(aria_fund_t h) { return stage_check(h, {{ERRBIT_FUND_INPUT, ARIA_E_INVALID}}); }

int aria_fund_estimate_batch_device(aria_fund_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                    const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                    const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                    int query_is_first, int pair_base, aria_fund_result* d_out, uint8_t* d_mask,
                                    aria_match* d_inliers, int* d_ninliers) {
    if (!h || !d_kp_query || !d_nq || !d_kp_train || !d_nt || !d_matches || !d_nmatches || !d_out || n_pairs < 0 ||
        match_cap < 1 || match_cap > (1 << 20) || kp_stride < 0 || pair_base < 0 || (!d_inliers) != (!d_ninliers))
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return fund_enqueue(h, d_kp_query, d_nq, d_kp_train, d_nt, kp_stride, d_matches, d_nmatches, n_pairs, match_cap,
                        query_is_first, pair_base, d_out, d_mask, d_inliers, d_ninliers, nullptr, true);
}

int aria_fund_estimate(aria_fund_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                       const aria_match* matches, int n_matches, int query_is_first, int pair_base, aria_fund_result* out,
                       uint8_t* mask) {
    if (!h || !out || pair_base < 0 || n_matches > (1 << 20)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->pair.upload(h->stream, kp_query, nq, kp_train, nt, matches, n_matches);
    if (rc != ARIA_OK) return rc;
    if ((rc = fund_enqueue_staged(h, query_is_first, pair_base, nullptr, true)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(out, h->d_res, sizeof(aria_fund_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && n_matches) ARIA_HIP(hipMemcpyAsync(mask, h->pair.d_mask, (size_t)n_matches, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_fund_check(h);
}

int aria_fund_debug_hypotheses(aria_fund_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                               const aria_match* matches, int n_matches, int query_is_first, int pair_base, int* sample_idx,
                               int* n_models, double* F, int* counts) {
    if (!h || !sample_idx || !n_models || !F || !counts || pair_base < 0 || n_matches > (1 << 20)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->pair.upload(h->stream, kp_query, nq, kp_train, nt, matches, n_matches);
    if (rc != ARIA_OK) return rc;
    const int H = h->cfg.hypotheses;
    if ((rc = h->d_dbg.reserve(h->stream, (size_t)H * 7)) != ARIA_OK) return rc;
    if ((rc = fund_enqueue_staged(h, query_is_first, pair_base, h->d_dbg, false)) != ARIA_OK) return rc;
    std::vector<double> soa((size_t)27 * H);
    ARIA_HIP(hipMemcpyAsync(sample_idx, h->d_dbg, sizeof(int) * 7 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(n_models, h->d_nmod, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(soa.data(), h->d_F, sizeof(double) * 27 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(counts, h->d_cnt, sizeof(int) * 3 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    unpack_models(soa.data(), H, 0, 27, F);
    return aria_fund_check(h);
}

}  // extern "C"
