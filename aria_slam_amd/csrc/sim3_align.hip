// Loop alignment on the device: the similarity X2 = s R X1 + t between the landmarks two keyframes own -- Sim(3) RANSAC
// (three-point closed form in fp64, two-sided fp32 reprojection scoring, Gauss-Newton over (w, v, sigma) on the winner's
// inliers), batched over pairs, and the join of a match list with the point map that feeds it. Semantics in
// include/aria_orb_hip.h ("loop alignment"); aria_slam_amd/sim3_ref.py restates every step in NumPy and is the definition.
//
// Four launches on the handle's stream, in the manner of pnp_ransac.hip:
//   k_sim3_stage   one workgroup per pair: the count check BEFORE any correspondence is read, the finiteness scan BEFORE any
//                  arithmetic, then the scoring values in fp32 as three planes: (X1, x1.x), (X2, x2.x), (x1.y, x2.y)
//   k_sim3_hyp     a lane per hypothesis, 256 hypotheses of one pair per workgroup: sample of 3, the closed form -- all 3x3
//                  code written out with constant indices. No LDS, no scratch
//   k_sim3_score   a lane per hypothesis, 256 hypotheses per workgroup, the model (13 floats) in registers, the pair's
//                  correspondences staged in LDS tiles of SIM3_TILE (40 B each, 80 KiB) and read as a broadcast: integer
//                  inlier counts, the tail tile exact. No scratch
//   k_sim3_finish  one workgroup per pair: argmax over (count, -h), the winner's closed form again in one lane, Gauss-Newton
//                  (28 + 7 sums in fp64, strided per-thread sums + the fixed reductions of solver_device.h, 7x7 Cholesky in
//                  one lane), rescoring, mask, rms_px
// The association is three launches: the PnP join's table fill twice (integer atomicMin of the arena position, one table
// per keyframe) and a lane per match with the wave-ordered compaction of ransac_device.h.
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

constexpr int SIM3_TILE = 2048;            // correspondences per LDS tile of k_sim3_score (32 + 32 + 16 KiB)
constexpr int SIM3_BLOCK = 256;            // every kernel's workgroup
constexpr int SIM3_WAVES = SIM3_BLOCK / 64;
constexpr int SIM3_MAX_RETRY = 256;
constexpr int SIM3_MIN = 3;                // correspondences of a sample
constexpr int SIM3_MIN_REFINE = 4;         // the least inliers a refinement starts from
constexpr int SIM3_MODEL = 13;             // R (9), t (3), s
constexpr int SIM3_EXP_TERMS = 12;
constexpr double SIM3_AREA_TOL = 1e-12;    // |(Xb - Xa) x (Xc - Xa)|^2 <= tol * max(side^2)^2: collinear or coincident sample
constexpr double SIM3_RANGE = 1e15;        // scoring values and |t| beyond this never score
constexpr double SIM3_STEP_TOL = 1e-12;
constexpr int SIM3_EMPTY = 0x7F7F7F7F;     // association tables: no map point (the fill byte 0x7F)
constexpr int ERRBIT_SIM3_INPUT = 1;       // a pair's counts, values or match indices were refused (pair skipped)

struct S3 {
    double x, y, z;
};
__device__ __forceinline__ S3 s3_sub(S3 a, S3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ S3 s3_cross(S3 a, S3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double s3_dot(S3 a, S3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ bool s3_degenerate(S3 a, S3 b, S3 c) {
    const S3 e1 = s3_sub(b, a), e2 = s3_sub(c, a), e3 = s3_sub(c, b);
    const S3 n = s3_cross(e1, e2);
    const double amax = fmax(fmax(s3_dot(e1, e1), s3_dot(e2, e2)), s3_dot(e3, e3));
    return !(s3_dot(n, n) > SIM3_AREA_TOL * (amax * amax));
}

__device__ __forceinline__ bool sim3_finite(const double* v, int n) {
    bool ok = true;
    for (int k = 0; k < n; k++) ok &= isfinite(v[k]);
    return ok;
}

// The three-point closed form, sim3_ref.solve_minimal line by line: every sum in its order, no contraction.
__device__ __forceinline__ bool sim3_solve(const aria_sim3_corr& qa, const aria_sim3_corr& qb, const aria_sim3_corr& qc, int fix_scale,
                                           double min_scale, double max_scale, double R[9], double t[3], double& s) {
    const S3 A0 = {qa.X1[0], qa.X1[1], qa.X1[2]}, A1 = {qb.X1[0], qb.X1[1], qb.X1[2]}, A2 = {qc.X1[0], qc.X1[1], qc.X1[2]};
    const S3 B0 = {qa.X2[0], qa.X2[1], qa.X2[2]}, B1 = {qb.X2[0], qb.X2[1], qb.X2[2]}, B2 = {qc.X2[0], qc.X2[1], qc.X2[2]};
    bool ok = !s3_degenerate(A0, A1, A2) && !s3_degenerate(B0, B1, B2);
    const S3 c1 = {((A0.x + A1.x) + A2.x) / 3.0, ((A0.y + A1.y) + A2.y) / 3.0, ((A0.z + A1.z) + A2.z) / 3.0};
    const S3 c2 = {((B0.x + B1.x) + B2.x) / 3.0, ((B0.y + B1.y) + B2.y) / 3.0, ((B0.z + B1.z) + B2.z) / 3.0};
    const S3 q0 = s3_sub(A0, c1), q1 = s3_sub(A1, c1), q2 = s3_sub(A2, c1);
    const S3 p0 = s3_sub(B0, c2), p1 = s3_sub(B1, c2), p2 = s3_sub(B2, c2);
    const double P[3][3] = {{p0.x, p0.y, p0.z}, {p1.x, p1.y, p1.z}, {p2.x, p2.y, p2.z}};
    const double Q[3][3] = {{q0.x, q0.y, q0.z}, {q1.x, q1.y, q1.z}, {q2.x, q2.y, q2.z}};
    double M[9], G[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r * 3 + c] = (P[0][r] * Q[0][c] + P[1][r] * Q[1][c]) + P[2][r] * Q[2][c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) G[r * 3 + c] = (M[r] * M[c] + M[3 + r] * M[3 + c]) + M[6 + r] * M[6 + c];
    jacobi3(G, V);
    double l0 = G[0], l1 = G[4], l2 = G[8];
    double a0 = V[0], a1 = V[3], a2 = V[6];   // columns as (x, y, z)
    double b0 = V[1], b1 = V[4], b2 = V[7];
    double c0 = V[2], c1v = V[5], c2v = V[8];
    bool sw = l1 > l0;
    swap_if(sw, l0, l1); swap_if(sw, a0, b0); swap_if(sw, a1, b1); swap_if(sw, a2, b2);
    sw = l2 > l1;
    swap_if(sw, l1, l2); swap_if(sw, b0, c0); swap_if(sw, b1, c1v); swap_if(sw, b2, c2v);
    sw = l1 > l0;
    swap_if(sw, l0, l1); swap_if(sw, a0, b0); swap_if(sw, a1, b1); swap_if(sw, a2, b2);
    const double sig1 = sqrt(fmax(l0, 0.0)), sig2 = sqrt(fmax(l1, 0.0));
    const double v1[3] = {a0, a1, a2}, v2[3] = {b0, b1, b2};
    double u1[3], u2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        u1[r] = ((M[3 * r] * v1[0] + M[3 * r + 1] * v1[1]) + M[3 * r + 2] * v1[2]) / sig1;
        u2[r] = ((M[3 * r] * v2[0] + M[3 * r + 1] * v2[1]) + M[3 * r + 2] * v2[2]) / sig2;
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
    s = 1.0;
    if (!fix_scale) {
        const double den = (s3_dot(q0, q0) + s3_dot(q1, q1)) + s3_dot(q2, q2);
        s = (sig1 + sig2) / den;
        ok &= s >= min_scale && s <= max_scale;
    }
    t[0] = c2.x - s * ((R[0] * c1.x + R[1] * c1.y) + R[2] * c1.z);
    t[1] = c2.y - s * ((R[3] * c1.x + R[4] * c1.y) + R[5] * c1.z);
    t[2] = c2.z - s * ((R[6] * c1.x + R[7] * c1.y) + R[8] * c1.z);
    ok &= sim3_finite(R, 9) && sim3_finite(t, 3) && isfinite(s);
    ok &= fabs(t[0]) <= SIM3_RANGE && fabs(t[1]) <= SIM3_RANGE && fabs(t[2]) <= SIM3_RANGE;
    return ok;
}

// The model as scored: fp32, false when a value is not finite or |t| is beyond SIM3_RANGE (sim3_ref.scored_model).
__device__ __forceinline__ bool sim3_round(const double R[9], const double t[3], double s, float m[SIM3_MODEL]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) { m[k] = (float)R[k]; ok &= isfinite(m[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { m[9 + k] = (float)t[k]; ok &= fabsf(m[9 + k]) <= (float)SIM3_RANGE; }
    m[12] = (float)s;
    ok &= isfinite(m[12]);
    return ok;
}

// The two-sided reprojection test, division-free, every sum left to right. a = (X1, x1.x), b = (X2, x2.x), c = (x1.y, x2.y);
// m = R (9), t (3), s. Y2 = s R X1 + t against x2; Y1 = R^T (X2 - t) against x1.
__device__ __forceinline__ int sim3_inlier(const float m[SIM3_MODEL], float4 a, float4 b, float2 c, float thr2) {
    const float X = m[12] * ((m[0] * a.x + m[1] * a.y) + m[2] * a.z) + m[9];
    const float Y = m[12] * ((m[3] * a.x + m[4] * a.y) + m[5] * a.z) + m[10];
    const float Z = m[12] * ((m[6] * a.x + m[7] * a.y) + m[8] * a.z) + m[11];
    const float ex = X - b.w * Z, ey = Y - c.y * Z;
    const bool in2 = Z > 0.0f && ex * ex + ey * ey <= thr2 * (Z * Z);
    const float d0 = b.x - m[9], d1 = b.y - m[10], d2 = b.z - m[11];
    const float U = (m[0] * d0 + m[3] * d1) + m[6] * d2;
    const float V = (m[1] * d0 + m[4] * d1) + m[7] * d2;
    const float W = (m[2] * d0 + m[5] * d1) + m[8] * d2;
    const float fx = U - a.w * W, fy = V - c.x * W;
    const bool in1 = W > 0.0f && fx * fx + fy * fy <= thr2 * (W * W);
    return (in2 && in1) ? 1 : 0;
}

// ---- stage: count check, finiteness scan, the scoring planes ----------------------------------------------------------------
__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_stage(const aria_sim3_corr* __restrict__ corr, const int* __restrict__ ncorr,
                                                           int corr_cap, double fx, double fy, double cx, double cy,
                                                           float4* __restrict__ pa, float4* __restrict__ pb, float2* __restrict__ pc,
                                                           int* __restrict__ npts, int* __restrict__ err) {
    __shared__ int bad;
    const int p = blockIdx.x;
    const int n = ncorr[p];
    if (n < 0 || n > corr_cap) {             // uniform over the workgroup
        if (threadIdx.x == 0) {
            npts[p] = 0;
            atomicOr(err, ERRBIT_SIM3_INPUT);
        }
        return;
    }
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const aria_sim3_corr* cp = corr + (int64_t)p * corr_cap;
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += SIM3_BLOCK) {
        const aria_sim3_corr c = cp[i];
        const bool fin = isfinite(c.X1[0]) && isfinite(c.X1[1]) && isfinite(c.X1[2]) && isfinite(c.X2[0]) && isfinite(c.X2[1]) &&
                         isfinite(c.X2[2]) && isfinite(c.u1) && isfinite(c.v1) && isfinite(c.u2) && isfinite(c.v2);
        mine |= fin ? 0 : 1;
    }
    if (mine) atomicOr(&bad, 1);
    __syncthreads();
    if (bad) {                               // uniform: read after the barrier
        if (threadIdx.x == 0) {
            npts[p] = 0;
            atomicOr(err, ERRBIT_SIM3_INPUT);
        }
        return;
    }
    if (threadIdx.x == 0) npts[p] = n;
    float4* oa = pa + (int64_t)p * corr_cap;
    float4* ob = pb + (int64_t)p * corr_cap;
    float2* oc = pc + (int64_t)p * corr_cap;
    const float lim = (float)SIM3_RANGE;
    for (int i = threadIdx.x; i < n; i += SIM3_BLOCK) {
        const aria_sim3_corr c = cp[i];
        float4 a = make_float4((float)c.X1[0], (float)c.X1[1], (float)c.X1[2], (float)(((double)c.u1 - cx) / fx));
        float4 b = make_float4((float)c.X2[0], (float)c.X2[1], (float)c.X2[2], (float)(((double)c.u2 - cx) / fx));
        float2 y = make_float2((float)(((double)c.v1 - cy) / fy), (float)(((double)c.v2 - cy) / fy));
        const bool ok = fabsf(a.x) <= lim && fabsf(a.y) <= lim && fabsf(a.z) <= lim && fabsf(a.w) <= lim && fabsf(b.x) <= lim &&
                        fabsf(b.y) <= lim && fabsf(b.z) <= lim && fabsf(b.w) <= lim && fabsf(y.x) <= lim && fabsf(y.y) <= lim;
        if (!ok) {
            const float q = __builtin_nanf("");
            a = make_float4(q, q, q, q);
            b = a;
            y = make_float2(q, q);
        }
        oa[i] = a;
        ob[i] = b;
        oc[i] = y;
    }
}

// ---- hypotheses: sample of 3 + the closed form, a lane per hypothesis ---------------------------------------------------------
// The model in fp32, structure-of-arrays per pair: Ms[(p * 13 + k) * H + h], k = 0..8 R, 9..11 t, 12 s; cnt[p * H + h] = 0
// (valid, to be scored) or -1.
__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_hyp(const aria_sim3_corr* __restrict__ corr, const int* __restrict__ npts,
                                                         int corr_cap, int H, uint64_t seed, int pair_base, int fix_scale,
                                                         double min_scale, double max_scale, float* __restrict__ Ms,
                                                         int* __restrict__ cnt, int* __restrict__ dbg_idx) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * SIM3_BLOCK + threadIdx.x;
    if (h >= H) return;
    const int n = npts[p];
    bool ok = n >= SIM3_MIN;
    int idx[3] = {-1, -1, -1};
    if (ok) ok = draw_sample<3, SIM3_MAX_RETRY>(seed, (uint32_t)(pair_base + p), h, n, idx);
    if (dbg_idx) {
#pragma unroll
        for (int j = 0; j < 3; j++) dbg_idx[h * 3 + j] = idx[j];
    }
    float m[SIM3_MODEL];
#pragma unroll
    for (int k = 0; k < SIM3_MODEL; k++) m[k] = 0.0f;
    if (ok) {
        const aria_sim3_corr* cp = corr + (int64_t)p * corr_cap;
        double R[9], t[3], s;
        ok = sim3_solve(cp[idx[0]], cp[idx[1]], cp[idx[2]], fix_scale, min_scale, max_scale, R, t, s);
        float f[SIM3_MODEL];
        ok &= sim3_round(R, t, s, f);
#pragma unroll
        for (int k = 0; k < SIM3_MODEL; k++) m[k] = ok ? f[k] : 0.0f;
    }
    float* Mp = Ms + (int64_t)p * SIM3_MODEL * H;
#pragma unroll
    for (int k = 0; k < SIM3_MODEL; k++) Mp[(int64_t)k * H + h] = m[k];
    cnt[(int64_t)p * H + h] = ok ? 0 : -1;
}

// ---- scoring: the hot loop ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_score(const float4* __restrict__ pa, const float4* __restrict__ pb,
                                                           const float2* __restrict__ pc, const int* __restrict__ npts,
                                                           int corr_cap, int H, const float* __restrict__ Ms,
                                                           int* __restrict__ cnt, float thr2) {
    __shared__ float4 ta[SIM3_TILE];
    __shared__ float4 tb[SIM3_TILE];
    __shared__ float2 tc[SIM3_TILE];
    const int p = blockIdx.x;
    const int h = blockIdx.y * SIM3_BLOCK + threadIdx.x;
    const int n = npts[p];
    const bool live = h < H && cnt[(int64_t)p * H + h] == 0;
    float m[SIM3_MODEL];
    const float* Mp = Ms + (int64_t)p * SIM3_MODEL * H;
#pragma unroll
    for (int k = 0; k < SIM3_MODEL; k++) m[k] = live ? Mp[(int64_t)k * H + h] : 0.0f;
    const float4* qa = pa + (int64_t)p * corr_cap;
    const float4* qb = pb + (int64_t)p * corr_cap;
    const float2* qc = pc + (int64_t)p * corr_cap;
    int count = 0;
    for (int base = 0; base < n; base += SIM3_TILE) {
        const int mt = min(SIM3_TILE, n - base);
        __syncthreads();
        for (int i = threadIdx.x; i < mt; i += SIM3_BLOCK) {
            ta[i] = qa[base + i];
            tb[i] = qb[base + i];
            tc[i] = qc[base + i];
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < mt; i++) count += sim3_inlier(m, ta[i], tb[i], tc[i], thr2);
        }
    }
    if (live) cnt[(int64_t)p * H + h] = count;
}

// ---- finish: winner, Gauss-Newton, rescoring, outputs -------------------------------------------------------------------------
struct Sim3Point {
    double X1[3], X2[3], x1[2], x2[2];
};

__device__ __forceinline__ Sim3Point sim3_point(const aria_sim3_corr& c, double fx, double fy, double cx, double cy) {
    Sim3Point q;
#pragma unroll
    for (int k = 0; k < 3; k++) { q.X1[k] = c.X1[k]; q.X2[k] = c.X2[k]; }
    q.x1[0] = ((double)c.u1 - cx) / fx;
    q.x1[1] = ((double)c.v1 - cy) / fy;
    q.x2[0] = ((double)c.u2 - cx) / fx;
    q.x2[1] = ((double)c.v2 - cy) / fy;
    return q;
}

// Y2 = s R X1 + t and Y1 = R^T (X2 - t)
__device__ __forceinline__ void sim3_transfer(const double* R, const double* t, double s, const Sim3Point& q, double Y2[3], double Y1[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) Y2[k] = s * ((R[3 * k] * q.X1[0] + R[3 * k + 1] * q.X1[1]) + R[3 * k + 2] * q.X1[2]) + t[k];
    const double d0 = q.X2[0] - t[0], d1 = q.X2[1] - t[1], d2 = q.X2[2] - t[2];
#pragma unroll
    for (int k = 0; k < 3; k++) Y1[k] = (R[k] * d0 + R[3 + k] * d1) + R[6 + k] * d2;
}

// E(x): the degree-12 Taylor sum of exp in Horner form, + * / only (sim3_ref.exp_series)
__device__ __forceinline__ double sim3_exp_series(double x) {
    double acc = 1.0;
    for (int k = SIM3_EXP_TERMS; k > 0; k--) acc = 1.0 + (x / (double)k) * acc;
    return acc;
}

// One Gauss-Newton step from the summed normal equations S (28 upper entries of the 7x7 row by row, then the 7 of J^T r), by
// one lane: Cholesky of the leading npar x npar block, the left update of (R, t, s). Returns 0 = no step (the refinement ends
// with the model untouched), 1 = step taken, 2 = step taken and small.
__device__ int sim3_gn_step(const double* S, double* L, double* R, double* t, double* sc, int npar, double min_scale, double max_scale) {
    int k = 0;
    for (int r = 0; r < 7; r++)
        for (int c = r; c < 7; c++) L[c * 7 + r] = S[k++];      // lower triangle of A
    for (int j = 0; j < npar; j++) {
        double d = L[j * 7 + j];
        for (int q = 0; q < j; q++) d = d - L[j * 7 + q] * L[j * 7 + q];
        if (!(d > 0.0) || !isfinite(d)) return 0;
        const double dj = sqrt(d);
        L[j * 7 + j] = dj;
        for (int i = j + 1; i < npar; i++) {
            double v = L[i * 7 + j];
            for (int q = 0; q < j; q++) v = v - L[i * 7 + q] * L[j * 7 + q];
            L[i * 7 + j] = v / dj;
        }
    }
    double y[7], x[7];
    for (int i = 0; i < 7; i++) { y[i] = 0.0; x[i] = 0.0; }
    for (int i = 0; i < npar; i++) {
        double v = -S[28 + i];
        for (int q = 0; q < i; q++) v = v - L[i * 7 + q] * y[q];
        y[i] = v / L[i * 7 + i];
    }
    for (int i = npar - 1; i >= 0; i--) {
        double v = y[i];
        for (int q = i + 1; q < npar; q++) v = v - L[q * 7 + i] * x[q];
        x[i] = v / L[i * 7 + i];
    }
    double nrm = 0.0;
    for (int i = 0; i < npar; i++) nrm = nrm + x[i] * x[i];
    if (!isfinite(nrm)) return 0;
    const double es = npar == 7 ? sim3_exp_series(x[6]) : 1.0;
    const double sn = es * (*sc);
    if (npar == 7 && !(sn >= min_scale && sn <= max_scale)) return 0;
    double E[9];
    exp_so3(x, E);
    double Rn[9], tn[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rn[r * 3 + c] = E[r * 3] * R[c] + E[r * 3 + 1] * R[3 + c] + E[r * 3 + 2] * R[6 + c];
        tn[r] = es * (E[r * 3] * t[0] + E[r * 3 + 1] * t[1] + E[r * 3 + 2] * t[2]) + x[3 + r];
    }
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    for (int i = 0; i < 3; i++) t[i] = tn[i];
    *sc = sn;
    return sqrt(nrm) <= SIM3_STEP_TOL ? 2 : 1;
}

__device__ __forceinline__ void sim3_write_invalid(aria_sim3_result* o, int n) {
    for (int k = 0; k < 9; k++) o->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 3; k++) o->t[k] = 0.0;
    o->s = 1.0;
    o->rms_px = 0.0;
    o->n_corr = n; o->n_inliers = 0; o->best_hypothesis = -1; o->iterations = 0; o->refined = 0; o->valid = 0;
}

__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_finish(const aria_sim3_corr* __restrict__ corr, const float4* __restrict__ pa,
                                                            const float4* __restrict__ pb, const float2* __restrict__ pc,
                                                            const int* __restrict__ npts, int corr_cap, int H,
                                                            const float* __restrict__ Ms, const int* __restrict__ cnt, float thr2,
                                                            double fx, double fy, double cx, double cy, int refine_iters,
                                                            int fix_scale, double min_scale, double max_scale, uint64_t seed,
                                                            int pair_base, uint8_t* __restrict__ ws, uint8_t* __restrict__ mask,
                                                            aria_sim3_result* __restrict__ out) {
    __shared__ int red_c[SIM3_BLOCK], red_h[SIM3_BLOCK];
    __shared__ double red[2 * 2 * SIM3_WAVES], S[35], L[49];
    __shared__ double Mc[SIM3_MODEL], Mw[SIM3_MODEL];       // the current model and the winner's closed form: R, t, s
    __shared__ float Pw[SIM3_MODEL], Pf[SIM3_MODEL];
    __shared__ int n_in, n_ref, stop, iters, have_ref, out_ok;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = npts[p];
    const aria_sim3_corr* cp = corr + (int64_t)p * corr_cap;
    const float4* qa = pa + (int64_t)p * corr_cap;
    const float4* qb = pb + (int64_t)p * corr_cap;
    const float2* qc = pc + (int64_t)p * corr_cap;
    uint8_t* w = ws + (int64_t)p * corr_cap;
    int phase = 0;

    // argmax over (count, -h): ascending scan per lane, then a fixed tree
    int bc = -1, bh = -1;
    for (int h = tid; h < H; h += SIM3_BLOCK) {
        const int c = cnt[(int64_t)p * H + h];
        if (c > bc) { bc = c; bh = h; }
    }
    red_c[tid] = bc;
    red_h[tid] = bh;
    __syncthreads();
    for (int s = SIM3_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int c2 = red_c[tid + s], h2 = red_h[tid + s];
            if (c2 > red_c[tid] || (c2 == red_c[tid] && c2 >= 0 && h2 < red_h[tid])) { red_c[tid] = c2; red_h[tid] = h2; }
        }
        __syncthreads();
    }
    const int win_c = red_c[0], win_h = red_h[0];
    aria_sim3_result* o = out + p;
    uint8_t* mk = mask ? mask + (int64_t)p * corr_cap : nullptr;
    if (n < SIM3_MIN || win_c < 0) {
        if (mk)
            for (int i = tid; i < corr_cap; i += SIM3_BLOCK) mk[i] = 0;
        if (tid == 0) sim3_write_invalid(o, n);
        return;
    }
    if (tid < SIM3_MODEL) Pw[tid] = Ms[((int64_t)p * SIM3_MODEL + tid) * H + win_h];
    if (tid == 0) {
        n_in = 0; n_ref = 0; iters = 0; have_ref = 0; out_ok = 0;
        // the winner's closed form again, in fp64: what was scored is its fp32 rounding
        int idx[3] = {0, 0, 0};
        bool ok = draw_sample<3, SIM3_MAX_RETRY>(seed, (uint32_t)(pair_base + p), win_h, n, idx);
        double R[9], t[3], s = 1.0;
        if (ok) ok = sim3_solve(cp[idx[0]], cp[idx[1]], cp[idx[2]], fix_scale, min_scale, max_scale, R, t, s);
        // the fallback reads the scored model where the hypothesis kernel left it: Pw is being written by other lanes
        const float* Mp = Ms + (int64_t)p * SIM3_MODEL * H + win_h;
        for (int k = 0; k < 9; k++) Mw[k] = ok ? R[k] : (double)Mp[(int64_t)k * H];
        for (int k = 0; k < 3; k++) Mw[9 + k] = ok ? t[k] : (double)Mp[(int64_t)(9 + k) * H];
        Mw[12] = ok ? s : (double)Mp[(int64_t)12 * H];
        for (int k = 0; k < SIM3_MODEL; k++) Mc[k] = Mw[k];
        stop = ok ? 0 : 1;
    }
    __syncthreads();
    {   // the winner's inliers (the same test, on the same fp32 model, as its score)
        float m[SIM3_MODEL];
        for (int k = 0; k < SIM3_MODEL; k++) m[k] = Pw[k];
        int c = 0;
        for (int i = tid; i < n; i += SIM3_BLOCK) {
            const int in = sim3_inlier(m, qa[i], qb[i], qc[i], thr2);
            w[i] = (uint8_t)in;
            c += in;
        }
        atomicAdd(&n_in, c);
    }
    __syncthreads();
    const int win_in = n_in;
    const int npar = fix_scale ? 6 : 7;
    if (win_in >= SIM3_MIN_REFINE && refine_iters > 0) {
        for (int it = 0; it < refine_iters; it++) {
            if (stop) break;                 // read between two barriers that no write to `stop` lies between
            double R[9], t[3];
            for (int k = 0; k < 9; k++) R[k] = Mc[k];
            for (int k = 0; k < 3; k++) t[k] = Mc[9 + k];
            const double s = Mc[12];
            double wv[3];                    // R^T t
            for (int k = 0; k < 3; k++) wv[k] = (R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2];
            double acc[36];
#pragma unroll
            for (int k = 0; k < 36; k++) acc[k] = 0.0;
            for (int i = tid; i < n; i += SIM3_BLOCK) {
                if (!w[i]) continue;
                const Sim3Point q = sim3_point(cp[i], fx, fy, cx, cy);
                double Y2[3], Y1[3];
                sim3_transfer(R, t, s, q, Y2, Y1);
                double J[4][7], r[4];
                {
                    const double iz = 1.0 / Y2[2];
                    const double px = Y2[0] * iz, py = Y2[1] * iz;
                    r[0] = px - q.x2[0];
                    r[1] = py - q.x2[1];
                    J[0][0] = -(px * py); J[0][1] = 1.0 + px * px; J[0][2] = -py; J[0][3] = iz; J[0][4] = 0.0; J[0][5] = -(px * iz);
                    J[1][0] = -(1.0 + py * py); J[1][1] = px * py; J[1][2] = px; J[1][3] = 0.0; J[1][4] = iz; J[1][5] = -(py * iz);
                    J[0][6] = 0.0;
                    J[1][6] = 0.0;
                }
                {
                    const double iz = 1.0 / Y1[2];
                    const double px = Y1[0] * iz, py = Y1[1] * iz, pxz = px * iz, pyz = py * iz;
                    r[2] = px - q.x1[0];
                    r[3] = py - q.x1[1];
                    const double x = q.X2[0], y = q.X2[1], z = q.X2[2];
                    double D[3][3];          // R^T [X2]x
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        D[a][0] = R[3 + a] * z - R[6 + a] * y;
                        D[a][1] = R[6 + a] * x - R[a] * z;
                        D[a][2] = R[a] * y - R[3 + a] * x;
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        J[2][k] = iz * D[0][k] - pxz * D[2][k];
                        J[3][k] = iz * D[1][k] - pyz * D[2][k];
                        J[2][3 + k] = -(iz * R[3 * k] - pxz * R[3 * k + 2]);
                        J[3][3 + k] = -(iz * R[3 * k + 1] - pyz * R[3 * k + 2]);
                    }
                    J[2][6] = fix_scale ? 0.0 : -(iz * wv[0] - pxz * wv[2]);
                    J[3][6] = fix_scale ? 0.0 : -(iz * wv[1] - pyz * wv[2]);
                }
                int k = 0;
#pragma unroll
                for (int a = 0; a < 7; a++)
#pragma unroll
                    for (int c = a; c < 7; c++) acc[k++] += ((J[0][a] * J[0][c] + J[1][a] * J[1][c]) + J[2][a] * J[2][c]) + J[3][a] * J[3][c];
#pragma unroll
                for (int a = 0; a < 7; a++) acc[28 + a] += ((J[0][a] * r[0] + J[1][a] * r[1]) + J[2][a] * r[2]) + J[3][a] * r[3];
            }
#pragma unroll
            for (int k = 0; k < 36; k += 2) {
                block_sum2<SIM3_WAVES>(red, phase, acc[k], acc[k + 1]);
                if (tid == 0) {
                    S[k] = acc[k];
                    if (k + 1 < 35) S[k + 1] = acc[k + 1];
                }
            }
            __syncthreads();
            if (tid == 0) {
                const int step = sim3_finite(S, 35) ? sim3_gn_step(S, L, Mc, Mc + 9, Mc + 12, npar, min_scale, max_scale) : 0;
                if (step) iters = iters + 1;
                if (step != 1) stop = 1;
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) {
            const bool ok = sim3_round(Mc, Mc + 9, Mc[12], Pf) && iters > 0;
            have_ref = ok ? 1 : 0;
        }
        __syncthreads();
        if (have_ref) {
            float m[SIM3_MODEL];
            for (int k = 0; k < SIM3_MODEL; k++) m[k] = Pf[k];
            int c = 0;
            for (int i = tid; i < n; i += SIM3_BLOCK) c += sim3_inlier(m, qa[i], qb[i], qc[i], thr2);
            atomicAdd(&n_ref, c);
        }
        __syncthreads();
    }
    const bool refined = have_ref && n_ref >= win_in;
    const int n_it = iters;
    __syncthreads();
    if (refined) {
        float m[SIM3_MODEL];
        for (int k = 0; k < SIM3_MODEL; k++) m[k] = Pf[k];
        for (int i = tid; i < n; i += SIM3_BLOCK) w[i] = (uint8_t)sim3_inlier(m, qa[i], qb[i], qc[i], thr2);
    } else if (tid < SIM3_MODEL) {           // the winner's closed form
        Mc[tid] = Mw[tid];
    }
    __syncthreads();
    const int final_in = refined ? n_ref : win_in;
    double sumsq = 0.0;
    {   // rms over the kept inliers, both directions
        double R[9], t[3];
        for (int k = 0; k < 9; k++) R[k] = Mc[k];
        for (int k = 0; k < 3; k++) t[k] = Mc[9 + k];
        const double s = Mc[12];
        for (int i = tid; i < n; i += SIM3_BLOCK) {
            if (!w[i]) continue;
            const Sim3Point q = sim3_point(cp[i], fx, fy, cx, cy);
            double Y2[3], Y1[3];
            sim3_transfer(R, t, s, q, Y2, Y1);
            const double r0 = Y2[0] / Y2[2] - q.x2[0], r1 = Y2[1] / Y2[2] - q.x2[1];
            const double r2 = Y1[0] / Y1[2] - q.x1[0], r3 = Y1[1] / Y1[2] - q.x1[1];
            sumsq += ((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3;
        }
        double zero = 0.0;
        block_sum2<SIM3_WAVES>(red, phase, sumsq, zero);
    }
    if (tid == 0) {
        const double rms = final_in > 0 ? sqrt(sumsq / (double)(2 * final_in)) * ((fx + fy) * 0.5) : 0.0;
        const bool ok = sim3_finite(Mc, SIM3_MODEL) && isfinite(rms);
        if (ok) {
            for (int k = 0; k < 9; k++) o->R[k] = Mc[k];
            for (int k = 0; k < 3; k++) o->t[k] = Mc[9 + k];
            o->s = Mc[12];
            o->rms_px = rms;
            o->n_corr = n; o->n_inliers = final_in; o->best_hypothesis = win_h; o->iterations = n_it;
            o->refined = refined ? 1 : 0; o->valid = 1;
        } else {
            sim3_write_invalid(o, n);
        }
        out_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (mk) {
        const bool ok = out_ok != 0;
        for (int i = tid; i < corr_cap; i += SIM3_BLOCK) mk[i] = (ok && i < n) ? w[i] : (uint8_t)0;
    }
}

// ---- association: match list x point map -> correspondences -------------------------------------------------------------------
// table[p * kp_stride + k] = the lowest arena position of a point whose pair is anchor[p] and whose keyframe index is k
__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_assoc_scatter(const aria_map_point* __restrict__ arena, const long long* __restrict__ d_size,
                                                                   long long capacity, const int* __restrict__ anchor, int view,
                                                                   int n_pairs, int64_t kp_stride, int* __restrict__ table) {
    long long size = *d_size;
    size = size < 0 ? 0 : (size > capacity ? capacity : size);
    if (size > (long long)SIM3_EMPTY) size = SIM3_EMPTY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += (long long)gridDim.x * blockDim.x) {
        const int pair = arena[i].pair;
        const int key = view == 1 ? arena[i].idx1 : arena[i].idx2;
        if (key < 0 || key >= kp_stride) continue;
        for (int p = 0; p < n_pairs; p++)
            if (anchor[p] == pair) atomicMin(&table[(int64_t)p * kp_stride + key], (int)i);
    }
}

__global__ __launch_bounds__(SIM3_BLOCK) void k_sim3_assoc_gather(const aria_map_point* __restrict__ arena, const int* __restrict__ table1,
                                                                  const int* __restrict__ table2, const double* __restrict__ pose1,
                                                                  const double* __restrict__ pose2, const aria_keypoint* __restrict__ kp1,
                                                                  const int* __restrict__ n1, const aria_keypoint* __restrict__ kp2,
                                                                  const int* __restrict__ n2, int64_t kp_stride,
                                                                  const aria_match* __restrict__ matches, const int* __restrict__ nmatches,
                                                                  int match_cap, aria_sim3_corr* __restrict__ corr, int* __restrict__ ncorr,
                                                                  int* __restrict__ corr_match, int* __restrict__ err) {
    __shared__ int bad_count, bad_index;       // written before / read after a barrier each
    __shared__ int wsum[SIM3_WAVES];
    const int p = blockIdx.x;
    const int n = nmatches[p], n1p = n1[p], n2p = n2[p];
    if (threadIdx.x == 0) {
        bad_count = (n < 0 || n > match_cap || n1p < 0 || n1p > kp_stride || n2p < 0 || n2p > kp_stride) ? 1 : 0;
        bad_index = 0;
    }
    __syncthreads();
    const aria_match* m = matches + (int64_t)p * match_cap;
    if (!bad_count) {
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += SIM3_BLOCK) {
            const aria_match a = m[i];
            mine |= (a.query_idx < 0 || a.query_idx >= n1p || a.train_idx < 0 || a.train_idx >= n2p);
        }
        if (mine) atomicOr(&bad_index, 1);
    }
    __syncthreads();
    if (bad_count | bad_index) {
        if (threadIdx.x == 0) {
            ncorr[p] = 0;
            atomicOr(err, ERRBIT_SIM3_INPUT);
        }
        return;
    }
    const aria_keypoint* k1 = kp1 + (int64_t)p * kp_stride;
    const aria_keypoint* k2 = kp2 + (int64_t)p * kp_stride;
    const int* t1 = table1 + (int64_t)p * kp_stride;
    const int* t2 = table2 + (int64_t)p * kp_stride;
    const double* T1 = pose1 + (int64_t)p * 12;
    const double* T2 = pose2 + (int64_t)p * 12;
    aria_sim3_corr* oc = corr + (int64_t)p * match_cap;
    int* om = corr_match ? corr_match + (int64_t)p * match_cap : nullptr;
    int o = 0;
    for (int base = 0; base < n; base += SIM3_BLOCK) {
        const int i = base + threadIdx.x;
        aria_match a{};
        int pos1 = SIM3_EMPTY, pos2 = SIM3_EMPTY;
        if (i < n) {
            a = m[i];
            pos1 = t1[a.query_idx];
            pos2 = t2[a.train_idx];
        }
        const bool keep = pos1 != SIM3_EMPTY && pos2 != SIM3_EMPTY;
        int total;
        const int slot = block_compact<SIM3_BLOCK>(keep, wsum, total);
        if (keep) {
            aria_sim3_corr c;
            const double* A = arena[pos1].X;
            const double* B = arena[pos2].X;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                c.X1[k] = ((T1[4 * k] * A[0] + T1[4 * k + 1] * A[1]) + T1[4 * k + 2] * A[2]) + T1[4 * k + 3];
                c.X2[k] = ((T2[4 * k] * B[0] + T2[4 * k + 1] * B[1]) + T2[4 * k + 2] * B[2]) + T2[4 * k + 3];
            }
            c.u1 = k1[a.query_idx].x;
            c.v1 = k1[a.query_idx].y;
            c.u2 = k2[a.train_idx].x;
            c.v2 = k2[a.train_idx].y;
            oc[o + slot] = c;
            if (om) om[o + slot] = i;
        }
        o += total;
    }
    if (threadIdx.x == 0) ncorr[p] = o;
}

}  // namespace

// ---- C-ABI ------------------------------------------------------------------------------------------------------------------
struct aria_sim3_s : StageHandle {
    aria_sim3_config cfg{};
    // grow-only workspace of the batch path
    DeviceBuffer<float4> d_pa, d_pb;      // [n_pairs][corr_cap] (X1, x1.x), (X2, x2.x)
    DeviceBuffer<float2> d_pc;            // [n_pairs][corr_cap] (x1.y, x2.y)
    DeviceBuffer<int> d_npts;             // [n_pairs]
    DeviceBuffer<float> d_M;              // [n_pairs][13][H]
    DeviceBuffer<int> d_cnt;              // [n_pairs][H]
    DeviceBuffer<uint8_t> d_ws;           // [n_pairs][corr_cap] inlier flags
    DeviceBuffer<int> d_table;            // [2][n_pairs][kp_stride] association tables
    // single-pair staging of the host forms
    CorrStaging<aria_sim3_corr> one;
    DeviceBuffer<aria_sim3_result> d_res;
    DeviceBuffer<int> d_dbg;
};

namespace {

float sim3_thr2(const aria_sim3_config& c) { return normalized_thr2(c.threshold_px, c.fx, c.fy); }

int enqueue(aria_sim3_t h, const aria_sim3_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap, int pair_base,
            aria_sim3_result* d_out, uint8_t* d_mask, int* d_dbg, bool finish) {
    const int H = h->cfg.hypotheses;
    int rc;
    if ((rc = h->d_pa.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_pb.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_pc.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_ws.reserve(h->stream, (size_t)n_pairs * corr_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_npts.reserve(h->stream, (size_t)n_pairs)) != ARIA_OK) return rc;
    if ((rc = h->d_M.reserve(h->stream, (size_t)n_pairs * H * SIM3_MODEL)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, (size_t)n_pairs * H)) != ARIA_OK) return rc;
    const aria_sim3_config& c = h->cfg;
    const dim3 per_hyp(n_pairs, (H + SIM3_BLOCK - 1) / SIM3_BLOCK);
    hipLaunchKernelGGL(k_sim3_stage, dim3(n_pairs), dim3(SIM3_BLOCK), 0, h->stream, d_corr, d_ncorr, corr_cap, c.fx, c.fy, c.cx, c.cy,
                       h->d_pa, h->d_pb, h->d_pc, h->d_npts, h->d_err);
    hipLaunchKernelGGL(k_sim3_hyp, per_hyp, dim3(SIM3_BLOCK), 0, h->stream, d_corr, h->d_npts, corr_cap, H, (uint64_t)c.seed, pair_base,
                       c.fix_scale, c.min_scale, c.max_scale, h->d_M, h->d_cnt, d_dbg);
    hipLaunchKernelGGL(k_sim3_score, per_hyp, dim3(SIM3_BLOCK), 0, h->stream, h->d_pa, h->d_pb, h->d_pc, h->d_npts, corr_cap, H, h->d_M,
                       h->d_cnt, sim3_thr2(c));
    if (finish)
        hipLaunchKernelGGL(k_sim3_finish, dim3(n_pairs), dim3(SIM3_BLOCK), 0, h->stream, d_corr, h->d_pa, h->d_pb, h->d_pc, h->d_npts,
                           corr_cap, H, h->d_M, h->d_cnt, sim3_thr2(c), c.fx, c.fy, c.cx, c.cy, c.refine_iters, c.fix_scale,
                           c.min_scale, c.max_scale, (uint64_t)c.seed, pair_base, h->d_ws, d_mask, d_out);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // namespace

extern "C" {

void aria_sim3_default_config(aria_sim3_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_sim3_config);
    c->device = 0;
    c->stream = nullptr;
    c->hypotheses = 1024;
    c->refine_iters = 5;
    c->fix_scale = 0;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0, as aria_pose_default_config
    c->threshold_px = 3.0;
    c->min_scale = 0.05;
    c->max_scale = 20.0;
    c->seed = 0;
}

int aria_sim3_create(const aria_sim3_config* c, aria_sim3_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_sim3_config)) return ARIA_E_INVALID;
    if (c->hypotheses < 64 || c->hypotheses > 16384 || (c->hypotheses % 64)) return ARIA_E_INVALID;
    if (c->refine_iters < 0 || c->refine_iters > 16 || (c->fix_scale != 0 && c->fix_scale != 1)) return ARIA_E_INVALID;
    if (bad_pinhole(c->fx, c->fy, c->cx, c->cy) || !(c->threshold_px > 0) || !std::isfinite(c->threshold_px)) return ARIA_E_INVALID;
    if (!(c->min_scale > 0) || !(c->max_scale >= c->min_scale) || !std::isfinite(c->max_scale)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_sim3_create", [](aria_sim3_s* h) {
        const int rc = h->d_res.reserve(h->stream, 1, "aria_sim3_create");
        return rc != ARIA_OK ? rc : h->one.create(h->stream, "aria_sim3_create");
    });
}

void aria_sim3_destroy(aria_sim3_t h) { stage_destroy(h); }

void* aria_sim3_stream(aria_sim3_t h) { return stage_stream(h); }

int aria_sim3_check(aria_sim3_t h) { return stage_check(h, {{ERRBIT_SIM3_INPUT, ARIA_E_INVALID}}); }

int aria_sim3_estimate_batch_device(aria_sim3_t h, const aria_sim3_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap,
                                    int pair_base, aria_sim3_result* d_out, uint8_t* d_mask) {
    if (!h || !d_corr || !d_ncorr || !d_out || n_pairs < 0 || corr_cap < 1 || corr_cap > (1 << 20) || pair_base < 0)
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return enqueue(h, d_corr, d_ncorr, n_pairs, corr_cap, pair_base, d_out, d_mask, nullptr, true);
}

int aria_sim3_estimate(aria_sim3_t h, const aria_sim3_corr* corr, int n, int pair_base, aria_sim3_result* out, uint8_t* mask) {
    if (!h || !out || pair_base < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    CorrStaging<aria_sim3_corr>& s = h->one;
    int rc = s.upload(h->stream, corr, n);
    if (rc != ARIA_OK) return rc;
    if ((rc = enqueue(h, s.d_corr, s.d_n, 1, s.cap, pair_base, h->d_res, s.d_mask, nullptr, true)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(out, h->d_res, sizeof(aria_sim3_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && n) ARIA_HIP(hipMemcpyAsync(mask, s.d_mask, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_sim3_check(h);
}

int aria_sim3_debug_hypotheses(aria_sim3_t h, const aria_sim3_corr* corr, int n, int pair_base, int* sample_idx, float* R, float* t,
                               float* s, int* counts) {
    if (!h || !sample_idx || !R || !t || !s || !counts || pair_base < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->one.upload(h->stream, corr, n);
    if (rc != ARIA_OK) return rc;
    const int H = h->cfg.hypotheses;
    if ((rc = h->d_dbg.reserve(h->stream, (size_t)H * 3)) != ARIA_OK) return rc;
    if ((rc = enqueue(h, h->one.d_corr, h->one.d_n, 1, h->one.cap, pair_base, nullptr, nullptr, h->d_dbg, false)) != ARIA_OK) return rc;
    std::vector<float> soa((size_t)SIM3_MODEL * H);
    ARIA_HIP(hipMemcpyAsync(sample_idx, h->d_dbg, sizeof(int) * 3 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(soa.data(), h->d_M, sizeof(float) * SIM3_MODEL * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(counts, h->d_cnt, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    unpack_models(soa.data(), H, 0, 9, R);
    unpack_models(soa.data(), H, 9, 3, t);
    unpack_models(soa.data(), H, 12, 1, s);
    return aria_sim3_check(h);
}

int aria_sim3_associate_batch_device(aria_sim3_t h, aria_map_t map, const int* d_anchor1, const int* d_anchor2, int view1, int view2,
                                     const double* d_pose1, const double* d_pose2, const aria_keypoint* d_kp1, const int* d_n1,
                                     const aria_keypoint* d_kp2, const int* d_n2, int64_t kp_stride, const aria_match* d_matches,
                                     const int* d_nmatches, int n_pairs, int match_cap, aria_sim3_corr* d_corr, int* d_ncorr,
                                     int* d_corr_match) {
    if (!h || !map || !d_anchor1 || !d_anchor2 || !d_pose1 || !d_pose2 || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches ||
        !d_nmatches || !d_corr || !d_ncorr || n_pairs < 0 || match_cap < 1 || match_cap > (1 << 20) || kp_stride < 1 ||
        kp_stride > (1 << 24) || (view1 != 1 && view1 != 2) || (view2 != 1 && view2 != 2))
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t cells = (size_t)n_pairs * (size_t)kp_stride;
    int rc;
    if ((rc = h->d_table.reserve(h->stream, 2 * cells)) != ARIA_OK) return rc;
    const aria_map_point* arena = nullptr;
    const long long* d_size = nullptr;
    int64_t capacity = 0;
    int map_device = -1;
    map_device_view(map, &arena, &d_size, &capacity, &map_device);
    if (map_device != h->device) return ARIA_E_INVALID;          // the join reads the map's arena where it lies
    ARIA_HIP(hipMemsetAsync(h->d_table, 0x7F, 2 * cells * sizeof(int), h->stream));
    int* table1 = h->d_table;
    int* table2 = h->d_table + cells;
    if (arena && capacity > 0) {
        const int blocks = (int)std::min<int64_t>((capacity + SIM3_BLOCK - 1) / SIM3_BLOCK, 2048);
        hipLaunchKernelGGL(k_sim3_assoc_scatter, dim3(blocks), dim3(SIM3_BLOCK), 0, h->stream, arena, d_size, (long long)capacity,
                           d_anchor1, view1, n_pairs, kp_stride, table1);
        hipLaunchKernelGGL(k_sim3_assoc_scatter, dim3(blocks), dim3(SIM3_BLOCK), 0, h->stream, arena, d_size, (long long)capacity,
                           d_anchor2, view2, n_pairs, kp_stride, table2);
    }
    hipLaunchKernelGGL(k_sim3_assoc_gather, dim3(n_pairs), dim3(SIM3_BLOCK), 0, h->stream, arena, table1, table2, d_pose1, d_pose2,
                       d_kp1, d_n1, d_kp2, d_n2, kp_stride, d_matches, d_nmatches, match_cap, d_corr, d_ncorr, d_corr_match, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // extern "C"
