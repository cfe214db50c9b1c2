// Two-view relative pose on the device: essential-matrix RANSAC (normalised 8-point minimal solver, Sampson scoring, one
// least-squares refit) + recoverPose's cheirality test, batched over pairs. Semantics in include/aria_orb_hip.h
// ("two-view relative pose"); aria_slam_amd/pose_ref.py restates every step in NumPy.
//
// Four launches on the handle's stream:
//   k_pose_stage   one workgroup per pair: validates every match index against the pair's keypoint counts BEFORE any
//                  keypoint is read, then writes the normalised point pairs (x1, y1, x2, y2) as one float4 per match
//   k_pose_hyp     one lane per hypothesis: 8 sample indices from the counter-based hash, fp64 elimination with partial
//                  pivoting on the 8x9 system, projection onto the essential manifold; E (fp32, unit Frobenius norm) or "invalid"
//   k_pose_score   one lane per hypothesis, the pair's points staged in LDS tiles (16 B per match) and read as a broadcast:
//                  inlier count per hypothesis (the hot loop: ~26 fp32 ops per evaluation, no scratch -- tests/test_pose_host.py)
//   k_pose_finish  one workgroup per pair: argmax over (count, -h), refit over the winner's inliers (9x9 normal matrix in
//                  fp64, strided per-thread sums + fixed butterfly, Jacobi eigen-solver in LDS), rescore, decomposition
//                  into the four (R, +-t) candidates, cheirality counts, result record and mask
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

constexpr int POSE_TILE = 2048;            // points per LDS tile of k_pose_score (32 KB)
constexpr int POSE_SCORE_BLOCK = 256;
constexpr int POSE_FINISH_BLOCK = 256;
constexpr int POSE_MAX_RETRY = 256;        // redraws per sample slot (header: a slot that exhausts them invalidates the hypothesis)
constexpr double POSE_PIVOT_TOL = 1e-9;    // |pivot| <= tol * max|A_ij|: rank-deficient sample
constexpr double POSE_RANK_TOL = 1e-9;     // sigma2 <= tol * sigma1 after the solve: not an essential matrix
constexpr int ERRBIT_POSE_INPUT = 1;       // a pair's counts or match indices were out of range (pair skipped)

// Sampson test of findEssentialMat in normalised coordinates, division-free: r^2 <= thr2 * d with d > 0
__device__ __forceinline__ int pose_inlier(const float e[9], float4 q, float thr2) {
    const float ex0 = e[0] * q.x + e[1] * q.y + e[2];
    const float ex1 = e[3] * q.x + e[4] * q.y + e[5];
    const float ex2 = e[6] * q.x + e[7] * q.y + e[8];
    const float et0 = e[0] * q.z + e[3] * q.w + e[6];
    const float et1 = e[1] * q.z + e[4] * q.w + e[7];
    const float r = q.z * ex0 + q.w * ex1 + ex2;
    const float d = ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1;
    return (d > 0.0f && r * r <= thr2 * d) ? 1 : 0;
}

// Closest essential matrix (singular values (s, s, 0)) of e, scaled to unit Frobenius norm: (u1 v1^T + u2 v2^T) / sqrt(2),
// u_i = E v_i / sigma_i from the eigenvectors v_i of E^T E. Also returns U, V (right-handed, columns) for the decomposition.
// False when sigma2 <= POSE_RANK_TOL * sigma1.
__device__ __forceinline__ bool project_essential(const double e[9], double out[9], double U[9], double Vo[9]) {
    double G[9], V[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) G[r * 3 + c] = e[r] * e[c] + e[3 + r] * e[3 + c] + e[6 + r] * e[6 + c];
    jacobi3(G, V);
    double l0 = G[0], l1 = G[4], l2 = G[8];
    double a0 = V[0], a1 = V[3], a2 = V[6];   // columns as (x, y, z)
    double b0 = V[1], b1 = V[4], b2 = V[7];
    double c0 = V[2], c1 = V[5], c2 = V[8];
    // sort descending by eigenvalue (a three-element network of selects: no dynamic register indexing)
    bool s = l1 > l0;
    swap_if(s, l0, l1); swap_if(s, a0, b0); swap_if(s, a1, b1); swap_if(s, a2, b2);
    s = l2 > l1;
    swap_if(s, l1, l2); swap_if(s, b0, c0); swap_if(s, b1, c1); swap_if(s, b2, c2);
    s = l1 > l0;
    swap_if(s, l0, l1); swap_if(s, a0, b0); swap_if(s, a1, b1); swap_if(s, a2, b2);
    const double s0 = sqrt(fmax(l0, 0.0)), s1 = sqrt(fmax(l1, 0.0));
    if (!(s1 > POSE_RANK_TOL * s0)) return false;
    const double v1[3] = {a0, a1, a2}, v2[3] = {b0, b1, b2};
    double u1[3], u2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        u1[r] = (e[3 * r] * v1[0] + e[3 * r + 1] * v1[1] + e[3 * r + 2] * v1[2]) / s0;
        u2[r] = (e[3 * r] * v2[0] + e[3 * r + 1] * v2[1] + e[3 * r + 2] * v2[2]) / s1;
    }
    const double k = 1.0 / sqrt(2.0);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = (u1[r] * v1[c] + u2[r] * v2[c]) * k;
    // right-handed bases: third columns as cross products
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        U[r * 3 + 0] = u1[r]; U[r * 3 + 1] = u2[r]; U[r * 3 + 2] = u3[r];
        Vo[r * 3 + 0] = v1[r]; Vo[r * 3 + 1] = v2[r]; Vo[r * 3 + 2] = v3[r];
    }
    return true;
}

// ---- stage: validate, normalise ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pose_stage(const aria_keypoint* __restrict__ kq, const int* __restrict__ nq,
                                                    const aria_keypoint* __restrict__ kt, const int* __restrict__ nt,
                                                    int64_t kp_stride, const aria_match* __restrict__ matches,
                                                    const int* __restrict__ nmatches, int match_cap, int query_is_first,
                                                    double fx, double fy, double cx, double cy, float4* __restrict__ pts,
                                                    int* __restrict__ npts, int* __restrict__ err) {
    __shared__ int bad;
    const int p = blockIdx.x;
    const int n = nmatches[p], nqp = nq[p], ntp = nt[p];
    if (threadIdx.x == 0) bad = (n < 0 || n > match_cap || nqp < 0 || nqp > kp_stride || ntp < 0 || ntp > kp_stride) ? 1 : 0;
    __syncthreads();
    const aria_match* m = matches + (int64_t)p * match_cap;
    if (!bad) {
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const aria_match a = m[i];
            mine |= (a.query_idx < 0 || a.query_idx >= nqp || a.train_idx < 0 || a.train_idx >= ntp);
        }
        if (mine) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (bad) {
        if (threadIdx.x == 0) {
            npts[p] = 0;
            atomicOr(err, ERRBIT_POSE_INPUT);
        }
        return;
    }
    if (threadIdx.x == 0) npts[p] = n;
    const aria_keypoint* q = kq + (int64_t)p * kp_stride;
    const aria_keypoint* t = kt + (int64_t)p * kp_stride;
    float4* o = pts + (int64_t)p * match_cap;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const aria_match a = m[i];
        const aria_keypoint k1 = query_is_first ? q[a.query_idx] : t[a.train_idx];
        const aria_keypoint k2 = query_is_first ? t[a.train_idx] : q[a.query_idx];
        o[i] = make_float4((float)(((double)k1.x - cx) / fx), (float)(((double)k1.y - cy) / fy),
                           (float)(((double)k2.x - cx) / fx), (float)(((double)k2.y - cy) / fy));
    }
}

// ---- hypotheses: sample + minimal solve ---------------------------------------------------------------------------------
// E is stored structure-of-arrays per pair: E[(p * 9 + k) * H + h]; cnt[p * H + h] = 0 (valid, to be scored) or -1.
__global__ __launch_bounds__(64) void k_pose_hyp(const float4* __restrict__ pts, const int* __restrict__ npts, int match_cap,
                                                 int H, uint64_t seed, int pair_base, float* __restrict__ E, int* __restrict__ cnt,
                                                 int* __restrict__ dbg_idx) {
    const int p = blockIdx.x;
    const int h = blockIdx.y * 64 + threadIdx.x;
    const int n = npts[p];
    float* Ep = E + (int64_t)p * 9 * H;
    bool ok = n >= 8;
    int idx[8];
#pragma unroll
    for (int j = 0; j < 8; j++) idx[j] = -1;
    if (ok) ok = draw_sample<8, POSE_MAX_RETRY>(seed, (uint32_t)(pair_base + p), h, n, idx);
    if (dbg_idx) {
#pragma unroll
        for (int j = 0; j < 8; j++) dbg_idx[h * 8 + j] = idx[j];
    }
    double e[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const float4* pp = pts + (int64_t)p * match_cap;
        double a[8][9];
        double amax = 0.0;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const float4 q = pp[idx[r]];
            const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
            a[r][0] = x2 * x1; a[r][1] = x2 * y1; a[r][2] = x2;
            a[r][3] = y2 * x1; a[r][4] = y2 * y1; a[r][5] = y2;
            a[r][6] = x1;      a[r][7] = y1;      a[r][8] = 1.0;
#pragma unroll
            for (int k = 0; k < 9; k++) amax = fmax(amax, fabs(a[r][k]));
        }
        // Gaussian elimination with partial pivoting (first row of largest |a[r][c]|, r >= c); row swaps as selects
#pragma unroll
        for (int c = 0; c < 8; c++) {
            int piv = c;
            double best = fabs(a[c][c]);
#pragma unroll
            for (int r = c + 1; r < 8; r++) {
                const double v = fabs(a[r][c]);
                if (v > best) { best = v; piv = r; }
            }
            ok &= best > POSE_PIVOT_TOL * amax;
#pragma unroll
            for (int r = c + 1; r < 8; r++)
#pragma unroll
                for (int k = c; k < 9; k++) swap_if(piv == r, a[c][k], a[r][k]);
            const double inv = 1.0 / (ok ? a[c][c] : 1.0);
#pragma unroll
            for (int r = c + 1; r < 8; r++) {
                const double f = a[r][c] * inv;
#pragma unroll
                for (int k = c + 1; k < 9; k++) a[r][k] = a[r][k] - f * a[c][k];
            }
        }
        if (ok) {
            double f[9];
            f[8] = 1.0;
#pragma unroll
            for (int c = 7; c >= 0; c--) {
                double s = 0.0;
#pragma unroll
                for (int k = c + 1; k < 9; k++) s = s + a[c][k] * f[k];
                f[c] = -s / a[c][c];
            }
            double nrm = 0.0;
#pragma unroll
            for (int k = 0; k < 9; k++) nrm = nrm + f[k] * f[k];
            nrm = sqrt(nrm);
#pragma unroll
            for (int k = 0; k < 9; k++) f[k] = f[k] / nrm;
            double U[9], V[9];
            ok = project_essential(f, e, U, V);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) Ep[(int64_t)k * H + h] = ok ? (float)e[k] : 0.0f;
    cnt[(int64_t)p * H + h] = ok ? 0 : -1;
}

// ---- scoring: the hot loop ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POSE_SCORE_BLOCK) void k_pose_score(const float4* __restrict__ pts, const int* __restrict__ npts,
                                                                 int match_cap, int H, const float* __restrict__ E,
                                                                 int* __restrict__ cnt, float thr2) {
    __shared__ float4 tile[POSE_TILE];
    const int p = blockIdx.x;
    const int h = blockIdx.y * POSE_SCORE_BLOCK + threadIdx.x;
    const int n = npts[p];
    const bool live = h < H && cnt[(int64_t)p * H + h] == 0;
    float e[9];
    const float* Ep = E + (int64_t)p * 9 * H;
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = live ? Ep[(int64_t)k * H + h] : 0.0f;
    const float4* pp = pts + (int64_t)p * match_cap;
    int count = 0;
    for (int base = 0; base < n; base += POSE_TILE) {
        const int m = min(POSE_TILE, n - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += POSE_SCORE_BLOCK) tile[i] = pp[base + i];
        __syncthreads();
        if (live) {
            for (int i = 0; i < m; i++) count += pose_inlier(e, tile[i], thr2);
        }
    }
    if (live) cnt[(int64_t)p * H + h] = count;
}

// ---- finish: winner, refit, recoverPose ---------------------------------------------------------------------------------
__device__ __forceinline__ void pose_row(float4 q, double r[9]) {
    const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
    r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
}

// recoverPose's cheirality test of one point under (R, t): least-squares depths (z1, z2) of z2 x2 = z1 R x1 + t,
// counted when 0 < z1 < dist and 0 < z2 < dist
__device__ __forceinline__ int pose_cheiral(const double* R, const double* t, float4 q, double dist) {
    const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
    const double a0 = R[0] * x1 + R[1] * y1 + R[2], a1 = R[3] * x1 + R[4] * y1 + R[5], a2 = R[6] * x1 + R[7] * y1 + R[8];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = x2 * x2 + y2 * y2 + 1.0, ab = a0 * x2 + a1 * y2 + a2;
    const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = x2 * t[0] + y2 * t[1] + t[2];
    const double det = aa * bb - ab * ab;
    if (!(det > 0.0)) return 0;
    const double z1 = (ab * bt - at * bb) / det, z2 = (aa * bt - ab * at) / det;
    return (z1 > 0.0 && z1 < dist && z2 > 0.0 && z2 < dist) ? 1 : 0;
}

__global__ __launch_bounds__(POSE_FINISH_BLOCK) void k_pose_finish(const float4* __restrict__ pts, const int* __restrict__ npts,
                                                                   int match_cap, int H, const float* __restrict__ E,
                                                                   const int* __restrict__ cnt, float thr2, double dist,
                                                                   uint8_t* __restrict__ ws, uint8_t* __restrict__ mask,
                                                                   aria_pose_result* __restrict__ out) {
    __shared__ int red_c[POSE_FINISH_BLOCK], red_h[POSE_FINISH_BLOCK];
    __shared__ double M[81], MV[81], Mw[POSE_FINISH_BLOCK / 64][45];
    __shared__ double Efin[9], Rc[4][9], tc[4][3];
    __shared__ float Ef[9];
    __shared__ int n_in, n_ref, good[4], refit_ok, best_c;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = npts[p];
    const float4* pp = pts + (int64_t)p * match_cap;
    uint8_t* w = ws + (int64_t)p * match_cap;

    // argmax over (count, -h): ascending scan per lane, then a fixed tree
    int bc = -1, bh = -1;
    for (int h = tid; h < H; h += POSE_FINISH_BLOCK) {
        const int c = cnt[(int64_t)p * H + h];
        if (c > bc) { bc = c; bh = h; }
    }
    red_c[tid] = bc;
    red_h[tid] = bh;
    __syncthreads();
    for (int s = POSE_FINISH_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int c2 = red_c[tid + s], h2 = red_h[tid + s];
            if (c2 > red_c[tid] || (c2 == red_c[tid] && c2 >= 0 && h2 < red_h[tid])) { red_c[tid] = c2; red_h[tid] = h2; }
        }
        __syncthreads();
    }
    const int win_c = red_c[0], win_h = red_h[0];
    aria_pose_result* o = out + p;
    uint8_t* mk = mask ? mask + (int64_t)p * match_cap : nullptr;
    if (n < 8 || win_c < 0) {
        if (mk)
            for (int i = tid; i < match_cap; i += POSE_FINISH_BLOCK) mk[i] = 0;
        if (tid == 0) {
            for (int k = 0; k < 9; k++) { o->R[k] = (k % 4 == 0) ? 1.0 : 0.0; o->E[k] = 0.0; }
            for (int k = 0; k < 3; k++) o->t[k] = 0.0;
            o->n_matches = n; o->n_inliers = 0; o->n_pose_inliers = 0; o->best_hypothesis = -1; o->refined = 0; o->valid = 0;
        }
        return;
    }
    if (tid < 9) Ef[tid] = E[((int64_t)p * 9 + tid) * H + win_h];
    if (tid == 0) { n_in = 0; n_ref = 0; good[0] = good[1] = good[2] = good[3] = 0; refit_ok = 0; }
    __syncthreads();
    {   // the winner's inliers (the same test, on the same fp32 E, as its score)
        float e[9];
        for (int k = 0; k < 9; k++) e[k] = Ef[k];
        int c = 0;
        for (int i = tid; i < n; i += POSE_FINISH_BLOCK) {
            const int in = pose_inlier(e, pp[i], thr2);
            w[i] = (uint8_t)in;
            c += in;
        }
        atomicAdd(&n_in, c);
    }
    __syncthreads();
    const int win_in = n_in;
    // refit: the normal matrix's 45 entries (r <= c) over the winner's inliers -- every thread sums its strided share of the
    // matches in match order, then a fixed xor butterfly inside each wave and the four waves' sums in wave order
    if (win_in >= 8) {
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; k++) acc[k] = 0.0;
        for (int i = tid; i < n; i += POSE_FINISH_BLOCK) {
            if (!w[i]) continue;
            double row[9];
            pose_row(pp[i], row);
            int k = 0;
#pragma unroll
            for (int r = 0; r < 9; r++)
#pragma unroll
                for (int c = r; c < 9; c++) acc[k++] += row[r] * row[c];
        }
#pragma unroll
        for (int k = 0; k < 45; k++) {
            double v = acc[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
            if ((tid & 63) == 0) Mw[tid >> 6][k] = v;
        }
        __syncthreads();
        if (tid < 45) {
            int r = 0, k = tid;
            while (k >= 9 - r) { k -= 9 - r; r++; }
            const int c = r + k;
            double v = 0.0;
            for (int wv = 0; wv < POSE_FINISH_BLOCK / 64; wv++) v = v + Mw[wv][tid];
            M[r * 9 + c] = v;
            M[c * 9 + r] = v;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < 81; i++) MV[i] = (i % 10 == 0) ? 1.0 : 0.0;
            for (int sweep = 0; sweep < 16; sweep++) {
                double off = 0.0, diag = 0.0;      // cyclic Jacobi until the off-diagonal mass is negligible
                for (int a = 0; a < 9; a++) {
                    diag = diag + fabs(M[a * 10]);
                    for (int b = a + 1; b < 9; b++) off = off + fabs(M[a * 9 + b]);
                }
                if (off <= 1e-15 * diag) break;
                for (int a = 0; a < 8; a++)
                    for (int b = a + 1; b < 9; b++) jacobi_rotate<9>((double*)M, (double*)MV, a, b);
            }
            int mi = 0;
            for (int i = 1; i < 9; i++)
                if (M[i * 10] < M[mi * 10]) mi = i;
            double f[9], e2[9], U[9], V[9];
            for (int k = 0; k < 9; k++) f[k] = MV[k * 9 + mi];
            if (project_essential(f, e2, U, V)) {
                for (int k = 0; k < 9; k++) Efin[k] = e2[k];
                refit_ok = 1;
            }
        }
        __syncthreads();
        if (refit_ok) {
            float e[9];
            for (int k = 0; k < 9; k++) e[k] = (float)Efin[k];
            int c = 0;
            for (int i = tid; i < n; i += POSE_FINISH_BLOCK) c += pose_inlier(e, pp[i], thr2);
            atomicAdd(&n_ref, c);
        }
        __syncthreads();
    }
    const bool refined = refit_ok && n_ref >= win_in;
    __syncthreads();
    if (tid < 9) {
        if (refined) Ef[tid] = (float)Efin[tid];
        else Efin[tid] = (double)Ef[tid];
    }
    __syncthreads();
    if (refined) {   // the RANSAC mask of the refitted model
        float e[9];
        for (int k = 0; k < 9; k++) e[k] = Ef[k];
        for (int i = tid; i < n; i += POSE_FINISH_BLOCK) w[i] = (uint8_t)pose_inlier(e, pp[i], thr2);
    }
    const int final_in = refined ? n_ref : win_in;
    // decomposeEssentialMat: R1 = U W V^T, R2 = U W^T V^T, t = u3; candidates (R1, t), (R2, t), (R1, -t), (R2, -t)
    if (tid == 0) {
        double e[9], e2[9], U[9], V[9];
        for (int k = 0; k < 9; k++) e[k] = Efin[k];
        if (project_essential(e, e2, U, V)) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) {
                    // U W = [-u2, u1, u3]... W = [[0,1,0],[-1,0,0],[0,0,1]]: (U W)[:,0] = -u2, [:,1] = u1, [:,2] = u3
                    const double r1 = -U[r * 3 + 1] * V[c * 3 + 0] + U[r * 3 + 0] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2];
                    // U W^T = [u2, -u1, u3]
                    const double r2 = U[r * 3 + 1] * V[c * 3 + 0] - U[r * 3 + 0] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2];
                    Rc[0][r * 3 + c] = r1; Rc[2][r * 3 + c] = r1;
                    Rc[1][r * 3 + c] = r2; Rc[3][r * 3 + c] = r2;
                }
            for (int r = 0; r < 3; r++) {
                tc[0][r] = tc[1][r] = U[r * 3 + 2];
                tc[2][r] = tc[3][r] = -U[r * 3 + 2];
            }
        } else {
            for (int c = 0; c < 4; c++) {
                for (int k = 0; k < 9; k++) Rc[c][k] = (k % 4 == 0) ? 1.0 : 0.0;
                for (int k = 0; k < 3; k++) tc[c][k] = 0.0;
            }
        }
    }
    __syncthreads();
    {
        int g[4] = {0, 0, 0, 0};
        for (int i = tid; i < n; i += POSE_FINISH_BLOCK) {
            if (!w[i]) continue;
            const float4 q = pp[i];
            for (int c = 0; c < 4; c++) g[c] += pose_cheiral(Rc[c], tc[c], q, dist);
        }
        for (int c = 0; c < 4; c++) atomicAdd(&good[c], g[c]);
    }
    __syncthreads();
    if (tid == 0) {   // recoverPose's order of preference
        const int g1 = good[0], g2 = good[1], g3 = good[2], g4 = good[3];
        best_c = (g1 >= g2 && g1 >= g3 && g1 >= g4) ? 0 : (g2 >= g3 && g2 >= g4) ? 1 : (g3 >= g4) ? 2 : 3;
    }
    __syncthreads();
    const int bcand = best_c;
    if (mk) {
        for (int i = tid; i < match_cap; i += POSE_FINISH_BLOCK)
            mk[i] = (i < n && w[i]) ? (uint8_t)pose_cheiral(Rc[bcand], tc[bcand], pp[i], dist) : (uint8_t)0;
    }
    if (tid == 0) {
        for (int k = 0; k < 9; k++) { o->R[k] = Rc[bcand][k]; o->E[k] = Efin[k]; }
        for (int k = 0; k < 3; k++) o->t[k] = tc[bcand][k];
        o->n_matches = n; o->n_inliers = final_in; o->n_pose_inliers = good[bcand]; o->best_hypothesis = win_h;
        o->refined = refined ? 1 : 0; o->valid = 1;
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_pose_s : StageHandle {
    aria_pose_config cfg{};
    // grow-only workspace of the batch path
    DeviceBuffer<float4> d_pts;           // [n_pairs][match_cap]
    DeviceBuffer<int> d_npts;             // [n_pairs]
    DeviceBuffer<float> d_E;              // [n_pairs][9][H]
    DeviceBuffer<int> d_cnt;              // [n_pairs][H]
    DeviceBuffer<uint8_t> d_ws;           // [n_pairs][match_cap] inlier flags
    PairStaging pair;                     // aria_pose_estimate, aria_pose_debug_hypotheses
    DeviceBuffer<aria_pose_result> d_res;
    DeviceBuffer<int> d_dbg;
};

namespace {

float pose_thr2(const aria_pose_config& c) { return normalized_thr2(c.threshold_px, c.fx, c.fy); }

int enqueue(aria_pose_t h, const aria_keypoint* d_kq, const int* d_nq, const aria_keypoint* d_kt, const int* d_nt,
            int64_t kp_stride, const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap, int query_is_first,
            int pair_base, aria_pose_result* d_out, uint8_t* d_mask, int* d_dbg, bool finish) {
    const int H = h->cfg.hypotheses;
    int rc;
    if ((rc = h->d_pts.reserve(h->stream, (size_t)n_pairs * match_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_ws.reserve(h->stream, (size_t)n_pairs * match_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_npts.reserve(h->stream, (size_t)n_pairs)) != ARIA_OK) return rc;
    if ((rc = h->d_E.reserve(h->stream, (size_t)n_pairs * H * 9)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, (size_t)n_pairs * H)) != ARIA_OK) return rc;
    const aria_pose_config& c = h->cfg;
    hipLaunchKernelGGL(k_pose_stage, dim3(n_pairs), dim3(256), 0, h->stream, d_kq, d_nq, d_kt, d_nt, kp_stride, d_matches,
                       d_nmatches, match_cap, query_is_first ? 1 : 0, c.fx, c.fy, c.cx, c.cy, h->d_pts, h->d_npts, h->d_err);
    hipLaunchKernelGGL(k_pose_hyp, dim3(n_pairs, H / 64), dim3(64), 0, h->stream, h->d_pts, h->d_npts, match_cap, H,
                       (uint64_t)c.seed, pair_base, h->d_E, h->d_cnt, d_dbg);
    hipLaunchKernelGGL(k_pose_score, dim3(n_pairs, (H + POSE_SCORE_BLOCK - 1) / POSE_SCORE_BLOCK), dim3(POSE_SCORE_BLOCK), 0,
                       h->stream, h->d_pts, h->d_npts, match_cap, H, h->d_E, h->d_cnt, pose_thr2(c));
    if (finish)
        hipLaunchKernelGGL(k_pose_finish, dim3(n_pairs), dim3(POSE_FINISH_BLOCK), 0, h->stream, h->d_pts, h->d_npts, match_cap,
                           H, h->d_E, h->d_cnt, pose_thr2(c), c.distance_thresh, h->d_ws, d_mask, d_out);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

// the batch form over the one staged pair
int enqueue_staged(aria_pose_t h, int query_is_first, int pair_base, int* d_dbg, bool finish) {
    const PairStaging& s = h->pair;
    return enqueue(h, s.d_kq, s.d_counts, s.d_kt, s.d_counts + 1, s.kp_stride, s.d_m, s.d_counts + 2, 1, s.match_cap, query_is_first,
                   pair_base, finish ? h->d_res.p : nullptr, finish ? s.d_mask.p : nullptr, d_dbg, finish);
}

}  // namespace

extern "C" {

void aria_pose_default_config(aria_pose_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_pose_config);
    c->device = 0;
    c->stream = nullptr;
    c->hypotheses = 1024;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0 (src/legacy/EuRoCReader.cpp:11-17)
    c->threshold_px = 1.0;
    c->distance_thresh = 50.0;
    c->seed = 0;
}

int aria_pose_create(const aria_pose_config* c, aria_pose_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_pose_config)) return ARIA_E_INVALID;
    if (c->hypotheses < 64 || c->hypotheses > 16384 || (c->hypotheses % 64)) return ARIA_E_INVALID;
    if (bad_pinhole(c->fx, c->fy, c->cx, c->cy) || !(c->threshold_px > 0) || !(c->distance_thresh > 0)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_pose_create", [](aria_pose_s* h) {
        const int rc = h->pair.create(h->stream);
        return rc != ARIA_OK ? rc : h->d_res.reserve(h->stream, 1, "aria_pose_create");
    });
}

void aria_pose_destroy(aria_pose_t h) { stage_destroy(h); }

void* aria_pose_stream(aria_pose_t h) { return stage_stream(h); }

int aria_pose_check(aria_pose_t h) { return stage_check(h, {{ERRBIT_POSE_INPUT, ARIA_E_INVALID}}); }

int aria_pose_estimate_batch_device(aria_pose_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                    const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                    const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                    int query_is_first, int pair_base, aria_pose_result* d_out, uint8_t* d_mask) {
    if (!h || !d_kp_query || !d_nq || !d_kp_train || !d_nt || !d_matches || !d_nmatches || !d_out || n_pairs < 0 ||
        match_cap < 1 || match_cap > (1 << 20) || kp_stride < 0 || pair_base < 0)
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return enqueue(h, d_kp_query, d_nq, d_kp_train, d_nt, kp_stride, d_matches, d_nmatches, n_pairs, match_cap, query_is_first,
                   pair_base, d_out, d_mask, nullptr, true);
}

int aria_pose_estimate(aria_pose_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                       const aria_match* matches, int n_matches, int query_is_first, int pair_base, aria_pose_result* out,
                       uint8_t* mask) {
    if (!h || !out || pair_base < 0 || n_matches > (1 << 20)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->pair.upload(h->stream, kp_query, nq, kp_train, nt, matches, n_matches);
    if (rc != ARIA_OK) return rc;
    if ((rc = enqueue_staged(h, query_is_first, pair_base, nullptr, true)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(out, h->d_res, sizeof(aria_pose_result), hipMemcpyDeviceToHost, h->stream));
    if (mask && n_matches) ARIA_HIP(hipMemcpyAsync(mask, h->pair.d_mask, (size_t)n_matches, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_pose_check(h);
}

int aria_pose_debug_hypotheses(aria_pose_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                               const aria_match* matches, int n_matches, int query_is_first, int pair_base, int* sample_idx,
                               float* E, int* counts) {
    if (!h || !sample_idx || !E || !counts || pair_base < 0 || n_matches > (1 << 20)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = h->pair.upload(h->stream, kp_query, nq, kp_train, nt, matches, n_matches);
    if (rc != ARIA_OK) return rc;
    const int H = h->cfg.hypotheses;
    if ((rc = h->d_dbg.reserve(h->stream, (size_t)H * 8)) != ARIA_OK) return rc;
    if ((rc = enqueue_staged(h, query_is_first, pair_base, h->d_dbg, false)) != ARIA_OK) return rc;
    std::vector<float> soa((size_t)9 * H);
    ARIA_HIP(hipMemcpyAsync(sample_idx, h->d_dbg, sizeof(int) * 8 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(soa.data(), h->d_E, sizeof(float) * 9 * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(counts, h->d_cnt, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    unpack_models(soa.data(), H, 0, 9, E);
    return aria_pose_check(h);
}

}  // extern "C"
