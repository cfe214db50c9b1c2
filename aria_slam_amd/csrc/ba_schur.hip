// Local bundle adjustment, batched over windows (include/aria_orb_hip.h, "local bundle adjustment"): the poses and points of a
// sliding window refined together under Levenberg-Marquardt, the points eliminated by a Schur complement.
// aria_slam_amd/ba_ref.py is the specification; DESIGN.md section 25 the record.
//
// One kernel, k_ba_lm: ONE WORKGROUP PER WINDOW, persistent over every LM iteration and trial of its window, workgroup
// barriers only (the shape of k_graph_lm). Nothing waits on another workgroup.
//   stage      validate the counts and the records before anything they index is read; the used mask; every point's
//              observation range (the list is sorted by point); a per-pose observation list by a counting sort whose counts
//              are per lane and per pose (no atomics): a list sorted by point stays sorted by point.
//   point side one lane per point over its contiguous range: V, bp, and W_o = w Jc^T Jp per observation into HBM scratch.
//   pose side  one WAVE per free pose over its list: the 21 + 6 entries of U and bc, finished by a wave butterfly. In LDS.
//   trial      one lane per point: Vd^-1 through its 3x3 Cholesky factor and E_o = W_o Vd^-1 per observation;
//              one WAVE per lower block (i, k) of S: lanes stride pose i's list, each scans its point's range (<= 16
//              entries) for pose k and accumulates E_o W_o'^T privately, a wave butterfly finishes the block -- no barrier
//              and no cross-wave sum inside the build; S (96 x 96 fp64, rows padded to 97) lives in LDS;
//              Cholesky by the workgroup (two barriers per column), the two triangular solves by one wave in registers;
//              back-substitution and updates a lane per point or pose; chi2 a lane per observation with the fixed tree.
//              A rejected trial restores the points from a backup in HBM scratch and the poses from one in LDS.
// fp64 throughout, -ffp-contract=off, no float atomics: every sum's order depends on the window alone, so results are
// bitwise reproducible and independent of the window's place in a batch and of the slot it runs in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "solver_device.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int BA_BLOCK = 512;             // 8 waves: 2 per SIMD, 256 VGPRs each
constexpr int BA_WAVES = BA_BLOCK / 64;
constexpr int BA_P = ARIA_BA_MAX_POSES;
constexpr int BA_N = 6 * BA_P;            // rows of the reduced system
constexpr int BA_LD = BA_N + 1;           // padded row: a column read touches every bank once
constexpr int ERRBIT_BA_INPUT = 1;
constexpr int ERRBIT_BA_CAPACITY = 2;     // track builder: more points or observations than the caller's capacity

struct BaArgs {
    double* poses;
    const uint8_t* pose_fixed;
    double* points;
    const uint8_t* point_fixed;
    const aria_ba_obs* obs;
    const int *n_poses, *n_points, *n_obs;
    int pose_cap, point_cap, obs_cap;
    aria_ba_result* out;
    uint8_t* used;
    double fx, fy, cx, cy, huber, min_depth;
    int iterations, window_base, mode;
    double dbg_lambda;
    double* dbg;          // mode 1: S (BA_N x BA_N, lower blocks) then g (BA_N)
    double* dscr;
    int* iscr;
    int* err;
};

// per-window slice of the handle's scratch
__host__ __device__ inline size_t ba_slot_doubles(int Np, int No) { return 18 * (size_t)Np + 36 * (size_t)No; }
__host__ __device__ inline size_t ba_slot_ints(int Np, int No) { return 2 * (size_t)Np + 1 + 2 * (size_t)No; }

struct Scratch {
    double *xbak, *V, *bp, *Vi, *W, *E;   // [3], [6], [3], [6] per point; [18], [18] per observation
    int *pstart, *pfree, *used, *plist;
};

__device__ inline Scratch scratch_of(double* d, int* i, int slot, int Np, int No) {
    Scratch s;
    d += (size_t)slot * ba_slot_doubles(Np, No);
    s.xbak = d;  s.V = s.xbak + 3 * (size_t)Np;  s.bp = s.V + 6 * (size_t)Np;  s.Vi = s.bp + 3 * (size_t)Np;
    s.W = s.Vi + 6 * (size_t)Np;  s.E = s.W + 18 * (size_t)No;
    i += (size_t)slot * ba_slot_ints(Np, No);
    s.pstart = i;  s.pfree = s.pstart + Np + 1;  s.used = s.pfree + Np;  s.plist = s.used + No;
    return s;
}

struct Lds {
    double S[BA_N * BA_LD];        // the reduced system; the counting sort's counters before the first linearisation
    double U[BA_P * 21], bc[BA_P * 6];
    double P[BA_P * 12], Pbak[BA_P * 12];
    double g[BA_N], dc[BA_N], dl[BA_N];
    double red[2 * 2 * BA_WAVES];
    int poff[BA_P + 1], tot[BA_P], fidx[BA_P], fpose[BA_P];
    int nfree, nused, phase;
};

// threadIdx.x through an opaque copy: it is invariant over the whole kernel, and the addresses derived from it would
// otherwise be hoisted out of the LM loops and held (and spilled) across everything else (k_graph_lm's remedy).
__device__ inline int tid_here() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__device__ constexpr int tri3(int a, int c) { return a <= c ? 3 * a - a * (a - 1) / 2 + (c - a) : 3 * c - c * (c - 1) / 2 + (a - c); }

// ---- one observation ------------------------------------------------------------------------------------------------------
struct Cam { double fx, fy, cx, cy, huber, min_depth; };

// residual and depth
__device__ inline void obs_residual(const double* P, const double* X, const aria_ba_obs& ob, const Cam& K, double& r0,
                                    double& r1, double* Xc) {
#pragma unroll
    for (int r = 0; r < 3; r++) Xc[r] = (P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2]) + P[4 * r + 3];
    r0 = K.fx * Xc[0] / Xc[2] + K.cx - (double)ob.u;
    r1 = K.fy * Xc[1] / Xc[2] + K.cy - (double)ob.v;
}

// Huber: weight, and the cost of e2 = |r|^2
__device__ inline double huber_weight(double e2, double delta, double& cost) {
    const double e = sqrt(e2);
    if (delta > 0.0 && e > delta) {
        cost = 2.0 * delta * e - delta * delta;
        return delta / e;
    }
    cost = e2;
    return 1.0;
}

// Jc (2x6, parameters (w, v)) and Jp (2x3) at the state
__device__ inline void obs_jacobians(const double* P, const double* Xc, const Cam& K, double* Jc, double* Jp) {
    const double x = Xc[0], y = Xc[1], z = Xc[2];
    const double a00 = K.fx / z, a02 = -K.fx * x / (z * z), a11 = K.fy / z, a12 = -K.fy * y / (z * z);
    Jc[0] = a02 * y;             Jc[1] = a00 * z - a02 * x;  Jc[2] = -a00 * y;  Jc[3] = a00;  Jc[4] = 0.0;  Jc[5] = a02;
    Jc[6] = a12 * y - a11 * z;   Jc[7] = -a12 * x;           Jc[8] = a11 * x;   Jc[9] = 0.0;  Jc[10] = a11; Jc[11] = a12;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        Jp[c] = a00 * P[c] + a02 * P[8 + c];
        Jp[3 + c] = a11 * P[4 + c] + a12 * P[8 + c];
    }
}

// ---- the point side: V, bp and W_o at the state; returns the largest diagonal entry of V over this lane's free points -------
__device__ inline double point_pass(const Lds& L, const BaArgs& A, const double* points, const aria_ba_obs* obs, int npts,
                                    const Scratch& S, const Cam& K) {
    double mx = 0.0;
    for (int j = tid_here(); j < npts; j += BA_BLOCK) {
        const double X[3] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
        double V[6] = {0, 0, 0, 0, 0, 0}, bp[3] = {0, 0, 0};
        const int o0 = S.pstart[j], o1 = S.pstart[j + 1];
        const bool fr = S.pfree[j] != 0;
        for (int o = o0; o < o1; o++) {
            if (!S.used[o]) continue;
            const aria_ba_obs ob = obs[o];
            double Xc[3], r0, r1, cost, Jc[12], Jp[6];
            obs_residual(L.P + 12 * ob.pose, X, ob, K, r0, r1, Xc);
            const double w = huber_weight(r0 * r0 + r1 * r1, K.huber, cost);
            obs_jacobians(L.P + 12 * ob.pose, Xc, K, Jc, Jp);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                bp[a] -= w * (Jp[a] * r0 + Jp[3 + a] * r1);
#pragma unroll
                for (int c = a; c < 3; c++) V[tri3(a, c)] += w * (Jp[a] * Jp[c] + Jp[3 + a] * Jp[3 + c]);
            }
            if (fr) {
                double* Wo = S.W + 18 * (size_t)o;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int c = 0; c < 3; c++) Wo[3 * a + c] = w * (Jc[a] * Jp[c] + Jc[6 + a] * Jp[3 + c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 6; c++) S.V[6 * (size_t)j + c] = V[c];
#pragma unroll
        for (int c = 0; c < 3; c++) S.bp[3 * (size_t)j + c] = bp[c];
        if (fr) mx = fmax(mx, fmax(V[0], fmax(V[3], V[5])));
    }
    return mx;
}

// ---- the pose side: U and bc of every free pose, one wave per pose over its list; returns the largest diagonal entry ----------
__device__ inline double pose_pass(Lds& L, const double* points, const aria_ba_obs* obs, int nposes, const Scratch& S,
                                   const Cam& K) {
    const int th = tid_here(), lane = th & 63, wv = th >> 6;
    double mx = 0.0;
    for (int i = wv; i < nposes; i += BA_WAVES) {
        if (L.fidx[i] < 0) continue;
        double U[21], bc[6];
#pragma unroll
        for (int c = 0; c < 21; c++) U[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) bc[c] = 0.0;
        const int e1 = L.poff[i + 1];
        for (int e = L.poff[i] + lane; e < e1; e += 64) {
            const int o = S.plist[e];
            const aria_ba_obs ob = obs[o];
            const double X[3] = {points[3 * (size_t)ob.point], points[3 * (size_t)ob.point + 1], points[3 * (size_t)ob.point + 2]};
            double Xc[3], r0, r1, cost, Jc[12], Jp[6];
            obs_residual(L.P + 12 * i, X, ob, K, r0, r1, Xc);
            const double w = huber_weight(r0 * r0 + r1 * r1, K.huber, cost);
            obs_jacobians(L.P + 12 * i, Xc, K, Jc, Jp);
#pragma unroll
            for (int a = 0; a < 6; a++) {
                bc[a] -= w * (Jc[a] * r0 + Jc[6 + a] * r1);
#pragma unroll
                for (int c = a; c < 6; c++) U[tri6(a, c)] += w * (Jc[a] * Jc[c] + Jc[6 + a] * Jc[6 + c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 21; c++) U[c] = wave_sum(U[c]);
#pragma unroll
        for (int c = 0; c < 6; c++) bc[c] = wave_sum(bc[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 21; c++) L.U[21 * i + c] = U[c];
#pragma unroll
            for (int c = 0; c < 6; c++) L.bc[6 * i + c] = bc[c];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) mx = fmax(mx, U[tri6(a, a)]);
    }
    return mx;
}

// ---- a trial's point side: Vd^-1 and E_o = W_o Vd^-1. Returns nonzero when some Vd is not positive definite ---------------------
__device__ inline int point_trial(int npts, double lambda, const Scratch& S) {
    int bad = 0;
    for (int j = tid_here(); j < npts; j += BA_BLOCK) {
        if (!S.pfree[j]) continue;
        const double* V = S.V + 6 * (size_t)j;
        const double a = V[0] + lambda, b = V[1], c = V[2], d = V[3] + lambda, e = V[4], f = V[5] + lambda;
        // Cholesky of [[a b c], [b d e], [c e f]]
        bool ok = a > 0.0 && a < INFINITY;
        const double l00 = sqrt(ok ? a : 1.0);
        const double l10 = b / l00, l20 = c / l00;
        const double d1 = d - l10 * l10;
        ok = ok && d1 > 0.0 && d1 < INFINITY;
        const double l11 = sqrt(ok ? d1 : 1.0);
        const double l21 = (e - l20 * l10) / l11;
        const double d2 = f - l20 * l20 - l21 * l21;
        ok = ok && d2 > 0.0 && d2 < INFINITY;
        const double l22 = sqrt(ok ? d2 : 1.0);
        if (!ok) { bad = 1;  continue; }
        // M = L^-1 (lower), Vd^-1 = M^T M
        const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
        const double m10 = -l10 * m00 / l11;
        const double m21 = -l21 * m11 / l22;
        const double m20 = -(l20 * m00 + l21 * m10) / l22;
        double Vi[6];
        Vi[0] = m00 * m00 + m10 * m10 + m20 * m20;  Vi[1] = m10 * m11 + m20 * m21;  Vi[2] = m20 * m22;
        Vi[3] = m11 * m11 + m21 * m21;              Vi[4] = m21 * m22;              Vi[5] = m22 * m22;
#pragma unroll
        for (int q = 0; q < 6; q++) S.Vi[6 * (size_t)j + q] = Vi[q];
        const int o1 = S.pstart[j + 1];
        for (int o = S.pstart[j]; o < o1; o++) {
            if (!S.used[o]) continue;
            const double* Wo = S.W + 18 * (size_t)o;
            double* Eo = S.E + 18 * (size_t)o;
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int q = 0; q < 3; q++)
                    Eo[3 * r + q] = Wo[3 * r] * Vi[tri3(0, q)] + Wo[3 * r + 1] * Vi[tri3(1, q)] + Wo[3 * r + 2] * Vi[tri3(2, q)];
        }
    }
    return bad;
}

// ---- the reduced system: one wave per lower block (a, b) of the free poses ------------------------------------------------------
__device__ inline void build_reduced(Lds& L, const aria_ba_obs* obs, double lambda, const Scratch& S) {
    const int th = tid_here(), lane = th & 63, wv = th >> 6;
    const int nf = L.nfree, nblk = nf * (nf + 1) / 2;
    for (int q = wv; q < nblk; q += BA_WAVES) {
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= q) a++;
        const int b = q - a * (a + 1) / 2;
        const int i = L.fpose[a], k = L.fpose[b];
        double acc[36], ag[6];
#pragma unroll
        for (int c = 0; c < 36; c++) acc[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) ag[c] = 0.0;
        const int e1 = L.poff[i + 1];
        for (int e = L.poff[i] + lane; e < e1; e += 64) {
            const int o = S.plist[e];
            const int j = obs[o].point;
            if (!S.pfree[j]) continue;
            int o2 = -1;
            if (a == b) {
                o2 = o;
            } else {
                const int s1 = S.pstart[j + 1];
                for (int s = S.pstart[j]; s < s1; s++)
                    if (obs[s].pose == k && S.used[s]) o2 = s;
            }
            if (o2 < 0) continue;
            const double* Eo = S.E + 18 * (size_t)o;
            const double* Wk = S.W + 18 * (size_t)o2;
            double Er[18], Wr[18];
#pragma unroll
            for (int c = 0; c < 18; c++) { Er[c] = Eo[c];  Wr[c] = Wk[c]; }
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 6; c++)
                    acc[6 * r + c] += Er[3 * r] * Wr[3 * c] + Er[3 * r + 1] * Wr[3 * c + 1] + Er[3 * r + 2] * Wr[3 * c + 2];
            if (a == b) {
                const double* bp = S.bp + 3 * (size_t)j;
#pragma unroll
                for (int r = 0; r < 6; r++) ag[r] += Er[3 * r] * bp[0] + Er[3 * r + 1] * bp[1] + Er[3 * r + 2] * bp[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 36; c++) acc[c] = wave_sum(acc[c]);
        if (a == b) {
#pragma unroll
            for (int c = 0; c < 6; c++) ag[c] = wave_sum(ag[c]);
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double v = -acc[6 * r + c];
                    if (a == b) v = (L.U[21 * i + tri6(r, c)] + (r == c ? lambda : 0.0)) - acc[6 * r + c];
                    L.S[(6 * a + r) * BA_LD + 6 * b + c] = v;
                }
            if (a == b) {
#pragma unroll
                for (int r = 0; r < 6; r++) L.g[6 * a + r] = L.bc[6 * i + r] - ag[r];
            }
        }
    }
}

// ---- Cholesky of S's lower triangle in place (the diagonal keeps d, its root goes to dl). Returns false on a bad pivot ----------
__device__ inline bool cholesky_lds(Lds& L, int n) {
    for (int j = 0; j < n; j++) {
        const int th = tid_here(), ti = th >> 5, tk = th & 31;
        const double d = L.S[j * BA_LD + j];
        if (!(d > 0.0) || !(d < INFINITY)) return false;     // the same value in every lane
        const double l = sqrt(d);
        if (th == 0) L.dl[j] = l;
        for (int r = j + 1 + th; r < n; r += BA_BLOCK) L.S[r * BA_LD + j] = L.S[r * BA_LD + j] / l;
        __syncthreads();
        for (int r = j + 1 + ti; r < n; r += BA_BLOCK / 32) {
            const double lr = L.S[r * BA_LD + j];
            for (int c = j + 1 + tk; c <= r; c += 32) L.S[r * BA_LD + c] -= lr * L.S[c * BA_LD + j];
        }
        __syncthreads();
    }
    return true;
}

// ---- L y = g, L^T x = y by wave 0, the vector in registers (rows lane and lane + 64); x to L.dc -----------------------------------
__device__ inline void solve_lds(Lds& L, int n) {
    const int lane = tid_here();
    if (lane >= 64) return;
    const int r0 = lane, r1 = lane + 64;
    double v0 = r0 < n ? L.g[r0] : 0.0, v1 = r1 < n ? L.g[r1] : 0.0;
    for (int j = 0; j < n; j++) {
        const double src = j < 64 ? v0 : v1;
        const double y = __shfl(src, j & 63, 64) / L.dl[j];
        if (r0 == j) v0 = y;
        if (r1 == j) v1 = y;
        if (r0 > j && r0 < n) v0 -= L.S[r0 * BA_LD + j] * y;
        if (r1 > j && r1 < n) v1 -= L.S[r1 * BA_LD + j] * y;
    }
    for (int j = n - 1; j >= 0; j--) {
        const double src = j < 64 ? v0 : v1;
        const double x = __shfl(src, j & 63, 64) / L.dl[j];
        if (r0 == j) v0 = x;
        if (r1 == j) v1 = x;
        if (r0 < j) v0 -= L.S[j * BA_LD + r0] * x;
        if (r1 < j) v1 -= L.S[j * BA_LD + r1] * x;
    }
    if (r0 < n) L.dc[r0] = v0;
    if (r1 < n) L.dc[r1] = v1;
}

// R <- Exp(w) R, t <- Exp(w) t + v on the 12 doubles of [R t]
__device__ inline void pose_update(double* P, const double* x) {
    double E[9];
    exp_so3(x, E);
    double Q[12];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Q[4 * r + c] = E[r * 3] * P[c] + E[r * 3 + 1] * P[4 + c] + E[r * 3 + 2] * P[8 + c];
        Q[4 * r + 3] = (E[r * 3] * P[3] + E[r * 3 + 1] * P[7] + E[r * 3 + 2] * P[11]) + x[3 + r];
    }
#pragma unroll
    for (int c = 0; c < 12; c++) P[c] = Q[c];
}

// chi2 and sum e^2 over the used observations at the state; bad = some used observation at or behind min_depth
__device__ inline void chi2_pass(Lds& L, int& phase, const double* points, const aria_ba_obs* obs, int nobs, const Scratch& S,
                                 const Cam& K, double& chi2, double& e2sum, int& bad) {
    double c2 = 0.0, es = 0.0;
    int b = 0;
    for (int o = tid_here(); o < nobs; o += BA_BLOCK) {
        if (!S.used[o]) continue;
        const aria_ba_obs ob = obs[o];
        const double X[3] = {points[3 * (size_t)ob.point], points[3 * (size_t)ob.point + 1], points[3 * (size_t)ob.point + 2]};
        double Xc[3], r0, r1, cost;
        obs_residual(L.P + 12 * ob.pose, X, ob, K, r0, r1, Xc);
        if (!(Xc[2] > K.min_depth)) { b = 1;  continue; }
        const double e2 = r0 * r0 + r1 * r1;
        huber_weight(e2, K.huber, cost);
        c2 += cost;
        es += e2;
    }
    block_sum2<BA_WAVES>(L.red, phase, c2, es);
    bad = __syncthreads_or(b);
    chi2 = c2;
    e2sum = es;
}

__device__ inline bool finite_d(double v) { return v == v && v < INFINITY && v > -INFINITY; }

// ---- the kernel -------------------------------------------------------------------------------------------------------------
// mode 0: optimise. mode 1 (aria_ba_debug_linearize): linearise once, damp with dbg_lambda, write S and g to dbg; V and bp
// stay in slot 0 of the scratch for the host to read.
__global__ __launch_bounds__(BA_BLOCK) void k_ba_lm(const BaArgs A) {
    __shared__ Lds L;
    const int tid = threadIdx.x;
    const int slot = blockIdx.x;
    const int win = A.window_base + slot;
    int phase = 0;
    const Cam K{A.fx, A.fy, A.cx, A.cy, A.huber, A.min_depth};

    aria_ba_result res;
    res.chi2_initial = res.chi2_final = res.lambda = res.rms_px = 0.0;
    res.n_obs_used = res.iterations_done = res.trials = 0;
    res.stop_reason = STOP_INVALID;
    res.valid = 0;
    res.reserved = 0;

    // ---- validate before anything the records index is read
    const int nposes = A.n_poses[win], npts = A.n_points[win], nobs = A.n_obs[win];
    double* poses = A.poses + (size_t)win * A.pose_cap * 12;
    const uint8_t* pose_fixed = A.pose_fixed + (size_t)win * A.pose_cap;
    double* points = A.points + (size_t)win * A.point_cap * 3;
    const uint8_t* point_fixed = A.point_fixed + (size_t)win * A.point_cap;
    const aria_ba_obs* obs = A.obs + (size_t)win * A.obs_cap;
    uint8_t* used_out = A.used ? A.used + (size_t)win * A.obs_cap : nullptr;
    int bad = nposes < 0 || nposes > BA_P || nposes > A.pose_cap || npts < 0 || npts > A.point_cap || nobs < 0 ||
              nobs > A.obs_cap;
    if (!bad) {
        int b = 0;
        for (int o = tid; o < nobs; o += BA_BLOCK) {
            const aria_ba_obs ob = obs[o];
            if (ob.point < 0 || ob.point >= npts || ob.pose < 0 || ob.pose >= nposes) b = 1;
            if (!finite_d((double)ob.u) || !finite_d((double)ob.v)) b = 1;
            if (o > 0) {
                const aria_ba_obs pr = obs[o - 1];
                if (!(pr.point < ob.point || (pr.point == ob.point && pr.pose < ob.pose))) b = 1;
            }
        }
        for (int c = tid; c < nposes * 12; c += BA_BLOCK) b |= !finite_d(poses[c]);
        for (int c = tid; c < npts * 3; c += BA_BLOCK) b |= !finite_d(points[c]);
        bad = b;
    }
    if (__syncthreads_or(bad)) {
        if (used_out)
            for (int o = tid; o < A.obs_cap; o += BA_BLOCK) used_out[o] = 0;
        if (tid == 0) {
            atomicOr(A.err, ERRBIT_BA_INPUT);
            A.out[win] = res;
        }
        return;
    }
    res.valid = 1;
    res.stop_reason = STOP_ITERATIONS;
    const Scratch S = scratch_of(A.dscr, A.iscr, slot, max(A.point_cap, 1), max(A.obs_cap, 1));

    // ---- stage: poses to LDS, the free poses, the used mask, the point ranges
    for (int c = tid; c < nposes * 12; c += BA_BLOCK) L.P[c] = poses[c];
    if (tid == 0) {
        int nf = 0;
        for (int i = 0; i < BA_P; i++) {
            const bool fr = i < nposes && pose_fixed[i] == 0;
            L.fidx[i] = fr ? nf : -1;
            if (fr) L.fpose[nf++] = i;
        }
        L.nfree = nf;
        L.nused = 0;
    }
    __syncthreads();
    {
        int cnt = 0;
        for (int o = tid; o < nobs; o += BA_BLOCK) {
            const aria_ba_obs ob = obs[o];
            const double* X = points + 3 * (size_t)ob.point;
            const double* P = L.P + 12 * ob.pose;
            const double z = (P[8] * X[0] + P[9] * X[1] + P[10] * X[2]) + P[11];
            const int u = z > K.min_depth ? 1 : 0;
            S.used[o] = u;
            cnt += u;
        }
        if (used_out)
            for (int o = tid; o < A.obs_cap; o += BA_BLOCK) used_out[o] = 0;
        if (cnt) atomicAdd(&L.nused, cnt);        // an integer count: its order changes nothing
    }
    for (int j = tid; j <= npts; j += BA_BLOCK) {         // lower bound of point j in the sorted list
        int lo = 0, hi = nobs;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (obs[mid].point < j) lo = mid + 1; else hi = mid;
        }
        S.pstart[j] = lo;
    }
    __syncthreads();
    if (used_out)
        for (int o = tid; o < nobs; o += BA_BLOCK) used_out[o] = (uint8_t)S.used[o];
    for (int j = tid; j < npts; j += BA_BLOCK) {
        int n = 0;
        for (int o = S.pstart[j]; o < S.pstart[j + 1]; o++) n += S.used[o];
        S.pfree[j] = (point_fixed[j] == 0 && n >= 2) ? 1 : 0;
    }
    res.n_obs_used = L.nused;

    // ---- the per-pose lists: counting sort by pose with per-lane counters (in S's storage), stable, so sorted by point
    {
        int* cnt = reinterpret_cast<int*>(L.S);            // [BA_P][BA_BLOCK]
        const int chunk = (nobs + BA_BLOCK - 1) / BA_BLOCK;
        const int lo = min(tid * chunk, nobs), hi = min(lo + chunk, nobs);
        for (int i = 0; i < BA_P; i++) cnt[i * BA_BLOCK + tid] = 0;
        for (int o = lo; o < hi; o++)
            if (S.used[o]) cnt[obs[o].pose * BA_BLOCK + tid]++;
        __syncthreads();
        if (tid < BA_P) {
            int run = 0;
            for (int t = 0; t < BA_BLOCK; t++) {
                const int c = cnt[tid * BA_BLOCK + t];
                cnt[tid * BA_BLOCK + t] = run;
                run += c;
            }
            L.tot[tid] = run;
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int i = 0; i < BA_P; i++) { L.poff[i] = run;  run += L.tot[i]; }
            L.poff[BA_P] = run;
        }
        __syncthreads();
        for (int o = lo; o < hi; o++)
            if (S.used[o]) {
                const int i = obs[o].pose;
                S.plist[L.poff[i] + cnt[i * BA_BLOCK + tid]++] = o;
            }
        __syncthreads();
    }

    // ---- linearise at the input state
    double chi2, e2sum;
    int behind;
    chi2_pass(L, phase, points, obs, nobs, S, K, chi2, e2sum, behind);
    double mx = point_pass(L, A, points, obs, npts, S, K);
    mx = fmax(mx, pose_pass(L, points, obs, nposes, S, K));
    const double maxdiag = block_max<BA_WAVES>(L.red, phase, mx);   // its barrier publishes V, bp, W, U and bc
    res.chi2_initial = res.chi2_final = chi2;
    const int n = 6 * L.nfree;
    if (A.mode == 1) {
        point_trial(npts, A.dbg_lambda, S);
        __syncthreads();
        build_reduced(L, obs, A.dbg_lambda, S);
        __syncthreads();
        for (int c = tid; c < n * n; c += BA_BLOCK) {
            const int r = c / n, q = c % n;
            A.dbg[c] = (q / 6 <= r / 6) ? L.S[r * BA_LD + q] : L.S[q * BA_LD + r];
        }
        for (int c = tid; c < n; c += BA_BLOCK) A.dbg[(size_t)BA_N * BA_N + c] = L.g[c];
        if (tid == 0) A.out[win] = res;
        return;
    }
    LmDamping lm;
    lm.start(maxdiag);

    for (int it = 0; it < A.iterations; it++) {
        bool accepted = false;
        for (int trial = 0; trial < LM_MAX_TRIALS; trial++) {
            res.trials++;
            const int tid = tid_here();
            bool solved = !__syncthreads_or(point_trial(npts, lm.lambda, S));     // barrier: Vd^-1 and E are visible
            if (solved) {
                build_reduced(L, obs, lm.lambda, S);
                __syncthreads();
                solved = cholesky_lds(L, n);
            }
            double chi2_new = INFINITY, e2_new = INFINITY, rho = 0.0;
            if (solved) {
                solve_lds(L, n);
                __syncthreads();
                // updates (with backups) and the gain's denominator dx.(lambda dx + b)
                double den = 0.0;
                if (tid < nposes && L.fidx[tid] >= 0) {
                    double Pn[12], d[6];
#pragma unroll
                    for (int c = 0; c < 12; c++) { Pn[c] = L.P[12 * tid + c];  L.Pbak[12 * tid + c] = Pn[c]; }
#pragma unroll
                    for (int c = 0; c < 6; c++) {
                        d[c] = L.dc[6 * L.fidx[tid] + c];
                        den += d[c] * (lm.lambda * d[c] + L.bc[6 * tid + c]);
                    }
                    pose_update(Pn, d);
#pragma unroll
                    for (int c = 0; c < 12; c++) L.P[12 * tid + c] = Pn[c];
                }
                for (int j = tid; j < npts; j += BA_BLOCK) {
                    if (!S.pfree[j]) continue;
                    double rhs[3] = {S.bp[3 * (size_t)j], S.bp[3 * (size_t)j + 1], S.bp[3 * (size_t)j + 2]};
                    const double bpj[3] = {rhs[0], rhs[1], rhs[2]};
                    const int o1 = S.pstart[j + 1];
                    for (int o = S.pstart[j]; o < o1; o++) {
                        if (!S.used[o]) continue;
                        const int f = L.fidx[obs[o].pose];
                        if (f < 0) continue;
                        const double* Wo = S.W + 18 * (size_t)o;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            double t = 0.0;
#pragma unroll
                            for (int r = 0; r < 6; r++) t += Wo[3 * r + c] * L.dc[6 * f + r];
                            rhs[c] -= t;
                        }
                    }
                    const double* Vi = S.Vi + 6 * (size_t)j;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const double dx = Vi[tri3(c, 0)] * rhs[0] + Vi[tri3(c, 1)] * rhs[1] + Vi[tri3(c, 2)] * rhs[2];
                        const double x = points[3 * (size_t)j + c];
                        S.xbak[3 * (size_t)j + c] = x;
                        points[3 * (size_t)j + c] = x + dx;
                        den += dx * (lm.lambda * dx + bpj[c]);
                    }
                }
                double zero = 0.0;
                block_sum2<BA_WAVES>(L.red, phase, den, zero);   // barrier: the new state is visible
                den += 1e-3;
                int bh;
                chi2_pass(L, phase, points, obs, nobs, S, K, chi2_new, e2_new, bh);
                if (bh || !finite_d(chi2_new)) chi2_new = INFINITY;
                rho = (chi2 - chi2_new) / den;
            }
            if (solved && rho > 0.0 && chi2_new < INFINITY) {
                chi2 = chi2_new;
                e2sum = e2_new;
                point_pass(L, A, points, obs, npts, S, K);
                pose_pass(L, points, obs, nposes, S, K);
                __syncthreads();
                lm.accept(rho);
                accepted = true;
                break;
            }
            if (solved) {
                if (tid < nposes && L.fidx[tid] >= 0) {
#pragma unroll
                    for (int c = 0; c < 12; c++) L.P[12 * tid + c] = L.Pbak[12 * tid + c];
                }
                for (int j = tid; j < npts; j += BA_BLOCK) {
                    if (!S.pfree[j]) continue;
#pragma unroll
                    for (int c = 0; c < 3; c++) points[3 * (size_t)j + c] = S.xbak[3 * (size_t)j + c];
                }
                __syncthreads();
            }
            lm.reject();
        }
        if (!accepted) {
            res.stop_reason = STOP_TRIALS;
            break;
        }
        res.iterations_done++;
    }
    // the free poses go back; a fixed pose was never written
    if (tid < nposes && L.fidx[tid] >= 0) {
#pragma unroll
        for (int c = 0; c < 12; c++) poses[12 * (size_t)tid + c] = L.P[12 * tid + c];
    }
    res.chi2_final = chi2;
    res.lambda = lm.lambda;
    res.rms_px = res.n_obs_used > 0 ? sqrt(e2sum / (double)res.n_obs_used) : 0.0;
    if (tid == 0) A.out[win] = res;
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_ba_s : StageHandle {
    aria_ba_config cfg{};
    DeviceBuffer<double> d_scr;      // [max_windows] ba_slot_doubles
    DeviceBuffer<int> i_scr;         // [max_windows] ba_slot_ints
    DeviceBuffer<double> d_dbg;      // S and g of aria_ba_debug_linearize
    // single-window staging (aria_ba_optimize, aria_ba_debug_linearize)
    DeviceBuffer<double> d_poses, d_points;
    DeviceBuffer<uint8_t> d_bytes;   // pose_fixed [16], point_fixed [point cap], used [obs cap]
    DeviceBuffer<aria_ba_obs> d_obs;
    DeviceBuffer<int> d_counts;      // n_poses, n_points, n_obs
    DeviceBuffer<aria_ba_result> d_res;
    DeviceBuffer<int> d_table;       // track builder: [windows][15 pairs][kp_stride] view-1 index -> lowest match index
    DeviceBuffer<int> d_wflag;       // track builder: per window, nonzero = refused
};

namespace {

int ba_launch(aria_ba_t h, double* d_poses, const uint8_t* d_pose_fixed, double* d_points, const uint8_t* d_point_fixed,
              const aria_ba_obs* d_obs, const int* d_np, const int* d_npts, const int* d_nobs, int n_windows, int pose_cap,
              int point_cap, int obs_cap, int iterations, aria_ba_result* d_out, uint8_t* d_used, int mode, double dbg_lambda) {
    const aria_ba_config& c = h->cfg;
    const int Np = std::max(point_cap, 1), No = std::max(obs_cap, 1);
    int rc;
    if ((rc = h->d_scr.reserve(h->stream, (size_t)c.max_windows * ba_slot_doubles(Np, No))) != ARIA_OK) return rc;
    if ((rc = h->i_scr.reserve(h->stream, (size_t)c.max_windows * ba_slot_ints(Np, No))) != ARIA_OK) return rc;
    BaArgs a{};
    a.poses = d_poses;  a.pose_fixed = d_pose_fixed;  a.points = d_points;  a.point_fixed = d_point_fixed;  a.obs = d_obs;
    a.n_poses = d_np;  a.n_points = d_npts;  a.n_obs = d_nobs;
    a.pose_cap = pose_cap;  a.point_cap = point_cap;  a.obs_cap = obs_cap;
    a.out = d_out;  a.used = d_used;
    a.fx = c.fx;  a.fy = c.fy;  a.cx = c.cx;  a.cy = c.cy;  a.huber = c.huber_px;  a.min_depth = c.min_depth;
    a.iterations = iterations > 0 ? iterations : c.max_iterations;
    a.mode = mode;  a.dbg_lambda = dbg_lambda;  a.dbg = h->d_dbg;
    a.dscr = h->d_scr;  a.iscr = h->i_scr;  a.err = h->d_err;
    // more windows than the handle has scratch slots run as consecutive launches on the stream; a window's result does
    // not depend on which launch or which slot it gets
    for (int base = 0; base < n_windows; base += c.max_windows) {
        a.window_base = base;
        hipLaunchKernelGGL(k_ba_lm, dim3(std::min(c.max_windows, n_windows - base)), dim3(BA_BLOCK), 0, h->stream, a);
    }
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

// uploads one window (host buffers) into the single-window staging
int ba_stage_single(aria_ba_t h, const double* poses, const uint8_t* pose_fixed, int n_poses, const double* points,
                    const uint8_t* point_fixed, int n_points, const aria_ba_obs* obs, int n_obs) {
    if (n_poses < 0 || n_points < 0 || n_obs < 0 || (n_poses && (!poses || !pose_fixed)) ||
        (n_points && (!points || !point_fixed)) || (n_obs && !obs))
        return ARIA_E_INVALID;
    const int Pc = std::max(n_poses, 1), Np = std::max(n_points, 1), No = std::max(n_obs, 1);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = h->d_poses.reserve(st, 12 * (size_t)Pc)) != ARIA_OK) return rc;
    if ((rc = h->d_points.reserve(st, 3 * (size_t)Np)) != ARIA_OK) return rc;
    if ((rc = h->d_bytes.reserve(st, (size_t)Pc + Np + No)) != ARIA_OK) return rc;
    if ((rc = h->d_obs.reserve(st, (size_t)No)) != ARIA_OK) return rc;
    const int counts[3] = {n_poses, n_points, n_obs};
    if (n_poses) {
        ARIA_HIP(hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 12 * (size_t)n_poses, hipMemcpyHostToDevice, st));
        ARIA_HIP(hipMemcpyAsync(h->d_bytes, pose_fixed, (size_t)n_poses, hipMemcpyHostToDevice, st));
    }
    if (n_points) {
        ARIA_HIP(hipMemcpyAsync(h->d_points, points, sizeof(double) * 3 * (size_t)n_points, hipMemcpyHostToDevice, st));
        ARIA_HIP(hipMemcpyAsync(h->d_bytes + Pc, point_fixed, (size_t)n_points, hipMemcpyHostToDevice, st));
    }
    if (n_obs) ARIA_HIP(hipMemcpyAsync(h->d_obs, obs, sizeof(aria_ba_obs) * (size_t)n_obs, hipMemcpyHostToDevice, st));
    ARIA_HIP(memcpy_on(st, h->d_counts, counts, sizeof(counts), hipMemcpyHostToDevice));
    return ARIA_OK;
}

}  // namespace

extern "C" {

void aria_ba_default_config(aria_ba_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_ba_config);
    c->device = 0;
    c->stream = nullptr;
    c->fx = 458.654;  c->fy = 457.296;  c->cx = 367.215;  c->cy = 248.375;
    c->huber_px = std::sqrt(5.991);
    c->min_depth = 1e-6;
    c->max_iterations = 10;
    c->max_windows = 256;
}

int aria_ba_create(const aria_ba_config* c, aria_ba_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_ba_config)) return ARIA_E_INVALID;
    if (c->max_iterations < 1 || c->max_iterations > 100 || c->max_windows < 1 || c->max_windows > 65535 ||
        !(c->huber_px >= 0) || !std::isfinite(c->huber_px) || !(c->min_depth >= 0) || !std::isfinite(c->min_depth) ||
        !std::isfinite(c->fx) || !std::isfinite(c->fy) || !std::isfinite(c->cx) || !std::isfinite(c->cy) || c->fx == 0 ||
        c->fy == 0)
        return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_ba_create", [](aria_ba_s* h) {
        const char* what = "aria_ba_create";
        int rc;
        if ((rc = h->d_counts.reserve(h->stream, 4, what)) != ARIA_OK) return rc;
        if ((rc = h->d_res.reserve(h->stream, 1, what)) != ARIA_OK) return rc;
        return h->d_dbg.reserve(h->stream, (size_t)BA_N * BA_N + BA_N, what);
    });
}

void aria_ba_destroy(aria_ba_t h) { stage_destroy(h); }

void* aria_ba_stream(aria_ba_t h) { return stage_stream(h); }

int aria_ba_check(aria_ba_t h) {
    return stage_check(h, {{ERRBIT_BA_INPUT, ARIA_E_INVALID}, {ERRBIT_BA_CAPACITY, ARIA_E_OUTPUT_TOO_SMALL}});
}

int aria_ba_optimize_batch_device(aria_ba_t h, double* d_poses, const uint8_t* d_pose_fixed, double* d_points,
                                  const uint8_t* d_point_fixed, const aria_ba_obs* d_obs, const int* d_n_poses,
                                  const int* d_n_points, const int* d_n_obs, int n_windows, int pose_cap, int point_cap,
                                  int obs_cap, int iterations, aria_ba_result* d_out, uint8_t* d_used) {
    if (!h || !d_poses || !d_pose_fixed || !d_points || !d_point_fixed || !d_obs || !d_n_poses || !d_n_points || !d_n_obs ||
        !d_out || n_windows < 0 || pose_cap < 0 || point_cap < 0 || obs_cap < 0 || iterations < 0 || iterations > 100)
        return ARIA_E_INVALID;
    if (n_windows == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return ba_launch(h, d_poses, d_pose_fixed, d_points, d_point_fixed, d_obs, d_n_poses, d_n_points, d_n_obs, n_windows,
                     pose_cap, point_cap, obs_cap, iterations, d_out, d_used, 0, 0.0);
}

int aria_ba_optimize(aria_ba_t h, double* poses_inout, const uint8_t* pose_fixed, int n_poses, double* points_inout,
                     const uint8_t* point_fixed, int n_points, const aria_ba_obs* obs, int n_obs, int iterations,
                     aria_ba_result* result, uint8_t* used) {
    if (!h || !result || iterations < 0 || iterations > 100) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = ba_stage_single(h, poses_inout, pose_fixed, n_poses, points_inout, point_fixed, n_points, obs, n_obs);
    if (rc != ARIA_OK) return rc;
    const int Pc = std::max(n_poses, 1), Np = std::max(n_points, 1), No = std::max(n_obs, 1);
    uint8_t* d_used = h->d_bytes + Pc + Np;
    rc = ba_launch(h, h->d_poses, h->d_bytes, h->d_points, h->d_bytes + Pc, h->d_obs, h->d_counts, h->d_counts + 1,
                   h->d_counts + 2, 1, Pc, Np, No, iterations, h->d_res, d_used, 0, 0.0);
    if (rc != ARIA_OK) return rc;
    hipStream_t st = h->stream;
    if (n_poses) ARIA_HIP(hipMemcpyAsync(poses_inout, h->d_poses, sizeof(double) * 12 * (size_t)n_poses, hipMemcpyDeviceToHost, st));
    if (n_points) ARIA_HIP(hipMemcpyAsync(points_inout, h->d_points, sizeof(double) * 3 * (size_t)n_points, hipMemcpyDeviceToHost, st));
    if (used && n_obs) ARIA_HIP(hipMemcpyAsync(used, d_used, (size_t)n_obs, hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipMemcpyAsync(result, h->d_res, sizeof(aria_ba_result), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipStreamSynchronize(st));
    return aria_ba_check(h);
}

int aria_ba_debug_linearize(aria_ba_t h, const double* poses, const uint8_t* pose_fixed, int n_poses, const double* points,
                            const uint8_t* point_fixed, int n_points, const aria_ba_obs* obs, int n_obs, double lambda,
                            double* chi2, int* n_obs_used, double* S, double* g, double* V, double* bp) {
    if (!h || !chi2 || !n_obs_used || !S || !g || !V || !bp) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = ba_stage_single(h, poses, pose_fixed, n_poses, points, point_fixed, n_points, obs, n_obs);
    if (rc != ARIA_OK) return rc;
    const int Pc = std::max(n_poses, 1), Np = std::max(n_points, 1), No = std::max(n_obs, 1);
    rc = ba_launch(h, h->d_poses, h->d_bytes, h->d_points, h->d_bytes + Pc, h->d_obs, h->d_counts, h->d_counts + 1,
                   h->d_counts + 2, 1, Pc, Np, No, 1, h->d_res, nullptr, 1, lambda);
    if (rc != ARIA_OK) return rc;
    hipStream_t st = h->stream;
    std::vector<double> dbg((size_t)BA_N * BA_N + BA_N), Vt(6 * (size_t)Np), bt(3 * (size_t)Np);
    aria_ba_result res;
    // slot 0 of the scratch: V behind the 3 backup doubles per point, bp behind V (scratch_of)
    ARIA_HIP(hipMemcpyAsync(dbg.data(), h->d_dbg, sizeof(double) * dbg.size(), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipMemcpyAsync(Vt.data(), h->d_scr + 3 * (size_t)Np, sizeof(double) * Vt.size(), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipMemcpyAsync(bt.data(), h->d_scr + 9 * (size_t)Np, sizeof(double) * bt.size(), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipMemcpyAsync(&res, h->d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipStreamSynchronize(st));
    rc = aria_ba_check(h);
    if (rc != ARIA_OK) return rc;
    *chi2 = res.chi2_initial;
    *n_obs_used = res.n_obs_used;
    int nf = 0;
    for (int i = 0; i < n_poses; i++) nf += pose_fixed[i] == 0;
    const int n = 6 * nf;
    for (int c = 0; c < n * n; c++) S[c] = dbg[c];
    for (int c = 0; c < n; c++) g[c] = dbg[(size_t)BA_N * BA_N + c];
    for (int j = 0; j < n_points; j++) {
        const double* v = Vt.data() + 6 * (size_t)j;
        const double full[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]};
        for (int c = 0; c < 9; c++) V[9 * (size_t)j + c] = full[c];
        for (int c = 0; c < 3; c++) bp[3 * (size_t)j + c] = bt[3 * (size_t)j + c];
    }
    return ARIA_OK;
}

}  // extern "C"

// ---- the track builder (ba_ref.window_from_chain): integers and copies only, equal to the restatement bit for bit -------------
// k_ba_link_table: per window and pair, view-1 keypoint index -> lowest match index (the table of the absolute-pose join).
// k_ba_link_emit: one workgroup per window walks the arena in its order, tile by tile: count (a lane per point follows its
// track through the tables), scan (wave prefix, then the four waves' sums), emit. Arena order in, arena order out.
namespace {

constexpr int LINK_BLOCK = 256;
constexpr int LINK_WAVES = LINK_BLOCK / 64;
constexpr int LINK_PAIRS = BA_P - 1;
constexpr int LINK_EMPTY = 0x7F7F7F7F;

struct LinkArgs {
    const aria_map_point* arena;
    const long long* d_size;
    long long capacity;
    const int *pair_first, *n_pairs;
    int pair_base, n_chain;
    const aria_keypoint *kp1, *kp2;
    const int *n1, *n2;
    long long kp_stride;
    const aria_match* matches;
    const int* nmatches;
    int match_cap, query_is_first, point_cap, obs_cap;
    double* points;
    aria_ba_obs* obs;
    int *point_src, *n_points, *n_obs;
    int *table, *wflag, *err;
};

// the window's pairs lie in the chain, and every count of theirs is in range
__device__ inline bool link_window_ok(const LinkArgs& A, int b, int& q0, int& np) {
    np = A.n_pairs[b];
    q0 = A.pair_first[b] - A.pair_base;
    if (np < 1 || np > LINK_PAIRS || q0 < 0 || q0 > A.n_chain - np) return false;
    for (int q = q0; q < q0 + np; q++)
        if (A.nmatches[q] < 0 || A.nmatches[q] > A.match_cap || A.n1[q] < 0 || A.n1[q] > A.kp_stride || A.n2[q] < 0 ||
            A.n2[q] > A.kp_stride)
            return false;
    return true;
}

__global__ __launch_bounds__(LINK_BLOCK) void k_ba_link_table(const LinkArgs A) {
    const int b = blockIdx.y, w = blockIdx.x;          // window, pair of the window
    int q0, np;
    if (!link_window_ok(A, b, q0, np)) {
        if (threadIdx.x == 0 && w == 0) A.wflag[b] = 1;
        return;
    }
    if (w >= np) return;
    const int q = q0 + w;
    const aria_match* m = A.matches + (size_t)q * A.match_cap;
    int* tab = A.table + ((size_t)b * LINK_PAIRS + w) * A.kp_stride;
    const int nm = A.nmatches[q], n1 = A.n1[q], n2 = A.n2[q];
    int bad = 0;
    for (int k = threadIdx.x; k < nm; k += LINK_BLOCK) {
        const int i1 = A.query_is_first ? m[k].query_idx : m[k].train_idx;
        const int i2 = A.query_is_first ? m[k].train_idx : m[k].query_idx;
        if (i1 < 0 || i1 >= n1 || i2 < 0 || i2 >= n2) bad = 1;
        else atomicMin(&tab[i1], k);                    // integers: the lowest match index, whatever the order
    }
    if (bad) A.wflag[b] = 1;
}

__global__ __launch_bounds__(LINK_BLOCK) void k_ba_link_emit(const LinkArgs A) {
    __shared__ int wsum[2][2][LINK_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int q0, np;
    const bool ok = link_window_ok(A, b, q0, np);
    long long pbase = 0, obase = 0;
    int bad = 0, full = 0;
    if (ok) {
        const long long size = A.capacity > 0 ? min(*A.d_size, A.capacity) : 0;
        const int first = A.pair_first[b];
        const int* tab = A.table + (size_t)b * LINK_PAIRS * A.kp_stride;
        double* out_x = A.points + (size_t)b * A.point_cap * 3;
        aria_ba_obs* out_o = A.obs + (size_t)b * A.obs_cap;
        int* out_s = A.point_src + (size_t)b * A.point_cap;
        int par = 0;
        for (long long base = 0; base < size; base += LINK_BLOCK, par ^= 1) {
            const long long pos = base + tid;
            int isp = 0, no = 0, f = 0, i1 = 0, i2 = 0;
            if (pos < size) {
                const int pair = A.arena[pos].pair;
                if (pair >= first && pair < first + np) {
                    f = pair - first;
                    i1 = A.arena[pos].idx1;
                    i2 = A.arena[pos].idx2;
                    if (i1 < 0 || i1 >= A.n1[q0 + f] || i2 < 0 || i2 >= A.n2[q0 + f]) {
                        bad = 1;
                    } else {
                        isp = 1;
                        no = 2;
                        int cur = i2;
                        for (int w = f + 1; w < np; w++) {          // the first pair without a match from `cur` ends the track
                            const int k = tab[(size_t)w * A.kp_stride + cur];
                            if (k == LINK_EMPTY) break;
                            const aria_match mk = A.matches[(size_t)(q0 + w) * A.match_cap + k];
                            cur = A.query_is_first ? mk.train_idx : mk.query_idx;
                            no++;
                        }
                    }
                }
            }
            // scan: inclusive prefix inside the wave, then the waves' sums in order
            int sp = isp, so = no;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int tp = __shfl_up(sp, d, 64), to = __shfl_up(so, d, 64);
                if (lane >= d) { sp += tp;  so += to; }
            }
            if (lane == 63) { wsum[par][0][wv] = sp;  wsum[par][1][wv] = so; }
            __syncthreads();                                     // the other parity's sums are free again after this barrier
            int bp = 0, bo = 0, tp = 0, to = 0;
#pragma unroll
            for (int w = 0; w < LINK_WAVES; w++) {
                if (w < wv) { bp += wsum[par][0][w];  bo += wsum[par][1][w]; }
                tp += wsum[par][0][w];
                to += wsum[par][1][w];
            }
            if (isp) {
                const long long j = pbase + bp + sp - 1, o = obase + bo + so - no;
                if (j >= A.point_cap || o + no > A.obs_cap) {
                    full = 1;
                } else {
                    const aria_map_point mp = A.arena[pos];
                    out_x[3 * j] = mp.X[0];  out_x[3 * j + 1] = mp.X[1];  out_x[3 * j + 2] = mp.X[2];
                    out_s[j] = (int)pos;
                    const aria_keypoint k1 = A.kp1[(size_t)(q0 + f) * A.kp_stride + i1];
                    const aria_keypoint k2 = A.kp2[(size_t)(q0 + f) * A.kp_stride + i2];
                    out_o[o] = aria_ba_obs{(int)j, f, k1.x, k1.y};
                    out_o[o + 1] = aria_ba_obs{(int)j, f + 1, k2.x, k2.y};
                    int cur = i2, n = 2;
                    for (int w = f + 1; w < np; w++) {
                        const int k = tab[(size_t)w * A.kp_stride + cur];
                        if (k == LINK_EMPTY) break;
                        const aria_match mk = A.matches[(size_t)(q0 + w) * A.match_cap + k];
                        cur = A.query_is_first ? mk.train_idx : mk.query_idx;
                        const aria_keypoint kk = A.kp2[(size_t)(q0 + w) * A.kp_stride + cur];
                        out_o[o + n] = aria_ba_obs{(int)j, w + 1, kk.x, kk.y};
                        n++;
                    }
                }
            }
            pbase += tp;
            obase += to;
        }
    }
    const int any_bad = __syncthreads_or(bad), any_full = __syncthreads_or(full);
    if (tid == 0) {
        const bool wrong = !ok || A.wflag[b] || any_bad;
        const bool refuse = wrong || any_full;
        if (refuse) atomicOr(A.err, wrong ? ERRBIT_BA_INPUT : ERRBIT_BA_CAPACITY);
        A.n_points[b] = refuse ? 0 : (int)pbase;
        A.n_obs[b] = refuse ? 0 : (int)obase;
    }
}

}  // namespace

extern "C" int aria_ba_window_from_chain_device(aria_ba_t h, aria_map_t map, const int* d_pair_first, const int* d_n_pairs,
                                                int n_windows, int pair_base, int n_chain_pairs, const aria_keypoint* d_kp1,
                                                const int* d_n1, const aria_keypoint* d_kp2, const int* d_n2, int64_t kp_stride,
                                                const aria_match* d_matches, const int* d_nmatches, int match_cap,
                                                int query_is_first, int point_cap, int obs_cap, double* d_points,
                                                aria_ba_obs* d_obs, int* d_point_src, int* d_n_points, int* d_n_obs) {
    if (!h || !map || !d_pair_first || !d_n_pairs || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches || !d_nmatches ||
        !d_points || !d_obs || !d_point_src || !d_n_points || !d_n_obs || n_windows < 0 || n_windows > 65535 ||
        n_chain_pairs < 0 || kp_stride < 1 || kp_stride > (1 << 24) || match_cap < 1 || point_cap < 0 || obs_cap < 0)
        return ARIA_E_INVALID;
    if (n_windows == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    LinkArgs a{};
    int map_device = -1;
    int64_t capacity = 0;
    map_device_view(map, &a.arena, &a.d_size, &capacity, &map_device);
    if (map_device != h->device) return ARIA_E_INVALID;          // the builder reads the map's arena where it lies
    const size_t cells = (size_t)n_windows * LINK_PAIRS * (size_t)kp_stride;
    int rc;
    if ((rc = h->d_table.reserve(h->stream, cells)) != ARIA_OK) return rc;
    if ((rc = h->d_wflag.reserve(h->stream, (size_t)n_windows)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemsetAsync(h->d_table, 0x7F, cells * sizeof(int), h->stream));
    ARIA_HIP(hipMemsetAsync(h->d_wflag, 0, (size_t)n_windows * sizeof(int), h->stream));
    a.capacity = a.arena ? (long long)capacity : 0;
    a.pair_first = d_pair_first;  a.n_pairs = d_n_pairs;  a.pair_base = pair_base;  a.n_chain = n_chain_pairs;
    a.kp1 = d_kp1;  a.kp2 = d_kp2;  a.n1 = d_n1;  a.n2 = d_n2;  a.kp_stride = kp_stride;
    a.matches = d_matches;  a.nmatches = d_nmatches;  a.match_cap = match_cap;  a.query_is_first = query_is_first ? 1 : 0;
    a.point_cap = point_cap;  a.obs_cap = obs_cap;
    a.points = d_points;  a.obs = d_obs;  a.point_src = d_point_src;  a.n_points = d_n_points;  a.n_obs = d_n_obs;
    a.table = h->d_table;  a.wflag = h->d_wflag;  a.err = h->d_err;
    hipLaunchKernelGGL(k_ba_link_table, dim3(LINK_PAIRS, n_windows), dim3(LINK_BLOCK), 0, h->stream, a);
    hipLaunchKernelGGL(k_ba_link_emit, dim3(n_windows), dim3(LINK_BLOCK), 0, h->stream, a);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}
