// Trajectory evaluation on the device (include/aria_orb_hip.h, "trajectory evaluation"): ground-truth sampling
// (EuRoCReader::getGroundTruth), the reference's ATE / RPE and the Umeyama-aligned ATE / RPE, batched. fp64 throughout.
// aria_slam_amd/eval_ref.py is the definition; the arithmetic below follows it operation by operation except for the order
// of the sums, which is a fixed tree here and sequential there.
//
// k_truth_scan     grid-stride over the ground-truth rows: non-finite field or decreasing timestamp -> one int flag.
// k_truth_sample   one lane per query: lower bound, clamp or lerp / slerp.
// k_traj_eval      one workgroup of 256 per trajectory, three strided passes over its poses (sums; centred covariance;
//                  aligned residuals), every pass reduced by a 64-lane butterfly and a fixed sum over the four waves. The
//                  3x3 SVD (one-sided Jacobi on the covariance itself) is evaluated redundantly by every lane from
//                  identical inputs, which saves a broadcast and a barrier.
// No float atomics: the only atomic is the integer OR on the deferred-error word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int ERRBIT_EVAL_INPUT = 1;
constexpr int EVAL_BLOCK = 256;
constexpr int EVAL_WAVES = EVAL_BLOCK / 64;
constexpr int EVAL_MAX_GRID = 32768;      // trajectories per launch (aria_orb_hip.h: larger calls are split)
constexpr int SCAN_BLOCK = 256;
constexpr int TRUTH_DOUBLES = 17;
static_assert(sizeof(aria_eval_truth) == TRUTH_DOUBLES * sizeof(double), "aria_eval_truth is 17 packed doubles");
static_assert(sizeof(aria_eval_result) == 200, "aria_eval_result layout");

__device__ inline bool finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// ---- ground-truth sampling ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_BLOCK) void k_truth_scan(const aria_eval_truth* __restrict__ gt, int n_gt, int* __restrict__ flag) {
    bool bad = false;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n_gt; i += (int)(gridDim.x * blockDim.x)) {
        const double* r = (const double*)(gt + i);
#pragma unroll
        for (int k = 0; k < TRUTH_DOUBLES; k++) bad |= !isfinite(r[k]);
        if (i > 0) bad |= !(gt[i - 1].t <= r[0]);
    }
    if (bad) atomicOr(flag, 1);
}

__device__ inline void lerp3(const double* a, const double* b, double alpha, double* o) {
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = (1.0 - alpha) * a[k] + alpha * b[k];
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_truth_sample(const aria_eval_truth* __restrict__ gt, int n_gt,
                                                             const double* __restrict__ ts, int n, const int* __restrict__ flag,
                                                             aria_eval_truth* __restrict__ out, int* __restrict__ valid,
                                                             int* __restrict__ err) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    aria_eval_truth o;
    double* od = (double*)&o;
#pragma unroll
    for (int k = 0; k < TRUTH_DOUBLES; k++) od[k] = 0.0;
    const double t = ts[i];
    if (n_gt < 1 || *flag != 0 || !isfinite(t)) {
        out[i] = o;
        if (valid) valid[i] = 0;
        atomicOr(err, ERRBIT_EVAL_INPUT);
        return;
    }
    int lo = 0, hi = n_gt;                   // first row with timestamp >= t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (gt[mid].t < t) lo = mid + 1; else hi = mid;
    }
    if (lo == n_gt) {
        o = gt[n_gt - 1];
    } else if (lo == 0) {
        o = gt[0];
    } else {
        const aria_eval_truth a = gt[lo - 1], b = gt[lo];
        const double alpha = (t - a.t) / (b.t - a.t);
        o.t = t;
        lerp3(a.p, b.p, alpha, o.p);
        lerp3(a.v, b.v, alpha, o.v);
        lerp3(a.bg, b.bg, alpha, o.bg);
        lerp3(a.ba, b.ba, alpha, o.ba);
        const double d = ((a.q[0] * b.q[0] + a.q[1] * b.q[1]) + a.q[2] * b.q[2]) + a.q[3] * b.q[3];
        const double ad = fabs(d);
        double w0, w1;
        if (ad >= 1.0 - 0x1p-52) {
            w0 = 1.0 - alpha;
            w1 = alpha;
        } else {
            const double th = acos(ad), sth = sin(th);
            w0 = sin((1.0 - alpha) * th) / sth;
            w1 = sin(alpha * th) / sth;
        }
        if (d < 0.0) w1 = -w1;
#pragma unroll
        for (int k = 0; k < 4; k++) o.q[k] = w0 * a.q[k] + w1 * b.q[k];
    }
    out[i] = o;
    if (valid) valid[i] = 1;
}

// ---- trajectory metrics ------------------------------------------------------------------------------------------------
struct Src {
    const char* est;
    int kind;
    const aria_eval_truth* truth;
    const uint8_t* mask;
};

__device__ inline bool pose_used(const Src& s, int i) {
    if (s.mask && s.mask[i] == 0) return false;
    if (s.kind == ARIA_EVAL_EST_FUSE_STATE) {
        const aria_fuse_state* st = (const aria_fuse_state*)s.est + i;
        return st->initialized != 0 && st->valid != 0;
    }
    return true;
}

__device__ inline void load_est(const Src& s, int i, double* e) {
    if (s.kind == ARIA_EVAL_EST_POSE12) {
        const double* r = (const double*)s.est + (size_t)12 * i;
        e[0] = r[3]; e[1] = r[7]; e[2] = r[11];
    } else if (s.kind == ARIA_EVAL_EST_FUSE_STATE) {
        const aria_fuse_state* st = (const aria_fuse_state*)s.est + i;
        e[0] = st->p[0]; e[1] = st->p[1]; e[2] = st->p[2];
    } else {
        const double* r = (const double*)s.est + (size_t)3 * i;
        e[0] = r[0]; e[1] = r[1]; e[2] = r[2];
    }
}

__device__ inline void load_truth(const Src& s, int j, double* g) {
    const double* p = s.truth[j].p;
    g[0] = p[0]; g[1] = p[1]; g[2] = p[2];
}

__device__ inline double sqnorm3(const double* d) { return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]; }

// Sum over the workgroup, the same bits in every lane: butterfly over the 64 lanes (fp addition commutes, so both partners
// of an exchange hold the same sum), then the four waves in a fixed order.
template <typename T, int N>
__device__ inline void block_sum(T (&v)[N], T* lds) {
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; k++) lds[wave * N + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = (lds[k] + lds[N + k]) + (lds[2 * N + k] + lds[3 * N + k]);
}

// One Jacobi rotation of the columns P, Q of A (3x3 row-major) and of V; returns whether it rotated.
template <int P, int Q>
__device__ inline bool jacobi_pair(double (&A)[9], double (&V)[9]) {
    const double alpha = (A[P] * A[P] + A[3 + P] * A[3 + P]) + A[6 + P] * A[6 + P];
    const double beta = (A[Q] * A[Q] + A[3 + Q] * A[3 + Q]) + A[6 + Q] * A[6 + Q];
    const double gamma = (A[P] * A[Q] + A[3 + P] * A[3 + Q]) + A[6 + P] * A[6 + Q];
    if (!(fabs(gamma) > 0x1p-52 * sqrt(alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double ap = A[3 * r + P], aq = A[3 * r + Q];
        A[3 * r + P] = c * ap - s * aq;
        A[3 * r + Q] = s * ap + c * aq;
        const double vp = V[3 * r + P], vq = V[3 * r + Q];
        V[3 * r + P] = c * vp - s * vq;
        V[3 * r + Q] = s * vp + c * vq;
    }
    return true;
}

template <int P, int Q>
__device__ inline void sort_pair(double (&A)[9], double (&V)[9], double (&sg)[3]) {
    if (sg[P] < sg[Q]) {
        double x = sg[P]; sg[P] = sg[Q]; sg[Q] = x;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            x = A[3 * r + P]; A[3 * r + P] = A[3 * r + Q]; A[3 * r + Q] = x;
            x = V[3 * r + P]; V[3 * r + P] = V[3 * r + Q]; V[3 * r + Q] = x;
        }
    }
}

__device__ inline double det3(const double (&M)[9]) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// C -> sigma (descending), R = [u1 u2 u1xu2] diag(1, 1, det V) V^T and d = det U det V. Returns false when sigma2 is not
// greater than 1e-10 sigma1 (R and d are not written then).
__device__ inline bool umeyama_rotation(const double (&Cm)[9], double (&sg)[3], double (&R)[9], double& d) {
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = Cm[k];
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rot = jacobi_pair<0, 1>(A, V);
        rot |= jacobi_pair<0, 2>(A, V);
        rot |= jacobi_pair<1, 2>(A, V);
        if (!rot) break;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) sg[c] = sqrt((A[c] * A[c] + A[3 + c] * A[3 + c]) + A[6 + c] * A[6 + c]);
    sort_pair<0, 1>(A, V, sg);
    sort_pair<0, 2>(A, V, sg);
    sort_pair<1, 2>(A, V, sg);
    if (!(sg[1] > 1e-10 * sg[0])) return false;
    double U[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        U[3 * r + 0] = A[3 * r + 0] / sg[0];
        U[3 * r + 1] = A[3 * r + 1] / sg[1];
    }
    U[2] = U[3] * U[7] - U[6] * U[4];       // u1 x u2
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
    const double du = ((A[2] * U[2] + A[5] * U[5]) + A[8] * U[8]) < 0.0 ? -1.0 : 1.0;   // sign of det U of the full SVD
    const double dv = det3(V) < 0.0 ? -1.0 : 1.0;
    d = du * dv;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            R[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + (U[3 * r + 2] * dv) * V[3 * c + 2];
    return true;
}

__device__ inline void rot3(const double (&R)[9], const double* x, double* y) {
#pragma unroll
    for (int r = 0; r < 3; r++) y[r] = (R[3 * r] * x[0] + R[3 * r + 1] * x[1]) + R[3 * r + 2] * x[2];
}

__global__ __launch_bounds__(EVAL_BLOCK) void k_traj_eval(const void* __restrict__ est, int est_kind, const int* __restrict__ offset,
                                                          int n_poses_total, int traj0, const aria_eval_truth* __restrict__ truth,
                                                          int n_truth, int truth_shared, const uint8_t* __restrict__ mask,
                                                          int align_mode, int delta, double* __restrict__ pose_err,
                                                          aria_eval_result* __restrict__ results, int* __restrict__ err) {
    __shared__ double lds[EVAL_WAVES * 12];
    const int k = traj0 + (int)blockIdx.x, tid = (int)threadIdx.x;
    const int o0 = offset[k], o1 = offset[k + 1];
    aria_eval_result* const res = results + k;      // written by lane 0 only

    // ---- the trajectory's frame: nothing of it is read before this holds
    bool range_ok = o0 >= 0 && o0 <= o1 && o1 <= n_poses_total;
    bool ok = range_ok && delta >= 1 && align_mode >= ARIA_EVAL_ALIGN_NONE && align_mode <= ARIA_EVAL_ALIGN_SIM3 &&
              est_kind >= ARIA_EVAL_EST_POSE12 && est_kind <= ARIA_EVAL_EST_XYZ;
    if (ok) ok = truth_shared ? (o1 - o0 == n_truth) : (o1 <= n_truth);
    const Src src = {(const char*)est, est_kind, truth, mask};
    const int tshift = truth_shared ? o0 : 0;      // truth record of pose i: i - tshift

    // ---- pass 1: counts, sums for the centroids, the reference's ATE and RPE
    double s1[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // sum e (3), sum g (3), sum |e - g|^2, sum of squared RPE differences
    int c1[3] = {0, 0, 0};                         // used poses, RPE pairs, non-finite
    if (ok) {
        for (int i = o0 + tid; i < o1; i += EVAL_BLOCK) {
            if (!pose_used(src, i)) continue;
            double e[3], g[3];
            load_est(src, i, e);
            load_truth(src, i - tshift, g);
            if (!finite3(e) || !finite3(g)) { c1[2] = 1; continue; }
            c1[0]++;
            const double d[3] = {e[0] - g[0], e[1] - g[1], e[2] - g[2]};
#pragma unroll
            for (int a = 0; a < 3; a++) { s1[a] += e[a]; s1[3 + a] += g[a]; }
            s1[6] += sqnorm3(d);
            if (i - o0 >= delta && pose_used(src, i - delta)) {
                double e0[3], g0[3];
                load_est(src, i - delta, e0);
                load_truth(src, i - delta - tshift, g0);
                const double dd[3] = {(e[0] - e0[0]) - (g[0] - g0[0]), (e[1] - e0[1]) - (g[1] - g0[1]), (e[2] - e0[2]) - (g[2] - g0[2])};
                const double q = sqnorm3(dd);
                if (isfinite(q)) { s1[7] += q; c1[1]++; }      // a non-finite far end is counted by its own iteration
            }
        }
    }
    block_sum(s1, lds);
    block_sum(c1, (int*)lds);
    if (ok && c1[2] != 0) ok = false;
    if (!ok) {                                     // block-uniform
        if (range_ok && pose_err)
            for (int i = o0 + tid; i < o1; i += EVAL_BLOCK) pose_err[i] = 0.0;
        if (tid == 0) {
            double* z = (double*)res;
            for (int a = 0; a < (int)(sizeof(aria_eval_result) / sizeof(double)); a++) z[a] = 0.0;
            atomicOr(err, ERRBIT_EVAL_INPUT);
        }
        return;
    }
    const int n = c1[0], pairs = c1[1];
    const double ate_raw = n > 0 ? sqrt(s1[6] / (double)n) : -1.0;
    const double rpe_raw = pairs > 0 ? sqrt(s1[7] / (double)pairs) : -1.0;

    // ---- pass 2: centred covariance and variance
    double mu_e[3] = {0, 0, 0}, mu_g[3] = {0, 0, 0};
    if (n > 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { mu_e[a] = s1[a] / (double)n; mu_g[a] = s1[3 + a] / (double)n; }
    }
    double s2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = o0 + tid; i < o1; i += EVAL_BLOCK) {
        if (!pose_used(src, i)) continue;
        double e[3], g[3];
        load_est(src, i, e);
        load_truth(src, i - tshift, g);
#pragma unroll
        for (int a = 0; a < 3; a++) { e[a] -= mu_e[a]; g[a] -= mu_g[a]; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) s2[3 * r + c] += g[r] * e[c];
        s2[9] += sqnorm3(e);
    }
    block_sum(s2, lds);

    // ---- alignment (every lane, identical inputs)
    double scale = 1.0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    double sg[3] = {0, 0, 0};
    bool aligned = n > 0;
    if (n > 0) {
        double Cm[9], Ru[9], d = 1.0;
#pragma unroll
        for (int a = 0; a < 9; a++) Cm[a] = s2[a] / (double)n;
        const double var = s2[9] / (double)n;
        const bool full = umeyama_rotation(Cm, sg, Ru, d);
        if (align_mode != ARIA_EVAL_ALIGN_NONE) {
            aligned = full && n >= 3;
            if (aligned) {
#pragma unroll
                for (int a = 0; a < 9; a++) R[a] = Ru[a];
                if (align_mode == ARIA_EVAL_ALIGN_SIM3) scale = ((sg[0] + sg[1]) + d * sg[2]) / var;
                double Rm[3];
                rot3(R, mu_e, Rm);
#pragma unroll
                for (int a = 0; a < 3; a++) t[a] = mu_g[a] - scale * Rm[a];
            }
        }
    }

    // ---- pass 3: aligned residuals
    double s3[3] = {0, 0, 0};      // sum err^2, sum err, sum of squared aligned RPE differences
    double emax = 0.0;
    for (int i = o0 + tid; i < o1; i += EVAL_BLOCK) {
        const bool u = aligned && pose_used(src, i);
        double ei = -1.0;
        if (u) {
            double e[3], g[3], Re[3];
            load_est(src, i, e);
            load_truth(src, i - tshift, g);
            rot3(R, e, Re);
            const double d[3] = {(scale * Re[0] + t[0]) - g[0], (scale * Re[1] + t[1]) - g[1], (scale * Re[2] + t[2]) - g[2]};
            const double q = sqnorm3(d);
            ei = sqrt(q);
            s3[0] += q;
            s3[1] += ei;
            emax = fmax(emax, ei);
            if (i - o0 >= delta && pose_used(src, i - delta)) {
                double e0[3], g0[3];
                load_est(src, i - delta, e0);
                load_truth(src, i - delta - tshift, g0);
                const double de[3] = {e[0] - e0[0], e[1] - e0[1], e[2] - e0[2]};
                rot3(R, de, Re);
                const double dd[3] = {scale * Re[0] - (g[0] - g0[0]), scale * Re[1] - (g[1] - g0[1]), scale * Re[2] - (g[2] - g0[2])};
                s3[2] += sqnorm3(dd);
            }
        }
        if (pose_err) pose_err[i] = ei;
    }
    block_sum(s3, lds);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) emax = fmax(emax, __shfl_xor(emax, off));
    __syncthreads();
    if ((tid & 63) == 0) lds[tid >> 6] = emax;
    __syncthreads();
    emax = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));

    if (tid == 0) {
        res->ate_raw = ate_raw;
        res->rpe_raw = rpe_raw;
        res->sigma[0] = sg[0]; res->sigma[1] = sg[1]; res->sigma[2] = sg[2];
        res->n_poses = o1 - o0;
        res->n_used = n;
        res->n_rpe_pairs = pairs;
        res->align_valid = aligned ? 1 : 0;
        res->valid = 1;
        res->reserved = 0;
        if (aligned) {
            res->scale = scale;
#pragma unroll
            for (int a = 0; a < 9; a++) res->R[a] = R[a];
#pragma unroll
            for (int a = 0; a < 3; a++) res->t[a] = t[a];
            res->ate_rmse = sqrt(s3[0] / (double)n);
            res->ate_mean = s3[1] / (double)n;
            res->ate_max = emax;
            res->rpe_aligned = pairs > 0 ? sqrt(s3[2] / (double)pairs) : -1.0;
        } else {
            res->scale = -1.0;
#pragma unroll
            for (int a = 0; a < 9; a++) res->R[a] = -1.0;
#pragma unroll
            for (int a = 0; a < 3; a++) res->t[a] = -1.0;
            res->ate_rmse = res->ate_mean = res->ate_max = res->rpe_aligned = -1.0;
        }
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_eval_s : StageHandle {   // d_err: [0] deferred error bits, [1] the sampler's scan flag
    aria_eval_config cfg{};
    // staging of the host forms, grown on demand
    DeviceBuffer<uint8_t> d_buf[6];   // bytes: each host form lays its own arrays over the slots
};

namespace {

int eval_reserve(aria_eval_t h, int k, size_t bytes) { return h->d_buf[k].reserve(h->stream, std::max<size_t>(bytes, 64)); }

size_t est_stride(int kind) {
    return kind == ARIA_EVAL_EST_POSE12 ? 12 * sizeof(double) : kind == ARIA_EVAL_EST_FUSE_STATE ? sizeof(aria_fuse_state) : 3 * sizeof(double);
}

}  // namespace

extern "C" {

void aria_eval_default_config(aria_eval_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_eval_config);
    c->device = 0;
    c->stream = nullptr;
    c->align_mode = ARIA_EVAL_ALIGN_SIM3;
    c->rpe_delta = 10;
}

int aria_eval_create(const aria_eval_config* c, aria_eval_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_eval_config)) return ARIA_E_INVALID;
    return stage_create(c, out, 2, "aria_eval_create", [](aria_eval_s*) { return (int)ARIA_OK; });
}

void aria_eval_destroy(aria_eval_t h) { stage_destroy(h); }

void* aria_eval_stream(aria_eval_t h) { return stage_stream(h); }

int aria_eval_check(aria_eval_t h) { return stage_check(h, {{ERRBIT_EVAL_INPUT, ARIA_E_INVALID}}); }

int aria_eval_sample_truth_device(aria_eval_t h, const aria_eval_truth* d_gt, int n_gt, const double* d_ts, int n,
                                  aria_eval_truth* d_out, int* d_valid) {
    if (!h || n_gt < 0 || n < 0 || (n_gt && !d_gt) || (n && (!d_ts || !d_out))) return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int* flag = h->d_err + 1;
    ARIA_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
    if (n_gt > 0) {
        const int blocks = std::min((n_gt + SCAN_BLOCK - 1) / SCAN_BLOCK, 2048);
        hipLaunchKernelGGL(k_truth_scan, dim3(blocks), dim3(SCAN_BLOCK), 0, h->stream, d_gt, n_gt, flag);
        ARIA_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_truth_sample, dim3((n + SCAN_BLOCK - 1) / SCAN_BLOCK), dim3(SCAN_BLOCK), 0, h->stream, d_gt, n_gt, d_ts, n,
                       flag, d_out, d_valid, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_eval_sample_truth(aria_eval_t h, const aria_eval_truth* gt, int n_gt, const double* ts, int n, aria_eval_truth* out,
                           int* valid) {
    if (!h || n_gt < 0 || n < 0 || (n_gt && !gt) || (n && (!ts || !out))) return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t M = (size_t)n_gt, N = (size_t)n;
    int rc;
    if ((rc = eval_reserve(h, 0, M * sizeof(aria_eval_truth))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 1, N * sizeof(double))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 2, N * sizeof(aria_eval_truth))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 3, N * sizeof(int))) != ARIA_OK) return rc;
    hipStream_t st = h->stream;
    if (M) ARIA_HIP(hipMemcpyAsync(h->d_buf[0], gt, M * sizeof(aria_eval_truth), hipMemcpyHostToDevice, st));
    ARIA_HIP(memcpy_on(st, h->d_buf[1], ts, N * sizeof(double), hipMemcpyHostToDevice));
    rc = aria_eval_sample_truth_device(h, (const aria_eval_truth*)h->d_buf[0].p, n_gt, (const double*)h->d_buf[1].p, n,
                                       (aria_eval_truth*)h->d_buf[2].p, (int*)h->d_buf[3].p);
    if (rc != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(out, h->d_buf[2], N * sizeof(aria_eval_truth), hipMemcpyDeviceToHost, st));
    if (valid) ARIA_HIP(hipMemcpyAsync(valid, h->d_buf[3], N * sizeof(int), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipStreamSynchronize(st));
    return aria_eval_check(h);
}

int aria_eval_batch_device(aria_eval_t h, const void* d_est, int est_kind, const int* d_offset, int n_poses_total, int n_traj,
                           const aria_eval_truth* d_truth, int n_truth, int truth_shared, const uint8_t* d_mask, int align_mode,
                           int rpe_delta, double* d_pose_err, aria_eval_result* d_results) {
    if (!h || !d_offset || !d_results || n_traj < 0 || n_poses_total < 0 || n_truth < 0 || (n_poses_total && !d_est) ||
        (n_truth && !d_truth) || n_traj > (1 << 26))
        return ARIA_E_INVALID;
    if (n_traj == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    for (int k0 = 0; k0 < n_traj; k0 += EVAL_MAX_GRID) {
        const int nb = std::min(EVAL_MAX_GRID, n_traj - k0);
        hipLaunchKernelGGL(k_traj_eval, dim3(nb), dim3(EVAL_BLOCK), 0, h->stream, d_est, est_kind, d_offset, n_poses_total, k0,
                           d_truth, n_truth, truth_shared, d_mask, align_mode, rpe_delta, d_pose_err, d_results, h->d_err);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_eval_batch(aria_eval_t h, const void* est, int est_kind, const int* offset, int n_poses_total, int n_traj,
                    const aria_eval_truth* truth, int n_truth, int truth_shared, const uint8_t* mask, int align_mode, int rpe_delta,
                    double* pose_err, aria_eval_result* results) {
    if (!h || !offset || !results || n_traj < 0 || n_poses_total < 0 || n_truth < 0 || (n_poses_total && !est) ||
        (n_truth && !truth) || est_kind < ARIA_EVAL_EST_POSE12 || est_kind > ARIA_EVAL_EST_XYZ)
        return ARIA_E_INVALID;
    if (n_traj == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t NP = (size_t)n_poses_total, NT = (size_t)n_truth, B = (size_t)n_traj, stride = est_stride(est_kind);
    int rc;
    if ((rc = eval_reserve(h, 0, NP * stride)) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 1, (B + 1) * sizeof(int))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 2, NT * sizeof(aria_eval_truth))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 3, NP)) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 4, NP * sizeof(double))) != ARIA_OK) return rc;
    if ((rc = eval_reserve(h, 5, B * sizeof(aria_eval_result))) != ARIA_OK) return rc;
    hipStream_t st = h->stream;
    if (NP) ARIA_HIP(hipMemcpyAsync(h->d_buf[0], est, NP * stride, hipMemcpyHostToDevice, st));
    if (NT) ARIA_HIP(hipMemcpyAsync(h->d_buf[2], truth, NT * sizeof(aria_eval_truth), hipMemcpyHostToDevice, st));
    if (NP && mask) ARIA_HIP(hipMemcpyAsync(h->d_buf[3], mask, NP, hipMemcpyHostToDevice, st));
    if (pose_err) ARIA_HIP(hipMemsetAsync(h->d_buf[4], 0, std::max<size_t>(NP * sizeof(double), 8), st));
    ARIA_HIP(memcpy_on(st, h->d_buf[1], offset, (B + 1) * sizeof(int), hipMemcpyHostToDevice));
    rc = aria_eval_batch_device(h, h->d_buf[0], est_kind, (const int*)h->d_buf[1].p, n_poses_total, n_traj,
                                (const aria_eval_truth*)h->d_buf[2].p, n_truth, truth_shared, mask ? h->d_buf[3].p : nullptr, align_mode,
                                rpe_delta, pose_err ? (double*)h->d_buf[4].p : nullptr, (aria_eval_result*)h->d_buf[5].p);
    if (rc != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(results, h->d_buf[5], B * sizeof(aria_eval_result), hipMemcpyDeviceToHost, st));
    if (pose_err && NP) ARIA_HIP(hipMemcpyAsync(pose_err, h->d_buf[4], NP * sizeof(double), hipMemcpyDeviceToHost, st));
    ARIA_HIP(hipStreamSynchronize(st));
    return aria_eval_check(h);
}

}  // extern "C"
