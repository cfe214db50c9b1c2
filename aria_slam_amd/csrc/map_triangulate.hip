// Two-view triangulation into an HBM-resident point map: the reference's Mapper::triangulate (DLT, depth / parallax /
// reprojection tests, colour, quality) batched over pairs, plus its filterOutliers and filterByDistance. Semantics in
// include/aria_orb_hip.h ("two-view triangulation and point map"); aria_slam_amd/map_ref.py restates every step in NumPy.
//
// Append (three launches on the handle's stream, no host round trip -- the map size lives on the device):
//   k_map_tri      256 threads per pair, a lane per match: validates the pair's counts and every match index BEFORE any
//                  keypoint is read, then per match the fp64 DLT (one-sided Jacobi SVD of the 4x4 in registers), the three
//                  tests and the gray fetch; kept points are compacted stably (wave ballot + mbcnt, waves in order) into
//                  the pair's staging slot at p * match_cap
//   k_map_scan     one workgroup: exclusive scan of the pair counts -> arena offsets of the whole pairs that fit, the
//                  capacity verdict, the new device-resident size and next id
//   k_map_scatter  one workgroup per pair: staging -> arena, ids assigned in order
// Filters (four launches): per-block fp64 partial sums -> one-workgroup sum in block order (k_map_stats, outliers only),
//   keep flags + per-block counts (k_map_flag), block scan (k_map_fscan), stable scatter into the other arena (k_map_fscatter).
// No float atomics anywhere; every floating-point sum has a fixed order. No grid barrier: every step is its own launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "ransac_device.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_map_point) == 72, "aria_map_point is 72 bytes");
static_assert(offsetof(aria_map_point, X) == 8 && offsetof(aria_map_point, quality) == 32 && offsetof(aria_map_point, err) == 40 &&
              offsetof(aria_map_point, pair) == 48 && offsetof(aria_map_point, gray) == 64, "aria_map_point layout");

namespace {

constexpr int MAP_BLOCK = 256;              // k_map_tri / k_map_scatter: threads per pair
constexpr int MAP_SCAN_BLOCK = 1024;        // k_map_scan / k_map_fscan
constexpr int MAP_FILT_ITEMS = 4;           // filter kernels: points per thread
constexpr int MAP_FILT_SPAN = MAP_BLOCK * MAP_FILT_ITEMS;   // points per filter block
constexpr int MAP_SVD_SWEEPS = 30;          // header: sweep cap of the Jacobi SVD
constexpr double MAP_SVD_EPS = 10.0 * 2.220446049250313e-16;   // header: convergence test, 10 * DBL_EPSILON
constexpr double MAP_W_EPS = 1e-10;         // |X[3]| below this: point at infinity
constexpr int MAP_MIN_MATCHES = 8;          // Mapper.cpp:13: fewer matches -> nothing
constexpr int ERRBIT_MAP_INPUT = 1;         // a pair's counts or match indices were out of range (pair skipped)
constexpr int ERRBIT_MAP_FULL = 2;          // an append did not fit the capacity (trailing pairs dropped)

// device-resident map state, int64 slots
enum : int { META_SIZE = 0, META_NEXT_ID = 1, META_NEEDED = 2, META_BASE_SIZE = 3, META_BASE_ID = 4, META_SLOTS = 8 };

struct MapParams {
    double fx, fy, cx, cy, min_depth, max_depth, min_parallax, max_reproj;
};

// One Hestenes rotation orthogonalising columns I and J of a (column-major 4x4), accumulated into v. False when the pair
// already is orthogonal to the convergence test.
template <int I, int J>
__device__ __forceinline__ bool hj_pair(double a[16], double v[16]) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        alpha += a[I * 4 + r] * a[I * 4 + r];
        beta += a[J * 4 + r] * a[J * 4 + r];
        gamma += a[I * 4 + r] * a[J * 4 + r];
    }
    if (!(fabs(gamma) > MAP_SVD_EPS * sqrt(alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double x = a[I * 4 + r], y = a[J * 4 + r];
        a[I * 4 + r] = c * x - s * y;
        a[J * 4 + r] = s * x + c * y;
        const double p = v[I * 4 + r], q = v[J * 4 + r];
        v[I * 4 + r] = c * p - s * q;
        v[J * 4 + r] = s * p + c * q;
    }
    return true;
}

// Right singular vector of the smallest singular value of the 4x4 A (rows given), by one-sided Jacobi in registers
__device__ __forceinline__ void dlt_null_vector(const double A[16], double X[4]) {
    double a[16], v[16];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            a[c * 4 + r] = A[r * 4 + c];                 // column c of A
            v[c * 4 + r] = (r == c) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < MAP_SVD_SWEEPS; sweep++) {
        bool rot = false;
        rot |= hj_pair<0, 1>(a, v);
        rot |= hj_pair<0, 2>(a, v);
        rot |= hj_pair<0, 3>(a, v);
        rot |= hj_pair<1, 2>(a, v);
        rot |= hj_pair<1, 3>(a, v);
        rot |= hj_pair<2, 3>(a, v);
        if (!rot) break;
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double n2 = a[c * 4 + 0] * a[c * 4 + 0] + a[c * 4 + 1] * a[c * 4 + 1] + a[c * 4 + 2] * a[c * 4 + 2] +
                          a[c * 4 + 3] * a[c * 4 + 3];
        const bool take = (c == 0) || n2 < best;         // ties keep the lowest column
        best = take ? n2 : best;
#pragma unroll
        for (int r = 0; r < 4; r++) X[r] = take ? v[c * 4 + r] : X[r];
    }
}

// Mapper::triangulate for one match (fp64). E1/E2: world-to-camera [R | t] rows (12 each); KP1/KP2 = K E. Returns true
// when the point is kept; fills X (dehomogenised) and the two reprojection errors.
__device__ __forceinline__ bool triangulate_one(const double KP1[12], const double KP2[12], const double E1[12],
                                                const double E2[12], const double C1[3], const double C2[3], const MapParams& m,
                                                float x1, float y1, float x2, float y2, double Xo[3], double err[2]) {
    const double u1 = x1, v1 = y1, u2 = x2, v2 = y2;
    double A[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        A[0 * 4 + k] = u1 * KP1[8 + k] - KP1[0 + k];
        A[1 * 4 + k] = v1 * KP1[8 + k] - KP1[4 + k];
        A[2 * 4 + k] = u2 * KP2[8 + k] - KP2[0 + k];
        A[3 * 4 + k] = v2 * KP2[8 + k] - KP2[4 + k];
    }
    double X[4] = {0.0, 0.0, 0.0, 0.0};
    dlt_null_vector(A, X);
    if (!(fabs(X[3]) >= MAP_W_EPS)) return false;
    const double px = X[0] / X[3], py = X[1] / X[3], pz = X[2] / X[3];
    double c1[3], c2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        c1[r] = E1[r * 4 + 0] * px + E1[r * 4 + 1] * py + E1[r * 4 + 2] * pz + E1[r * 4 + 3];
        c2[r] = E2[r * 4 + 0] * px + E2[r * 4 + 1] * py + E2[r * 4 + 2] * pz + E2[r * 4 + 3];
    }
    if (!(c1[2] >= m.min_depth && c1[2] <= m.max_depth)) return false;
    if (!(c2[2] >= m.min_depth && c2[2] <= m.max_depth)) return false;
    const double r1x = px - C1[0], r1y = py - C1[1], r1z = pz - C1[2];
    const double r2x = px - C2[0], r2y = py - C2[1], r2z = pz - C2[2];
    const double n1 = sqrt(r1x * r1x + r1y * r1y + r1z * r1z), n2 = sqrt(r2x * r2x + r2y * r2y + r2z * r2z);
    const double cosp = (r1x / n1) * (r2x / n2) + (r1y / n1) * (r2y / n2) + (r1z / n1) * (r2z / n2);
    const double parallax = acos(fmin(1.0, fabs(cosp))) * 180.0 / M_PI;
    if (!(parallax >= m.min_parallax)) return false;
    const double e1x = m.fx * c1[0] / c1[2] + m.cx - u1, e1y = m.fy * c1[1] / c1[2] + m.cy - v1;
    const double e2x = m.fx * c2[0] / c2[2] + m.cx - u2, e2y = m.fy * c2[1] / c2[2] + m.cy - v2;
    err[0] = sqrt(e1x * e1x + e1y * e1y);
    err[1] = sqrt(e2x * e2x + e2y * e2y);
    if (!(err[0] <= m.max_reproj && err[1] <= m.max_reproj)) return false;
    Xo[0] = px; Xo[1] = py; Xo[2] = pz;
    return true;
}

// ---- append 1: triangulate + compact into the pair's staging slot --------------------------------------------------------
__global__ __launch_bounds__(MAP_BLOCK) void k_map_tri(const aria_keypoint* __restrict__ kq, const int* __restrict__ nq,
                                                       const aria_keypoint* __restrict__ kt, const int* __restrict__ nt,
                                                       int64_t kp_stride, const aria_match* __restrict__ matches,
                                                       const int* __restrict__ nmatches, int match_cap, int query_is_first,
                                                       int pair_base, const double* __restrict__ ext,
                                                       const aria_pose_result* __restrict__ pose, int min_pose_inliers,
                                                       const uint8_t* __restrict__ cand, const uint8_t* __restrict__ img,
                                                       int64_t img_stride, int W, int H, int pitch, MapParams prm,
                                                       aria_map_point* __restrict__ stage, int* __restrict__ cnt,
                                                       int* __restrict__ err) {
    __shared__ int bad;
    __shared__ int wsum[MAP_BLOCK / 64];
    const int p = blockIdx.x;
    const int n = nmatches[p], nqp = nq[p], ntp = nt[p];
    if (threadIdx.x == 0) bad = (n < 0 || n > match_cap || nqp < 0 || nqp > kp_stride || ntp < 0 || ntp > kp_stride) ? 1 : 0;
    __syncthreads();
    const aria_match* mp = matches + (int64_t)p * match_cap;
    if (!bad) {
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += MAP_BLOCK) {
            const aria_match a = mp[i];
            mine |= (a.query_idx < 0 || a.query_idx >= nqp || a.train_idx < 0 || a.train_idx >= ntp);
        }
        if (mine) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (bad) {
        if (threadIdx.x == 0) {
            cnt[p] = 0;
            atomicOr(err, ERRBIT_MAP_INPUT);
        }
        return;
    }
    // extrinsics: per-pair [R1|t1], [R2|t2], or the pose record as [I|0], [R|t] behind its acceptance gate
    double E1[12], E2[12];
    if (ext) {
        const double* e = ext + (int64_t)p * 24;
#pragma unroll
        for (int k = 0; k < 12; k++) { E1[k] = e[k]; E2[k] = e[12 + k]; }
    } else {
        const aria_pose_result* r = pose + p;
        if (!r->valid || r->n_pose_inliers <= min_pose_inliers) {
            if (threadIdx.x == 0) cnt[p] = 0;
            return;
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                E1[i * 4 + j] = (i == j) ? 1.0 : 0.0;
                E2[i * 4 + j] = (j < 3) ? r->R[i * 3 + j] : r->t[i];
            }
    }
    if (n < MAP_MIN_MATCHES) {
        if (threadIdx.x == 0) cnt[p] = 0;
        return;
    }
    double KP1[12], KP2[12], C1[3], C2[3];
#pragma unroll
    for (int k = 0; k < 4; k++) {                        // P = K [R | t]
        KP1[k] = prm.fx * E1[k] + prm.cx * E1[8 + k];
        KP1[4 + k] = prm.fy * E1[4 + k] + prm.cy * E1[8 + k];
        KP1[8 + k] = E1[8 + k];
        KP2[k] = prm.fx * E2[k] + prm.cx * E2[8 + k];
        KP2[4 + k] = prm.fy * E2[4 + k] + prm.cy * E2[8 + k];
        KP2[8 + k] = E2[8 + k];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {                        // C = -R^T t
        C1[c] = -(E1[0 * 4 + c] * E1[3] + E1[1 * 4 + c] * E1[7] + E1[2 * 4 + c] * E1[11]);
        C2[c] = -(E2[0 * 4 + c] * E2[3] + E2[1 * 4 + c] * E2[7] + E2[2 * 4 + c] * E2[11]);
    }
    const aria_keypoint* q = kq + (int64_t)p * kp_stride;
    const aria_keypoint* t = kt + (int64_t)p * kp_stride;
    const uint8_t* cp = cand ? cand + (int64_t)p * match_cap : nullptr;
    const uint8_t* im = img ? img + (int64_t)p * img_stride : nullptr;
    aria_map_point* out = stage + (int64_t)p * match_cap;
    int run = 0;
    for (int base = 0; base < n; base += MAP_BLOCK) {    // uniform trip count: every lane reaches the ballots
        const int i = base + (int)threadIdx.x;
        bool keep = false;
        double X[3] = {0.0, 0.0, 0.0}, e[2] = {0.0, 0.0};
        int i1 = 0, i2 = 0;
        float x1 = 0.0f, y1 = 0.0f;
        if (i < n && (!cp || cp[i])) {
            const aria_match a = mp[i];
            i1 = query_is_first ? a.query_idx : a.train_idx;
            i2 = query_is_first ? a.train_idx : a.query_idx;
            const aria_keypoint k1 = query_is_first ? q[i1] : t[i1];
            const aria_keypoint k2 = query_is_first ? t[i2] : q[i2];
            x1 = k1.x; y1 = k1.y;
            keep = triangulate_one(KP1, KP2, E1, E2, C1, C2, prm, k1.x, k1.y, k2.x, k2.y, X, e);
        }
        int total;
        const int slot = block_compact<MAP_BLOCK>(keep, wsum, total);
        if (keep) {
            uint8_t g = 127;                             // (int)(0.5 * 255): the reference's default colour
            if (im) {
                // clamp((int)x, 0, W - 1) with the clamp taken in float first: identical for every finite x, defined for any
                const int px = (int)fminf(fmaxf(x1, 0.0f), (float)(W - 1));
                const int py = (int)fminf(fmaxf(y1, 0.0f), (float)(H - 1));
                g = im[(int64_t)py * pitch + px];
            }
            aria_map_point o;
            o.id = 0;
            o.X[0] = X[0]; o.X[1] = X[1]; o.X[2] = X[2];
            o.quality = 1.0 / (e[0] + e[1] + 0.1);
            o.err[0] = (float)e[0]; o.err[1] = (float)e[1];
            o.pair = pair_base + p; o.match = i; o.idx1 = i1; o.idx2 = i2;
            o.gray = g;
#pragma unroll
            for (int k = 0; k < 7; k++) o.pad[k] = 0;
            out[run + slot] = o;
        }
        run += total;
    }
    if (threadIdx.x == 0) cnt[p] = run;
}

// inclusive scan of one value per thread over a MAP_SCAN_BLOCK workgroup (Hillis-Steele in LDS, fixed order)
__device__ __forceinline__ long long block_scan_incl(long long x, long long* buf) {
    buf[threadIdx.x] = x;
    __syncthreads();
    for (int d = 1; d < MAP_SCAN_BLOCK; d <<= 1) {
        const long long y = (threadIdx.x >= (unsigned)d) ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += y;
        __syncthreads();
    }
    const long long r = buf[threadIdx.x];
    __syncthreads();
    return r;
}

// ---- append 2: offsets of the whole pairs that fit, capacity verdict, new size ------------------------------------------
__global__ __launch_bounds__(MAP_SCAN_BLOCK) void k_map_scan(const int* __restrict__ cnt, int n_pairs, long long capacity,
                                                             long long* __restrict__ off, int* __restrict__ added,
                                                             long long* __restrict__ meta, int* __restrict__ err) {
    __shared__ long long buf[MAP_SCAN_BLOCK];
    __shared__ unsigned long long appended;
    __shared__ long long carry_s;
    const long long size0 = meta[META_SIZE], id0 = meta[META_NEXT_ID];
    if (threadIdx.x == 0) appended = 0;
    long long carry = 0;
    for (int base = 0; base < n_pairs; base += MAP_SCAN_BLOCK) {
        const int p = base + (int)threadIdx.x;
        const long long c = (p < n_pairs) ? (long long)cnt[p] : 0;
        const long long incl = carry + block_scan_incl(c, buf);
        const bool fits = size0 + incl <= capacity;      // prefix sums grow: the pairs that fit are a prefix
        if (p < n_pairs) {
            off[p] = fits ? size0 + incl - c : -1;
            if (added) added[p] = fits ? (int)c : 0;
            if (fits) atomicMax(&appended, (unsigned long long)incl);   // integer max: order-free
        }
        if (threadIdx.x == MAP_SCAN_BLOCK - 1) carry_s = incl;
        __syncthreads();
        carry = carry_s;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long total = carry, app = (long long)appended;
        meta[META_BASE_SIZE] = size0;
        meta[META_BASE_ID] = id0;
        meta[META_SIZE] = size0 + app;
        meta[META_NEXT_ID] = id0 + app;
        if (size0 + total > meta[META_NEEDED]) meta[META_NEEDED] = size0 + total;
        if (app < total) atomicOr(err, ERRBIT_MAP_FULL);
    }
}

// ---- append 3: staging -> arena, ids in order ---------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_BLOCK) void k_map_scatter(const aria_map_point* __restrict__ stage, int match_cap,
                                                           const int* __restrict__ cnt, const long long* __restrict__ off,
                                                           const long long* __restrict__ meta, aria_map_point* __restrict__ arena) {
    const int p = blockIdx.x;
    const long long o = off[p];
    if (o < 0) return;
    const int c = cnt[p];
    const unsigned long long id = (unsigned long long)(meta[META_BASE_ID] + (o - meta[META_BASE_SIZE]));
    const aria_map_point* s = stage + (int64_t)p * match_cap;
    for (int j = threadIdx.x; j < c; j += MAP_BLOCK) {
        aria_map_point r = s[j];
        r.id = id + (unsigned long long)j;
        arena[o + j] = r;
    }
}

// ---- filters ------------------------------------------------------------------------------------------------------------
// per-block fp64 sums over points [b * SPAN, (b + 1) * SPAN) of the current size: mode 0 = sum of positions (3 values),
// mode 1 = sum of |p - mean|^2 (1 value). Each thread sums its items in order, then a fixed tree over the block.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_psum(const aria_map_point* __restrict__ arena,
                                                        const long long* __restrict__ meta, int mode,
                                                        const double* __restrict__ stats, double* __restrict__ partial) {
    __shared__ double red[3][MAP_BLOCK];
    const long long n = meta[META_SIZE];
    const long long b0 = (long long)blockIdx.x * MAP_FILT_SPAN;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < MAP_FILT_ITEMS; k++) {
        const long long i = b0 + k * MAP_BLOCK + threadIdx.x;
        if (i < n) {
            const double x = arena[i].X[0], y = arena[i].X[1], z = arena[i].X[2];
            if (mode == 0) { s0 += x; s1 += y; s2 += z; }
            else {
                const double dx = x - stats[0], dy = y - stats[1], dz = z - stats[2];
                s0 += dx * dx + dy * dy + dz * dz;
            }
        }
    }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int h = MAP_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int c = 0; c < 3; c++) red[c][threadIdx.x] += red[c][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; c++) partial[(int64_t)blockIdx.x * 3 + c] = red[c][0];
}

// one workgroup: sums the partials in block order (thread t: blocks t, t + 256, ... in turn; then a fixed tree).
// mode 0: stats[0..2] = mean; mode 1: stats[3] = 3 * sqrt(sum / n), the outlier threshold
__global__ __launch_bounds__(MAP_BLOCK) void k_map_stats(const double* __restrict__ partial, int n_blocks,
                                                         const long long* __restrict__ meta, int mode, double* __restrict__ stats) {
    __shared__ double red[3][MAP_BLOCK];
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < n_blocks; b += MAP_BLOCK)
        for (int c = 0; c < 3; c++) s[c] += partial[(int64_t)b * 3 + c];
    for (int c = 0; c < 3; c++) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int h = MAP_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int c = 0; c < 3; c++) red[c][threadIdx.x] += red[c][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)(meta[META_SIZE] > 0 ? meta[META_SIZE] : 1);
        if (mode == 0) {
            for (int c = 0; c < 3; c++) stats[c] = red[c][0] / n;
        } else {
            stats[3] = 3.0 * sqrt(red[0][0] / n);
        }
    }
}

// keep flags + per-block keep counts. mode 0 (outliers): keep |p - mean| <= stats[3], everything when size < 10;
// mode 1 (distance): keep |p| <= dist. Flags past the size are 0.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_flag(const aria_map_point* __restrict__ arena,
                                                        const long long* __restrict__ meta, int mode,
                                                        const double* __restrict__ stats, double dist,
                                                        uint8_t* __restrict__ flags, int* __restrict__ bcnt) {
    __shared__ int wsum[MAP_BLOCK / 64];
    const long long n = meta[META_SIZE];
    const long long b0 = (long long)blockIdx.x * MAP_FILT_SPAN;
    int kept = 0;
    for (int k = 0; k < MAP_FILT_ITEMS; k++) {
        const long long i = b0 + k * MAP_BLOCK + threadIdx.x;
        bool keep = false;
        if (i < n) {
            const double x = arena[i].X[0], y = arena[i].X[1], z = arena[i].X[2];
            if (mode == 0) {
                const double dx = x - stats[0], dy = y - stats[1], dz = z - stats[2];
                keep = (n < 10) || !(sqrt(dx * dx + dy * dy + dz * dz) > stats[3]);
            } else {
                keep = !(sqrt(x * x + y * y + z * z) > dist);
            }
        }
        flags[i] = keep ? 1 : 0;
        int total;
        block_compact<MAP_BLOCK>(keep, wsum, total);
        kept += total;
    }
    if (threadIdx.x == 0) bcnt[blockIdx.x] = kept;
}

// one workgroup: exclusive scan of the block counts -> block offsets; new size
__global__ __launch_bounds__(MAP_SCAN_BLOCK) void k_map_fscan(const int* __restrict__ bcnt, int n_blocks,
                                                              long long* __restrict__ boff, long long* __restrict__ meta) {
    __shared__ long long buf[MAP_SCAN_BLOCK];
    __shared__ long long carry_s;
    long long carry = 0;
    for (int base = 0; base < n_blocks; base += MAP_SCAN_BLOCK) {
        const int b = base + (int)threadIdx.x;
        const long long c = (b < n_blocks) ? (long long)bcnt[b] : 0;
        const long long incl = carry + block_scan_incl(c, buf);
        if (b < n_blocks) boff[b] = incl - c;
        if (threadIdx.x == MAP_SCAN_BLOCK - 1) carry_s = incl;
        __syncthreads();
        carry = carry_s;
        __syncthreads();
    }
    if (threadIdx.x == 0) meta[META_SIZE] = carry;
}

// stable scatter of the kept points into the other arena (same item order and compaction as k_map_flag)
__global__ __launch_bounds__(MAP_BLOCK) void k_map_fscatter(const aria_map_point* __restrict__ src, const uint8_t* __restrict__ flags,
                                                            const long long* __restrict__ boff, aria_map_point* __restrict__ dst) {
    __shared__ int wsum[MAP_BLOCK / 64];
    const long long b0 = (long long)blockIdx.x * MAP_FILT_SPAN;
    long long o = boff[blockIdx.x];
    for (int k = 0; k < MAP_FILT_ITEMS; k++) {
        const long long i = b0 + k * MAP_BLOCK + threadIdx.x;
        const bool keep = flags[i] != 0;
        int total;
        const int slot = block_compact<MAP_BLOCK>(keep, wsum, total);
        if (keep) dst[o + slot] = src[i];
        o += total;
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_map_s : StageHandle {
    aria_map_config cfg{};
    DeviceBuffer<long long> d_meta;                      // META_* slots
    DeviceBuffer<double> d_stats;                        // mean[3], threshold
    // the arena and its ping-pong twin (the filters scatter into the other one), `capacity` points each
    aria_map_point* d_arena = nullptr;
    aria_map_point* d_arena2 = nullptr;
    int64_t capacity = 0;
    // grow-only workspace of the append path
    DeviceBuffer<aria_map_point> d_stage;                // [n_pairs][match_cap]
    DeviceBuffer<int> d_cnt;                             // [n_pairs]
    DeviceBuffer<long long> d_off;                       // [n_pairs]
    // grow-only workspace of the filters
    DeviceBuffer<double> d_part;                         // [n_blocks][3]
    DeviceBuffer<int> d_bcnt;                            // [n_blocks]
    DeviceBuffer<long long> d_boff;                      // [n_blocks]
    DeviceBuffer<uint8_t> d_flags;                       // [n_blocks * span]
    // single-pair staging (aria_map_triangulate): the pair, view 1's image, the two extrinsics
    PairStaging pair;
    DeviceBuffer<uint8_t> d_img;
    DeviceBuffer<double> d_ext;                          // 24 doubles
};

namespace {

MapParams map_params(const aria_map_config& c) {
    return MapParams{c.fx, c.fy, c.cx, c.cy, c.min_depth, c.max_depth, c.min_parallax_deg, c.max_reproj_px};
}

int read_meta(aria_map_t h, int slot, int64_t* out) {
    long long v = 0;
    ARIA_HIP(hipStreamSynchronize(h->stream));
    ARIA_HIP(memcpy_on(h->stream, &v, h->d_meta + slot, sizeof(v), hipMemcpyDeviceToHost));
    *out = (int64_t)v;
    return ARIA_OK;
}

// k_map_tri over n_pairs pairs into the staging slots (counts in d_cnt)
int enqueue_tri(aria_map_t h, const aria_keypoint* d_kq, const int* d_nq, const aria_keypoint* d_kt, const int* d_nt,
                int64_t kp_stride, const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                int query_is_first, int pair_base, const double* d_ext, const aria_pose_result* d_pose, const uint8_t* d_cand,
                const uint8_t* d_img, int64_t img_stride, int W, int H, int pitch) {
    int rc;
    if ((rc = h->d_stage.reserve(h->stream, (size_t)n_pairs * match_cap)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, (size_t)n_pairs)) != ARIA_OK) return rc;
    if ((rc = h->d_off.reserve(h->stream, (size_t)n_pairs)) != ARIA_OK) return rc;
    hipLaunchKernelGGL(k_map_tri, dim3(n_pairs), dim3(MAP_BLOCK), 0, h->stream, d_kq, d_nq, d_kt, d_nt, kp_stride, d_matches,
                       d_nmatches, match_cap, query_is_first ? 1 : 0, pair_base, d_ext, d_pose, h->cfg.min_pose_inliers, d_cand,
                       d_img, img_stride, W, H, pitch, map_params(h->cfg), h->d_stage, h->d_cnt, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

// k_map_scan + k_map_scatter: append the staged pairs that fit
int enqueue_append(aria_map_t h, int n_pairs, int match_cap, int* d_added) {
    hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(MAP_SCAN_BLOCK), 0, h->stream, h->d_cnt, n_pairs, (long long)h->capacity,
                       h->d_off, d_added, h->d_meta, h->d_err);
    hipLaunchKernelGGL(k_map_scatter, dim3(n_pairs), dim3(MAP_BLOCK), 0, h->stream, h->d_stage, match_cap, h->d_cnt, h->d_off,
                       h->d_meta, h->d_arena);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

// mode 0: filterOutliers, mode 1: filterByDistance(dist)
int enqueue_filter(aria_map_t h, int mode, double dist) {
    if (h->capacity == 0) return ARIA_OK;
    const int nb = (int)((h->capacity + MAP_FILT_SPAN - 1) / MAP_FILT_SPAN);
    int rc;
    if ((rc = h->d_part.reserve(h->stream, (size_t)nb * 3)) != ARIA_OK) return rc;
    if ((rc = h->d_bcnt.reserve(h->stream, (size_t)nb)) != ARIA_OK) return rc;
    if ((rc = h->d_boff.reserve(h->stream, (size_t)nb)) != ARIA_OK) return rc;
    if ((rc = h->d_flags.reserve(h->stream, (size_t)nb * MAP_FILT_SPAN)) != ARIA_OK) return rc;
    if (mode == 0) {
        hipLaunchKernelGGL(k_map_psum, dim3(nb), dim3(MAP_BLOCK), 0, h->stream, h->d_arena, h->d_meta, 0, h->d_stats, h->d_part);
        hipLaunchKernelGGL(k_map_stats, dim3(1), dim3(MAP_BLOCK), 0, h->stream, h->d_part, nb, h->d_meta, 0, h->d_stats);
        hipLaunchKernelGGL(k_map_psum, dim3(nb), dim3(MAP_BLOCK), 0, h->stream, h->d_arena, h->d_meta, 1, h->d_stats, h->d_part);
        hipLaunchKernelGGL(k_map_stats, dim3(1), dim3(MAP_BLOCK), 0, h->stream, h->d_part, nb, h->d_meta, 1, h->d_stats);
    }
    hipLaunchKernelGGL(k_map_flag, dim3(nb), dim3(MAP_BLOCK), 0, h->stream, h->d_arena, h->d_meta, mode, h->d_stats, dist,
                       h->d_flags, h->d_bcnt);
    hipLaunchKernelGGL(k_map_fscan, dim3(1), dim3(MAP_SCAN_BLOCK), 0, h->stream, h->d_bcnt, nb, h->d_boff, h->d_meta);
    hipLaunchKernelGGL(k_map_fscatter, dim3(nb), dim3(MAP_BLOCK), 0, h->stream, h->d_arena, h->d_flags, h->d_boff, h->d_arena2);
    ARIA_HIP(hipGetLastError());
    std::swap(h->d_arena, h->d_arena2);
    return ARIA_OK;
}

int reserve(aria_map_t h, int64_t n) {
    if (n <= h->capacity) return ARIA_OK;
    int64_t size = 0;
    int rc = read_meta(h, META_SIZE, &size);
    if (rc != ARIA_OK) return rc;
    aria_map_point *a = nullptr, *b = nullptr;
    hipError_t e = hipMalloc((void**)&a, (size_t)n * sizeof(aria_map_point));
    if (e == hipSuccess) e = hipMalloc((void**)&b, (size_t)n * sizeof(aria_map_point));
    if (e == hipSuccess && size > 0)
        e = memcpy_on(h->stream, a, h->d_arena, (size_t)size * sizeof(aria_map_point), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        if (a) hipFree(a);
        if (b) hipFree(b);
        return hip_fail(e, "aria_map_reserve", __FILE__, __LINE__);
    }
    if (h->d_arena) hipFree(h->d_arena);
    if (h->d_arena2) hipFree(h->d_arena2);
    h->d_arena = a;
    h->d_arena2 = b;
    h->capacity = n;
    return ARIA_OK;
}

bool bad_config(const aria_map_config* c) {
    return !c || c->struct_size != (int)sizeof(aria_map_config) || bad_pinhole(c->fx, c->fy, c->cx, c->cy) ||
           !std::isfinite(c->min_depth) || !std::isfinite(c->max_depth) || !(c->max_depth >= c->min_depth) || !std::isfinite(c->min_parallax_deg) ||
           !(c->max_reproj_px >= 0) || !std::isfinite(c->max_reproj_px) || c->capacity < 0 || c->capacity > ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

void aria_map_default_config(aria_map_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_map_config);
    c->device = 0;
    c->stream = nullptr;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0 (src/legacy/EuRoCReader.cpp:11-17)
    c->min_depth = 0.1;                                                    // include/legacy/Mapper.hpp:67-70
    c->max_depth = 50.0;
    c->min_parallax_deg = 1.0;
    c->max_reproj_px = 2.0;
    c->capacity = 1 << 16;
    c->min_pose_inliers = 10;                                              // euroc_eval.cpp:191: n_pose_inliers > 10
}

int aria_map_create(const aria_map_config* c, aria_map_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    // reserve() comes last: it alone sets the arenas, so a create that fails has none for stage_create to free
    return stage_create(c, out, 1, "aria_map_create", [](aria_map_s* h) {
        const char* what = "aria_map_create";
        int rc;
        if ((rc = h->pair.create(h->stream)) != ARIA_OK) return rc;
        if ((rc = h->d_meta.reserve(h->stream, META_SLOTS, what)) != ARIA_OK) return rc;
        if ((rc = h->d_stats.reserve(h->stream, 4, what)) != ARIA_OK) return rc;
        if ((rc = h->d_ext.reserve(h->stream, 24, what)) != ARIA_OK) return rc;
        hipError_t e = memset_on(h->stream, h->d_meta, 0, META_SLOTS * sizeof(long long));
        if (e == hipSuccess) e = memset_on(h->stream, h->d_stats, 0, 4 * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
        return reserve(h, std::max<int64_t>(h->cfg.capacity, 1));
    });
}

void aria_map_destroy(aria_map_t h) {
    if (!h) return;
    stage_destroy(h, {h->d_arena, h->d_arena2});   // plain pointers: the filters swap them and reserve() replaces both
}

void* aria_map_stream(aria_map_t h) { return stage_stream(h); }

int aria_map_check(aria_map_t h) {
    return stage_check(h, {{ERRBIT_MAP_INPUT, ARIA_E_INVALID}, {ERRBIT_MAP_FULL, ARIA_E_OUTPUT_TOO_SMALL}});
}

int aria_map_triangulate(aria_map_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                         const aria_match* matches, int n_matches, int query_is_first, const double* pose1,
                         const double* pose2, const uint8_t* image1, int width, int height, int pitch, const uint8_t* mask,
                         int pair_id, int* n_added) {
    if (!h || !pose1 || !pose2 || n_matches > (1 << 20) || pair_id < 0) return ARIA_E_INVALID;
    if (image1 && (width < 1 || height < 1 || pitch < width)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    PairStaging& s = h->pair;
    int rc = s.prepare(h->stream, kp_query, nq, kp_train, nt, matches, n_matches);
    if (rc != ARIA_OK) return rc;
    if (n_added) *n_added = 0;
    if (image1 && (rc = h->d_img.reserve(h->stream, (size_t)width * height)) != ARIA_OK) return rc;
    double ext[24];
    std::memcpy(ext, pose1, 12 * sizeof(double));
    std::memcpy(ext + 12, pose2, 12 * sizeof(double));
    if (image1)
        ARIA_HIP(hipMemcpy2DAsync(h->d_img, (size_t)width, image1, (size_t)pitch, (size_t)width, (size_t)height,
                                  hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(hipMemcpyAsync(h->d_ext, ext, sizeof(ext), hipMemcpyHostToDevice, h->stream));
    if ((rc = s.copy(h->stream, kp_query, nq, kp_train, nt, matches, n_matches, mask)) != ARIA_OK) return rc;
    const int cap = s.match_cap;
    rc = enqueue_tri(h, s.d_kq, s.d_counts, s.d_kt, s.d_counts + 1, s.kp_stride, s.d_m, s.d_counts + 2, 1, cap, query_is_first,
                     pair_id, h->d_ext, nullptr, mask ? s.d_mask.p : nullptr, image1 ? h->d_img.p : nullptr, 0, width, height,
                     width);
    if (rc != ARIA_OK) return rc;
    // the blocking form grows the arena itself
    int kept = 0;
    int64_t size = 0;
    ARIA_HIP(memcpy_on(h->stream, &kept, h->d_cnt, sizeof(int), hipMemcpyDeviceToHost));
    if ((rc = read_meta(h, META_SIZE, &size)) != ARIA_OK) return rc;
    if (size + kept > h->capacity && (rc = reserve(h, std::max<int64_t>(2 * h->capacity, size + kept))) != ARIA_OK) return rc;
    if ((rc = enqueue_append(h, 1, cap, nullptr)) != ARIA_OK) return rc;
    ARIA_HIP(hipStreamSynchronize(h->stream));
    if (n_added) *n_added = kept;
    return aria_map_check(h);
}

int aria_map_triangulate_batch_device(aria_map_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                      const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                      const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                      int query_is_first, int pair_base, const double* d_extrinsics,
                                      const aria_pose_result* d_pose, const uint8_t* d_mask, const uint8_t* d_img,
                                      int64_t img_stride, int width, int height, int pitch, int* d_added) {
    if (!h || !d_kp_query || !d_nq || !d_kp_train || !d_nt || !d_matches || !d_nmatches || (!d_extrinsics && !d_pose) ||
        n_pairs < 0 || match_cap < 1 || match_cap > (1 << 20) || kp_stride < 0 || pair_base < 0)
        return ARIA_E_INVALID;
    if (d_img && (width < 1 || height < 1 || pitch < width || img_stride < (int64_t)pitch * (height - 1) + width))
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = enqueue_tri(h, d_kp_query, d_nq, d_kp_train, d_nt, kp_stride, d_matches, d_nmatches, n_pairs, match_cap,
                         query_is_first, pair_base, d_extrinsics, d_pose, d_mask, d_img, img_stride, width, height, pitch);
    if (rc != ARIA_OK) return rc;
    return enqueue_append(h, n_pairs, match_cap, d_added);
}

int aria_map_points_needed(aria_map_t h, int64_t* needed) {
    if (!h || !needed) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return read_meta(h, META_NEEDED, needed);
}

int aria_map_size(aria_map_t h, int64_t* size) {
    if (!h || !size) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return read_meta(h, META_SIZE, size);
}

int64_t aria_map_capacity(aria_map_t h) { return h ? h->capacity : 0; }

int aria_map_clear(aria_map_t h) {
    if (!h) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(memset_on(h->stream, h->d_meta, 0, META_SLOTS * sizeof(long long)));
    return ARIA_OK;
}

int aria_map_reserve(aria_map_t h, int64_t capacity) {
    if (!h || capacity < 0 || capacity > ((int64_t)1 << 31)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return reserve(h, capacity);
}

int aria_map_read(aria_map_t h, int64_t first, int64_t count, aria_map_point* out) {
    if (!h || first < 0 || count < 0 || (count && !out)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int64_t size = 0;
    int rc = read_meta(h, META_SIZE, &size);
    if (rc != ARIA_OK) return rc;
    if (first + count > size) return ARIA_E_INVALID;
    if (count) ARIA_HIP(memcpy_on(h->stream, out, h->d_arena + first, (size_t)count * sizeof(aria_map_point), hipMemcpyDeviceToHost));
    return ARIA_OK;
}

const aria_map_point* aria_map_device_points(aria_map_t h) { return h ? h->d_arena : nullptr; }

int aria_map_filter_outliers(aria_map_t h) {
    if (!h) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return enqueue_filter(h, 0, 0.0);
}

int aria_map_filter_distance(aria_map_t h, double max_distance) {
    if (!h || std::isnan(max_distance)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return enqueue_filter(h, 1, max_distance);
}

}  // extern "C"

// Internal (stage_handle.h): what aria_pnp_associate_batch_device reads of the map without a host round trip.
namespace aria {
void map_device_view(aria_map_t h, const aria_map_point** arena, const long long** d_size, int64_t* capacity, int* device) {
    *arena = h->d_arena;
    *d_size = h->d_meta + META_SIZE;
    *capacity = h->capacity;
    *device = h->device;
}
}  // namespace aria
