// Guided matching: landmarks projected into frames by a predicted pose, keypoints searched in a window around each
// projection. Semantics in include/aria_orb_hip.h ("guided matching"); aria_slam_amd/proj_ref.py is the definition and this
// file equals it bit for bit.
//
// k_proj_bin      one 256-thread workgroup per frame: the frame is validated (counts, range, pose) before anything of it is
//                 read; its keypoints are counting-sorted by 32 x 32 pixel cell into the handle's workspace (histogram,
//                 scan and scatter with integer LDS atomics; the order inside a cell is free because best and second are the
//                 two least of the distinct keys distance << 13 | k); the frame's claim words are reset.
// k_proj_search   grid (chunks of 256 landmarks, frames). A lane per landmark projects it (fp64, the pose through scalar
//                 loads) into LDS; then 16 lanes per landmark, 16 landmarks per round, walk the cell rows the window touches
//                 -- the cells of one row are one contiguous span of the sorted list -- take the exact fp32 tests of the
//                 header on every entry and 4 x (xor + 64-bit popcount) on the descriptor of each candidate, keep a running
//                 top-2 per lane and merge it over the 16 lanes by shuffles. Lane 0 decides acceptance, writes the record and
//                 claims the keypoint by an integer atomic-min of hamming << 20 | i.
// k_proj_resolve  a lane per landmark: it has won when the word of its keypoint holds its own key.
// k_proj_compact  one workgroup per frame: the winners in ascending i (ballot + mbcnt) as aria_pnp_corr and aria_proj_pair.
// k_proj_from_map a lane per arena position: integer copies of X, the descriptor row and the octave.
// The cell size and the chunking appear in no result: a window's cell range is a superset of its candidates (one pixel of
// slack for the fp32 subtraction), and every test on a candidate is the header's. No float atomics, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "ransac_device.h"
#include "stage_handle.h"
#include "orb_plan.h"

using namespace aria;

static_assert(sizeof(aria_proj_landmark) == 64, "aria_proj_landmark is 64 bytes");
static_assert(sizeof(aria_proj_obs) == 24, "aria_proj_obs is 24 bytes");
static_assert(sizeof(aria_proj_pair) == 8, "aria_proj_pair is 8 bytes");
static_assert(sizeof(aria_proj_config) == 80, "aria_proj_config is 80 bytes");

#define PROJ_HD __host__ __device__ __forceinline__

namespace {

// ---- the plain per-landmark arithmetic (compiles for the host too: no LDS, no barrier, no cross-lane operation) ----
constexpr int PJ_NONE = INT_MAX;          // "no key" of the running top-2
constexpr int PJ_KSHIFT = 13;             // key = distance << 13 | k, k < 8192
constexpr int PJ_CELL_LOG2 = 5;           // 32 x 32 pixel cells

struct ProjParams {
    double fx, fy, cx, cy, min_depth;
    float radius, ratio;
    int th, mod;
    float scale[8];
};

struct ProjView {
    float u, v;
    int visible;
};

// rule 1
PROJ_HD ProjView proj_project(const double* P, const double* X, int octave, const ProjParams& prm, int width, int height) {
    ProjView r;
    r.u = 0.0f; r.v = 0.0f; r.visible = 0;
    const double x = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const double y = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const double z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    if (!(octave >= 0) || !(z > prm.min_depth)) return r;
    const float u = (float)(prm.fx * x / z + prm.cx);
    const float v = (float)(prm.fy * y / z + prm.cy);
    if (!(u >= 0.0f && u < (float)width && v >= 0.0f && v < (float)height)) return r;
    r.u = u; r.v = v; r.visible = 1;
    return r;
}

PROJ_HD int proj_clamp_octave(int o) { return o < 0 ? 0 : (o > 7 ? 7 : o); }

PROJ_HD float proj_level_scale(const ProjParams& prm, int o) {
    const int k = proj_clamp_octave(o);
    float s = prm.scale[0];
#pragma unroll
    for (int l = 1; l < 8; l++) s = (k == l) ? prm.scale[l] : s;   // no runtime-indexed array: stays in registers
    return s;
}

// rule 2; oi is the landmark's clamped octave, ok the keypoint's stored one
PROJ_HD bool proj_candidate(float u, float v, float r, int oi, float xk, float yk, int ok, int mod) {
    const int d = proj_clamp_octave(ok) - oi;
    return d <= mod && -d <= mod && fabsf(xk - u) <= r && fabsf(yk - v) <= r;
}

PROJ_HD int proj_hamming(const uint64_t a[4], const uint64_t b[4]) {
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) +
           __builtin_popcountll(a[3] ^ b[3]);
}

// rule 3: the two least of a set of DISTINCT keys, whatever the order they arrive in
PROJ_HD void proj_top2(int key, int& m1, int& m2) {
    const int hi = key > m1 ? key : m1;
    m1 = key < m1 ? key : m1;
    m2 = hi < m2 ? hi : m2;
}

PROJ_HD void proj_top2_merge(int a1, int a2, int& m1, int& m2) {   // two disjoint sets
    const int hi = a1 > m1 ? a1 : m1, lo2 = a2 < m2 ? a2 : m2;
    m1 = a1 < m1 ? a1 : m1;
    m2 = hi < lo2 ? hi : lo2;
}

// rules 3, 4 and 6 for a visible landmark, before uniqueness: kp_idx holds the best keypoint whenever there was a candidate
PROJ_HD aria_proj_obs proj_decide(float u, float v, int m1, int m2, const ProjParams& prm) {
    aria_proj_obs o;
    o.u = u; o.v = v; o.kp_idx = -1; o.hamming = -1; o.second = -1; o.flags = 1;
    if (m1 == PJ_NONE) return o;
    o.kp_idx = m1 & ((1 << PJ_KSHIFT) - 1);
    o.hamming = m1 >> PJ_KSHIFT;
    o.second = m2 == PJ_NONE ? -1 : (m2 >> PJ_KSHIFT);
    o.flags = 3;
    const bool ok = o.hamming < prm.th && (o.second < 0 || (float)o.hamming < prm.ratio * (float)o.second);
    if (ok) o.flags = 7;
    return o;
}

PROJ_HD aria_proj_obs proj_not_visible() {
    aria_proj_obs o;
    o.u = 0.0f; o.v = 0.0f; o.kp_idx = -1; o.hamming = -1; o.second = -1; o.flags = 0;
    return o;
}

// the cell of a coordinate along an axis of g cells: monotone in x, total (a NaN lands in cell 0)
PROJ_HD int proj_cell(float x, int g) {
    const float c = floorf(x * (1.0f / (float)(1 << PJ_CELL_LOG2)));
    return (int)fminf(fmaxf(c, 0.0f), (float)(g - 1));
}

PROJ_HD int proj_claim_key(int hamming, int i) { return (hamming << 20) | i; }

PROJ_HD bool proj_is_finite(double v) { return v - v == 0.0; }
// ---- end of the plain arithmetic ----

constexpr int PJ_BLOCK = 256;
constexpr int PJ_GROUP = 16;                        // lanes per landmark
constexpr int PJ_LPR = PJ_BLOCK / PJ_GROUP;         // landmarks per round
constexpr int PJ_MAX_KP = 8192;
constexpr int PJ_MAX_DIM = 4096;
constexpr int PJ_MAX_LAND = 1 << 20;
constexpr int PJ_MAX_CELLS = (PJ_MAX_DIM >> PJ_CELL_LOG2) * (PJ_MAX_DIM >> PJ_CELL_LOG2);
constexpr int ERRBIT_PROJ_INPUT = 1;

struct ProjEntry {                                  // a keypoint in cell order
    float x, y;
    int octave, k;
};
static_assert(sizeof(ProjEntry) == 16, "ProjEntry is one 16-byte load");

__device__ __forceinline__ int cells_of(int dim) { return (dim + (1 << PJ_CELL_LOG2) - 1) >> PJ_CELL_LOG2; }

__global__ __launch_bounds__(PJ_BLOCK) void k_proj_bin(const double* __restrict__ pose, const aria_keypoint* __restrict__ kp,
                                                       const int* __restrict__ n_kp, int64_t kp_stride, int width, int height,
                                                       int n_landmarks, const int* __restrict__ range, int land_cap,
                                                       int* __restrict__ ok_out, int* __restrict__ cell_start,
                                                       int cell_stride, ProjEntry* __restrict__ sorted, int* __restrict__ claims,
                                                       int* __restrict__ err) {
    extern __shared__ int pj_pos[];                     // [cells]: histogram -> cell starts -> (after the scatter) cell ends
    __shared__ int s_part[PJ_BLOCK];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = n_kp[f], first = range[2 * f], count = range[2 * f + 1];
    bool ok = n >= 0 && n <= kp_stride && first >= 0 && count >= 0 && count <= land_cap &&
              (long long)first + (long long)count <= (long long)n_landmarks;
#pragma unroll
    for (int k = 0; k < 12; k++) ok = ok && proj_is_finite(pose[(int64_t)f * 12 + k]);
    if (!ok) {                                          // uniform: nothing of the frame is read
        if (tid == 0) {
            ok_out[f] = 0;
            atomicOr(err, ERRBIT_PROJ_INPUT);
        }
        return;
    }
    const int gx = cells_of(width), gy = cells_of(height), cells = gx * gy;
    const aria_keypoint* kf = kp + (int64_t)f * kp_stride;
    int* cs = cell_start + (int64_t)f * cell_stride;
    ProjEntry* sf = sorted + (int64_t)f * kp_stride;
    int* cl = claims + (int64_t)f * kp_stride;
    if (tid == 0) ok_out[f] = 1;
    for (int c = tid; c < cells; c += PJ_BLOCK) pj_pos[c] = 0;
    for (int k = tid; k < n; k += PJ_BLOCK) cl[k] = PJ_NONE;
    __syncthreads();
    for (int k = tid; k < n; k += PJ_BLOCK) atomicAdd(&pj_pos[proj_cell(kf[k].y, gy) * gx + proj_cell(kf[k].x, gx)], 1);
    __syncthreads();
    {
        const int chunk = (cells + PJ_BLOCK - 1) / PJ_BLOCK, c0 = min(tid * chunk, cells), c1 = min(c0 + chunk, cells);
        int sum = 0;
        for (int c = c0; c < c1; c++) sum += pj_pos[c];
        s_part[tid] = sum;
        __syncthreads();
        int run = 0;
        for (int t = 0; t < tid; t++) run += s_part[t];
        for (int c = c0; c < c1; c++) {
            const int m = pj_pos[c];
            pj_pos[c] = run;
            cs[c] = run;
            run += m;
        }
        if (tid == 0) cs[cells] = n;
    }
    __syncthreads();
    for (int k = tid; k < n; k += PJ_BLOCK) {
        const aria_keypoint q = kf[k];
        const int slot = atomicAdd(&pj_pos[proj_cell(q.y, gy) * gx + proj_cell(q.x, gx)], 1);
        ProjEntry e;
        e.x = q.x; e.y = q.y; e.octave = q.octave; e.k = k;
        sf[slot] = e;
    }
}

__global__ __launch_bounds__(PJ_BLOCK) void k_proj_search(
    const double* __restrict__ pose, const uint8_t* __restrict__ desc, int64_t kp_stride, int width, int height,
    const aria_proj_landmark* __restrict__ land, const int* __restrict__ range, int land_cap, const int* __restrict__ ok_in,
    const int* __restrict__ cell_start, int cell_stride, const ProjEntry* __restrict__ sorted, int* __restrict__ claims,
    ProjParams prm,
    aria_proj_obs* __restrict__ obs) {
    __shared__ float s_u[PJ_BLOCK], s_v[PJ_BLOCK];
    __shared__ int s_o[PJ_BLOCK];                       // the landmark's clamped octave, -1 when it is not visible
    const int f = blockIdx.y, tid = threadIdx.x;
    const int base = blockIdx.x * PJ_BLOCK;
    aria_proj_obs* of = obs + (int64_t)f * land_cap;
    const bool ok = ok_in[f] != 0;
    const int first = ok ? range[2 * f] : 0, count = ok ? range[2 * f + 1] : 0;
    if (base >= count) {                                // uniform: only records beyond the range
        if (base + tid < land_cap) of[base + tid] = proj_not_visible();
        return;
    }
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; k++) P[k] = pose[(int64_t)f * 12 + k];
    {
        const int i = base + tid;
        int o = -1;
        float u = 0.0f, v = 0.0f;
        if (i < count) {
            const aria_proj_landmark* lm = land + (int64_t)first + i;
            const double X[3] = {lm->X[0], lm->X[1], lm->X[2]};
            const int oct = lm->octave;
            const ProjView pv = proj_project(P, X, oct, prm, width, height);
            u = pv.u; v = pv.v;
            o = pv.visible ? proj_clamp_octave(oct) : -1;
        }
        if (o < 0 && i < land_cap) of[i] = proj_not_visible();
        s_u[tid] = u; s_v[tid] = v; s_o[tid] = o;
    }
    __syncthreads();
    const int gx = cells_of(width), gy = cells_of(height);
    const int* cs = cell_start + (int64_t)f * cell_stride;
    const ProjEntry* sf = sorted + (int64_t)f * kp_stride;
    const uint8_t* df = desc + (int64_t)f * kp_stride * 32;
    int* cl = claims + (int64_t)f * kp_stride;
    const int g = tid / PJ_GROUP, l = tid % PJ_GROUP;
    for (int round = 0; round < PJ_BLOCK / PJ_LPR; round++) {   // uniform trip count: every lane reaches the shuffles
        const int li = round * PJ_LPR + g, i = base + li;
        const int oi = s_o[li];
        const float u = s_u[li], v = s_v[li];
        int m1 = PJ_NONE, m2 = PJ_NONE;
        if (oi >= 0) {
            const aria_proj_landmark* lm = land + (int64_t)first + i;
            const uint64_t* la = reinterpret_cast<const uint64_t*>(lm->desc);   // 8-byte aligned inside the record
            const uint64_t a[4] = {la[0], la[1], la[2], la[3]};
            const float r = prm.radius * proj_level_scale(prm, oi);
            const int cx0 = proj_cell(u - r - 1.0f, gx), cx1 = proj_cell(u + r + 1.0f, gx);
            const int cy0 = proj_cell(v - r - 1.0f, gy), cy1 = proj_cell(v + r + 1.0f, gy);
            for (int cy = cy0; cy <= cy1; cy++) {
                const int s = cs[cy * gx + cx0], e = cs[cy * gx + cx1 + 1];
                for (int c = s + l; c < e; c += PJ_GROUP) {
                    const ProjEntry q = sf[c];
                    if (proj_candidate(u, v, r, oi, q.x, q.y, q.octave, prm.mod)) {
                        const ulonglong2 b0 = *reinterpret_cast<const ulonglong2*>(df + (int64_t)q.k * 32);
                        const ulonglong2 b1 = *reinterpret_cast<const ulonglong2*>(df + (int64_t)q.k * 32 + 16);
                        const uint64_t b[4] = {b0.x, b0.y, b1.x, b1.y};
                        proj_top2((proj_hamming(a, b) << PJ_KSHIFT) | q.k, m1, m2);
                    }
                }
            }
        }
#pragma unroll
        for (int m = PJ_GROUP / 2; m > 0; m >>= 1) {
            const int b1 = __shfl_xor(m1, m, PJ_GROUP), b2 = __shfl_xor(m2, m, PJ_GROUP);
            proj_top2_merge(b1, b2, m1, m2);
        }
        if (oi >= 0 && l == 0) {
            const aria_proj_obs o = proj_decide(u, v, m1, m2, prm);
            of[i] = o;
            if (o.flags & 4) atomicMin(&cl[o.kp_idx], proj_claim_key(o.hamming, i));
        }
    }
}

// rule 5: the record of k_proj_search holds the best keypoint in kp_idx; it stays only for the landmark whose key the
// keypoint's word holds
__global__ __launch_bounds__(PJ_BLOCK) void k_proj_resolve(const int* __restrict__ range, int land_cap, const int* __restrict__ ok_in,
                                                           const int* __restrict__ claims, int64_t kp_stride,
                                                           aria_proj_obs* __restrict__ obs) {
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!ok_in[f] || i >= range[2 * f + 1]) return;
    aria_proj_obs* o = obs + (int64_t)f * land_cap + i;
    const int flags = o->flags, k = o->kp_idx;
    if (!(flags & 2)) return;
    const bool won = (flags & 4) && claims[(int64_t)f * kp_stride + k] == proj_claim_key(o->hamming, i);
    if (won) o->flags = flags | 8;
    else o->kp_idx = -1;
}

__global__ __launch_bounds__(PJ_BLOCK) void k_proj_compact(const aria_keypoint* __restrict__ kp, int64_t kp_stride,
                                                           const aria_proj_landmark* __restrict__ land,
                                                           const int* __restrict__ range, int land_cap,
                                                           const int* __restrict__ ok_in, const aria_proj_obs* __restrict__ obs,
                                                           aria_pnp_corr* __restrict__ corr, aria_proj_pair* __restrict__ pairs,
                                                           int* __restrict__ ncorr) {
    __shared__ int wsum[PJ_BLOCK / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (!ok_in[f]) {
        if (tid == 0) ncorr[f] = 0;
        return;
    }
    const int first = range[2 * f], count = range[2 * f + 1];
    const aria_proj_obs* of = obs + (int64_t)f * land_cap;
    const aria_keypoint* kf = kp + (int64_t)f * kp_stride;
    aria_pnp_corr* oc = corr + (int64_t)f * land_cap;
    aria_proj_pair* op = pairs + (int64_t)f * land_cap;
    int run = 0;
    for (int base = 0; base < count; base += PJ_BLOCK) {
        const int i = base + tid;
        int k = -1;
        if (i < count && (of[i].flags & 8)) k = of[i].kp_idx;
        const bool keep = k >= 0;
        int total;
        const int slot = block_compact<PJ_BLOCK>(keep, wsum, total);
        if (keep) {
            const aria_proj_landmark* lm = land + (int64_t)first + i;
            aria_pnp_corr c;
            c.X[0] = lm->X[0]; c.X[1] = lm->X[1]; c.X[2] = lm->X[2];
            c.u = kf[k].x; c.v = kf[k].y;
            oc[run + slot] = c;
            aria_proj_pair pr;
            pr.landmark = first + i; pr.keypoint = k;
            op[run + slot] = pr;
        }
        run += total;
    }
    if (tid == 0) ncorr[f] = run;
}

// the join with the map: integer copies only (X travels as its 64-bit patterns)
__global__ __launch_bounds__(PJ_BLOCK) void k_proj_from_map(const aria_map_point* __restrict__ arena, const long long* __restrict__ d_size,
                                                            long long capacity, long long first, long long max_count, int pair_base,
                                                            int view, const aria_keypoint* __restrict__ kp,
                                                            const uint8_t* __restrict__ desc, const int* __restrict__ n_kp,
                                                            int64_t kp_stride, int n_slots, aria_proj_landmark* __restrict__ land,
                                                            int* __restrict__ nland, int* __restrict__ err) {
    long long size = *d_size;
    size = size < 0 ? 0 : (size > capacity ? capacity : size);
    long long cnt = (first + max_count < size ? first + max_count : size) - first;
    cnt = cnt < 0 ? 0 : cnt;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) nland[0] = (int)cnt;
    if (j >= max_count) return;
    unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the record as eight 64-bit words
    int octave = -1, source = -1;
    if (j < cnt) {
        const aria_map_point* pt = arena + (first + j);
        source = (int)(first + j);
        const long long s = (long long)pt->pair - (long long)pair_base;
        const int idx = view == 1 ? pt->idx1 : pt->idx2;
        bool ok = s >= 0 && s < n_slots;
        if (ok) {
            const int ns = n_kp[s];
            ok = ns >= 0 && ns <= kp_stride && idx >= 0 && idx < ns;
        }
        if (ok) {
            const unsigned long long* px = reinterpret_cast<const unsigned long long*>(pt->X);
            const unsigned long long* pd = reinterpret_cast<const unsigned long long*>(desc + (s * kp_stride + idx) * 32);
            w[0] = px[0]; w[1] = px[1]; w[2] = px[2];
            w[3] = pd[0]; w[4] = pd[1]; w[5] = pd[2]; w[6] = pd[3];
            octave = kp[s * kp_stride + idx].octave;
        } else {
            atomicOr(err, ERRBIT_PROJ_INPUT);
        }
    }
    w[7] = (unsigned long long)(unsigned int)octave | ((unsigned long long)(unsigned int)source << 32);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(land + j);
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = w[k];
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_proj_s : StageHandle {
    aria_proj_config cfg{};
    ProjParams prm{};
    // grow-only workspace of the batch path
    DeviceBuffer<int> d_ok;                // [n_frames]
    DeviceBuffer<int> d_cells;             // [n_frames][cells + 1]: where each cell starts in d_sorted
    DeviceBuffer<ProjEntry> d_sorted;      // [n_frames][kp_stride]
    DeviceBuffer<int> d_claims;            // [n_frames][kp_stride]
    // single-frame staging of the blocking host form (grow-only)
    DeviceBuffer<aria_keypoint> d_kp;
    DeviceBuffer<uint8_t> d_desc;
    DeviceBuffer<aria_proj_landmark> d_land;
    DeviceBuffer<aria_proj_obs> d_obs;
    DeviceBuffer<aria_pnp_corr> d_corr;
    DeviceBuffer<aria_proj_pair> d_pairs;
    DeviceBuffer<double> d_pose;           // 12 doubles
    DeviceBuffer<int> d_counts;            // n, first, count, n_corr
};

namespace {

bool fin(double v) { return std::isfinite(v); }

bool bad_config(const aria_proj_config* c) {
    return !c || c->struct_size != (int)sizeof(aria_proj_config) || bad_pinhole(c->fx, c->fy, c->cx, c->cy) || !fin(c->min_depth) || !(c->radius_px >= 0) || !(c->radius_px <= 1024) ||
           !(c->ratio >= 0) || !(c->ratio <= 1) || c->th_hamming < 0 || c->th_hamming > 257 || c->max_octave_diff < 0 ||
           c->max_octave_diff > kLevels;
}

ProjParams make_params(const aria_proj_config& c) {
    ProjParams p{};
    p.fx = c.fx; p.fy = c.fy; p.cx = c.cx; p.cy = c.cy; p.min_depth = c.min_depth;
    p.radius = (float)c.radius_px; p.ratio = c.ratio;
    p.th = c.th_hamming; p.mod = c.max_octave_diff;
    // scale[o] of aria_orb_level_info (orb_plan.cpp layer_scale)
    for (int l = 0; l < kLevels; l++) p.scale[l] = (float)std::pow((double)kScaleFactor, (double)l);
    return p;
}

}  // namespace

extern "C" {

void aria_proj_default_config(aria_proj_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_proj_config);
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0, as the pose and map stages
    c->min_depth = 0.1;                                                    // the map stage's
    // ORB-SLAM's published tracking constants; not tuned on a recording here
    c->radius_px = 15.0;
    c->ratio = 0.9f;
    c->th_hamming = 100;
    c->max_octave_diff = 1;
}

int aria_proj_create(const aria_proj_config* c, aria_proj_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_proj_create", [](aria_proj_s* h) {
        const char* what = "aria_proj_create";
        h->prm = make_params(h->cfg);
        int rc;
        if ((rc = h->d_counts.reserve(h->stream, 4, what)) != ARIA_OK) return rc;
        if ((rc = h->d_pose.reserve(h->stream, 12, what)) != ARIA_OK) return rc;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_proj_bin), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 PJ_MAX_CELLS * (int)sizeof(int));
        return e == hipSuccess ? (int)ARIA_OK : hip_fail(e, what, __FILE__, __LINE__);
    });
}

void aria_proj_destroy(aria_proj_t h) { stage_destroy(h); }

void* aria_proj_stream(aria_proj_t h) { return stage_stream(h); }

int aria_proj_check(aria_proj_t h) { return stage_check(h, {{ERRBIT_PROJ_INPUT, ARIA_E_INVALID}}); }

int aria_proj_search_batch_device(aria_proj_t h, const double* d_pose, const aria_keypoint* d_kp, const uint8_t* d_desc,
                                  const int* d_n, int64_t kp_stride, int width, int height, const aria_proj_landmark* d_land,
                                  int n_landmarks, const int* d_range, int land_cap, int n_frames, aria_proj_obs* d_obs,
                                  aria_pnp_corr* d_corr, aria_proj_pair* d_pairs, int* d_ncorr) {
    if (!h || !d_pose || !d_kp || !d_desc || !d_n || !d_range || !d_obs || !d_corr || !d_pairs || !d_ncorr || n_frames < 0 ||
        kp_stride < 1 || kp_stride > PJ_MAX_KP || width < 1 || height < 1 || width > PJ_MAX_DIM || height > PJ_MAX_DIM ||
        n_landmarks < 0 || (n_landmarks && !d_land) || land_cap < 1 || land_cap > PJ_MAX_LAND)
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const int cells = ((width + 31) >> PJ_CELL_LOG2) * ((height + 31) >> PJ_CELL_LOG2);
    int rc;
    if ((rc = h->d_ok.reserve(h->stream, (size_t)n_frames)) != ARIA_OK) return rc;
    if ((rc = h->d_cells.reserve(h->stream, (size_t)n_frames * (size_t)(cells + 1))) != ARIA_OK) return rc;
    if ((rc = h->d_sorted.reserve(h->stream, (size_t)n_frames * (size_t)kp_stride)) != ARIA_OK) return rc;
    if ((rc = h->d_claims.reserve(h->stream, (size_t)n_frames * (size_t)kp_stride)) != ARIA_OK) return rc;
    const int chunks = (land_cap + PJ_BLOCK - 1) / PJ_BLOCK;
    hipLaunchKernelGGL(k_proj_bin, dim3(n_frames), dim3(PJ_BLOCK), (size_t)cells * sizeof(int), h->stream, d_pose, d_kp, d_n,
                       kp_stride, width, height, n_landmarks, d_range, land_cap, h->d_ok.p, h->d_cells.p, cells + 1,
                       h->d_sorted.p, h->d_claims.p, h->d_err);
    hipLaunchKernelGGL(k_proj_search, dim3(chunks, n_frames), dim3(PJ_BLOCK), 0, h->stream, d_pose, d_desc, kp_stride, width,
                       height, d_land, d_range, land_cap, h->d_ok.p, h->d_cells.p, cells + 1, h->d_sorted.p, h->d_claims.p, h->prm,
                       d_obs);
    hipLaunchKernelGGL(k_proj_resolve, dim3(chunks, n_frames), dim3(PJ_BLOCK), 0, h->stream, d_range, land_cap, h->d_ok.p,
                       h->d_claims.p, kp_stride, d_obs);
    hipLaunchKernelGGL(k_proj_compact, dim3(n_frames), dim3(PJ_BLOCK), 0, h->stream, d_kp, kp_stride, d_land, d_range, land_cap,
                       h->d_ok.p, d_obs, d_corr, d_pairs, d_ncorr);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_proj_search(aria_proj_t h, const double* pose, const aria_keypoint* kp, const uint8_t* desc, int n, int width,
                     int height, const aria_proj_landmark* land, int n_landmarks, aria_proj_obs* obs, aria_pnp_corr* corr,
                     aria_proj_pair* pairs, int* n_corr) {
    if (!h || !pose || n < 0 || n > PJ_MAX_KP || (n && (!kp || !desc)) || width < 1 || height < 1 || width > PJ_MAX_DIM ||
        height > PJ_MAX_DIM || n_landmarks < 0 || n_landmarks > PJ_MAX_LAND || (n_landmarks && (!land || !obs || !corr || !pairs)))
        return ARIA_E_INVALID;
    if (n_corr) *n_corr = 0;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t kcap = (size_t)std::max(n, 1), lcap = (size_t)std::max(n_landmarks, 1);
    int rc;
    if ((rc = h->d_kp.reserve(h->stream, kcap)) != ARIA_OK) return rc;
    if ((rc = h->d_desc.reserve(h->stream, kcap * 32)) != ARIA_OK) return rc;
    if ((rc = h->d_land.reserve(h->stream, lcap)) != ARIA_OK) return rc;
    if ((rc = h->d_obs.reserve(h->stream, lcap)) != ARIA_OK) return rc;
    if ((rc = h->d_corr.reserve(h->stream, lcap)) != ARIA_OK) return rc;
    if ((rc = h->d_pairs.reserve(h->stream, lcap)) != ARIA_OK) return rc;
    const int counts[4] = {n, 0, n_landmarks, 0};
    if (n) {
        ARIA_HIP(hipMemcpyAsync(h->d_kp, kp, sizeof(aria_keypoint) * n, hipMemcpyHostToDevice, h->stream));
        ARIA_HIP(hipMemcpyAsync(h->d_desc, desc, (size_t)32 * n, hipMemcpyHostToDevice, h->stream));
    }
    if (n_landmarks)
        ARIA_HIP(hipMemcpyAsync(h->d_land, land, sizeof(aria_proj_landmark) * n_landmarks, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(hipMemcpyAsync(h->d_pose, pose, 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_counts, counts, sizeof(counts), hipMemcpyHostToDevice));
    rc = aria_proj_search_batch_device(h, h->d_pose, h->d_kp, h->d_desc, h->d_counts, (int64_t)kcap, width, height, h->d_land,
                                       n_landmarks, h->d_counts + 1, (int)lcap, 1, h->d_obs, h->d_corr, h->d_pairs,
                                       h->d_counts + 3);
    if (rc != ARIA_OK) return rc;
    int nc = 0;
    ARIA_HIP(memcpy_on(h->stream, &nc, h->d_counts + 3, sizeof(int), hipMemcpyDeviceToHost));
    if (n_landmarks) ARIA_HIP(memcpy_on(h->stream, obs, h->d_obs, sizeof(aria_proj_obs) * n_landmarks, hipMemcpyDeviceToHost));
    if (nc > 0 && nc <= n_landmarks) {
        ARIA_HIP(memcpy_on(h->stream, corr, h->d_corr, sizeof(aria_pnp_corr) * nc, hipMemcpyDeviceToHost));
        ARIA_HIP(memcpy_on(h->stream, pairs, h->d_pairs, sizeof(aria_proj_pair) * nc, hipMemcpyDeviceToHost));
    }
    if (n_corr) *n_corr = nc;
    return aria_proj_check(h);
}

int aria_proj_landmarks_from_map_device(aria_proj_t h, aria_map_t map, int64_t first, int64_t max_count, int pair_base, int view,
                                        const aria_keypoint* d_kp, const uint8_t* d_desc, const int* d_n, int64_t kp_stride,
                                        int n_slots, aria_proj_landmark* d_land, int* d_nland) {
    if (!h || !map || first < 0 || max_count < 0 || first + max_count >= (int64_t)INT_MAX || (view != 1 && view != 2) || !d_kp ||
        !d_desc || !d_n || kp_stride < 1 || kp_stride > PJ_MAX_KP || n_slots < 0 || !d_nland || (max_count && !d_land))
        return ARIA_E_INVALID;
    const aria_map_point* arena = nullptr;
    const long long* d_size = nullptr;
    int64_t capacity = 0;
    int map_device = -1;
    map_device_view(map, &arena, &d_size, &capacity, &map_device);
    if (map_device != h->device || !d_size) return ARIA_E_INVALID;   // the join reads the map's arena where it lies
    ARIA_HIP(hipSetDevice(h->device));
    const int blocks = (int)std::max<int64_t>((max_count + PJ_BLOCK - 1) / PJ_BLOCK, 1);
    hipLaunchKernelGGL(k_proj_from_map, dim3(blocks), dim3(PJ_BLOCK), 0, h->stream, arena, d_size,
                       (long long)(arena ? capacity : 0), (long long)first, (long long)max_count, pair_base, view, d_kp, d_desc, d_n,
                       kp_stride, n_slots, d_land, d_nland, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // extern "C"
