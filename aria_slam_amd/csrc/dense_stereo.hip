// Dense stereo on rectified pairs: census, four-path semi-global matching over 64 disparities, a disparity map in 1/16 px
// and a depth map. Semantics in include/aria_orb_hip.h ("dense stereo"); aria_slam_amd/dense_ref.py is the definition and
// this file equals it bit for bit.
//
// D = 64 is one wave: a lane holds a disparity. L_r(q, d -+ 1) are wave shifts by one lane (DPP), min_k L_r(q, k) is a DPP
// wave reduction, and the cost volume is never stored: C(y, x, d) is an xor and a 64-bit popcount of two census words
// wherever a path needs it. Only the running sum of the paths lives in HBM, as uint16 per cell.
//
// k_dense_census    a thread per pixel of either image: 62 clamped comparisons -> one uint64
// k_dense_horiz     a wave per row: the left-to-right walk writes L, the right-to-left walk adds its L to what the same lane
//                   wrote (a lane re-reads only its own stores)
// k_dense_down      a wave per column, four adjacent columns per workgroup: top-to-bottom, S += L
// k_dense_up_win    a wave per column, bottom-to-top; S = partial + L stays in registers: winner as the wave minimum of
//                   (S << 8 | d), uniqueness by ballot, the winner's neighbours by readlane, sub-pixel on one lane; every
//                   lane lowers the right view's packed minimum at (y, x - d) with an integer atomic-min
// k_dense_finish    a thread per pixel: left-right check against the packed minimum, final disparity, fp32 depth
// k_dense_sample    a thread per keypoint record: the stereo observation at the rounded keypoint
// The loads of the next pixel of a walk are issued before the current pixel's chain, so memory is off the serial path.
// No float atomics. No grid barrier. No LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_dense_config) == 96, "aria_dense_config is 96 bytes");
static_assert(sizeof(aria_stereo_obs) == 32, "aria_stereo_obs is 32 bytes");

namespace {

constexpr int DN_D = 64;                             // disparities = lanes of a wave
constexpr int DN_BLOCK = 256;
constexpr int DN_WAVES = DN_BLOCK / DN_D;            // rows / columns per workgroup of the walks
constexpr int DN_MAX_DIM = 4096;
constexpr int DN_MAX_IN_FLIGHT = 4096;               // grid.y of the census launch is twice this
constexpr int DN_MAX_KP = 1 << 20;
constexpr int DN_OUTSIDE = 64;                       // C where x - d < 0
constexpr int DN_BIG = 1 << 20;
constexpr int DN_INVALID = -16;
constexpr int64_t DN_BYTES_PER_PIXEL = 16 + 2 * DN_D + 4;   // two census words, 64 uint16 sums, the right view's minimum
constexpr int ERRBIT_DENSE_INPUT = 1;

struct DenseParams {
    float fx, fy, cx, cy, fb;
    int P1, P2, uniq, lr;
};

// ---- wave primitives (all 64 lanes active at every call site) ----
__device__ __forceinline__ int wave_min(int v) {
    constexpr int top = 0x7FFFFFFF;                      // the identity of min: lanes a control does not write keep it
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0xB1, 0xF, 0xF, false));    // quad_perm:[1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x4E, 0xF, 0xF, false));    // quad_perm:[2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x140, 0xF, 0xF, false));   // row_mirror: every lane holds its row's minimum
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x142, 0xA, 0xF, false));   // row_bcast:15 into rows 1, 3
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x143, 0xC, 0xF, false));   // row_bcast:31 into rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

// One step of rule 3 on lane d: Lq = L_r(q, d), m = min_k L_r(q, k).
__device__ __forceinline__ int sgm_step(int C, int Lq, int m, int d, int P1, int P2) {
    // lane 0 of wave_shr:1 and lane 63 of wave_shl:1 have no source lane and keep DN_BIG: those neighbours do not take part
    const int lo = __builtin_amdgcn_update_dpp(DN_BIG, Lq, 0x138, 0xF, 0xF, false);    // wave_shr:1: lane d reads lane d - 1
    const int hi = __builtin_amdgcn_update_dpp(DN_BIG, Lq, 0x130, 0xF, 0xF, false);    // wave_shl:1: lane d reads lane d + 1
    const int t = min(min(Lq, min(lo, hi) + P1), m + P2);
    return C + t - m;
}

__device__ __forceinline__ int cell_cost(uint64_t a, uint64_t b, int xr) { return xr >= 0 ? __popcll(a ^ b) : DN_OUTSIDE; }

__global__ __launch_bounds__(DN_BLOCK) void k_dense_census(const uint8_t* __restrict__ img_l, const uint8_t* __restrict__ img_r,
                                                           int64_t img_stride, int W, int H, int pitch,
                                                           uint64_t* __restrict__ cen) {
    const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= W * H) return;
    const int side = blockIdx.y & 1, p = blockIdx.y >> 1;
    const uint8_t* img = (side ? img_r : img_l) + (int64_t)p * img_stride;
    const int y = i / W, x = i - y * W;
    const int c = img[(int64_t)y * pitch + x];
    uint64_t bits = 0;
    int k = 0;
#pragma unroll
    for (int dy = -3; dy <= 3; dy++) {
        const uint8_t* row = img + (int64_t)min(max(y + dy, 0), H - 1) * pitch;
#pragma unroll
        for (int dx = -4; dx <= 4; dx++) {
            if (dy == 0 && dx == 0) continue;
            const int nb = row[min(max(x + dx, 0), W - 1)];
            bits |= (uint64_t)(nb < c) << k;
            k++;
        }
    }
    cen[((int64_t)(2 * p + side) * H + y) * W + x] = bits;
}

__global__ __launch_bounds__(DN_BLOCK) void k_dense_horiz(const uint64_t* __restrict__ cen, int W, int H, int P1, int P2,
                                                          uint16_t* __restrict__ S) {
    const int p = blockIdx.y, y = blockIdx.x * DN_WAVES + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (y >= H) return;                                  // a whole wave leaves
    const uint64_t* cl = cen + ((int64_t)(2 * p) * H + y) * W;
    const uint64_t* cr = cen + ((int64_t)(2 * p + 1) * H + y) * W;
    uint16_t* srow = S + ((int64_t)p * H + y) * W * DN_D + d;
    int Lq = 0, m = 0;
    uint64_t a = cl[0], b = d == 0 ? cr[0] : 0;
    for (int x = 0; x < W; x++) {                        // left to right
        uint64_t an = 0, bn = 0;
        if (x + 1 < W) {
            an = cl[x + 1];
            if (x + 1 - d >= 0) bn = cr[x + 1 - d];
        }
        const int C = cell_cost(a, b, x - d);
        const int step = sgm_step(C, Lq, m, d, P1, P2);
        Lq = x == 0 ? C : step;
        m = wave_min(Lq);
        srow[(int64_t)x * DN_D] = (uint16_t)Lq;
        a = an;
        b = bn;
    }
    a = cl[W - 1];
    b = W - 1 - d >= 0 ? cr[W - 1 - d] : 0;
    int s = srow[(int64_t)(W - 1) * DN_D];
    for (int x = W - 1; x >= 0; x--) {                   // right to left
        uint64_t an = 0, bn = 0;
        int sn = 0;
        if (x > 0) {
            an = cl[x - 1];
            if (x - 1 - d >= 0) bn = cr[x - 1 - d];
            sn = srow[(int64_t)(x - 1) * DN_D];
        }
        const int C = cell_cost(a, b, x - d);
        const int step = sgm_step(C, Lq, m, d, P1, P2);
        Lq = x == W - 1 ? C : step;
        m = wave_min(Lq);
        srow[(int64_t)x * DN_D] = (uint16_t)(s + Lq);
        a = an;
        b = bn;
        s = sn;
    }
}

__global__ __launch_bounds__(DN_BLOCK) void k_dense_down(const uint64_t* __restrict__ cen, int W, int H, int P1, int P2,
                                                         uint16_t* __restrict__ S) {
    const int p = blockIdx.y, x = blockIdx.x * DN_WAVES + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (x >= W) return;
    const int xr = x - d, xc = max(xr, 0);
    const uint64_t* cl = cen + (int64_t)(2 * p) * H * W + x;
    const uint64_t* cr = cen + (int64_t)(2 * p + 1) * H * W + xc;
    uint16_t* scol = S + ((int64_t)p * H * W + x) * DN_D + d;
    const int64_t srow = (int64_t)W * DN_D;
    int Lq = 0, m = 0;
    uint64_t a = cl[0], b = cr[0];
    int s = scol[0];
    for (int y = 0; y < H; y++) {
        uint64_t an = 0, bn = 0;
        int sn = 0;
        if (y + 1 < H) {
            an = cl[(int64_t)(y + 1) * W];
            bn = cr[(int64_t)(y + 1) * W];
            sn = scol[(y + 1) * srow];
        }
        const int C = cell_cost(a, b, xr);
        const int step = sgm_step(C, Lq, m, d, P1, P2);
        Lq = y == 0 ? C : step;
        m = wave_min(Lq);
        scol[y * srow] = (uint16_t)(s + Lq);
        a = an;
        b = bn;
        s = sn;
    }
}

__global__ __launch_bounds__(DN_BLOCK) void k_dense_up_win(const uint64_t* __restrict__ cen, int W, int H, int P1, int P2,
                                                           int uniq, const uint16_t* __restrict__ S,
                                                           unsigned int* __restrict__ right_min, int16_t* __restrict__ disp,
                                                           int64_t disp_stride, int disp_pitch) {
    const int p = blockIdx.y, x = blockIdx.x * DN_WAVES + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (x >= W) return;
    const int xr = x - d, xc = max(xr, 0);
    const uint64_t* cl = cen + (int64_t)(2 * p) * H * W + x;
    const uint64_t* cr = cen + (int64_t)(2 * p + 1) * H * W + xc;
    const uint16_t* scol = S + ((int64_t)p * H * W + x) * DN_D + d;
    unsigned int* rcol = right_min + (int64_t)p * H * W + xc;
    int16_t* dcol = disp + (int64_t)p * disp_stride + x;
    const int64_t srow = (int64_t)W * DN_D;
    int Lq = 0, m = 0;
    uint64_t a = cl[(int64_t)(H - 1) * W], b = cr[(int64_t)(H - 1) * W];
    int s = scol[(H - 1) * srow];
    for (int y = H - 1; y >= 0; y--) {
        uint64_t an = 0, bn = 0;
        int sn = 0;
        if (y > 0) {
            an = cl[(int64_t)(y - 1) * W];
            bn = cr[(int64_t)(y - 1) * W];
            sn = scol[(y - 1) * srow];
        }
        const int C = cell_cost(a, b, xr);
        const int step = sgm_step(C, Lq, m, d, P1, P2);
        Lq = y == H - 1 ? C : step;
        m = wave_min(Lq);
        const int St = s + Lq;                           // S(y, x, d), complete
        const int key = (St << 8) | d;                   // least S, ties to the lowest d
        const int kmin = wave_min(key);
        const int best = kmin & 255, sb = kmin >> 8;
        const bool far = d < best - 1 || d > best + 1;
        const bool ambiguous = __ballot(far && St * (100 - uniq) < sb * 100) != 0;
        const int sm = __builtin_amdgcn_readlane(St, max(best - 1, 0));
        const int sp = __builtin_amdgcn_readlane(St, min(best + 1, DN_D - 1));
        int d16 = 16 * best;
        if (best > 0 && best < DN_D - 1) {
            const int den2 = max(sm + sp - 2 * sb, 1);
            d16 += ((sm - sp) * 16 + den2) / (2 * den2);  // truncates towards zero
        }
        if (ambiguous) d16 = DN_INVALID;
        if (d == 0) dcol[(int64_t)y * disp_pitch] = (int16_t)d16;
        if (xr >= 0) atomicMin(rcol + (int64_t)y * W, (unsigned int)key);
        a = an;
        b = bn;
        s = sn;
    }
}

__global__ __launch_bounds__(DN_BLOCK) void k_dense_finish(const unsigned int* __restrict__ right_min, int W, int H, int lr,
                                                           float fb, int16_t* __restrict__ disp, int64_t disp_stride,
                                                           int disp_pitch, float* __restrict__ depth, int64_t depth_stride,
                                                           int depth_pitch) {
    const int i = blockIdx.x * DN_BLOCK + threadIdx.x, p = blockIdx.y;
    if (i >= W * H) return;
    const int y = i / W, x = i - y * W;
    int16_t* dp = disp + (int64_t)p * disp_stride + (int64_t)y * disp_pitch + x;
    int d16 = *dp;
    if (d16 >= 0 && lr >= 0) {
        const int best = (d16 + 7) >> 4;                 // d16 lies in [16 best - 7, 16 best + 8]
        const int xr = x - best;
        bool ok = xr >= 0;
        if (ok) {
            const int dr = (int)(right_min[((int64_t)p * H + y) * W + xr] & 255u);
            ok = abs(dr - best) <= lr;
        }
        if (!ok) {
            d16 = DN_INVALID;
            *dp = (int16_t)DN_INVALID;
        }
    }
    if (depth) depth[(int64_t)p * depth_stride + (int64_t)y * depth_pitch + x] = d16 > 0 ? fb / ((float)d16 * 0.0625f) : 0.0f;
}

__device__ __forceinline__ aria_stereo_obs unmatched_obs() {
    aria_stereo_obs o;
    o.u_right = 0.0f; o.disparity = 0.0f; o.depth = -1.0f; o.X = 0.0f; o.Y = 0.0f;
    o.right_idx = -1; o.hamming = 0; o.sad = 0;
    return o;
}

__global__ __launch_bounds__(DN_BLOCK) void k_dense_sample(const int16_t* __restrict__ disp, int64_t disp_stride, int disp_pitch,
                                                           int W, int H, const aria_keypoint* __restrict__ kp,
                                                           const int* __restrict__ n_kp, int64_t kp_stride, DenseParams prm,
                                                           aria_stereo_obs* __restrict__ obs, int* __restrict__ err) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    const int n = n_kp[f];
    const bool bad = n < 0 || n > kp_stride;             // uniform: the frame is skipped
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, ERRBIT_DENSE_INPUT);
    if (i >= kp_stride) return;
    aria_stereo_obs o = unmatched_obs();
    if (!bad && i < n) {
        const aria_keypoint k = kp[(int64_t)f * kp_stride + i];
        const float big = 1.0e6f;
        const int u = (int)rintf(fminf(fmaxf(k.x, -big), big));
        const int v = (int)rintf(fminf(fmaxf(k.y, -big), big));
        if (u >= 0 && u <= W - 1 && v >= 0 && v <= H - 1) {
            const int d16 = disp[(int64_t)f * disp_stride + (int64_t)v * disp_pitch + u];
            if (d16 > 0) {
                const float dsp = (float)d16 * 0.0625f;
                const float depth = prm.fb / dsp;
                o.u_right = k.x - dsp;
                o.disparity = dsp;
                o.depth = depth;
                o.X = (k.x - prm.cx) * depth / prm.fx;
                o.Y = (k.y - prm.cy) * depth / prm.fy;
                o.right_idx = ARIA_DENSE_NO_KEYPOINT; o.hamming = 0; o.sad = 0;
            }
        }
    }
    obs[(int64_t)f * kp_stride + i] = o;
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_dense_s : StageHandle {
    aria_dense_config cfg{};
    DenseParams prm{};
    int in_flight = 0;
    DeviceBuffer<uint8_t> d_scratch;                           // census, S and the right view's minimum of one group
    // single-pair staging of the blocking host forms (grow-only)
    DeviceBuffer<uint8_t> d_img;                               // left, right: 2 * W * H
    DeviceBuffer<int16_t> d_disp;
    DeviceBuffer<float> d_depth;
    DeviceBuffer<aria_keypoint> d_kp;
    DeviceBuffer<aria_stereo_obs> d_obs;
    DeviceBuffer<int> d_count;
};

namespace {

int64_t pairs_for(const aria_dense_config* c) {
    const int64_t per_pair = DN_BYTES_PER_PIXEL * c->max_width * c->max_height;
    return std::min<int64_t>(c->scratch_bytes / per_pair, DN_MAX_IN_FLIGHT);
}

bool bad_config(const aria_dense_config* c) {
    return !c || c->struct_size != (int)sizeof(aria_dense_config) || bad_pinhole(c->fx, c->fy, c->cx, c->cy) ||
           !(c->baseline > 0) || !std::isfinite(c->baseline) || c->num_disparities != DN_D || c->P1 < 1 ||
           c->P1 > c->P2 || c->P2 > 127 || c->uniqueness < 0 || c->uniqueness > 99 || c->lr_max_diff > DN_D - 1 ||
           c->max_width < 1 || c->max_width > DN_MAX_DIM || c->max_height < 1 || c->max_height > DN_MAX_DIM ||
           c->scratch_bytes < 1 || pairs_for(c) < 1;
}

}  // namespace

extern "C" {

void aria_dense_default_config(aria_dense_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_dense_config);
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0, as the sparse stage
    c->baseline = 0.110;
    c->num_disparities = DN_D;
    c->P1 = 8;
    c->P2 = 32;
    c->uniqueness = 10;
    c->lr_max_diff = 1;
    c->max_width = 752;
    c->max_height = 480;
    c->scratch_bytes = (int64_t)1 << 30;
}

int aria_dense_create(const aria_dense_config* c, aria_dense_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_dense_create", [](aria_dense_s* h) {
        const aria_dense_config& c = h->cfg;
        h->prm.fx = (float)c.fx; h->prm.fy = (float)c.fy; h->prm.cx = (float)c.cx; h->prm.cy = (float)c.cy;
        h->prm.fb = h->prm.fx * (float)c.baseline;           // the product formed once, in fp32
        h->prm.P1 = c.P1; h->prm.P2 = c.P2; h->prm.uniq = c.uniqueness; h->prm.lr = c.lr_max_diff;
        h->in_flight = (int)pairs_for(&c);
        return h->d_count.reserve(h->stream, 1, "aria_dense_create");
    });
}

void aria_dense_destroy(aria_dense_t h) { stage_destroy(h); }

void* aria_dense_stream(aria_dense_t h) { return stage_stream(h); }

int aria_dense_pairs_in_flight(aria_dense_t h) { return h ? h->in_flight : ARIA_E_INVALID; }

int64_t aria_dense_scratch_bytes_per_pair(int width, int height) {
    if (width < 1 || height < 1 || width > DN_MAX_DIM || height > DN_MAX_DIM) return ARIA_E_INVALID;
    return DN_BYTES_PER_PIXEL * width * height;
}

int64_t aria_dense_algorithmic_bytes(int width, int height) {
    if (width < 1 || height < 1) return ARIA_E_INVALID;
    return (int64_t)width * height * (2 + 2 + 4);        // both images read, int16 disparity and fp32 depth written
}

int aria_dense_check(aria_dense_t h) { return stage_check(h, {{ERRBIT_DENSE_INPUT, ARIA_E_INVALID}}); }

int aria_dense_compute_batch_device(aria_dense_t h, const uint8_t* d_left, const uint8_t* d_right, int64_t img_stride, int width,
                                    int height, int pitch, int n_pairs, int16_t* d_disp, int64_t disp_stride, int disp_pitch,
                                    float* d_depth, int64_t depth_stride, int depth_pitch) {
    if (!h || !d_left || !d_right || !d_disp || n_pairs < 0 || width < 1 || height < 1 || width > h->cfg.max_width ||
        height > h->cfg.max_height || pitch < width || disp_pitch < width || (d_depth && depth_pitch < width))
        return ARIA_E_INVALID;
    const int W = width, H = height;
    if (n_pairs > 1 && (img_stride < (int64_t)pitch * (H - 1) + W || disp_stride < (int64_t)disp_pitch * (H - 1) + W ||
                        (d_depth && depth_stride < (int64_t)depth_pitch * (H - 1) + W)))
        return ARIA_E_INVALID;
    if (n_pairs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const int G = std::min(h->in_flight, n_pairs);
    const int64_t px = (int64_t)W * H;
    const int rc = h->d_scratch.reserve(h->stream, (size_t)(DN_BYTES_PER_PIXEL * px * G));
    if (rc != ARIA_OK) return rc;
    uint64_t* cen = reinterpret_cast<uint64_t*>(h->d_scratch.p);                       // [G][2][H][W]
    uint16_t* S = reinterpret_cast<uint16_t*>(h->d_scratch.p + 16 * px * G);           // [G][H][W][64]
    unsigned int* rmin = reinterpret_cast<unsigned int*>(h->d_scratch.p + (16 + 2 * DN_D) * px * G);   // [G][H][W]
    const unsigned pix_blocks = (unsigned)((px + DN_BLOCK - 1) / DN_BLOCK);
    const unsigned row_blocks = (unsigned)((H + DN_WAVES - 1) / DN_WAVES), col_blocks = (unsigned)((W + DN_WAVES - 1) / DN_WAVES);
    const DenseParams& q = h->prm;
    for (int g0 = 0; g0 < n_pairs; g0 += G) {            // groups of pairs_in_flight share the scratch, in stream order
        const int g = std::min(G, n_pairs - g0);
        const uint8_t* il = d_left + (int64_t)g0 * img_stride;
        const uint8_t* ir = d_right + (int64_t)g0 * img_stride;
        int16_t* dd = d_disp + (int64_t)g0 * disp_stride;
        float* dz = d_depth ? d_depth + (int64_t)g0 * depth_stride : nullptr;
        ARIA_HIP(hipMemsetAsync(rmin, 0xFF, (size_t)(4 * px * g), h->stream));
        hipLaunchKernelGGL(k_dense_census, dim3(pix_blocks, 2 * g), dim3(DN_BLOCK), 0, h->stream, il, ir, img_stride, W, H, pitch, cen);
        hipLaunchKernelGGL(k_dense_horiz, dim3(row_blocks, g), dim3(DN_BLOCK), 0, h->stream, cen, W, H, q.P1, q.P2, S);
        hipLaunchKernelGGL(k_dense_down, dim3(col_blocks, g), dim3(DN_BLOCK), 0, h->stream, cen, W, H, q.P1, q.P2, S);
        hipLaunchKernelGGL(k_dense_up_win, dim3(col_blocks, g), dim3(DN_BLOCK), 0, h->stream, cen, W, H, q.P1, q.P2, q.uniq, S, rmin,
                           dd, disp_stride, disp_pitch);
        hipLaunchKernelGGL(k_dense_finish, dim3(pix_blocks, g), dim3(DN_BLOCK), 0, h->stream, rmin, W, H, q.lr, q.fb, dd, disp_stride,
                           disp_pitch, dz, depth_stride, depth_pitch);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_dense_compute(aria_dense_t h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                       int16_t* disp, float* depth) {
    if (!h || !left || !right || !disp || width < 1 || height < 1 || width > h->cfg.max_width || height > h->cfg.max_height ||
        pitch < width)
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t px = (size_t)width * height;
    int rc;
    if ((rc = h->d_img.reserve(h->stream, 2 * px)) != ARIA_OK) return rc;
    if ((rc = h->d_disp.reserve(h->stream, px)) != ARIA_OK) return rc;
    if (depth && (rc = h->d_depth.reserve(h->stream, px)) != ARIA_OK) return rc;
    uint8_t* d_ir = h->d_img + h->d_img.cap / 2;         // the staging halves sit at the buffer's current capacity
    ARIA_HIP(hipMemcpy2DAsync(h->d_img, (size_t)width, left, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice,
                              h->stream));
    ARIA_HIP(hipMemcpy2DAsync(d_ir, (size_t)width, right, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice,
                              h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));           // the host images are free again
    rc = aria_dense_compute_batch_device(h, h->d_img, d_ir, 0, width, height, width, 1, h->d_disp, 0, width,
                                         depth ? h->d_depth.p : nullptr, 0, width);
    if (rc != ARIA_OK) return rc;
    if (depth) ARIA_HIP(hipMemcpyAsync(depth, h->d_depth, px * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(memcpy_on(h->stream, disp, h->d_disp, px * sizeof(int16_t), hipMemcpyDeviceToHost));
    return aria_dense_check(h);
}

int aria_dense_sample_batch_device(aria_dense_t h, const int16_t* d_disp, int64_t disp_stride, int disp_pitch, int width,
                                   int height, const aria_keypoint* d_kp, const int* d_n, int64_t kp_stride, int n_frames,
                                   aria_stereo_obs* d_obs) {
    if (!h || !d_disp || !d_kp || !d_n || !d_obs || n_frames < 0 || n_frames > 65535 || kp_stride < 1 || kp_stride > DN_MAX_KP ||
        width < 1 || height < 1 || width > DN_MAX_DIM || height > DN_MAX_DIM || disp_pitch < width ||
        (n_frames > 1 && disp_stride < (int64_t)disp_pitch * (height - 1) + width))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dense_sample, dim3((unsigned)((kp_stride + DN_BLOCK - 1) / DN_BLOCK), n_frames), dim3(DN_BLOCK), 0, h->stream,
                       d_disp, disp_stride, disp_pitch, width, height, d_kp, d_n, kp_stride, h->prm, d_obs, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_dense_sample(aria_dense_t h, const int16_t* disp, int width, int height, int disp_pitch, const aria_keypoint* kp, int n,
                      aria_stereo_obs* obs) {
    if (!h || !disp || width < 1 || height < 1 || width > DN_MAX_DIM || height > DN_MAX_DIM || disp_pitch < width || n < 0 ||
        n > DN_MAX_KP || (n && (!kp || !obs)))
        return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t px = (size_t)width * height;
    int rc;
    if ((rc = h->d_disp.reserve(h->stream, px)) != ARIA_OK) return rc;
    if ((rc = h->d_kp.reserve(h->stream, (size_t)n)) != ARIA_OK) return rc;
    if ((rc = h->d_obs.reserve(h->stream, (size_t)n)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpy2DAsync(h->d_disp, (size_t)width * sizeof(int16_t), disp, (size_t)disp_pitch * sizeof(int16_t),
                              (size_t)width * sizeof(int16_t), (size_t)height, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(hipMemcpyAsync(h->d_kp, kp, sizeof(aria_keypoint) * n, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_count, &n, sizeof(int), hipMemcpyHostToDevice));
    rc = aria_dense_sample_batch_device(h, h->d_disp, 0, width, width, height, h->d_kp, h->d_count, n, 1, h->d_obs);
    if (rc != ARIA_OK) return rc;
    ARIA_HIP(memcpy_on(h->stream, obs, h->d_obs, sizeof(aria_stereo_obs) * n, hipMemcpyDeviceToHost));
    return aria_dense_check(h);
}

}  // extern "C"
