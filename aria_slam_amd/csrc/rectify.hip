// Undistortion and stereo rectification: the rectifying geometry from the calibration, image batches warped in HBM into the
// layout the batch extractor and the stereo stage read, keypoints moved into the undistorted / rectified frame. Semantics in
// include/aria_orb_hip.h ("rectification"); aria_slam_amd/rectify_ref.py is the definition and this file equals it bit for bit.
//
// k_rect_build_map  once per camera at create: a lane per destination pixel, fp64, the uint32 map (qx | qy << 16 in 1/32 px,
//                   0xFFFFFFFF = invalid). Map rows are padded to a multiple of four entries (invalid), so a lane's four
//                   entries are one aligned 16-byte load.
// k_rect_remap      the hot path. A 256-lane workgroup owns a 64 x 16 destination tile (compact source footprint: a 256-pixel
//                   row segment would span up to 28 source rows at EuRoC's distortion); a lane owns four horizontally adjacent
//                   pixels. It loads their map words once (one 16-byte load), decodes offset and the four bilinear weights
//                   once, and keeps them in registers over a loop of up to `group` frames of the batch: the 4 B / pixel of
//                   the map is read once per group, not once per frame. Per frame a lane whose taps lie within 8 columns
//                   and 3 rows (the usual case) issues three unaligned 8-byte loads and shifts the tap pairs out of the
//                   registers; otherwise two unaligned 16-bit loads per pixel. Four integer multiply-adds per pixel and one
//                   dword store per lane; tail columns and unaligned destination rows take a byte path. Padding is never
//                   written.
// k_rect_points     a lane per keypoint: 20 fixed-point iterations of the inverse distortion in fp64, rotation, projection.
// k_rect_build_map_kb4, k_rect_points_kb4   the same two jobs for the fisheye model KB4 (aria_rect_config::model): atan and
//                   tan from + - * / and sqrt (rect_atan, rect_tan), ten Newton steps per keypoint. k_rect_remap reads a map
//                   of either model.
// No atomics but the deferred-error OR. Plain HIP C++: the anonymous namespace below, up to the C-ABI, also compiles for the
// host (tests/test_rectify_kernel_emulation.py).
// The variants build (-DARIA_VARIANTS) adds k_rect_remap_lds, the measured and rejected read form (the tile's source bounding
// box staged in LDS per frame, the taps gathered from there), and the ARIA_RECT_GROUP / ARIA_RECT_READ (lds, taps) switches for
// tools/rect_rate.py's A/B. The numbers are in DESIGN.md section 18.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_rect_camera) == 144, "aria_rect_camera is 144 bytes");
static_assert(sizeof(aria_rect_config) == 368, "aria_rect_config is 368 bytes");

namespace {

constexpr int RECT_BLOCK = 256;
constexpr int RECT_TILE_W = 64, RECT_TILE_H = 16;     // destination tile of a workgroup: 16 lanes x 4 pixels wide, 16 rows
constexpr int RECT_GROUP = 8;                          // frames that share one load and decode of the map words
constexpr int RECT_MAX_DIM = 2047;                     // 11 bits of pixel + 5 bits of fraction per axis of a map word
constexpr int RECT_MAX_PITCH = 1 << 19;                // source row pitch bound: a tap's byte offset inside a frame fits an int
constexpr int RECT_POINT_ITERS = 20;
constexpr uint32_t RECT_INVALID = 0xFFFFFFFFu;
constexpr int ERRBIT_RECT_INPUT = 1;

struct RectCam {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3, R[9];
    double nfx, nfy, ncx, ncy;
};

struct RectKp { float x, y, size, angle, response; int octave; };   // aria_keypoint's 24 bytes

__device__ __forceinline__ bool rect_finite(double v) { return fabs(v) <= DBL_MAX; }

// rad, dx, dy of the radtan model at normalised (x, y): the header's expressions, left to right
__device__ __forceinline__ void rect_terms(const RectCam& c, double x, double y, double& rad, double& dx, double& dy) {
    const double r2 = x * x + y * y;
    rad = ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2 + 1.0;
    dx = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
    dy = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
}

__global__ __launch_bounds__(RECT_BLOCK) void k_rect_build_map(RectCam c, int src_w, int src_h, int dst_w, int dst_h, int map_pitch,
                                                               uint32_t* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * RECT_BLOCK + threadIdx.x;
    if (i >= (int64_t)map_pitch * dst_h) return;
    const int v = (int)(i / map_pitch), u = (int)(i % map_pitch);
    uint32_t word = RECT_INVALID;
    if (u < dst_w) {
        const double x = ((double)u - c.ncx) / c.nfx, y = ((double)v - c.ncy) / c.nfy;
        const double X = c.R[0] * x + c.R[3] * y + c.R[6];
        const double Y = c.R[1] * x + c.R[4] * y + c.R[7];
        const double Z = c.R[2] * x + c.R[5] * y + c.R[8];
        const double xn = X / Z, yn = Y / Z;
        double rad, dx, dy;
        rect_terms(c, xn, yn, rad, dx, dy);
        const double xd = xn * rad + dx, yd = yn * rad + dy;
        const double su = c.fx * xd + c.cx, sv = c.fy * yd + c.cy;
        const double qx = floor(su * 32.0 + 0.5), qy = floor(sv * 32.0 + 0.5);
        // ix >= 0 and ix + 1 <= Wsrc - 1 on the exact fp64 integers, before the conversion
        const bool ok = Z > 0.0 && rect_finite(su) && rect_finite(sv) && qx >= 0.0 && qy >= 0.0 &&
                        qx < (double)(src_w - 1) * 32.0 && qy < (double)(src_h - 1) * 32.0;
        if (ok) word = (uint32_t)(int)qx | ((uint32_t)(int)qy << 16);
    }
    map[i] = word;
}

__device__ __forceinline__ uint32_t rect_ld_u16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// one map word -> the byte offset of the upper-left tap and the four weights as (w00 | w01 << 16), (w10 | w11 << 16).
// An invalid word reads the image's first taps (always inside: the source is at least 2 x 2) with weight 0.
__device__ __forceinline__ void rect_decode(uint32_t word, int src_pitch, int& off, uint32_t& wt, uint32_t& wb, bool& ok) {
    ok = word != RECT_INVALID;
    const uint32_t m = ok ? word : 0u;
    const uint32_t qx = m & 0xFFFFu, qy = m >> 16;
    const uint32_t fx5 = qx & 31u, fy5 = qy & 31u;
    off = (int)(qy >> 5) * src_pitch + (int)(qx >> 5);
    wt = ((32u - fx5) * (32u - fy5)) | ((fx5 * (32u - fy5)) << 16);
    wb = ((32u - fx5) * fy5) | ((fx5 * fy5) << 16);
}

__device__ __forceinline__ uint32_t rect_pixel(const uint8_t* src, int off, int src_pitch, uint32_t wt, uint32_t wb, bool ok,
                                               uint32_t fill) {
    const uint32_t t = rect_ld_u16(src + off), b = rect_ld_u16(src + off + src_pitch);
    const uint32_t s = (t & 255u) * (wt & 0xFFFFu) + (t >> 8) * (wt >> 16) + (b & 255u) * (wb & 0xFFFFu) + (b >> 8) * (wb >> 16);
    return ok ? (s + 512u) >> 10 : fill;
}

__device__ __forceinline__ uint64_t rect_ld_u64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ uint32_t rect_blend(uint32_t t, uint32_t b, uint32_t wt, uint32_t wb, bool ok, uint32_t fill) {
    const uint32_t s = (t & 255u) * (wt & 0xFFFFu) + (t >> 8) * (wt >> 16) + (b & 255u) * (wb & 0xFFFFu) + (b >> 8) * (wb >> 16);
    return ok ? (s + 512u) >> 10 : fill;
}

// grid: (tiles across, tiles down, frame groups). How a lane reads the taps of its four pixels is decided once per map load:
//   rows    the valid pixels' taps lie within 8 columns and 3 rows that are inside the image: three unaligned 8-byte loads per
//           frame (rows iy_min, iy_min + 1, iy_min + 2, the last clamped to the image when no pixel needs it) and the taps
//           shifted out of the registers -- 3 load instructions instead of 8;
//   taps    otherwise (strong zoom-out, the image's right edge): the two 16-bit loads per pixel;
//   none    no valid pixel: no load at all.
// `rows_ok` = 0 forces the taps form (variants build: the A/B of tools/rect_rate.py).
__global__ __launch_bounds__(RECT_BLOCK) void k_rect_remap(const uint32_t* __restrict__ map, int map_pitch, int dst_w, int dst_h,
                                                           const uint8_t* __restrict__ src, int64_t src_stride, int src_pitch,
                                                           int src_w, int src_h, int rows_ok, int n_frames, int group,
                                                           uint8_t* __restrict__ dst, int64_t dst_stride, int dst_pitch,
                                                           uint32_t fill) {
    const int lx = threadIdx.x % (RECT_TILE_W / 4), ly = threadIdx.x / (RECT_TILE_W / 4);
    const int x = blockIdx.x * RECT_TILE_W + 4 * lx, y = blockIdx.y * RECT_TILE_H + ly;
    if (x >= dst_w || y >= dst_h) return;
    const uint4 w4 = *reinterpret_cast<const uint4*>(map + (int64_t)y * map_pitch + x);   // x % 4 == 0, map_pitch % 4 == 0
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    int off[4];
    uint32_t wt[4], wb[4];
    bool ok[4];
    int x0 = 1 << 30, y0 = 1 << 30, x1 = -1, y1 = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        rect_decode(w[k], src_pitch, off[k], wt[k], wb[k], ok[k]);
        const int ix = (int)((w[k] & 0xFFFFu) >> 5), iy = (int)(w[k] >> 21);
        x0 = ok[k] ? min(x0, ix) : x0; x1 = ok[k] ? max(x1, ix) : x1;
        y0 = ok[k] ? min(y0, iy) : y0; y1 = ok[k] ? max(y1, iy) : y1;
    }
    const bool any = x1 >= 0;
    const bool rows = any && rows_ok && x1 - x0 <= 6 && y1 - y0 <= 1 && x0 + 7 <= src_w - 1;
    int sh[4];                                               // rows form: bit shift of the pixel's tap pair, + 64 for the lower row pair
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ix = (int)((w[k] & 0xFFFFu) >> 5), iy = (int)(w[k] >> 21);
        sh[k] = (ok[k] && rows) ? 8 * (ix - x0) + 64 * (iy - y0) : 0;
    }
    const int base = rows ? y0 * src_pitch + x0 : 0;
    const int base2 = rows ? min(y0 + 2, src_h - 1) * src_pitch + x0 : 0;
    const int f0 = blockIdx.z * group, f1 = min(f0 + group, n_frames);
    const int64_t drow = (int64_t)y * dst_pitch + x;
    const int ncol = min(4, dst_w - x);
    for (int f = f0; f < f1; f++) {
        const uint8_t* s = src + (int64_t)f * src_stride;
        uint8_t* d = dst + (int64_t)f * dst_stride + drow;
        uint32_t px[4] = {fill, fill, fill, fill};
        if (rows) {
            const uint64_t r0 = rect_ld_u64(s + base), r1 = rect_ld_u64(s + base + src_pitch), r2 = rect_ld_u64(s + base2);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool low = sh[k] >= 64;
                const int b = sh[k] & 63;
                const uint32_t t = (uint32_t)((low ? r1 : r0) >> b) & 0xFFFFu, u = (uint32_t)((low ? r2 : r1) >> b) & 0xFFFFu;
                px[k] = rect_blend(t, u, wt[k], wb[k], ok[k], fill);
            }
        } else if (any) {
#pragma unroll
            for (int k = 0; k < 4; k++) px[k] = rect_pixel(s, off[k], src_pitch, wt[k], wb[k], ok[k], fill);
        }
        if (ncol == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
            *reinterpret_cast<uint32_t*>(d) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < ncol) d[k] = (uint8_t)px[k];
        }
    }
}

#ifdef ARIA_VARIANTS
// The other read form: the workgroup finds the source bounding box of its tile's valid pixels, stages it into LDS with dword
// loads for every frame and gathers the four taps from LDS. Tiles whose box does not fit (or is empty) read from global memory
// as k_rect_remap does. Same grid, same results.
constexpr int RECT_LDS_BYTES = 16384;
__global__ __launch_bounds__(RECT_BLOCK) void k_rect_remap_lds(const uint32_t* __restrict__ map, int map_pitch, int dst_w, int dst_h,
                                                               const uint8_t* __restrict__ src, int64_t src_stride, int src_pitch,
                                                               int src_w, int n_frames, int group, uint8_t* __restrict__ dst,
                                                               int64_t dst_stride, int dst_pitch, uint32_t fill) {
    __shared__ int s_box[4];                                  // x0, y0, x1, y1 of the upper-left taps
    __shared__ uint32_t s_tile[RECT_LDS_BYTES / 4];
    const int tid = threadIdx.x;
    const int lx = tid % (RECT_TILE_W / 4), ly = tid / (RECT_TILE_W / 4);
    const int x = blockIdx.x * RECT_TILE_W + 4 * lx, y = blockIdx.y * RECT_TILE_H + ly;
    const bool live = x < dst_w && y < dst_h;
    if (tid == 0) { s_box[0] = s_box[1] = 1 << 30; s_box[2] = s_box[3] = -1; }
    __syncthreads();
    uint32_t w[4] = {RECT_INVALID, RECT_INVALID, RECT_INVALID, RECT_INVALID};
    if (live) {
        const uint4 w4 = *reinterpret_cast<const uint4*>(map + (int64_t)y * map_pitch + x);
        w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
    }
    int off[4], ix[4], iy[4];
    uint32_t wt[4], wb[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        rect_decode(w[k], src_pitch, off[k], wt[k], wb[k], ok[k]);
        ix[k] = ok[k] ? (int)((w[k] & 0xFFFFu) >> 5) : 0;
        iy[k] = ok[k] ? (int)(w[k] >> 21) : 0;
        if (ok[k]) {
            atomicMin(&s_box[0], ix[k]); atomicMin(&s_box[1], iy[k]);
            atomicMax(&s_box[2], ix[k]); atomicMax(&s_box[3], iy[k]);
        }
    }
    __syncthreads();
    const int bx0 = s_box[0], by0 = s_box[1], bx1 = s_box[2] + 1, by1 = s_box[3] + 1;   // inclusive, with the right / lower taps
    const int lp = (bx1 - bx0 + 1 + 3) & ~3, rows = by1 - by0 + 1;                        // LDS row pitch in bytes
    const bool staged = s_box[2] >= 0 && lp * rows <= RECT_LDS_BYTES;                     // uniform
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(s_tile);
    const int f0 = blockIdx.z * group, f1 = min(f0 + group, n_frames);
    const int64_t drow = (int64_t)y * dst_pitch + x;
    const int ncol = min(4, dst_w - x);
    for (int f = f0; f < f1; f++) {
        const uint8_t* sf = src + (int64_t)f * src_stride;
        if (staged) {
            const int dpr = lp / 4;
            for (int i = tid; i < rows * dpr; i += RECT_BLOCK) {
                const int r = i / dpr, c = bx0 + 4 * (i % dpr);
                const uint8_t* p = sf + (int64_t)(by0 + r) * src_pitch + c;
                uint32_t v = 0;
                if (c + 3 < src_w) __builtin_memcpy(&v, p, 4);
                else
                    for (int b = 0; b < 4; b++)
                        if (c + b < src_w) v |= (uint32_t)p[b] << (8 * b);
                s_tile[i] = v;
            }
            __syncthreads();
        }
        if (live) {
            uint32_t px[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (staged) {
                    const int lo = (iy[k] - by0) * lp + (ix[k] - bx0);
                    const uint32_t a = t8[ok[k] ? lo : 0], b = t8[ok[k] ? lo + 1 : 0], c = t8[ok[k] ? lo + lp : 0], d = t8[ok[k] ? lo + lp + 1 : 0];
                    const uint32_t sum = a * (wt[k] & 0xFFFFu) + b * (wt[k] >> 16) + c * (wb[k] & 0xFFFFu) + d * (wb[k] >> 16);
                    px[k] = ok[k] ? (sum + 512u) >> 10 : fill;
                } else {
                    px[k] = rect_pixel(sf, off[k], src_pitch, wt[k], wb[k], ok[k], fill);
                }
            }
            uint8_t* d = dst + (int64_t)f * dst_stride + drow;
            if (ncol == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(d) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < ncol) d[k] = (uint8_t)px[k];
            }
        }
        if (staged) __syncthreads();                          // the tile is read before the next frame overwrites it
    }
}
#endif

// grid: (ceil(kp_stride / block), frames). In place (kp_out == kp_in) is allowed: a lane reads its record before it writes it.
__global__ __launch_bounds__(RECT_BLOCK) void k_rect_points(RectCam c, const RectKp* kp_in, const int* __restrict__ counts,
                                                            int64_t kp_stride, RectKp* kp_out, int* __restrict__ err) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * RECT_BLOCK + threadIdx.x;
    const int n = counts[f];
    if (n < 0 || n > kp_stride) {                        // uniform over the frame: it is skipped
        if (i == 0) atomicOr(err, ERRBIT_RECT_INPUT);
        return;
    }
    if (i >= n) return;
    RectKp k = kp_in[(int64_t)f * kp_stride + i];
    const double xd = ((double)k.x - c.cx) / c.fx, yd = ((double)k.y - c.cy) / c.fy;
    double x = xd, y = yd;
    for (int it = 0; it < RECT_POINT_ITERS; it++) {
        double rad, dx, dy;
        rect_terms(c, x, y, rad, dx, dy);
        x = (xd - dx) / rad;
        y = (yd - dy) / rad;
    }
    const double X = c.R[0] * x + c.R[1] * y + c.R[2];
    const double Y = c.R[3] * x + c.R[4] * y + c.R[5];
    const double Z = c.R[6] * x + c.R[7] * y + c.R[8];
    const float u = (float)(c.nfx * X / Z + c.ncx), v = (float)(c.nfy * Y / Z + c.ncy);
    const bool ok = Z > 0.0 && fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX;
    k.x = ok ? u : -1.0f;
    k.y = ok ? v : -1.0f;
    kp_out[(int64_t)f * kp_stride + i] = k;
}

// ---- the fisheye model KB4 (the header's steps 2k and 4k). A RectCam of a KB4 handle holds k1, k2, k3, k4 in the fields
// k1, k2, p1, p2 (dist[0..3] in both models) and 0 in k3. atan and tan are built from + - * / and sqrt with fixed loop counts,
// so every lane does the same work and the host computes the same bits.
constexpr int RECT_KB4_POINT_ITERS = 10;
constexpr double RECT_KB4_RESIDUAL = 1e-9;
constexpr double RECT_HALF_PI = 1.5707963267948966;

// atan(r), r >= 0: three half-angle steps, the Taylor series to t^25 in Horner form, times 8
__device__ __forceinline__ double rect_atan(double r) {
    double t = r;
    for (int i = 0; i < 3; i++) t = t / (1.0 + sqrt(1.0 + t * t));
    const double s = t * t;
    double p = 1.0 / 25.0;
    for (int k = 11; k >= 0; k--) p = 1.0 / (double)(2 * k + 1) - s * p;
    return 8.0 * (t * p);
}

// tan(a), 0 <= a < pi / 2: sin / cos of a / 8 by their Taylor series, three double-angle steps
__device__ __forceinline__ double rect_tan(double a) {
    const double h = a * 0.125, s = h * h;
    double ps = 1.0, pc = 1.0;
    for (int k = 8; k >= 1; k--) {
        ps = 1.0 - s / (double)((2 * k) * (2 * k + 1)) * ps;
        pc = 1.0 - s / (double)((2 * k - 1) * (2 * k)) * pc;
    }
    double t = (h * ps) / pc;
    for (int i = 0; i < 3; i++) t = (2.0 * t) / (1.0 - t * t);
    return t;
}

__device__ __forceinline__ double rect_kb4_P(const RectCam& c, double a) {
    const double q = a * a;
    return (((c.p2 * q + c.p1) * q + c.k2) * q + c.k1) * q + 1.0;
}

// d/da (a P(a)); <= 0 beyond the angle at which the polynomial folds back
__device__ __forceinline__ double rect_kb4_D(const RectCam& c, double a) {
    const double q = a * a;
    return (((9.0 * c.p2 * q + 7.0 * c.p1) * q + 5.0 * c.k2) * q + 3.0 * c.k1) * q + 1.0;
}

__global__ __launch_bounds__(RECT_BLOCK) void k_rect_build_map_kb4(RectCam c, int src_w, int src_h, int dst_w, int dst_h,
                                                                   int map_pitch, uint32_t* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * RECT_BLOCK + threadIdx.x;
    if (i >= (int64_t)map_pitch * dst_h) return;
    const int v = (int)(i / map_pitch), u = (int)(i % map_pitch);
    uint32_t word = RECT_INVALID;
    if (u < dst_w) {
        const double x = ((double)u - c.ncx) / c.nfx, y = ((double)v - c.ncy) / c.nfy;
        const double X = c.R[0] * x + c.R[3] * y + c.R[6];
        const double Y = c.R[1] * x + c.R[4] * y + c.R[7];
        const double Z = c.R[2] * x + c.R[5] * y + c.R[8];
        const double xn = X / Z, yn = Y / Z;
        const double r = sqrt(xn * xn + yn * yn);
        const double a = rect_atan(r);
        const double sc = r == 0.0 ? 1.0 : (a * rect_kb4_P(c, a)) / r;
        const double xd = xn * sc, yd = yn * sc;
        const double su = c.fx * xd + c.cx, sv = c.fy * yd + c.cy;
        const double qx = floor(su * 32.0 + 0.5), qy = floor(sv * 32.0 + 0.5);
        const bool ok = rect_kb4_D(c, a) > 0.0 && Z > 0.0 && rect_finite(su) && rect_finite(sv) && qx >= 0.0 && qy >= 0.0 &&
                        qx < (double)(src_w - 1) * 32.0 && qy < (double)(src_h - 1) * 32.0;
        if (ok) word = (uint32_t)(int)qx | ((uint32_t)(int)qy << 16);
    }
    map[i] = word;
}

// grid, deferred error and the in-place rule as k_rect_points
__global__ __launch_bounds__(RECT_BLOCK) void k_rect_points_kb4(RectCam c, const RectKp* kp_in, const int* __restrict__ counts,
                                                                int64_t kp_stride, RectKp* kp_out, int* __restrict__ err) {
    const int f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * RECT_BLOCK + threadIdx.x;
    const int n = counts[f];
    if (n < 0 || n > kp_stride) {                        // uniform over the frame: it is skipped
        if (i == 0) atomicOr(err, ERRBIT_RECT_INPUT);
        return;
    }
    if (i >= n) return;
    RectKp k = kp_in[(int64_t)f * kp_stride + i];
    const double xd = ((double)k.x - c.cx) / c.fx, yd = ((double)k.y - c.cy) / c.fy;
    const double td = sqrt(xd * xd + yd * yd);
    double a = td;
    for (int it = 0; it < RECT_KB4_POINT_ITERS; it++) a = a - (a * rect_kb4_P(c, a) - td) / rect_kb4_D(c, a);
    const bool conv = rect_finite(a) && a >= 0.0 && a < RECT_HALF_PI && rect_kb4_D(c, a) > 0.0 &&
                      fabs(a * rect_kb4_P(c, a) - td) <= RECT_KB4_RESIDUAL;
    const double sc = td == 0.0 ? 1.0 : rect_tan(a) / td;
    const double x = xd * sc, y = yd * sc;
    const double X = c.R[0] * x + c.R[1] * y + c.R[2];
    const double Y = c.R[3] * x + c.R[4] * y + c.R[5];
    const double Z = c.R[6] * x + c.R[7] * y + c.R[8];
    const float u = (float)(c.nfx * X / Z + c.ncx), v = (float)(c.nfy * Y / Z + c.ncy);
    const bool ok = conv && Z > 0.0 && fabsf(u) <= FLT_MAX && fabsf(v) <= FLT_MAX;
    k.x = ok ? u : -1.0f;
    k.y = ok ? v : -1.0f;
    kp_out[(int64_t)f * kp_stride + i] = k;
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
static_assert(sizeof(RectKp) == sizeof(aria_keypoint), "RectKp mirrors aria_keypoint");

struct aria_rect_s : StageHandle {
    aria_rect_config cfg{};
    RectCam cam[2]{};
    int map_pitch = 0;
    int group = RECT_GROUP;
    bool read_lds = false, read_taps = false;                  // variants build only
    DeviceBuffer<uint32_t> d_map;                              // n_cameras * map_pitch * dst_height
    // single-image staging of the blocking host forms (grow-only)
    DeviceBuffer<uint8_t> d_img;                               // source then destination
    DeviceBuffer<aria_keypoint> d_kp;
    DeviceBuffer<int> d_count;
};

namespace {

bool fin(double v) { return std::isfinite(v); }

bool bad_camera(const aria_rect_camera& c) {
    bool bad = bad_pinhole(c.fx, c.fy, c.cx, c.cy);
    for (double v : c.dist) bad |= !fin(v);
    for (double v : c.R) bad |= !fin(v);
    return bad;
}

bool bad_config(const aria_rect_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_rect_config)) return true;
    if (c->src_width < 2 || c->src_height < 2 || c->src_width > RECT_MAX_DIM || c->src_height > RECT_MAX_DIM || c->dst_width < 1 ||
        c->dst_height < 1 || c->dst_width > RECT_MAX_DIM || c->dst_height > RECT_MAX_DIM || c->n_cameras < 1 || c->n_cameras > 2 ||
        c->fill < 0 || c->fill > 255)
        return true;
    if (bad_pinhole(c->new_fx, c->new_fy, c->new_cx, c->new_cy)) return true;
    if (c->model != ARIA_RECT_MODEL_RADTAN && c->model != ARIA_RECT_MODEL_KB4) return true;
    for (int k = 0; k < c->n_cameras; k++)
        if (bad_camera(c->cam[k]) || (c->model == ARIA_RECT_MODEL_KB4 && c->cam[k].dist[4] != 0.0)) return true;
    return false;
}

RectCam make_cam(const aria_rect_config& c, int k) {
    const aria_rect_camera& a = c.cam[k];
    RectCam r{};
    r.fx = a.fx; r.fy = a.fy; r.cx = a.cx; r.cy = a.cy;
    r.k1 = a.dist[0]; r.k2 = a.dist[1]; r.p1 = a.dist[2]; r.p2 = a.dist[3]; r.k3 = a.dist[4];
    for (int i = 0; i < 9; i++) r.R[i] = a.R[i];
    r.nfx = c.new_fx; r.nfy = c.new_fy; r.ncx = c.new_cx; r.ncy = c.new_cy;
    return r;
}

void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace

extern "C" {

void aria_rect_default_config(aria_rect_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_rect_config);
    c->src_width = 752; c->src_height = 480; c->dst_width = 752; c->dst_height = 480;
    c->n_cameras = 1;
    for (int k = 0; k < 2; k++) {                                          // EuRoC cam0, plain undistortion
        aria_rect_camera& a = c->cam[k];
        a.fx = 458.654; a.fy = 457.296; a.cx = 367.215; a.cy = 248.375;
        a.dist[0] = -0.28340811; a.dist[1] = 0.07395907; a.dist[2] = 0.00019359; a.dist[3] = 1.76187114e-05; a.dist[4] = 0.0;
        a.R[0] = a.R[4] = a.R[8] = 1.0;
    }
    c->new_fx = 458.654; c->new_fy = 457.296; c->new_cx = 367.215; c->new_cy = 248.375;   // new K = K
    c->fill = 0;
}

int aria_rect_stereo_geometry(const double* K_l, const double* K_r, const double* T_BS_l, const double* T_BS_r, aria_rect_config* cfg,
                              double* baseline) {
    if (!K_l || !K_r || !T_BS_l || !T_BS_r || !cfg) return ARIA_E_INVALID;
    for (int k = 0; k < 4; k++)
        if (!fin(K_l[k]) || !fin(K_r[k])) return ARIA_E_INVALID;
    for (int k = 0; k < 16; k++)
        if (!fin(T_BS_l[k]) || !fin(T_BS_r[k])) return ARIA_E_INVALID;
    const double* A = T_BS_l;
    const double* B = T_BS_r;
    // inverse_rigid(T_BS_r) = [Rr^T | -(Rr^T tr)]
    double inv[3][4], R[3][3], t[3], c[3];
    for (int i = 0; i < 3; i++) {
        inv[i][0] = B[0 + i]; inv[i][1] = B[4 + i]; inv[i][2] = B[8 + i];
        inv[i][3] = -(B[0 + i] * B[3] + B[4 + i] * B[7] + B[8 + i] * B[11]);
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = inv[i][0] * A[j] + inv[i][1] * A[4 + j] + inv[i][2] * A[8 + j];
        t[i] = inv[i][0] * A[3] + inv[i][1] * A[7] + inv[i][2] * A[11] + inv[i][3];
    }
    {   // sensor.yaml's 12 digits leave R orthonormal to 1e-12 only: Gram-Schmidt on its rows
        const double n0 = std::sqrt(R[0][0] * R[0][0] + R[0][1] * R[0][1] + R[0][2] * R[0][2]);
        if (!(n0 > 0) || !fin(n0)) return ARIA_E_INVALID;
        const double r0[3] = {R[0][0] / n0, R[0][1] / n0, R[0][2] / n0};
        const double d = r0[0] * R[1][0] + r0[1] * R[1][1] + r0[2] * R[1][2];
        double r1[3] = {R[1][0] - d * r0[0], R[1][1] - d * r0[1], R[1][2] - d * r0[2]}, r2[3];
        const double n1 = std::sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
        if (!(n1 > 0) || !fin(n1)) return ARIA_E_INVALID;
        r1[0] = r1[0] / n1; r1[1] = r1[1] / n1; r1[2] = r1[2] / n1;
        cross3(r0, r1, r2);
        for (int j = 0; j < 3; j++) { R[0][j] = r0[j]; R[1][j] = r1[j]; R[2][j] = r2[j]; }
    }
    for (int i = 0; i < 3; i++) c[i] = -(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]);
    const double bl = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (!(bl > 0) || !fin(bl)) return ARIA_E_INVALID;
    double ex[3] = {c[0] / bl, c[1] / bl, c[2] / bl}, ey[3], ez[3];
    const double w[3] = {R[2][0], R[2][1], 1.0 + R[2][2]};                  // z + R^T z
    cross3(w, ex, ey);
    const double n = std::sqrt(ey[0] * ey[0] + ey[1] * ey[1] + ey[2] * ey[2]);
    if (!(n > 0) || !fin(n)) return ARIA_E_INVALID;
    ey[0] = ey[0] / n; ey[1] = ey[1] / n; ey[2] = ey[2] / n;
    cross3(ex, ey, ez);
    const double* R1[3] = {ex, ey, ez};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            cfg->cam[0].R[3 * i + j] = R1[i][j];
            cfg->cam[1].R[3 * i + j] = R1[i][0] * R[j][0] + R1[i][1] * R[j][1] + R1[i][2] * R[j][2];
        }
    const double f = (K_l[1] + K_r[1]) / 2.0;
    if (cfg->new_fx == 0.0) cfg->new_fx = f;
    if (cfg->new_fy == 0.0) cfg->new_fy = f;
    if (cfg->new_cx == 0.0) cfg->new_cx = (K_l[2] + K_r[2]) / 2.0;
    if (cfg->new_cy == 0.0) cfg->new_cy = (K_l[3] + K_r[3]) / 2.0;
    if (baseline) *baseline = bl;
    return ARIA_OK;
}

int aria_rect_create(const aria_rect_config* c, aria_rect_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_rect_create", [](aria_rect_s* h) {
        const aria_rect_config& c = h->cfg;
        const char* what = "aria_rect_create";
        h->map_pitch = (c.dst_width + 3) & ~3;
        if (const char* g = aria_getenv("ARIA_RECT_GROUP")) h->group = std::min(std::max(std::atoi(g), 1), 64);   // variants build: A/B
        if (const char* r = aria_getenv("ARIA_RECT_READ")) {
            h->read_lds = !std::strcmp(r, "lds");
            h->read_taps = !std::strcmp(r, "taps");
        }
        for (int k = 0; k < c.n_cameras; k++) h->cam[k] = make_cam(c, k);
        const size_t words = (size_t)h->map_pitch * c.dst_height;
        int rc;
        if ((rc = h->d_map.reserve(h->stream, words * c.n_cameras, what)) != ARIA_OK) return rc;
        if ((rc = h->d_count.reserve(h->stream, 1, what)) != ARIA_OK) return rc;
        const auto build = c.model == ARIA_RECT_MODEL_KB4 ? k_rect_build_map_kb4 : k_rect_build_map;
        for (int k = 0; k < c.n_cameras; k++)
            hipLaunchKernelGGL(build, dim3((unsigned)((words + RECT_BLOCK - 1) / RECT_BLOCK)), dim3(RECT_BLOCK), 0, h->stream,
                               h->cam[k], c.src_width, c.src_height, c.dst_width, c.dst_height, h->map_pitch, h->d_map + k * words);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        return e == hipSuccess ? (int)ARIA_OK : hip_fail(e, what, __FILE__, __LINE__);
    });
}

void aria_rect_destroy(aria_rect_t h) { stage_destroy(h); }

void* aria_rect_stream(aria_rect_t h) { return stage_stream(h); }

int aria_rect_check(aria_rect_t h) { return stage_check(h, {{ERRBIT_RECT_INPUT, ARIA_E_INVALID}}); }

int aria_rect_remap_batch_device(aria_rect_t h, int cam, const uint8_t* d_src, int64_t src_stride, int src_pitch, int n_frames,
                                 uint8_t* d_dst, int64_t dst_stride, int dst_pitch) {
    if (!h || cam < 0 || cam >= h->cfg.n_cameras || !d_src || !d_dst || n_frames < 0) return ARIA_E_INVALID;
    const aria_rect_config& c = h->cfg;
    if (src_pitch < c.src_width || src_pitch > RECT_MAX_PITCH || dst_pitch < c.dst_width ||
        (n_frames > 1 && (src_stride < (int64_t)src_pitch * (c.src_height - 1) + c.src_width ||
                          dst_stride < (int64_t)dst_pitch * (c.dst_height - 1) + c.dst_width)))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const int groups = (n_frames + h->group - 1) / h->group;
    if (groups > 65535) return ARIA_E_INVALID;
    const dim3 grid((c.dst_width + RECT_TILE_W - 1) / RECT_TILE_W, (c.dst_height + RECT_TILE_H - 1) / RECT_TILE_H, groups);
    const uint32_t* d_map = h->d_map + (size_t)cam * h->map_pitch * c.dst_height;
#ifdef ARIA_VARIANTS
    if (h->read_lds)
        hipLaunchKernelGGL(k_rect_remap_lds, grid, dim3(RECT_BLOCK), 0, h->stream, d_map, h->map_pitch, c.dst_width, c.dst_height, d_src,
                           src_stride, src_pitch, c.src_width, n_frames, h->group, d_dst, dst_stride, dst_pitch, (uint32_t)c.fill);
    else
#endif
    hipLaunchKernelGGL(k_rect_remap, grid, dim3(RECT_BLOCK), 0, h->stream, d_map, h->map_pitch, c.dst_width, c.dst_height, d_src,
                       src_stride, src_pitch, c.src_width, c.src_height, h->read_taps ? 0 : 1, n_frames, h->group, d_dst, dst_stride,
                       dst_pitch, (uint32_t)c.fill);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_rect_remap(aria_rect_t h, int cam, const uint8_t* src, int src_pitch, uint8_t* dst, int dst_pitch) {
    if (!h || cam < 0 || cam >= h->cfg.n_cameras || !src || !dst || src_pitch < h->cfg.src_width || src_pitch > RECT_MAX_PITCH ||
        dst_pitch < h->cfg.dst_width)
        return ARIA_E_INVALID;
    const aria_rect_config& c = h->cfg;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t ns = (size_t)c.src_width * c.src_height, nd = (size_t)c.dst_width * c.dst_height;
    int rc;
    if ((rc = h->d_img.reserve(h->stream, ns + nd)) != ARIA_OK) return rc;
    uint8_t* d_dst = h->d_img + ns;
    ARIA_HIP(hipMemcpy2DAsync(h->d_img, (size_t)c.src_width, src, (size_t)src_pitch, (size_t)c.src_width, (size_t)c.src_height,
                              hipMemcpyHostToDevice, h->stream));
    if ((rc = aria_rect_remap_batch_device(h, cam, h->d_img, 0, c.src_width, 1, d_dst, 0, c.dst_width)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpy2DAsync(dst, (size_t)dst_pitch, d_dst, (size_t)c.dst_width, (size_t)c.dst_width, (size_t)c.dst_height,
                              hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return ARIA_OK;
}

int aria_rect_points_batch_device(aria_rect_t h, int cam, const aria_keypoint* d_kp_in, const int* d_n, int64_t kp_stride,
                                  int n_frames, aria_keypoint* d_kp_out) {
    if (!h || cam < 0 || cam >= h->cfg.n_cameras || !d_kp_in || !d_n || !d_kp_out || n_frames < 0 || n_frames > 65535 ||
        kp_stride < 1 || kp_stride > (int64_t)1 << 30)
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(h->cfg.model == ARIA_RECT_MODEL_KB4 ? k_rect_points_kb4 : k_rect_points, dim3((unsigned)((kp_stride + RECT_BLOCK - 1) / RECT_BLOCK), n_frames), dim3(RECT_BLOCK), 0,
                       h->stream, h->cam[cam], reinterpret_cast<const RectKp*>(d_kp_in), d_n, kp_stride,
                       reinterpret_cast<RectKp*>(d_kp_out), h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_rect_points(aria_rect_t h, int cam, const aria_keypoint* kp_in, int n, aria_keypoint* kp_out) {
    if (!h || cam < 0 || cam >= h->cfg.n_cameras || n < 0 || (n && (!kp_in || !kp_out))) return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_kp.reserve(h->stream, (size_t)n)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(h->d_kp, kp_in, sizeof(aria_keypoint) * n, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_count, &n, sizeof(int), hipMemcpyHostToDevice));
    if ((rc = aria_rect_points_batch_device(h, cam, h->d_kp, h->d_count, (int64_t)h->d_kp.cap, 1, h->d_kp)) != ARIA_OK) return rc;
    ARIA_HIP(memcpy_on(h->stream, kp_out, h->d_kp, sizeof(aria_keypoint) * n, hipMemcpyDeviceToHost));
    return aria_rect_check(h);
}

int aria_rect_get_map(aria_rect_t h, int cam, uint32_t* out, int cap) {
    if (!h || cam < 0 || cam >= h->cfg.n_cameras || !out) return ARIA_E_INVALID;
    const aria_rect_config& c = h->cfg;
    const int n = c.dst_width * c.dst_height;
    if (cap < n) return ARIA_E_OUTPUT_TOO_SMALL;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(hipMemcpy2DAsync(out, (size_t)c.dst_width * 4, h->d_map + (size_t)cam * h->map_pitch * c.dst_height,
                              (size_t)h->map_pitch * 4, (size_t)c.dst_width * 4, (size_t)c.dst_height, hipMemcpyDeviceToHost,
                              h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return n;
}

int64_t aria_rect_algorithmic_bytes(int dst_w, int dst_h) { return 2 * (int64_t)dst_w * dst_h; }

}  // extern "C"
