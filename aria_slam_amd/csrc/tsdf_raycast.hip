// Ray casting of the volume: a ray per pixel marched through the aria_tsdf_voxel records of the dense depth fusion, the zero
// crossing refined on the trilinear interpolant and that interpolant differentiated: predicted depth maps, normals, gray and
// a head-light shade for a batch of views. Semantics in include/aria_orb_hip.h ("ray casting of the volume");
// aria_slam_amd/ray_ref.py is the definition and this file equals it bit for bit. The stage owns no volume.
//
// k_ray_prepare   a lane per view: the 12 doubles of [R|t] to fp32, the camera centre in grid units, the view mask, the
//                 non-finite check (deferred-error OR), the view record's start values. One 64-byte record per view.
// k_ray_bricks    a lane per run of 8 voxels along x (64 contiguous bytes): a run that holds a voxel with weight >= min_weight &&
//                 tsdf < 0 stores a 1 into its brick's byte; every writer writes the same value, so there is no atomic.
// k_ray_brick_words  a lane per word: 32 brick bytes packed into bits. One bit per 8 x 8 x 8 voxels: 2 KiB at the default volume.
// k_ray_march     the hot path. A lane owns one pixel, a 64-lane wave an 8 x 8 pixel tile and a 256-lane workgroup 16 x 16
//                 pixels of one view: neighbouring rays walk neighbouring voxels, so the 8-byte record gathers of a wave share
//                 lines. The view record is read at a workgroup-uniform address (scalar loads). The lane clips its k range to
//                 the volume's box (ray_clip, conservative; the restatement does not clip, so bitwise parity on grazing views
//                 is the check), walks it, and loads a record only where the sample's brick has its bit set (skip = 1): only a
//                 seen negative voxel can end a walk. At the ending sample it fetches sample k - 1 for rule 5, and rules 6-10
//                 run once, after the loop. No LDS, no barrier, no float atomics, no scratch.
// k_ray_finish    a lane per view: nearest = 0.0f where the view had no hit.
// Plain HIP C++. The text from "namespace {" to the C-ABI section also compiles for the host
// (tests/test_ray_kernel_emulation.py); the one cross-lane step, the view record's tally, sits above it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_tsdf_voxel) == 8, "aria_tsdf_voxel is 8 bytes");
static_assert(sizeof(aria_ray_view) == 16, "aria_ray_view is 16 bytes");
static_assert(sizeof(aria_ray_config) == 96, "aria_ray_config is 96 bytes");

// Rule 11 for one wave: the counts by ballot, the minimum of the hit depths' bit patterns (positive floats order like their
// bits) by a butterfly, then one integer atomic each from lane 0. Every lane of the wave calls it. The host emulation
// replaces it by its lane-serial form.
__device__ __forceinline__ void ray_tally(aria_ray_view* rec, bool ended, bool hit, float depth) {
    const unsigned long long me = __ballot(ended), mh = __ballot(hit);
    uint32_t bits = hit ? __float_as_uint(depth) : 0xFFFFFFFFu;
    for (int d = 32; d; d >>= 1) bits = min(bits, (uint32_t)__shfl_xor((int)bits, d, 64));
    if ((threadIdx.x & 63) != 0) return;
    if (me) atomicAdd(&rec->n_ended, (int)__popcll(me));
    if (mh) {
        atomicAdd(&rec->n_hit, (int)__popcll(mh));
        atomicMin(reinterpret_cast<uint32_t*>(&rec->nearest), bits);
    }
}

namespace {

constexpr int RAY_BLOCK = 256;
constexpr int RAY_TILE = 16;                                        // pixels of a workgroup per axis; a wave is one 8 x 8 tile
constexpr int RAY_MAX_DIM = 1024, RAY_MAX_IMAGE = 16384, RAY_MAX_VIEWS = 65535, RAY_MAX_STEPS = 8192;
constexpr int ERRBIT_RAY_INPUT = 1;
constexpr uint32_t RAY_NO_HIT_BITS = 0x7F800000u;                   // +Inf: above every hit depth

// What the kernels take by value: the config in fp32.
struct RayParams {
    int nx, ny, nz, min_weight;
    int bx, by, n_steps, skip;      // bricks along x and y
    float inv_voxel, ox, oy, oz;
    float near_z, step, inv_step, kmargin;
    float cx, cy, inv_fx, inv_fy;
    float hx, hy, hz;               // (float)(n - 1)
};

// Host side, inside the text the host emulation compiles, so that it runs on the constants the library uses. n_steps is
// (int)floorf((far - near) / step) + 1, or 0 when that is not in 1..RAY_MAX_STEPS.
inline RayParams ray_params(const int n[3], int min_weight, int skip, float voxel, const float origin[3], float near_z, float far_z,
                            float step, const double K[4]) {
    RayParams P{};
    P.nx = n[0]; P.ny = n[1]; P.nz = n[2]; P.min_weight = min_weight;
    P.bx = n[0] / 8; P.by = n[1] / 8; P.skip = skip;
    P.inv_voxel = 1.0f / voxel; P.ox = origin[0]; P.oy = origin[1]; P.oz = origin[2];
    P.near_z = near_z; P.step = step; P.inv_step = 1.0f / step;
    const float q = std::floor((far_z - near_z) / step);
    P.n_steps = q >= 0.0f && q <= (float)(RAY_MAX_STEPS - 1) ? (int)q + 1 : 0;
    // ray_clip: one sample, plus 1e-3 of the largest z in steps: four orders of magnitude above the fp32 rounding of z_k
    P.kmargin = 1.0f + 1e-3f * ((std::fabs(near_z) + std::fabs(far_z)) / step);
    P.cx = (float)K[2]; P.cy = (float)K[3]; P.inv_fx = 1.0f / (float)K[0]; P.inv_fy = 1.0f / (float)K[1];
    P.hx = (float)(n[0] - 1); P.hy = (float)(n[1] - 1); P.hz = (float)(n[2] - 1);
    return P;
}

// One view as the march reads it: 16 words at a workgroup-uniform address.
struct RayView {
    float r[9], og[3];
    int state;                      // 0: masked out; 1: cast; 2: a non-finite extrinsic, zeros are written
    int pad[3];
};

__device__ __forceinline__ bool ray_finite(double v) { return fabs(v) <= DBL_MAX; }

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_prepare(RayParams P, const double* __restrict__ ext, const uint8_t* __restrict__ mask,
                                                           int n_views, RayView* __restrict__ views, aria_ray_view* __restrict__ recs,
                                                           int* err) {
    const int f = (int)(blockIdx.x * RAY_BLOCK + threadIdx.x);
    if (f >= n_views) return;
    const double* e = ext + 12 * (int64_t)f;
    const bool wanted = !mask || mask[f] != 0;
    bool fin = true;
    for (int k = 0; k < 12; k++) fin = fin && ray_finite(e[k]);
    if (wanted && !fin) atomicOr(err, ERRBIT_RAY_INPUT);
    RayView V;
    float t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) V.r[3 * r + c] = (float)e[4 * r + c];
        t[r] = (float)e[4 * r + 3];
    }
    const float origin[3] = {P.ox, P.oy, P.oz};
    for (int a = 0; a < 3; a++) {
        const float o = -((V.r[a] * t[0] + V.r[3 + a] * t[1]) + V.r[6 + a] * t[2]);
        V.og[a] = (o - origin[a]) * P.inv_voxel - 0.5f;
    }
    V.state = !wanted ? 0 : fin ? 1 : 2;
    V.pad[0] = V.pad[1] = V.pad[2] = 0;
    views[f] = V;
    if (recs && wanted) {
        aria_ray_view rec;
        rec.n_hit = 0; rec.n_ended = 0;
        rec.nearest = fin ? __uint_as_float(RAY_NO_HIT_BITS) : 0.0f;
        rec.valid = fin ? 1 : 0;
        recs[f] = rec;
    }
}

__device__ __forceinline__ float ray_tsdf(unsigned long long rec) { return __uint_as_float((uint32_t)rec); }
__device__ __forceinline__ uint32_t ray_weight(unsigned long long rec) { return (uint32_t)(rec >> 32) & 0xFFFFu; }
__device__ __forceinline__ uint32_t ray_gray(unsigned long long rec) { return (uint32_t)(rec >> 48) & 0xFFu; }

// grid: ceil(n_vox / 8 / 256). A lane reads one run of 8 voxels along x, one row of one brick (64 contiguous bytes, the wave 4 KiB),
// and where the run holds a voxel that can end a walk it stores a 1 into its brick's byte. Every writer of a byte writes the
// same value, so no atomic is needed. flags: zeroed before the launch.
__global__ __launch_bounds__(RAY_BLOCK) void k_ray_bricks(RayParams P, const unsigned long long* __restrict__ vol, uint8_t* __restrict__ flags) {
    const uint32_t run = (uint32_t)(blockIdx.x * RAY_BLOCK + threadIdx.x), bx = (uint32_t)P.bx;      // at most 2^27 runs
    if (run >= bx * (uint32_t)P.ny * (uint32_t)P.nz) return;
    const uint32_t row = run / bx, ib = run - row * bx, k = row / (uint32_t)P.ny, j = row - k * (uint32_t)P.ny;
    bool any = false;
    for (int q = 0; q < 8; q++) {
        const unsigned long long rec = vol[(size_t)run * 8 + q];
        any |= ray_weight(rec) >= (uint32_t)P.min_weight && ray_tsdf(rec) < 0.0f;
    }
    if (any) flags[((k >> 3) * (uint32_t)P.by + (j >> 3)) * bx + ib] = 1;
}

// grid: ceil(n_words / 256). A lane packs 32 brick bytes into one word: bit b of word w is brick 32 w + b.
__global__ __launch_bounds__(RAY_BLOCK) void k_ray_brick_words(int n_bricks, const uint8_t* __restrict__ flags, uint32_t* __restrict__ words) {
    const int w = (int)(blockIdx.x * RAY_BLOCK + threadIdx.x);
    if (32 * w >= n_bricks) return;
    uint32_t bits = 0;
    for (int b = 0; b < 32 && 32 * w + b < n_bricks; b++) bits |= flags[32 * w + b] ? 1u << b : 0u;
    words[w] = bits;
}

// The samples k0 .. k1 outside which the ray cannot be inside the volume (k1 < k0: none). Conservative:
//   A sample is inside only when rintf(g_a) lies in [0, n_a - 1], so g_a, as computed, lies in [-0.5, n_a - 0.5]. The computed
//   g_a differs from the exact og_a + z dg_a at the computed z_k by the rounding of one product and one sum of terms no larger
//   than |og_a| + n_a there: the box is widened by m_a = 1e-3 (|og_a| + n_a), four orders of magnitude above that rounding,
//   which also covers the rounding of the two slab quotients below (each relative 2^-23 of a z whose g_a is on the box).
//   The z range of the widened box maps to k by (z - near) / step, where the computed z_k is within two roundings of
//   near + k step: kmargin holds one sample plus 1e-3 of (near + far) / step, and the bounds are rounded outward. An axis the ray does not move along (dg_a == 0)
//   excludes everything when og_a is outside its widened slab. A NaN, an overflow or an infinity makes a comparison false and
//   leaves its bound where it was: no clip.
__device__ __forceinline__ void ray_clip(const RayParams& P, const RayView& V, float dgx, float dgy, float dgz, int& k0, int& k1) {
    const float og[3] = {V.og[0], V.og[1], V.og[2]}, dg[3] = {dgx, dgy, dgz}, n[3] = {(float)P.nx, (float)P.ny, (float)P.nz};
    float zlo = -FLT_MAX, zhi = FLT_MAX;
    bool none = false;
    for (int a = 0; a < 3; a++) {
        const float m = 1e-3f * (fabsf(og[a]) + n[a]);
        const float lo = -0.5f - m, hi = (n[a] - 0.5f) + m;
        if (dg[a] != 0.0f) {
            const float z1 = (lo - og[a]) / dg[a], z2 = (hi - og[a]) / dg[a];
            const float zn = fminf(z1, z2), zf = fmaxf(z1, z2);       // fminf / fmaxf drop a NaN operand
            if (zn > zlo) zlo = zn;
            if (zf < zhi) zhi = zf;
        } else if (og[a] < lo || og[a] > hi) {
            none = true;
        }
    }
    const float a = floorf((zlo - P.near_z) * P.inv_step - P.kmargin), b = ceilf((zhi - P.near_z) * P.inv_step + P.kmargin);
    const float last = (float)(P.n_steps - 1);
    k0 = a > 0.0f ? (a <= last ? (int)a : P.n_steps) : 0;
    k1 = b < last ? (b >= 0.0f ? (int)b : -1) : P.n_steps - 1;
    if (none) k1 = -1;
}

// Rule 4: the voxel of sample z, false when it is outside.
__device__ __forceinline__ bool ray_voxel(const RayParams& P, const RayView& V, float dgx, float dgy, float dgz, float z, int& ix, int& iy,
                                          int& iz) {
    const float rx = rintf(V.og[0] + z * dgx), ry = rintf(V.og[1] + z * dgy), rz = rintf(V.og[2] + z * dgz);
    if (!(rx >= 0.0f && rx <= P.hx && ry >= 0.0f && ry <= P.hy && rz >= 0.0f && rz <= P.hz)) return false;
    ix = (int)rx; iy = (int)ry; iz = (int)rz;
    return true;
}

__device__ __forceinline__ size_t ray_index(const RayParams& P, int ix, int iy, int iz) {
    return ((size_t)iz * (size_t)P.ny + (size_t)iy) * (size_t)P.nx + (size_t)ix;
}

__device__ __forceinline__ float ray_lerp(float a, float b, float w) { return a + w * (b - a); }

// Rule 6: the cell at sample z, t[x + 2y + 4z]. False when it is not defined.
struct RayCell {
    float t[8], fx, fy, fz;
};
__device__ __forceinline__ bool ray_cell(const RayParams& P, const RayView& V, const unsigned long long* __restrict__ vol, float dgx,
                                         float dgy, float dgz, float z, RayCell& c) {
    const float gx = V.og[0] + z * dgx, gy = V.og[1] + z * dgy, gz = V.og[2] + z * dgz;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    c.fx = gx - bx; c.fy = gy - by; c.fz = gz - bz;
    if (!(bx >= 0.0f && bx + 1.0f <= P.hx && by >= 0.0f && by + 1.0f <= P.hy && bz >= 0.0f && bz + 1.0f <= P.hz)) return false;
    const size_t base = ray_index(P, (int)bx, (int)by, (int)bz), sy = (size_t)P.nx, sz = (size_t)P.nx * (size_t)P.ny;
    bool ok = true;
    for (int n = 0; n < 8; n++) {
        const unsigned long long rec = vol[base + (n & 1) + ((n >> 1) & 1) * sy + (n >> 2) * sz];
        ok = ok && ray_weight(rec) >= (uint32_t)P.min_weight;
        c.t[n] = ray_tsdf(rec);
    }
    return ok;
}

// c00, c10, c01, c11, c0, c1 of rule 6 into q[0..5]; returns T.
__device__ __forceinline__ float ray_interp(const RayCell& c, float q[6]) {
    q[0] = ray_lerp(c.t[0], c.t[1], c.fx); q[1] = ray_lerp(c.t[2], c.t[3], c.fx);
    q[2] = ray_lerp(c.t[4], c.t[5], c.fx); q[3] = ray_lerp(c.t[6], c.t[7], c.fx);
    q[4] = ray_lerp(q[0], q[1], c.fy); q[5] = ray_lerp(q[2], q[3], c.fy);
    return ray_lerp(q[4], q[5], c.fz);
}

// What a pixel's walk leaves behind.
struct RayPixel {
    float depth, nx, ny, nz;
    uint32_t gray, shade;
    bool ended, hit;
};

// Rules 3-10 for pixel (u, v).
__device__ __forceinline__ RayPixel ray_trace(const RayParams& P, const RayView& V, const unsigned long long* __restrict__ vol,
                                              const uint32_t* __restrict__ words, int u, int v) {
    RayPixel px{};
    const float pa = ((float)u - P.cx) * P.inv_fx, pb = ((float)v - P.cy) * P.inv_fy;
    const float dx = (V.r[0] * pa + V.r[3] * pb) + V.r[6];
    const float dy = (V.r[1] * pa + V.r[4] * pb) + V.r[7];
    const float dz = (V.r[2] * pa + V.r[5] * pb) + V.r[8];
    const float dgx = dx * P.inv_voxel, dgy = dy * P.inv_voxel, dgz = dz * P.inv_voxel;
    int k0, k1;
    ray_clip(P, V, dgx, dgy, dgz, k0, k1);

    // rule 5: the walk. Nothing but k and the ray lives across an iteration.
    int kend = -1;
    unsigned long long recB = 0;
    for (int k = k0; k <= k1; k++) {
        int ix, iy, iz;
        if (!ray_voxel(P, V, dgx, dgy, dgz, P.near_z + (float)k * P.step, ix, iy, iz)) continue;
        if (P.skip) {
            const uint32_t brick = (uint32_t)(((iz >> 3) * P.by + (iy >> 3)) * P.bx + (ix >> 3));
            if (!((words[brick >> 5] >> (brick & 31u)) & 1u)) continue;
        }
        const unsigned long long rec = vol[ray_index(P, ix, iy, iz)];
        if (ray_weight(rec) >= (uint32_t)P.min_weight && ray_tsdf(rec) < 0.0f) {
            kend = k;
            recB = rec;
            break;
        }
    }
    if (kend < 0) return px;
    px.ended = true;
    if (kend < 1) return px;
    const float z0 = P.near_z + (float)(kend - 1) * P.step, z1 = P.near_z + (float)kend * P.step;
    int ix, iy, iz;
    if (!ray_voxel(P, V, dgx, dgy, dgz, z0, ix, iy, iz)) return px;
    const unsigned long long recA = vol[ray_index(P, ix, iy, iz)];       // sample k - 1 again: the walk kept nothing of it
    if (!(ray_weight(recA) >= (uint32_t)P.min_weight && ray_tsdf(recA) >= 0.0f)) return px;
    px.hit = true;

    // rule 7
    RayCell c{};
    float q[6];
    float A = ray_tsdf(recA), B = ray_tsdf(recB);
    const bool ok0 = ray_cell(P, V, vol, dgx, dgy, dgz, z0, c);
    const float F0 = ray_interp(c, q);
    const bool ok1 = ray_cell(P, V, vol, dgx, dgy, dgz, z1, c);
    const float F1 = ray_interp(c, q);
    if (ok0 && ok1 && F0 >= 0.0f && F1 <= 0.0f && F0 > F1) {
        A = F0;
        B = F1;
    }
    const float alpha = A / (A - B);
    px.depth = z0 + alpha * P.step;
    px.gray = alpha < 0.5f ? ray_gray(recA) : ray_gray(recB);           // rule 8

    // rules 9 and 10
    if (!ray_cell(P, V, vol, dgx, dgy, dgz, px.depth, c)) return px;
    ray_interp(c, q);
    const float Gx = ray_lerp(ray_lerp(c.t[1] - c.t[0], c.t[3] - c.t[2], c.fy), ray_lerp(c.t[5] - c.t[4], c.t[7] - c.t[6], c.fy), c.fz);
    const float Gy = ray_lerp(q[1] - q[0], q[3] - q[2], c.fz);
    const float Gz = q[5] - q[4];
    const float len = sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz);
    if (!(len > 0.0f)) return px;
    px.nx = Gx / len; px.ny = Gy / len; px.nz = Gz / len;
    const float dl = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float cs = fabsf((px.nx * dx + px.ny * dy) + px.nz * dz) / dl;
    px.shade = (uint32_t)(int)rintf(fminf(255.0f, 255.0f * cs));
    return px;
}

// grid: (ceil(W / 16), ceil(H / 16), views). Each plane: view f at + f * stride, row v at + v * pitch; null = not written.
__global__ __launch_bounds__(RAY_BLOCK) void k_ray_march(RayParams P, const RayView* __restrict__ views,
                                                         const unsigned long long* __restrict__ vol, const uint32_t* __restrict__ words,
                                                         int W, int H, float* __restrict__ depth, int64_t depth_stride, int depth_pitch,
                                                         float* __restrict__ normal, int64_t normal_stride, int normal_pitch,
                                                         uint8_t* __restrict__ gray, int64_t gray_stride, int gray_pitch,
                                                         uint8_t* __restrict__ shade, int64_t shade_stride, int shade_pitch,
                                                         aria_ray_view* __restrict__ recs) {
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    const int u = (int)blockIdx.x * RAY_TILE + (wave & 1) * 8 + (lane & 7);
    const int v = (int)blockIdx.y * RAY_TILE + (wave >> 1) * 8 + (lane >> 3);
    const int64_t f = (int64_t)blockIdx.z;
    const RayView& V = views[f];                                      // workgroup-uniform
    if (V.state == 0) return;
    const bool in_image = u < W && v < H;
    RayPixel px{};
    if (in_image && V.state == 1) px = ray_trace(P, V, vol, words, u, v);
    if (in_image) {
        if (depth) depth[f * depth_stride + (int64_t)v * depth_pitch + u] = px.depth;
        if (normal) {
            float* n = normal + f * normal_stride + 3 * ((int64_t)v * normal_pitch + u);
            n[0] = px.nx; n[1] = px.ny; n[2] = px.nz;
        }
        if (gray) gray[f * gray_stride + (int64_t)v * gray_pitch + u] = (uint8_t)px.gray;
        if (shade) shade[f * shade_stride + (int64_t)v * shade_pitch + u] = (uint8_t)px.shade;
    }
    if (recs && V.state == 1) ray_tally(recs + f, px.ended, px.hit, px.depth);
}

__global__ __launch_bounds__(RAY_BLOCK) void k_ray_finish(const RayView* __restrict__ views, int n_views, aria_ray_view* __restrict__ recs) {
    const int f = (int)(blockIdx.x * RAY_BLOCK + threadIdx.x);
    if (f >= n_views || views[f].state != 1) return;
    if (recs[f].n_hit == 0) recs[f].nearest = 0.0f;
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_ray_s : StageHandle {
    aria_ray_config cfg{};
    RayParams P{};
    size_t n_vox = 0, n_words = 0;
    const unsigned long long* d_vol = nullptr;                 // the caller's records, remembered by update
    DeviceBuffer<uint32_t> d_words;                            // the skip bits
    DeviceBuffer<uint8_t> d_flags;                             // a byte per brick, packed into d_words by update
    int n_bricks = 0;
    DeviceBuffer<RayView> d_views;
    // host-form staging (grow-only)
    DeviceBuffer<float> d_depth, d_normal;
    DeviceBuffer<uint8_t> d_gray, d_shade;
    DeviceBuffer<double> d_ext;                                // 12 doubles
    DeviceBuffer<aria_ray_view> d_rec;
};

namespace {

bool ray_bad_config(const aria_ray_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_ray_config)) return true;
    for (int n : {c->nx, c->ny, c->nz})
        if (n < 8 || n > RAY_MAX_DIM || n % 8) return true;
    if (!(c->voxel > 0) || !std::isfinite(c->voxel)) return true;
    for (float v : c->origin)
        if (!std::isfinite(v)) return true;
    if (c->min_weight < 1 || c->min_weight > 65535 || (c->skip != 0 && c->skip != 1)) return true;
    if (!std::isfinite(c->near) || !std::isfinite(c->far) || !std::isfinite(c->step)) return true;
    if (!(c->near > 0) || !(c->far >= c->near) || !(c->step > 0)) return true;
    return !std::isfinite(c->fx) || !std::isfinite(c->fy) || !std::isfinite(c->cx) || !std::isfinite(c->cy);
}

RayParams ray_make_params(const aria_ray_config& c) {
    const int n[3] = {c.nx, c.ny, c.nz};
    const double K[4] = {c.fx, c.fy, c.cx, c.cy};
    return ray_params(n, c.min_weight, c.skip, c.voxel, c.origin, c.near, c.far, c.step, K);
}

bool ray_bad_plane(const void* p, int64_t stride, int pitch, int width, int height, int n_views, int per_pixel) {
    if (!p) return false;
    return pitch < width || (n_views > 1 && stride < per_pixel * ((int64_t)pitch * (height - 1) + width));
}

}  // namespace

extern "C" {

void aria_ray_default_config(aria_ray_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_ray_config);
    c->nx = 256; c->ny = 256; c->nz = 128;
    c->min_weight = 2; c->skip = 1;
    c->voxel = 0.05f;
    c->origin[0] = -6.4f; c->origin[1] = -6.4f; c->origin[2] = 0.0f;
    c->near = 0.3f; c->far = 10.0f; c->step = 0.05f;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0
}

int64_t aria_ray_algorithmic_bytes(int width, int height, int n_views, int planes) {
    if (width < 1 || height < 1 || width > RAY_MAX_IMAGE || height > RAY_MAX_IMAGE || n_views < 0 || n_views > RAY_MAX_VIEWS || planes < 0 ||
        planes > 15)
        return ARIA_E_INVALID;
    const int64_t per = ((planes & ARIA_RAY_DEPTH) ? 4 : 0) + ((planes & ARIA_RAY_NORMAL) ? 12 : 0) + ((planes & ARIA_RAY_GRAY) ? 1 : 0) +
                        ((planes & ARIA_RAY_SHADE) ? 1 : 0);
    return (per * width * height + (int64_t)sizeof(aria_ray_view)) * n_views;
}

int aria_ray_create(const aria_ray_config* c, aria_ray_t* out) {
    if (!out || ray_bad_config(c)) return ARIA_E_INVALID;
    *out = nullptr;
    const RayParams P = ray_make_params(*c);
    if (P.n_steps < 1) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_ray_create", [&P](aria_ray_s* h) {
        const char* what = "aria_ray_create";
        h->P = P;
        h->n_vox = (size_t)h->cfg.nx * h->cfg.ny * h->cfg.nz;
        h->n_bricks = (int)(h->n_vox / 512);
        h->n_words = ((size_t)h->n_bricks + 31) / 32;
        int rc;
        if ((rc = h->d_words.reserve(h->stream, h->n_words, what)) != ARIA_OK) return rc;
        if ((rc = h->d_flags.reserve(h->stream, (size_t)h->n_bricks, what)) != ARIA_OK) return rc;
        if ((rc = h->d_ext.reserve(h->stream, 12, what)) != ARIA_OK) return rc;
        return h->d_rec.reserve(h->stream, 1, what);
    });
}

void aria_ray_destroy(aria_ray_t h) { stage_destroy(h); }

void* aria_ray_stream(aria_ray_t h) { return stage_stream(h); }

int aria_ray_check(aria_ray_t h) { return stage_check(h, {{ERRBIT_RAY_INPUT, ARIA_E_INVALID}}); }

int aria_ray_update_from_volume_device(aria_ray_t h, const aria_tsdf_voxel* d_voxels) {
    if (!h || !d_voxels) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(hipMemsetAsync(h->d_flags, 0, (size_t)h->n_bricks, h->stream));
    hipLaunchKernelGGL(k_ray_bricks, dim3((unsigned)((h->n_vox / 8 + RAY_BLOCK - 1) / RAY_BLOCK)), dim3(RAY_BLOCK), 0, h->stream, h->P,
                       reinterpret_cast<const unsigned long long*>(d_voxels), h->d_flags);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ray_brick_words, dim3((unsigned)((h->n_words + RAY_BLOCK - 1) / RAY_BLOCK)), dim3(RAY_BLOCK), 0, h->stream,
                       h->n_bricks, (const uint8_t*)h->d_flags, h->d_words);
    ARIA_HIP(hipGetLastError());
    h->d_vol = reinterpret_cast<const unsigned long long*>(d_voxels);
    return ARIA_OK;
}

int aria_ray_cast_batch_device(aria_ray_t h, const double* d_extrinsics, const uint8_t* d_view_mask, int n_views, int width, int height,
                               float* d_depth, int64_t depth_stride, int depth_pitch, float* d_normal, int64_t normal_stride,
                               int normal_pitch, uint8_t* d_gray, int64_t gray_stride, int gray_pitch, uint8_t* d_shade,
                               int64_t shade_stride, int shade_pitch, aria_ray_view* d_views) {
    if (!h || n_views < 0 || n_views > RAY_MAX_VIEWS || width < 1 || height < 1 || width > RAY_MAX_IMAGE || height > RAY_MAX_IMAGE ||
        (n_views > 0 && !d_extrinsics))
        return ARIA_E_INVALID;
    if (ray_bad_plane(d_depth, depth_stride, depth_pitch, width, height, n_views, 1) ||
        ray_bad_plane(d_normal, normal_stride, normal_pitch, width, height, n_views, 3) ||
        ray_bad_plane(d_gray, gray_stride, gray_pitch, width, height, n_views, 1) ||
        ray_bad_plane(d_shade, shade_stride, shade_pitch, width, height, n_views, 1))
        return ARIA_E_INVALID;
    if (!h->d_vol) return ARIA_E_INVALID;                             // no update yet
    if (n_views == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_views.reserve(h->stream, (size_t)n_views)) != ARIA_OK) return rc;
    const dim3 per_view((unsigned)((n_views + RAY_BLOCK - 1) / RAY_BLOCK));
    hipLaunchKernelGGL(k_ray_prepare, per_view, dim3(RAY_BLOCK), 0, h->stream, h->P, d_extrinsics, d_view_mask, n_views,
                       (RayView*)h->d_views, d_views, h->d_err);
    ARIA_HIP(hipGetLastError());
    const dim3 grid((unsigned)((width + RAY_TILE - 1) / RAY_TILE), (unsigned)((height + RAY_TILE - 1) / RAY_TILE), (unsigned)n_views);
    hipLaunchKernelGGL(k_ray_march, grid, dim3(RAY_BLOCK), 0, h->stream, h->P, (const RayView*)h->d_views, h->d_vol,
                       (const uint32_t*)h->d_words, width, height, d_depth, depth_stride, depth_pitch, d_normal, normal_stride,
                       normal_pitch, d_gray, gray_stride, gray_pitch, d_shade, shade_stride, shade_pitch, d_views);
    ARIA_HIP(hipGetLastError());
    if (d_views) {
        hipLaunchKernelGGL(k_ray_finish, per_view, dim3(RAY_BLOCK), 0, h->stream, (const RayView*)h->d_views, n_views, d_views);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_ray_cast(aria_ray_t h, const double* extrinsics, int width, int height, float* depth, float* normal, uint8_t* gray, uint8_t* shade,
                  aria_ray_view* view) {
    if (!h || !extrinsics || width < 1 || height < 1 || width > RAY_MAX_IMAGE || height > RAY_MAX_IMAGE) return ARIA_E_INVALID;
    if (!h->d_vol) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)width * height;
    int rc;
    if (depth && (rc = h->d_depth.reserve(h->stream, n)) != ARIA_OK) return rc;
    if (normal && (rc = h->d_normal.reserve(h->stream, 3 * n)) != ARIA_OK) return rc;
    if (gray && (rc = h->d_gray.reserve(h->stream, n)) != ARIA_OK) return rc;
    if (shade && (rc = h->d_shade.reserve(h->stream, n)) != ARIA_OK) return rc;
    ARIA_HIP(memcpy_on(h->stream, h->d_ext, extrinsics, 12 * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = aria_ray_cast_batch_device(h, h->d_ext, nullptr, 1, width, height, depth ? (float*)h->d_depth : nullptr, 0, width,
                                         normal ? (float*)h->d_normal : nullptr, 0, width, gray ? (uint8_t*)h->d_gray : nullptr, 0, width,
                                         shade ? (uint8_t*)h->d_shade : nullptr, 0, width, h->d_rec)) != ARIA_OK)
        return rc;
    if (depth) ARIA_HIP(hipMemcpyAsync(depth, h->d_depth, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (normal) ARIA_HIP(hipMemcpyAsync(normal, h->d_normal, 3 * n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (gray) ARIA_HIP(hipMemcpyAsync(gray, h->d_gray, n, hipMemcpyDeviceToHost, h->stream));
    if (shade) ARIA_HIP(hipMemcpyAsync(shade, h->d_shade, n, hipMemcpyDeviceToHost, h->stream));
    if (view) ARIA_HIP(hipMemcpyAsync(view, h->d_rec, sizeof(aria_ray_view), hipMemcpyDeviceToHost, h->stream));
    return aria_ray_check(h);
}

}  // extern "C"
