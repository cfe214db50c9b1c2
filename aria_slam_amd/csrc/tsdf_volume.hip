// Dense depth fusion: the fp32 depth maps of the dense stage integrated along the trajectory into one truncated signed
// distance volume in HBM, and the surface points read back out of it. Semantics in include/aria_orb_hip.h ("dense depth
// fusion"); aria_slam_amd/tsdf_ref.py is the definition and this file equals it bit for bit.
//
// k_tsdf_prepare    a lane per frame: the 12 doubles of [R|t] to fp32, the frame mask, the non-finite check (deferred-error OR),
//                   and the frame's cull bounds (below). One 80-byte record per frame.
// k_tsdf_cull       a lane per 8 x 8 x 4 tile of voxels and 32 frames: bit b of its word is set when frame 32 w + b is valid and
//                   some voxel of the tile may pass rules 3b and 3d (the frustum test, conservative: see tsdf_cull). 38 vector
//                   instructions per tile and frame, 0.15 per voxel-frame, against the 45 a lane spends to reject a voxel.
// k_tsdf_integrate  the hot path. A lane owns one voxel, a 64-lane wave an 8 x 8 x 1 slab of them and a 256-lane workgroup an
//                   8 x 8 x 4 tile: the record accesses are 64-byte x-runs, and the tile projects onto a compact pixel patch, so
//                   neighbouring lanes gather neighbouring depth pixels. The lane loads its 8-byte record once, walks the
//                   frames of the call whose bit is set in its tile's words with tsdf, weight and gray in registers, and
//                   stores the record once, and only if some frame touched it: 16 B per voxel per call, not per frame. The
//                   words and the frame records are read at workgroup-uniform addresses (scalar loads into SGPRs), so the
//                   frame loop is scalar control flow. The restatement does not cull, so bitwise parity on poses that straddle
//                   the frustum is the check. No LDS, no barrier, no atomics, no scratch.
// k_tsdf_count      a lane per voxel, a workgroup per chunk of 256 consecutive linear voxels: the points of the chunk.
// k_tsdf_scan       one workgroup: the exclusive scan of the chunk counts, the total to the count word, the capacity check.
// k_tsdf_emit       the same walk as k_tsdf_count; a point lands at chunk offset + in-chunk prefix (ballot and popcount inside
//                   a wave, wave offsets through LDS). Launch boundaries carry the data between the three: no workgroup waits
//                   for another inside a launch.
// Plain HIP C++. The text from "namespace {" to the extraction section also compiles for the host
// (tests/test_tsdf_kernel_emulation.py). The variants build (-DARIA_VARIANTS) adds the ARIA_TSDF_CULL=0 switch (every valid
// frame's bit set) for tools/tsdf_rate.py's A/B of the frustum test.
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
static_assert(sizeof(aria_tsdf_point) == 16, "aria_tsdf_point is 16 bytes");
static_assert(sizeof(aria_tsdf_config) == 104, "aria_tsdf_config is 104 bytes");

namespace {

constexpr int TSDF_BLOCK = 256;
constexpr int TSDF_TILE_X = 8, TSDF_TILE_Y = 8, TSDF_TILE_Z = 4;   // voxels of a workgroup; a wave is one 8 x 8 z-slab
constexpr int TSDF_MAX_DIM = 1024, TSDF_MAX_IMAGE = 16384, TSDF_MAX_FRAMES = 65535;
constexpr int ERRBIT_TSDF_INPUT = 1, ERRBIT_TSDF_CAP = 2;

// What the kernels take by value: the config in fp32 and the per-call image geometry.
struct TsdfParams {
    int nx, ny, nz, max_weight;
    float voxel, ox, oy, oz;
    float trunc, inv_trunc, min_depth, max_depth;
    float fx, fy, cx, cy;
    float wm1, hm1;                 // (float)(W - 1), (float)(H - 1)
    float rad, ext;                 // cull: 4 voxels (a tile's half extent is 3.5), and max |cX| + |cY| + |cZ| over the volume
    float al, ar, at, ab;           // cull: cx + 0.5, cx - (W - 0.5), cy + 0.5, cy - (H - 0.5)
};

// Host side: the config in fp32 with the cull constants of the volume, and the per-call image geometry. Inside the text the
// host emulation compiles, so that it runs on the constants the library uses.
inline TsdfParams tsdf_params(const int n[3], int max_weight, float voxel, const float origin[3], float trunc, float min_depth,
                              float max_depth, const double K[4]) {
    TsdfParams P{};
    P.nx = n[0]; P.ny = n[1]; P.nz = n[2]; P.max_weight = max_weight;
    P.voxel = voxel; P.ox = origin[0]; P.oy = origin[1]; P.oz = origin[2];
    P.trunc = trunc; P.inv_trunc = 1.0f / trunc; P.min_depth = min_depth; P.max_depth = max_depth;
    P.fx = (float)K[0]; P.fy = (float)K[1]; P.cx = (float)K[2]; P.cy = (float)K[3];
    P.rad = 4.0f * voxel;
    for (int a = 0; a < 3; a++) P.ext += std::max(std::fabs(origin[a]), std::fabs(origin[a] + (float)n[a] * voxel));
    return P;
}

inline TsdfParams tsdf_with_image(TsdfParams P, int width, int height) {
    P.wm1 = (float)(width - 1); P.hm1 = (float)(height - 1);
    P.al = P.cx + 0.5f; P.ar = P.cx - ((float)width - 0.5f);
    P.at = P.cy + 0.5f; P.ab = P.cy - ((float)height - 0.5f);
    return P;
}

// One frame as the integration reads it: 20 words at a workgroup-uniform address.
struct TsdfFrame {
    float r[9], t[3];
    float bz, bl, br, bt, bb;       // cull bounds of tsdf_cull
    int valid;                      // 0: masked out, or a non-finite extrinsic
    int pad[2];
};
constexpr size_t TSDF_MASK_BYTES = (size_t)16 << 20;   // the tile words of one launch; longer calls run in groups of frames

__device__ __forceinline__ bool tsdf_finite(double v) { return fabs(v) <= DBL_MAX; }

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_prepare(TsdfParams P, const double* __restrict__ ext, const uint8_t* __restrict__ mask,
                                                             int n_frames, TsdfFrame* __restrict__ frames, int* err) {
    const int f = (int)(blockIdx.x * TSDF_BLOCK + threadIdx.x);
    if (f >= n_frames) return;
    const double* e = ext + 12 * (int64_t)f;
    const bool wanted = !mask || mask[f] != 0;
    bool fin = true;
    for (int k = 0; k < 12; k++) fin = fin && tsdf_finite(e[k]);
    if (wanted && !fin) atomicOr(err, ERRBIT_TSDF_INPUT);
    TsdfFrame F;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) F.r[3 * r + c] = (float)e[4 * r + c];
        F.t[r] = (float)e[4 * r + 3];
    }
    // |coordinate(p) - coordinate(tile centre)| <= (L1 norm of the row) * 3.5 voxels for every voxel centre p of a tile; `rad`
    // is 4 voxels. On top, 1e-3 of the largest magnitude the coordinate's terms can take anywhere in the volume: three orders
    // of magnitude above the fp32 rounding of the chains of rules 3a and 3c.
    const float n0 = fabsf(F.r[0]) + fabsf(F.r[1]) + fabsf(F.r[2]);
    const float n1 = fabsf(F.r[3]) + fabsf(F.r[4]) + fabsf(F.r[5]);
    const float n2 = fabsf(F.r[6]) + fabsf(F.r[7]) + fabsf(F.r[8]);
    const float bx = n0 * P.rad + 1e-3f * (n0 * P.ext + fabsf(F.t[0]));
    const float by = n1 * P.rad + 1e-3f * (n1 * P.ext + fabsf(F.t[1]));
    const float bz = n2 * P.rad + 1e-3f * (n2 * P.ext + fabsf(F.t[2]));
    F.bz = bz;
    F.bl = fabsf(P.fx) * bx + (fabsf(P.al) + 1.0f) * bz;
    F.br = fabsf(P.fx) * bx + (fabsf(P.ar) + 1.0f) * bz;
    F.bt = fabsf(P.fy) * by + (fabsf(P.at) + 1.0f) * bz;
    F.bb = fabsf(P.fy) * by + (fabsf(P.ab) + 1.0f) * bz;
    F.valid = wanted && fin ? 1 : 0;
    F.pad[0] = F.pad[1] = 0;
    frames[f] = F;
}

// True when no voxel of the tile centred at (tx, ty, tz) can pass rules 3b and 3d for this frame. Conservative:
//   behind   zc(p) <= zc(centre) + bz < min_depth for every p: rule 3b rejects all.
//   beside   only when zc(p) >= zc(centre) - bz > 0 for every p. With z > 0, u < -0.5 is fx*xc + (cx + 0.5)*zc < 0; the left
//            side's value at p is within bl of the value at the centre, so value(centre) < -bl puts every u below -0.5 by more
//            than its rounding, and rintf(u) <= -1 fails rule 3d. The other three borders alike (rintf(u) >= W needs
//            u > W - 0.5). A NaN or an overflow makes a comparison false: no cull.
__device__ __forceinline__ bool tsdf_cull(const TsdfParams& P, const TsdfFrame& F, float tx, float ty, float tz) {
    const float zc = ((F.r[6] * tx + F.r[7] * ty) + F.r[8] * tz) + F.t[2];
    if (zc + F.bz < P.min_depth) return true;
    if (!(zc - F.bz > 0.0f)) return false;
    const float xc = ((F.r[0] * tx + F.r[1] * ty) + F.r[2] * tz) + F.t[0];
    const float yc = ((F.r[3] * tx + F.r[4] * ty) + F.r[5] * tz) + F.t[1];
    const float px = P.fx * xc, py = P.fy * yc;
    return px + P.al * zc < -F.bl || px + P.ar * zc > F.br || py + P.at * zc < -F.bt || py + P.ab * zc > F.bb;
}

// grid: (tiles / 256, words). mask[tile * n_words + w]: bit b = frame 32 w + b is to be walked by the tile. `cull` = 0 sets the
// bit of every valid frame (variants build: the A/B of tools/tsdf_rate.py).
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_cull(TsdfParams P, const TsdfFrame* __restrict__ frames, int n_frames, int n_words,
                                                          int cull, uint32_t* __restrict__ mask) {
    const int ntx = P.nx / TSDF_TILE_X, nty = P.ny / TSDF_TILE_Y, ntz = P.nz / TSDF_TILE_Z;
    const int tile = (int)(blockIdx.x * TSDF_BLOCK + threadIdx.x), w = (int)blockIdx.y;
    if (tile >= ntx * nty * ntz) return;
    // the tile's centre: the middle of voxel centres i0 + 0.5 .. i0 + 7.5 is i0 + 4 (z: k0 + 2)
    const float tx = P.ox + (float)((tile % ntx) * TSDF_TILE_X + TSDF_TILE_X / 2) * P.voxel;
    const float ty = P.oy + (float)((tile / ntx % nty) * TSDF_TILE_Y + TSDF_TILE_Y / 2) * P.voxel;
    const float tz = P.oz + (float)((tile / (ntx * nty)) * TSDF_TILE_Z + TSDF_TILE_Z / 2) * P.voxel;
    uint32_t bits = 0;
    for (int b = 0; b < 32 && 32 * w + b < n_frames; b++) {
        const TsdfFrame& F = frames[32 * w + b];
        if (F.valid && !(cull && tsdf_cull(P, F, tx, ty, tz))) bits |= 1u << b;
    }
    mask[(size_t)tile * n_words + w] = bits;
}

// grid: (nx / 8, ny / 8, nz / 4). depth / img: frame f at + f * stride; img may be null.
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate(TsdfParams P, const TsdfFrame* __restrict__ frames, int n_words,
                                                               const uint32_t* __restrict__ mask,
                                                               const float* __restrict__ depth, int64_t depth_stride, int depth_pitch,
                                                               const uint8_t* __restrict__ img, int64_t img_stride, int img_pitch,
                                                               unsigned long long* __restrict__ vol) {
    const int t = (int)threadIdx.x;
    const size_t tile = ((size_t)blockIdx.z * (P.ny / TSDF_TILE_Y) + blockIdx.y) * (P.nx / TSDF_TILE_X) + blockIdx.x;
    const int i = (int)blockIdx.x * TSDF_TILE_X + (t & 7);
    const int j = (int)blockIdx.y * TSDF_TILE_Y + ((t >> 3) & 7);
    const int k = (int)blockIdx.z * TSDF_TILE_Z + (t >> 6);
    const size_t idx = ((size_t)k * P.ny + j) * P.nx + i;
    const float cX = P.ox + ((float)i + 0.5f) * P.voxel;
    const float cY = P.oy + ((float)j + 0.5f) * P.voxel;
    const float cZ = P.oz + ((float)k + 0.5f) * P.voxel;

    const unsigned long long rec = vol[idx];
    float tsdf = __uint_as_float((uint32_t)rec);
    uint32_t weight = (uint32_t)(rec >> 32) & 0xFFFFu, gray = (uint32_t)(rec >> 48) & 0xFFu;
    bool dirty = false;

    for (int w = 0; w < n_words; w++)
    for (uint32_t m = mask[tile * n_words + w]; m; m &= m - 1) {         // workgroup-uniform: the frames this tile walks
        const int f = 32 * w + __builtin_ctz(m);
        const TsdfFrame& F = frames[f];
        const float xc = ((F.r[0] * cX + F.r[1] * cY) + F.r[2] * cZ) + F.t[0];
        const float yc = ((F.r[3] * cX + F.r[4] * cY) + F.r[5] * cZ) + F.t[1];
        const float zc = ((F.r[6] * cX + F.r[7] * cY) + F.r[8] * cZ) + F.t[2];
        if (!(zc >= P.min_depth)) continue;
        const float iz = 1.0f / zc;
        const float u = (P.fx * xc) * iz + P.cx;
        const float v = (P.fy * yc) * iz + P.cy;
        const float ur = rintf(u), vr = rintf(v);
        if (!(ur >= 0.0f && ur <= P.wm1 && vr >= 0.0f && vr <= P.hm1)) continue;
        const int ui = (int)ur, vi = (int)vr;
        const float D = depth[f * depth_stride + (int64_t)vi * depth_pitch + ui];
        if (!(D >= P.min_depth && D <= P.max_depth)) continue;
        const float sdf = D - zc;
        if (sdf < -P.trunc) continue;
        const float s = fminf(1.0f, sdf * P.inv_trunc);
        const float w = (float)weight;
        tsdf = (tsdf * w + s) / (w + 1.0f);
        if (img) {
            const uint32_t g = img[f * img_stride + (int64_t)vi * img_pitch + ui];
            gray = (gray * weight + g + ((weight + 1u) >> 1)) / (weight + 1u);
        }
        weight = min(weight + 1u, (uint32_t)P.max_weight);
        dirty = true;
    }
    if (dirty) vol[idx] = (unsigned long long)__float_as_uint(tsdf) | ((unsigned long long)(weight | (gray << 16)) << 32);
}

// ---- extraction ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tsdf_of(unsigned long long rec) { return __uint_as_float((uint32_t)rec); }
__device__ __forceinline__ uint32_t weight_of(unsigned long long rec) { return (uint32_t)(rec >> 32) & 0xFFFFu; }
__device__ __forceinline__ uint32_t gray_of(unsigned long long rec) { return (uint32_t)(rec >> 48) & 0xFFu; }

__device__ __forceinline__ bool tsdf_edge(unsigned long long a, unsigned long long b, uint32_t min_weight) {
    return weight_of(a) >= min_weight && weight_of(b) >= min_weight && ((tsdf_of(a) < 0.0f) != (tsdf_of(b) < 0.0f));
}

// Voxel idx and its +x, +y, +z neighbours; bit `axis` of the result is set when rule 4 emits a point there.
__device__ __forceinline__ uint32_t tsdf_edges(const unsigned long long* __restrict__ vol, int nx, int ny, int nz, uint32_t min_weight,
                                               size_t idx, int& i, int& j, int& k, unsigned long long& a, unsigned long long& bx,
                                               unsigned long long& by, unsigned long long& bz) {
    const uint32_t lin = (uint32_t)idx, row = lin / (uint32_t)nx;       // at most 2^30 voxels: 32-bit divisions
    i = (int)(lin - row * (uint32_t)nx);
    k = (int)(row / (uint32_t)ny);
    j = (int)(row - (uint32_t)k * (uint32_t)ny);
    a = vol[idx];
    bx = by = bz = 0;
    if (weight_of(a) < min_weight) return 0;
    uint32_t bits = 0;
    if (i + 1 < nx) { bx = vol[idx + 1]; bits |= tsdf_edge(a, bx, min_weight) ? 1u : 0u; }
    if (j + 1 < ny) { by = vol[idx + (size_t)nx]; bits |= tsdf_edge(a, by, min_weight) ? 2u : 0u; }
    if (k + 1 < nz) { bz = vol[idx + (size_t)nx * ny]; bits |= tsdf_edge(a, bz, min_weight) ? 4u : 0u; }
    return bits;
}

// grid: n_vox / 256 (the dims are multiples of 8, so n_vox is a multiple of 512)
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_count(const unsigned long long* __restrict__ vol, int nx, int ny, int nz,
                                                           uint32_t min_weight, int* __restrict__ counts) {
    __shared__ int s_wave[TSDF_BLOCK / 64];
    const size_t idx = (size_t)blockIdx.x * TSDF_BLOCK + threadIdx.x;
    int i, j, k;
    unsigned long long a, bx, by, bz;
    const uint32_t bits = tsdf_edges(vol, nx, ny, nz, min_weight, idx, i, j, k, a, bx, by, bz);
    const int n = __popcll(__ballot(bits & 1u)) + __popcll(__ballot(bits & 2u)) + __popcll(__ballot(bits & 4u));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// one workgroup of 1024 lanes: offsets[c] = the points before chunk c; *d_count = total
constexpr int TSDF_SCAN_BLOCK = 1024;
__global__ __launch_bounds__(TSDF_SCAN_BLOCK) void k_tsdf_scan(const int* __restrict__ counts, int n_chunks, long long* __restrict__ offsets,
                                                               long long cap, long long* __restrict__ d_count, int* err) {
    __shared__ int s_wave[TSDF_SCAN_BLOCK / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (int base = 0; base < n_chunks; base += TSDF_SCAN_BLOCK) {
        const int c = base + t < n_chunks ? counts[base + t] : 0;
        int incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < TSDF_SCAN_BLOCK / 64; w++) {
            const int v = s_wave[w];
            before += w < wave ? v : 0;
            all += v;
        }
        if (base + t < n_chunks) offsets[base + t] = carry + before + (incl - c);
        carry += all;
        __syncthreads();
    }
    if (t == 0) {
        *d_count = carry;
        if (carry > cap) atomicOr(err, ERRBIT_TSDF_CAP);
    }
}

__device__ __forceinline__ void tsdf_put(aria_tsdf_point* __restrict__ out, long long pos, long long cap, float voxel, float X0, float X1,
                                         float X2, int axis, unsigned long long a, unsigned long long b) {
    if (pos >= cap) return;
    const float ta = tsdf_of(a), tb = tsdf_of(b);
    const float alpha = ta / (ta - tb);
    const float step = alpha * voxel;
    aria_tsdf_point p;
    p.X[0] = axis == 0 ? X0 + step : X0;
    p.X[1] = axis == 1 ? X1 + step : X1;
    p.X[2] = axis == 2 ? X2 + step : X2;
    p.gray = (uint8_t)(alpha < 0.5f ? gray_of(a) : gray_of(b));
    p.axis = (uint8_t)axis;
    p.weight = (uint16_t)min(weight_of(a), weight_of(b));
    out[pos] = p;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_emit(const unsigned long long* __restrict__ vol, int nx, int ny, int nz,
                                                          uint32_t min_weight, float voxel, float ox, float oy, float oz,
                                                          const long long* __restrict__ offsets, aria_tsdf_point* __restrict__ out,
                                                          long long cap) {
    __shared__ int s_wave[TSDF_BLOCK / 64];
    const size_t idx = (size_t)blockIdx.x * TSDF_BLOCK + threadIdx.x;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int i, j, k;
    unsigned long long a, bx, by, bz;
    const uint32_t bits = tsdf_edges(vol, nx, ny, nz, min_weight, idx, i, j, k, a, bx, by, bz);
    const unsigned long long m0 = __ballot(bits & 1u), m1 = __ballot(bits & 2u), m2 = __ballot(bits & 4u);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int prefix = __popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below);
    if (lane == 0) s_wave[wave] = __popcll(m0) + __popcll(m1) + __popcll(m2);
    __syncthreads();
    if (!bits) return;
    long long pos = offsets[blockIdx.x] + prefix;
    for (int w = 0; w < wave; w++) pos += s_wave[w];
    const float X0 = ox + ((float)i + 0.5f) * voxel, X1 = oy + ((float)j + 0.5f) * voxel, X2 = oz + ((float)k + 0.5f) * voxel;
    if (bits & 1u) tsdf_put(out, pos++, cap, voxel, X0, X1, X2, 0, a, bx);
    if (bits & 2u) tsdf_put(out, pos++, cap, voxel, X0, X1, X2, 1, a, by);
    if (bits & 4u) tsdf_put(out, pos++, cap, voxel, X0, X1, X2, 2, a, bz);
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_tsdf_s : StageHandle {
    aria_tsdf_config cfg{};
    TsdfParams P{};
    size_t n_vox = 0;
    int cull = 1;
    DeviceBuffer<unsigned long long> d_vol;                    // the records, one word each
    DeviceBuffer<TsdfFrame> d_frames;
    DeviceBuffer<uint32_t> d_mask;                             // tiles x words of one launch
    DeviceBuffer<int> d_counts;                                // extraction: per chunk
    DeviceBuffer<long long> d_offsets;
    // single-frame / host-form staging (grow-only)
    DeviceBuffer<float> d_depth;
    DeviceBuffer<uint8_t> d_img;
    DeviceBuffer<aria_tsdf_point> d_points;
    DeviceBuffer<double> d_ext;                                // 12 doubles
    DeviceBuffer<int64_t> d_count;
};

namespace {

bool finf(float v) { return std::isfinite(v); }

bool bad_dims(int nx, int ny, int nz) {
    for (int n : {nx, ny, nz})
        if (n < 8 || n > TSDF_MAX_DIM || n % 8) return true;
    return false;
}

bool bad_config(const aria_tsdf_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_tsdf_config)) return true;
    if (bad_dims(c->nx, c->ny, c->nz)) return true;
    if (!(c->voxel > 0) || !finf(c->voxel) || !(c->trunc > 0) || !finf(c->trunc)) return true;
    for (float v : c->origin)
        if (!finf(v)) return true;
    if (!(c->min_depth <= c->max_depth)) return true;
    if (c->max_weight < 1 || c->max_weight > 65535 || c->min_weight < 1 || c->min_weight > 65535) return true;
    return !std::isfinite(c->fx) || !std::isfinite(c->fy) || !std::isfinite(c->cx) || !std::isfinite(c->cy);
}

TsdfParams make_params(const aria_tsdf_config& c) {
    const int n[3] = {c.nx, c.ny, c.nz};
    const double K[4] = {c.fx, c.fy, c.cx, c.cy};
    return tsdf_params(n, c.max_weight, c.voxel, c.origin, c.trunc, c.min_depth, c.max_depth, K);
}

}  // namespace

extern "C" {

void aria_tsdf_default_config(aria_tsdf_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_tsdf_config);
    c->nx = 256; c->ny = 256; c->nz = 128;
    c->max_weight = 64; c->min_weight = 2;
    c->voxel = 0.05f; c->trunc = 0.20f;
    c->origin[0] = -6.4f; c->origin[1] = -6.4f; c->origin[2] = 0.0f;
    c->min_depth = 0.3f; c->max_depth = 10.0f;
    c->fx = 458.654; c->fy = 457.296; c->cx = 367.215; c->cy = 248.375;   // EuRoC cam0
}

int64_t aria_tsdf_volume_bytes(int nx, int ny, int nz) {
    return bad_dims(nx, ny, nz) ? (int64_t)ARIA_E_INVALID : (int64_t)sizeof(aria_tsdf_voxel) * nx * ny * nz;
}

int64_t aria_tsdf_algorithmic_bytes(int nx, int ny, int nz, int width, int height, int n_frames) {
    if (bad_dims(nx, ny, nz) || width < 1 || height < 1 || n_frames < 0) return ARIA_E_INVALID;
    return 2 * aria_tsdf_volume_bytes(nx, ny, nz) + 4 * (int64_t)width * height * n_frames;
}

int aria_tsdf_create(const aria_tsdf_config* c, aria_tsdf_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_tsdf_create", [](aria_tsdf_s* h) {
        const aria_tsdf_config& c = h->cfg;
        const char* what = "aria_tsdf_create";
        h->P = make_params(c);
        h->n_vox = (size_t)c.nx * c.ny * c.nz;
        if (const char* s = aria_getenv("ARIA_TSDF_CULL")) h->cull = std::atoi(s) != 0;   // variants build: A/B
        int rc;
        if ((rc = h->d_vol.reserve(h->stream, h->n_vox, what)) != ARIA_OK) return rc;
        if ((rc = h->d_ext.reserve(h->stream, 12, what)) != ARIA_OK) return rc;
        if ((rc = h->d_count.reserve(h->stream, 1, what)) != ARIA_OK) return rc;
        const hipError_t e = memset_on(h->stream, h->d_vol, 0, h->n_vox * sizeof(aria_tsdf_voxel));
        return e == hipSuccess ? (int)ARIA_OK : hip_fail(e, what, __FILE__, __LINE__);
    });
}

void aria_tsdf_destroy(aria_tsdf_t h) { stage_destroy(h); }

void* aria_tsdf_stream(aria_tsdf_t h) { return stage_stream(h); }

int aria_tsdf_check(aria_tsdf_t h) {
    return stage_check(h, {{ERRBIT_TSDF_INPUT, ARIA_E_INVALID}, {ERRBIT_TSDF_CAP, ARIA_E_OUTPUT_TOO_SMALL}});
}

int aria_tsdf_clear(aria_tsdf_t h) {
    if (!h) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(hipMemsetAsync(h->d_vol, 0, h->n_vox * sizeof(aria_tsdf_voxel), h->stream));
    return ARIA_OK;
}

int aria_tsdf_integrate_batch_device(aria_tsdf_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int width, int height,
                                     const double* d_extrinsics, const uint8_t* d_frame_mask, const uint8_t* d_img, int64_t img_stride,
                                     int img_pitch, int n_frames) {
    if (!h || !d_depth || !d_extrinsics || n_frames < 0 || n_frames > TSDF_MAX_FRAMES || width < 1 || height < 1 ||
        width > TSDF_MAX_IMAGE || height > TSDF_MAX_IMAGE || depth_pitch < width)
        return ARIA_E_INVALID;
    if (n_frames > 1 && depth_stride < (int64_t)depth_pitch * (height - 1) + width) return ARIA_E_INVALID;
    if (d_img && (img_pitch < width || (n_frames > 1 && img_stride < (int64_t)img_pitch * (height - 1) + width))) return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_frames.reserve(h->stream, (size_t)n_frames)) != ARIA_OK) return rc;
    const TsdfParams P = tsdf_with_image(h->P, width, height);
    const dim3 grid(P.nx / TSDF_TILE_X, P.ny / TSDF_TILE_Y, P.nz / TSDF_TILE_Z);
    const size_t tiles = (size_t)grid.x * grid.y * grid.z;
    // frames per launch: all of them while their tile words fit TSDF_MASK_BYTES (4096 frames at the default volume, 32 at the
    // largest), else groups of that many
    const int max_words = (int)std::max<size_t>(TSDF_MASK_BYTES / (tiles * sizeof(uint32_t)), 1);
    const int group = std::min(n_frames, 32 * max_words), group_words = (group + 31) / 32;
    if ((rc = h->d_mask.reserve(h->stream, tiles * group_words)) != ARIA_OK) return rc;
    hipLaunchKernelGGL(k_tsdf_prepare, dim3((unsigned)((n_frames + TSDF_BLOCK - 1) / TSDF_BLOCK)), dim3(TSDF_BLOCK), 0, h->stream, P,
                       d_extrinsics, d_frame_mask, n_frames, (TsdfFrame*)h->d_frames, h->d_err);
    ARIA_HIP(hipGetLastError());
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int n = std::min(group, n_frames - f0), words = (n + 31) / 32;
        hipLaunchKernelGGL(k_tsdf_cull, dim3((unsigned)((tiles + TSDF_BLOCK - 1) / TSDF_BLOCK), words), dim3(TSDF_BLOCK), 0, h->stream, P,
                           (const TsdfFrame*)h->d_frames + f0, n, words, h->cull, (uint32_t*)h->d_mask);
        ARIA_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tsdf_integrate, grid, dim3(TSDF_BLOCK), 0, h->stream, P, (const TsdfFrame*)h->d_frames + f0, words,
                           (const uint32_t*)h->d_mask, d_depth + f0 * depth_stride, depth_stride, depth_pitch,
                           d_img ? d_img + f0 * img_stride : nullptr, img_stride, img_pitch, h->d_vol);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_tsdf_integrate(aria_tsdf_t h, const float* depth, int width, int height, int depth_pitch, const double* extrinsics,
                        const uint8_t* img, int img_pitch) {
    if (!h || !depth || !extrinsics || width < 1 || height < 1 || width > TSDF_MAX_IMAGE || height > TSDF_MAX_IMAGE ||
        depth_pitch < width || (img && img_pitch < width))
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)width * height;
    int rc;
    if ((rc = h->d_depth.reserve(h->stream, n)) != ARIA_OK) return rc;
    if (img && (rc = h->d_img.reserve(h->stream, n)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpy2DAsync(h->d_depth, (size_t)width * 4, depth, (size_t)depth_pitch * 4, (size_t)width * 4, (size_t)height,
                              hipMemcpyHostToDevice, h->stream));
    if (img)
        ARIA_HIP(hipMemcpy2DAsync(h->d_img, (size_t)width, img, (size_t)img_pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice,
                                  h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_ext, extrinsics, 12 * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = aria_tsdf_integrate_batch_device(h, h->d_depth, 0, width, width, height, h->d_ext, nullptr, img ? (uint8_t*)h->d_img : nullptr,
                                               0, width, 1)) != ARIA_OK)
        return rc;
    return aria_tsdf_check(h);
}

int aria_tsdf_extract_points_device(aria_tsdf_t h, aria_tsdf_point* d_points, int64_t cap, int64_t* d_count) {
    if (!h || !d_count || cap < 0 || (cap > 0 && !d_points)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const int n_chunks = (int)(h->n_vox / TSDF_BLOCK);
    int rc;
    if ((rc = h->d_counts.reserve(h->stream, (size_t)n_chunks)) != ARIA_OK) return rc;
    if ((rc = h->d_offsets.reserve(h->stream, (size_t)n_chunks)) != ARIA_OK) return rc;
    const TsdfParams& P = h->P;
    hipLaunchKernelGGL(k_tsdf_count, dim3((unsigned)n_chunks), dim3(TSDF_BLOCK), 0, h->stream, h->d_vol, P.nx, P.ny, P.nz,
                       (uint32_t)h->cfg.min_weight, (int*)h->d_counts);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(TSDF_SCAN_BLOCK), 0, h->stream, (const int*)h->d_counts, n_chunks, (long long*)h->d_offsets,
                       (long long)cap, (long long*)d_count, h->d_err);
    ARIA_HIP(hipGetLastError());
    if (cap > 0) {
        hipLaunchKernelGGL(k_tsdf_emit, dim3((unsigned)n_chunks), dim3(TSDF_BLOCK), 0, h->stream, h->d_vol, P.nx, P.ny, P.nz,
                           (uint32_t)h->cfg.min_weight, P.voxel, P.ox, P.oy, P.oz, (const long long*)h->d_offsets, d_points, (long long)cap);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_tsdf_extract_points(aria_tsdf_t h, aria_tsdf_point* points, int64_t cap, int64_t* total) {
    if (!h || !total || cap < 0 || (cap > 0 && !points)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if (cap > 0 && (rc = h->d_points.reserve(h->stream, (size_t)cap)) != ARIA_OK) return rc;
    if ((rc = aria_tsdf_extract_points_device(h, cap > 0 ? (aria_tsdf_point*)h->d_points : nullptr, cap, h->d_count)) != ARIA_OK)
        return rc;
    long long n = 0;
    ARIA_HIP(memcpy_on(h->stream, &n, h->d_count, sizeof(n), hipMemcpyDeviceToHost));
    *total = n;
    const int64_t written = std::min<int64_t>(n, cap);
    if (written > 0) ARIA_HIP(memcpy_on(h->stream, points, h->d_points, sizeof(aria_tsdf_point) * (size_t)written, hipMemcpyDeviceToHost));
    return aria_tsdf_check(h);
}

aria_tsdf_voxel* aria_tsdf_device_voxels(aria_tsdf_t h) { return h ? reinterpret_cast<aria_tsdf_voxel*>(h->d_vol.p) : nullptr; }

int aria_tsdf_read_box(aria_tsdf_t h, int i0, int j0, int k0, int ni, int nj, int nk, aria_tsdf_voxel* out) {
    if (!h || !out || i0 < 0 || j0 < 0 || k0 < 0 || ni < 1 || nj < 1 || nk < 1 || i0 > h->cfg.nx - ni || j0 > h->cfg.ny - nj ||
        k0 > h->cfg.nz - nk)
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t nx = (size_t)h->cfg.nx, ny = (size_t)h->cfg.ny, rec = sizeof(aria_tsdf_voxel);
    for (int k = 0; k < nk; k++)
        ARIA_HIP(hipMemcpy2DAsync(out + (size_t)k * nj * ni, (size_t)ni * rec, h->d_vol + ((size_t)(k0 + k) * ny + j0) * nx + i0, nx * rec,
                                  (size_t)ni * rec, (size_t)nj, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return ARIA_OK;
}

}  // extern "C"
