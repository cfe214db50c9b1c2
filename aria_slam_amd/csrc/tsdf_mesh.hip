// Mesh of the volume: the aria_tsdf_voxel records of the dense depth fusion contoured into a closed, oriented triangle mesh by
// marching tetrahedra on the Kuhn split of every cell. Semantics in include/aria_orb_hip.h ("mesh of the volume");
// aria_slam_amd/mesh_ref.py is the definition and this file equals it byte for byte. The stage owns no volume.
//
// The shape is that of k_tsdf_count / k_tsdf_scan / k_tsdf_emit: a lane per voxel, a workgroup per chunk of 256 consecutive
// linear voxels, so the canonical order falls out of offsets and nothing is sorted.
// k_mesh_count   (update) the lane loads its record and the seven at +{0,1}^3 (rows are 512-byte runs along x), forms the 7-bit
//                mask of the edges it owns that carry a vertex, the 8 corner signs of its cell, the live bit and the cell's
//                triangle count, and parks them in ONE word per voxel together with the vertex prefix inside the chunk
//                (at most 1792, 11 bits). The chunk's two counts go to d_vcount / d_tcount.
// k_mesh_scan    one workgroup: the exclusive scans of both counts with 64-bit carries, the totals to the count words, the
//                capacity and 2^32 comparisons.
// k_mesh_emit    a chunk that holds nothing leaves after reading its two counts. A vertex lands at chunk offset + parked
//                prefix; a triangle at chunk offset + the scan of the parked triangle counts. The number of a neighbour's
//                vertex is that neighbour's chunk offset + its parked prefix + the popcount of its edge mask below d: two
//                cached loads, nothing re-derived. Recomputing it instead would need the neighbour chunk's scan again; that
//                form is not built.
// Per-lane counts reach 7 and 12, so the prefix inside a wave is a __shfl_up scan, not ballots. No float atomics, no grid-wide
// barrier, no scratch memory; launch boundaries carry the data between the three.
// Plain HIP C++. The text from "namespace {" to the kernels section also compiles for the host
// (tests/test_mesh_kernel_emulation.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_mesh_vertex) == 16, "aria_mesh_vertex is 16 bytes");
static_assert(sizeof(aria_mesh_triangle) == 12, "aria_mesh_triangle is 12 bytes");
static_assert(sizeof(aria_mesh_config) == 48, "aria_mesh_config is 48 bytes");

namespace {

constexpr int MESH_BLOCK = 256;                     // voxels of a chunk; the parked prefix counts inside it
constexpr int MESH_MAX_DIM = 1024;
constexpr int ERRBIT_MESH_CAP = 1, ERRBIT_MESH_OVERFLOW = 2;

// The parked word of a voxel.
constexpr int MESH_W_PREFIX = 7, MESH_W_INSIDE = 18, MESH_W_LIVE = 26, MESH_W_NTRI = 27;
constexpr uint32_t MESH_W_EDGES = 0x7Fu, MESH_W_PREFIX_MASK = 0x7FFu;

struct MeshGeom {
    int nx, ny, nz;
    uint32_t min_weight;
    float voxel, ox, oy, oz;
};

__device__ const uint64_t MESH_TABLE[6][16] = {
#include "tsdf_mesh_table.inc"
};

__device__ __forceinline__ float mesh_tsdf(unsigned long long rec) { return __uint_as_float((uint32_t)rec); }
__device__ __forceinline__ uint32_t mesh_weight(unsigned long long rec) { return (uint32_t)(rec >> 32) & 0xFFFFu; }
__device__ __forceinline__ uint32_t mesh_gray(unsigned long long rec) { return (uint32_t)(rec >> 48) & 0xFFu; }

// The inside mask of tetrahedron p (rule 3) from the 8 corner signs of a cell: corners (0, 2^p0, 2^p0 + 2^p1, 7).
__device__ __forceinline__ uint32_t mesh_tet_mask(uint32_t inside8, int p) {
    const int a = p >> 1;                                               // p0: 0, 0, 1, 1, 2, 2
    const int b = (p & 1) ? (a == 2 ? 1 : 2) : (a == 0 ? 1 : 0);        // p1: 1, 2, 0, 2, 0, 1
    const int c1 = 1 << a, c2 = c1 + (1 << b);
    return (inside8 & 1u) | (((inside8 >> c1) & 1u) << 1) | (((inside8 >> c2) & 1u) << 2) | (((inside8 >> 7) & 1u) << 3);
}

// Rules 2 and 3 for voxel idx: the word without its prefix. A corner outside the volume is never loaded and never seen.
__device__ __forceinline__ uint32_t mesh_voxel(const unsigned long long* __restrict__ vol, const MeshGeom& G, size_t idx) {
    const uint32_t lin = (uint32_t)idx, row = lin / (uint32_t)G.nx;     // at most 2^30 voxels: 32-bit divisions
    const int i = (int)(lin - row * (uint32_t)G.nx), k = (int)(row / (uint32_t)G.ny), j = (int)(row - (uint32_t)k * (uint32_t)G.ny);
    const bool in_x = i + 1 < G.nx, in_y = j + 1 < G.ny, in_z = k + 1 < G.nz;
    const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
    uint32_t seen = 0, inside = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const bool in = (!(q & 1) || in_x) && (!(q & 2) || in_y) && (!(q & 4) || in_z);
        const unsigned long long rec = in ? vol[idx + (q & 1) + ((q >> 1) & 1) * sy + ((q >> 2) & 1) * sz] : 0ull;
        seen |= (in && mesh_weight(rec) >= G.min_weight) ? 1u << q : 0u;
        inside |= (mesh_tsdf(rec) < 0.0f) ? 1u << q : 0u;
    }
    uint32_t word = 0;
    if (seen & 1u) {
        // bit d - 1: corner d seen and exactly one of voxel and corner inside
        const uint32_t differs = (inside ^ (0u - (inside & 1u))) & seen;
        word |= (differs >> 1) & MESH_W_EDGES;
    }
    if (seen == 0xFFu) {                                                // all eight corners lie inside the volume and are seen
        uint32_t ntri = 0;
#pragma unroll
        for (int p = 0; p < 6; p++) ntri += (uint32_t)(MESH_TABLE[p][mesh_tet_mask(inside, p)] & 3u);
        word |= (inside << MESH_W_INSIDE) | (1u << MESH_W_LIVE) | (ntri << MESH_W_NTRI);
    }
    return word;
}

// The vertex of edge (voxel (i, j, k), d): rule 2. a is the voxel's record, b the far end's.
__device__ __forceinline__ aria_mesh_vertex mesh_vertex(const MeshGeom& G, int i, int j, int k, int d, unsigned long long a,
                                                        unsigned long long b) {
    const float ta = mesh_tsdf(a), tb = mesh_tsdf(b);
    const float alpha = ta / (ta - tb);
    const float step = alpha * G.voxel;
    const float X0 = G.ox + ((float)i + 0.5f) * G.voxel, X1 = G.oy + ((float)j + 0.5f) * G.voxel, X2 = G.oz + ((float)k + 0.5f) * G.voxel;
    aria_mesh_vertex v;
    v.X[0] = (d & 1) ? X0 + step : X0;
    v.X[1] = (d & 2) ? X1 + step : X1;
    v.X[2] = (d & 4) ? X2 + step : X2;
    v.gray = (uint8_t)(alpha < 0.5f ? mesh_gray(a) : mesh_gray(b));
    v.dir = (uint8_t)d;
    v.weight = (uint16_t)min(mesh_weight(a), mesh_weight(b));
    return v;
}

// The number of the vertex on edge (vox, d), which carries one: chunk offset + parked prefix + the voxel's edges below d.
__device__ __forceinline__ uint32_t mesh_vertex_number(const uint32_t* __restrict__ words, const long long* __restrict__ voff, size_t vox,
                                                       uint32_t d) {
    const uint32_t w = words[vox];
    return (uint32_t)(voff[vox / MESH_BLOCK] + (long long)((w >> MESH_W_PREFIX) & MESH_W_PREFIX_MASK) +
                      (long long)__popc(w & ((1u << (d - 1u)) - 1u)));
}

// Rules 4 and 5 for the live cell whose corner 0 is voxel idx: its triangles to out[pos...], those below cap only. Returns
// how many the cell has.
__device__ __forceinline__ int mesh_cell_triangles(const MeshGeom& G, const uint32_t* __restrict__ words, const long long* __restrict__ voff,
                                                   size_t idx, uint32_t inside8, aria_mesh_triangle* __restrict__ out, long long pos,
                                                   long long cap) {
    const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
    int n = 0;
    for (int p = 0; p < 6; p++) {
        const uint64_t e = MESH_TABLE[p][mesh_tet_mask(inside8, p)];
        const int count = (int)(e & 3u);
        for (int t = 0; t < count; t++, n++) {
            if (pos + n >= cap) continue;
            aria_mesh_triangle tri;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint32_t code = (uint32_t)(e >> (4 + 6 * (3 * t + c))) & 63u, lo = code >> 3;
                tri.v[c] = mesh_vertex_number(words, voff, idx + (lo & 1u) + ((lo >> 1) & 1u) * sy + ((lo >> 2) & 1u) * sz, code & 7u);
            }
            out[pos + n] = tri;
        }
    }
    return n;
}

// What the scan defers from the two totals (rule 6).
__device__ __forceinline__ int mesh_count_errors(long long n_vertices, long long n_triangles, long long vcap, long long tcap) {
    int bits = 0;
    if (n_vertices > vcap || n_triangles > tcap) bits |= ERRBIT_MESH_CAP;
    if (n_vertices > 0xFFFFFFFFll) bits |= ERRBIT_MESH_OVERFLOW;
    return bits;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
// Exclusive prefix of v over the 256 lanes of the workgroup (v <= 12: sums fit 16 bits many times over); total = the sum.
__device__ __forceinline__ int mesh_block_scan(int v, int* s_wave, int& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < MESH_BLOCK / 64; w++) {
        const int s = s_wave[w];
        before += w < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}

// grid: n_vox / 256 (the dims are multiples of 8, so n_vox is a multiple of 512)
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_count(const unsigned long long* __restrict__ vol, MeshGeom G,
                                                           uint32_t* __restrict__ words, int* __restrict__ vcount,
                                                           int* __restrict__ tcount) {
    __shared__ int s_wave[MESH_BLOCK / 64];
    const size_t idx = (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t word = mesh_voxel(vol, G, idx);
    int n_vert, n_tri;
    const int prefix = mesh_block_scan(__popc(word & MESH_W_EDGES), s_wave, n_vert);
    (void)mesh_block_scan((int)(word >> MESH_W_NTRI), s_wave, n_tri);
    words[idx] = word | ((uint32_t)prefix << MESH_W_PREFIX);
    if (threadIdx.x == 0) {
        vcount[blockIdx.x] = n_vert;
        tcount[blockIdx.x] = n_tri;
    }
}

// one workgroup of 1024 lanes: voff[c] / toff[c] = the vertices / triangles before chunk c; d_counts[0..1] = the totals. A lane
// takes 4 consecutive chunks, so a batch is 4096 chunks and the default volume 8 batches: each batch costs a barrier pair and a
// round of load latency that nothing overlaps, and with a chunk per lane (32 batches) this launch was the longest of the stage.
constexpr int MESH_SCAN_BLOCK = 1024, MESH_SCAN_ITEMS = 4;
__global__ __launch_bounds__(MESH_SCAN_BLOCK) void k_mesh_scan(const int* __restrict__ vcount, const int* __restrict__ tcount, int n_chunks,
                                                               long long* __restrict__ voff, long long* __restrict__ toff, long long vcap,
                                                               long long tcap, long long* __restrict__ d_counts, int* err) {
    __shared__ int s_wave[2][MESH_SCAN_BLOCK / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    long long vcarry = 0, tcarry = 0;
    for (int base = 0; base < n_chunks; base += MESH_SCAN_BLOCK * MESH_SCAN_ITEMS) {
        const int first = base + t * MESH_SCAN_ITEMS;
        int cv[MESH_SCAN_ITEMS], ct[MESH_SCAN_ITEMS], sv = 0, st = 0;
#pragma unroll
        for (int r = 0; r < MESH_SCAN_ITEMS; r++) {
            const bool in = first + r < n_chunks;
            cv[r] = in ? vcount[first + r] : 0;
            ct[r] = in ? tcount[first + r] : 0;
            sv += cv[r];
            st += ct[r];
        }
        int iv = sv, it = st;                                           // a batch holds at most 4096 * 3072 triangles: 32 bits
        for (int d = 1; d < 64; d <<= 1) {
            const int uv = __shfl_up(iv, d, 64), ut = __shfl_up(it, d, 64);
            if (lane >= d) { iv += uv; it += ut; }
        }
        if (lane == 63) { s_wave[0][wave] = iv; s_wave[1][wave] = it; }
        __syncthreads();
        int bv = 0, av = 0, bt = 0, at = 0;
        for (int w = 0; w < MESH_SCAN_BLOCK / 64; w++) {
            const int wv = s_wave[0][w], wt = s_wave[1][w];
            bv += w < wave ? wv : 0; av += wv;
            bt += w < wave ? wt : 0; at += wt;
        }
        long long pv = vcarry + bv + (iv - sv), pt = tcarry + bt + (it - st);
#pragma unroll
        for (int r = 0; r < MESH_SCAN_ITEMS; r++) {
            if (first + r < n_chunks) {
                voff[first + r] = pv;
                toff[first + r] = pt;
            }
            pv += cv[r];
            pt += ct[r];
        }
        vcarry += av;
        tcarry += at;
        __syncthreads();
    }
    if (t == 0) {
        d_counts[0] = vcarry;
        d_counts[1] = tcarry;
        const int bits = mesh_count_errors(vcarry, tcarry, vcap, tcap);
        if (bits) atomicOr(err, bits);
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_emit(const unsigned long long* __restrict__ vol, MeshGeom G,
                                                          const uint32_t* __restrict__ words, const int* __restrict__ vcount,
                                                          const int* __restrict__ tcount, const long long* __restrict__ voff,
                                                          const long long* __restrict__ toff, aria_mesh_vertex* __restrict__ vertices,
                                                          long long vcap, aria_mesh_triangle* __restrict__ triangles, long long tcap) {
    __shared__ int s_wave[MESH_BLOCK / 64];
    const int n_vert = vcount[blockIdx.x], n_tri = tcount[blockIdx.x];   // workgroup-uniform
    if (n_vert == 0 && n_tri == 0) return;
    const size_t idx = (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t word = words[idx];
    if (n_vert != 0 && (word & MESH_W_EDGES) != 0 && vcap > 0) {
        const uint32_t lin = (uint32_t)idx, row = lin / (uint32_t)G.nx;
        const int i = (int)(lin - row * (uint32_t)G.nx), k = (int)(row / (uint32_t)G.ny), j = (int)(row - (uint32_t)k * (uint32_t)G.ny);
        const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
        const unsigned long long a = vol[idx];
        long long pos = voff[blockIdx.x] + (long long)((word >> MESH_W_PREFIX) & MESH_W_PREFIX_MASK);
#pragma unroll
        for (int d = 1; d < 8; d++) {
            if (!((word >> (d - 1)) & 1u)) continue;                    // a set bit: the far end lies inside the volume
            if (pos < vcap) vertices[pos] = mesh_vertex(G, i, j, k, d, a, vol[idx + (d & 1) + ((d >> 1) & 1) * sy + ((d >> 2) & 1) * sz]);
            pos++;
        }
    }
    if (n_tri == 0 || tcap <= 0) return;                                // workgroup-uniform: the barrier below is met by all or none
    int total;
    const int prefix = mesh_block_scan((int)(word >> MESH_W_NTRI), s_wave, total);
    if (!((word >> MESH_W_LIVE) & 1u)) return;
    (void)mesh_cell_triangles(G, words, voff, idx, (word >> MESH_W_INSIDE) & 0xFFu, triangles, toff[blockIdx.x] + prefix, tcap);
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_mesh_s : StageHandle {
    aria_mesh_config cfg{};
    MeshGeom G{};
    size_t n_vox = 0;
    int n_chunks = 0;
    const unsigned long long* d_vol = nullptr;                 // the caller's records, remembered by update
    DeviceBuffer<uint32_t> d_words;                            // the parked word per voxel
    DeviceBuffer<int> d_vcount, d_tcount;                      // per chunk
    DeviceBuffer<long long> d_voff, d_toff;
    DeviceBuffer<int64_t> d_counts;                            // host form: the two totals
    // host-form staging (grow-only)
    DeviceBuffer<aria_mesh_vertex> d_vertices;
    DeviceBuffer<aria_mesh_triangle> d_triangles;
};

namespace {

bool mesh_bad_dims(int nx, int ny, int nz) {
    for (int n : {nx, ny, nz})
        if (n < 8 || n > MESH_MAX_DIM || n % 8) return true;
    return false;
}

bool mesh_bad_config(const aria_mesh_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_mesh_config)) return true;
    if (mesh_bad_dims(c->nx, c->ny, c->nz)) return true;
    if (!(c->voxel > 0) || !std::isfinite(c->voxel)) return true;
    for (float v : c->origin)
        if (!std::isfinite(v)) return true;
    return c->min_weight < 1 || c->min_weight > 65535;
}

bool mesh_bad_outputs(const void* vertices, int64_t vcap, const void* triangles, int64_t tcap, const void* counts) {
    return !counts || vcap < 0 || tcap < 0 || (vcap > 0 && !vertices) || (tcap > 0 && !triangles);
}

}  // namespace

extern "C" {

void aria_mesh_default_config(aria_mesh_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_mesh_config);
    c->nx = 256; c->ny = 256; c->nz = 128;
    c->min_weight = 2;
    c->voxel = 0.05f;
    c->origin[0] = -6.4f; c->origin[1] = -6.4f; c->origin[2] = 0.0f;
}

int64_t aria_mesh_scratch_bytes(int nx, int ny, int nz) {
    if (mesh_bad_dims(nx, ny, nz)) return ARIA_E_INVALID;
    const int64_t n = (int64_t)nx * ny * nz;
    return 4 * n + 24 * (n / MESH_BLOCK);
}

int64_t aria_mesh_algorithmic_bytes(int nx, int ny, int nz, int64_t n_vertices, int64_t n_triangles) {
    if (mesh_bad_dims(nx, ny, nz) || n_vertices < 0 || n_triangles < 0) return ARIA_E_INVALID;
    return 16 * (int64_t)nx * ny * nz + 16 * n_vertices + 12 * n_triangles;
}

int aria_mesh_create(const aria_mesh_config* c, aria_mesh_t* out) {
    if (!out || mesh_bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_mesh_create", [](aria_mesh_s* h) {
        const aria_mesh_config& c = h->cfg;
        h->G = MeshGeom{c.nx, c.ny, c.nz, (uint32_t)c.min_weight, c.voxel, c.origin[0], c.origin[1], c.origin[2]};
        h->n_vox = (size_t)c.nx * c.ny * c.nz;
        h->n_chunks = (int)(h->n_vox / MESH_BLOCK);
        const size_t nc = (size_t)h->n_chunks;
        const char* what = "aria_mesh_create";
        int rc;
        if ((rc = h->d_words.reserve(h->stream, h->n_vox, what)) != ARIA_OK) return rc;
        if ((rc = h->d_vcount.reserve(h->stream, nc, what)) != ARIA_OK) return rc;
        if ((rc = h->d_tcount.reserve(h->stream, nc, what)) != ARIA_OK) return rc;
        if ((rc = h->d_voff.reserve(h->stream, nc, what)) != ARIA_OK) return rc;
        if ((rc = h->d_toff.reserve(h->stream, nc, what)) != ARIA_OK) return rc;
        return h->d_counts.reserve(h->stream, 2, what);
    });
}

void aria_mesh_destroy(aria_mesh_t h) { stage_destroy(h); }

void* aria_mesh_stream(aria_mesh_t h) { return stage_stream(h); }

int aria_mesh_check(aria_mesh_t h) {
    return stage_check(h, {{ERRBIT_MESH_OVERFLOW, ARIA_E_OVERFLOW}, {ERRBIT_MESH_CAP, ARIA_E_OUTPUT_TOO_SMALL}});
}

int aria_mesh_update_from_volume_device(aria_mesh_t h, const aria_tsdf_voxel* d_voxels) {
    if (!h || !d_voxels) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const unsigned long long* vol = reinterpret_cast<const unsigned long long*>(d_voxels);
    hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)h->n_chunks), dim3(MESH_BLOCK), 0, h->stream, vol, h->G, h->d_words, h->d_vcount,
                       h->d_tcount);
    ARIA_HIP(hipGetLastError());
    h->d_vol = vol;
    return ARIA_OK;
}

int aria_mesh_extract_device(aria_mesh_t h, aria_mesh_vertex* d_vertices, int64_t vcap, aria_mesh_triangle* d_triangles, int64_t tcap,
                             int64_t* d_counts) {
    if (!h || mesh_bad_outputs(d_vertices, vcap, d_triangles, tcap, d_counts)) return ARIA_E_INVALID;
    if (!h->d_vol) return ARIA_E_INVALID;                               // no update yet
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_SCAN_BLOCK), 0, h->stream, (const int*)h->d_vcount, (const int*)h->d_tcount,
                       h->n_chunks, h->d_voff, h->d_toff, (long long)vcap, (long long)tcap, (long long*)d_counts, h->d_err);
    ARIA_HIP(hipGetLastError());
    if (vcap > 0 || tcap > 0) {
        hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)h->n_chunks), dim3(MESH_BLOCK), 0, h->stream, h->d_vol, h->G,
                           (const uint32_t*)h->d_words, (const int*)h->d_vcount, (const int*)h->d_tcount, (const long long*)h->d_voff,
                           (const long long*)h->d_toff, d_vertices, (long long)vcap, d_triangles, (long long)tcap);
        ARIA_HIP(hipGetLastError());
    }
    return ARIA_OK;
}

int aria_mesh_extract(aria_mesh_t h, aria_mesh_vertex* vertices, int64_t vcap, aria_mesh_triangle* triangles, int64_t tcap,
                      int64_t* counts) {
    if (!h || mesh_bad_outputs(vertices, vcap, triangles, tcap, counts)) return ARIA_E_INVALID;
    if (!h->d_vol) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if (vcap > 0 && (rc = h->d_vertices.reserve(h->stream, (size_t)vcap)) != ARIA_OK) return rc;
    if (tcap > 0 && (rc = h->d_triangles.reserve(h->stream, (size_t)tcap)) != ARIA_OK) return rc;
    if ((rc = aria_mesh_extract_device(h, vcap > 0 ? (aria_mesh_vertex*)h->d_vertices : nullptr, vcap,
                                       tcap > 0 ? (aria_mesh_triangle*)h->d_triangles : nullptr, tcap, h->d_counts)) != ARIA_OK)
        return rc;
    long long n[2] = {0, 0};
    ARIA_HIP(memcpy_on(h->stream, n, h->d_counts, sizeof(n), hipMemcpyDeviceToHost));
    counts[0] = n[0];
    counts[1] = n[1];
    const int64_t nv = std::min<int64_t>(n[0], vcap), nt = std::min<int64_t>(n[1], tcap);
    if (nv > 0) ARIA_HIP(memcpy_on(h->stream, vertices, h->d_vertices, sizeof(aria_mesh_vertex) * (size_t)nv, hipMemcpyDeviceToHost));
    if (nt > 0) ARIA_HIP(memcpy_on(h->stream, triangles, h->d_triangles, sizeof(aria_mesh_triangle) * (size_t)nt, hipMemcpyDeviceToHost));
    return aria_mesh_check(h);
}

}  // extern "C"
