// Path planning: a 2-D traversability grid collapsed out of a height band of the TSDF volume, an exact clearance field and an
// integer cost map, exact cost-to-go fields for a batch of goals and paths traced for a batch of queries. Semantics in
// include/aria_orb_hip.h ("path planning"); aria_slam_amd/nav_ref.py is the definition and this file equals it bit for bit.
// Everything is integer arithmetic except the one fp32 compare of rule 2.
//
// k_nav_columns    a lane per cell, walking the band of its column of voxels. Consecutive lanes are consecutive u, and for
//                  up_axis 1 and 2 the plane axis U is the volume's x: every step of the walk is one coalesced run of 8-byte
//                  records. For up_axis 0 a lane walks along x itself (one lane per 64-byte line and step): slower, correct.
// k_nav_validate   set_cells: any value above 2 raises the call's refusal word and the deferred-error bit.
// k_nav_adopt      set_cells: the new cells replace the old ones unless the refusal word is set.
// k_nav_span       clearance, column pass: the distance |dv| <= R to the nearest OCCUPIED cell of the same u, 255 = none.
// k_nav_clearance  clearance, row pass: d2 = min over |du| <= R of du*du + span(u + du, v)^2. The two passes give the
//                  brute-force window's minimum exactly, in 2 (2R + 1) reads per cell instead of (2R + 1)^2.
// k_nav_cost       rule 4.
// k_nav_moves      rule 5 per cell: the cost and the 8-bit set of allowed moves packed in one word, so that the field and trace
//                  kernels decide a move from one load.
// k_nav_trace      a lane per query: rule 7 over the finished fields.
// k_nav_field      one workgroup per goal, persistent until its field stops changing (below, "goal fields").
// Plain HIP C++. The text from "namespace {" to the goal-field section also compiles for the host
// (tests/test_nav_kernel_emulation.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_nav_record) == 16, "aria_nav_record is 16 bytes");
static_assert(sizeof(aria_nav_config) == 104, "aria_nav_config is 104 bytes");

namespace {

constexpr int NAV_BLOCK = 256;
constexpr int NAV_MAX_DIM = 1024, NAV_MAX_RADIUS = 64, NAV_MAX_PENALTY = 1000, NAV_MAX_GOALS = 65535;
constexpr uint32_t NAV_INF = 0x7FFFFFFFu, NAV_BLOCKED = 0xFFFFu;
constexpr int NAV_NO_SPAN = 255;
constexpr int ERRBIT_NAV_INPUT = 1, ERRBIT_NAV_FIELD = 2, ERRBIT_NAV_CAP = 4;

// What the kernels take by value.
struct NavParams {
    int nx, ny, nz, up_axis, band0, band1;
    int nu, nv;
    int min_weight, occ_count, free_count;
    int radius, block_d2, soft_d2, penalty, unknown_penalty, allow_unknown;
    float occ_tsdf;
};

// grid: cells / 256
__global__ __launch_bounds__(NAV_BLOCK) void k_nav_columns(NavParams P, const unsigned long long* __restrict__ vol, uint8_t* __restrict__ cells) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= P.nu * P.nv) return;
    const int v = c / P.nu, u = c - v * P.nu;
    // voxel (i, j, k) lies at (k*ny + j)*nx + i; (U, V) are the two axes other than up_axis, ascending
    size_t base, stride;
    if (P.up_axis == 0) { base = ((size_t)v * P.ny + u) * P.nx; stride = 1; }
    else if (P.up_axis == 1) { base = (size_t)v * P.ny * P.nx + u; stride = (size_t)P.nx; }
    else { base = (size_t)v * P.nx + u; stride = (size_t)P.nx * P.ny; }
    int n_seen = 0, n_solid = 0;
    for (int b = P.band0; b < P.band1; b++) {
        const unsigned long long rec = vol[base + (size_t)b * stride];
        const bool seen = (int)((uint32_t)(rec >> 32) & 0xFFFFu) >= P.min_weight;
        n_seen += seen ? 1 : 0;
        n_solid += seen && __uint_as_float((uint32_t)rec) < P.occ_tsdf ? 1 : 0;
    }
    cells[c] = (uint8_t)(n_solid >= P.occ_count ? 1 : n_seen >= P.free_count ? 0 : 2);
}

__global__ __launch_bounds__(NAV_BLOCK) void k_nav_validate(const uint8_t* __restrict__ in, int n, int* bad, int* err) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= n || in[c] <= 2) return;
    atomicOr(bad, 1);
    atomicOr(err, ERRBIT_NAV_INPUT);
}

__global__ __launch_bounds__(NAV_BLOCK) void k_nav_adopt(const uint8_t* __restrict__ in, int n, const int* __restrict__ bad, uint8_t* __restrict__ cells) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= n || *bad) return;
    cells[c] = in[c];
}

__global__ __launch_bounds__(NAV_BLOCK) void k_nav_span(NavParams P, const uint8_t* __restrict__ cells, uint8_t* __restrict__ span) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= P.nu * P.nv) return;
    const int v = c / P.nu;
    int best = NAV_NO_SPAN;
    for (int d = 0; d <= P.radius && best == NAV_NO_SPAN; d++) {
        const bool lo = v - d >= 0 && cells[c - d * P.nu] == 1;
        const bool hi = v + d < P.nv && cells[c + d * P.nu] == 1;
        if (lo || hi) best = d;
    }
    span[c] = (uint8_t)best;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_nav_clearance(NavParams P, const uint8_t* __restrict__ span, uint16_t* __restrict__ d2) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= P.nu * P.nv) return;
    const int v = c / P.nu, u = c - v * P.nu;
    int best = (P.radius + 1) * (P.radius + 1);
    const int lo = max(-P.radius, -u), hi = min(P.radius, P.nu - 1 - u);
    for (int du = lo; du <= hi; du++) {
        const int s = span[c + du];
        if (s != NAV_NO_SPAN) best = min(best, du * du + s * s);
    }
    d2[c] = (uint16_t)best;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_nav_cost(NavParams P, const uint8_t* __restrict__ cells, const uint16_t* __restrict__ d2,
                                                        uint16_t* __restrict__ cost) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= P.nu * P.nv) return;
    const int state = cells[c], d = d2[c];
    const bool blocked = state == 1 || d < P.block_d2 || (state == 2 && !P.allow_unknown);
    const int pen = (d < P.soft_d2 ? P.penalty * (P.soft_d2 - d) / P.soft_d2 : 0) + (state == 2 ? P.unknown_penalty : 0);
    cost[c] = (uint16_t)(blocked ? NAV_BLOCKED : (uint32_t)pen);
}

// Move m = 0..7: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1); base 10 for m < 4, else 14.
__device__ __forceinline__ int nav_du(int m) { return m < 2 ? 1 - 2 * m : m < 4 ? 0 : 1 - 2 * (m & 1); }
__device__ __forceinline__ int nav_dv(int m) { return m < 2 ? 0 : m < 4 ? 5 - 2 * m : m < 6 ? 1 : -1; }

// cm[c] = cost | moves << 16: bit m of `moves` is set when move m out of c is allowed (c itself may be blocked).
__global__ __launch_bounds__(NAV_BLOCK) void k_nav_moves(int nu, int nv, const uint16_t* __restrict__ cost, uint32_t* __restrict__ cm) {
    const int c = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (c >= nu * nv) return;
    const int v = c / nu, u = c - v * nu;
    uint32_t moves = 0;
    for (int m = 0; m < 8; m++) {
        const int du = nav_du(m), dv = nav_dv(m);
        const int bu = u + du, bv = v + dv;
        if (bu < 0 || bu >= nu || bv < 0 || bv >= nv) continue;
        bool ok = cost[bv * nu + bu] != NAV_BLOCKED;
        if (m >= 4) ok = ok && cost[v * nu + bu] != NAV_BLOCKED && cost[bv * nu + u] != NAV_BLOCKED;
        moves |= ok ? 1u << m : 0u;
    }
    cm[c] = (uint32_t)cost[c] | moves << 16;
}

// A lane per query. Every step reads cells the allowed-move bits vouch for, and the walk is bounded by the number of cells.
__global__ __launch_bounds__(NAV_BLOCK) void k_nav_trace(int nu, int nv, const uint32_t* __restrict__ cm, const uint16_t* __restrict__ d2,
                                                         const int32_t* __restrict__ fields, const int32_t* __restrict__ goals, int n_goals,
                                                         const int32_t* __restrict__ queries, int n_queries,
                                                         aria_nav_record* __restrict__ records, int32_t* __restrict__ paths, int path_cap,
                                                         int* err) {
    const int q = (int)(blockIdx.x * NAV_BLOCK + threadIdx.x);
    if (q >= n_queries) return;
    const int su = queries[3 * q], sv = queries[3 * q + 1], gi = queries[3 * q + 2];
    aria_nav_record r;
    r.cost = (int32_t)NAV_INF; r.n_cells = 0; r.min_d2 = 0; r.status = 2;
    bool inside = su >= 0 && su < nu && sv >= 0 && sv < nv && gi >= 0 && gi < n_goals;
    int gu = 0, gv = 0;
    if (inside) {
        gu = goals[2 * gi]; gv = goals[2 * gi + 1];
        inside = gu >= 0 && gu < nu && gv >= 0 && gv < nv;
    }
    if (!inside) { records[q] = r; return; }
    const int32_t* D = fields + (size_t)gi * nu * nv;
    int c = sv * nu + su;
    const int g = gv * nu + gu;
    uint32_t Dc = (uint32_t)D[c];
    if (Dc == NAV_INF) { r.status = 1; records[q] = r; return; }
    r.cost = (int32_t)Dc;
    int n = 0, lo = d2[c];
    for (;;) {
        if (n < path_cap) paths[(size_t)q * path_cap + n] = c;
        n++;
        lo = min(lo, (int)d2[c]);
        if (c == g) break;
        if (n >= nu * nv) { atomicOr(err, ERRBIT_NAV_FIELD); break; }
        const uint32_t moves = cm[c] >> 16;
        int next = -1;
        uint32_t Dn = 0;
        for (int m = 0; m < 8 && next < 0; m++) {
            if (!(moves >> m & 1u)) continue;
            const int b = c + nav_dv(m) * nu + nav_du(m);
            const uint32_t Db = (uint32_t)D[b];
            if (Db != NAV_INF && (m < 4 ? 10u : 14u) + (cm[b] & 0xFFFFu) + Db == Dc) { next = b; Dn = Db; }
        }
        if (next < 0) { atomicOr(err, ERRBIT_NAV_FIELD); break; }      // the field is not rule 6's
        c = next; Dc = Dn;
    }
    r.n_cells = n; r.min_d2 = lo; r.status = n > path_cap ? 3 : 0;
    if (n > path_cap) atomicOr(err, ERRBIT_NAV_CAP);
    records[q] = r;
}

// ---- goal fields --------------------------------------------------------------------------------------------------------
// Rule 6 has one least solution, so any schedule of relaxations that reaches a fixed point reaches THAT field, bit for bit.
// The kernel keeps E(c) = D(c) + pen(c), so that a relaxation is E(c) = pen(c) + min over allowed m of base(m) + E(b): one word
// of cm and up to eight words of E. Every value ever stored is the cost of a real path (never below the solution) and values only
// fall; when a whole round changes nothing every cell satisfies rule 6 with the values it read, which is the fixed point.
//
// Schedule: fast sweeping. A round is a row phase (a lane per row: u ascending, then descending) and a column phase (a lane per
// column: v ascending, then descending) with a barrier between; within a phase a cell is written by its owner only, and a
// neighbour read while its owner writes it gives the old or the new word, both valid. A straight or diagonal run of any length is
// settled by one sweep, so a round count follows the number of turns of the longest shortest path, not its length. The field sits
// in LDS with a row pitch of nu + 1 words when that fits (lanes of a row phase are nu + 1 words apart, lanes of a column phase one
// word: 32 distinct banks either way), else in the field buffer in HBM. `plain` (variants build) replaces the round by one sweep
// in which every lane relaxes every 256th cell, in HBM: the yardstick tools/nav_rate.py measures the schedule against.
// Rounds are bounded by nu*nv + 1: round k settles every cell whose shortest path has k cells, one more round sees no change.
constexpr int NAV_LDS_BYTES = 160 * 1024;

// The LDS copy is addressed through its own address space, so that the relaxations are ds_read / ds_write and not flat accesses.
typedef volatile uint32_t* nav_hbm_ptr;
typedef volatile __attribute__((address_space(3))) uint32_t* nav_lds_ptr;

template <typename Ptr>
__device__ __forceinline__ bool nav_relax(Ptr E, const uint32_t* __restrict__ cm, int c, int e, int pitch) {
    const uint32_t w = cm[c], pen = w & 0xFFFFu;
    if (pen == NAV_BLOCKED) return false;
    uint32_t best = NAV_INF;                                             // NAV_INF + 14 + 65534 does not wrap
    if (w & (1u << 16)) best = min(best, E[e + 1] + 10u);
    if (w & (1u << 17)) best = min(best, E[e - 1] + 10u);
    if (w & (1u << 18)) best = min(best, E[e + pitch] + 10u);
    if (w & (1u << 19)) best = min(best, E[e - pitch] + 10u);
    if (w & (1u << 20)) best = min(best, E[e + pitch + 1] + 14u);
    if (w & (1u << 21)) best = min(best, E[e + pitch - 1] + 14u);
    if (w & (1u << 22)) best = min(best, E[e - pitch + 1] + 14u);
    if (w & (1u << 23)) best = min(best, E[e - pitch - 1] + 14u);
    best += pen;
    if (best >= E[e]) return false;
    E[e] = best;
    return true;
}

template <bool LDS>
__global__ __launch_bounds__(NAV_BLOCK) void k_nav_field(int nu, int nv, const uint32_t* __restrict__ cm, const int32_t* __restrict__ goals,
                                                         int32_t* __restrict__ fields, int* __restrict__ rounds, int max_rounds, int plain,
                                                         int* err) {
    extern __shared__ uint32_t s_E[];
    __shared__ int s_changed[3];                                         // round r raises [r % 3] and clears [(r + 2) % 3]
    const int t = (int)threadIdx.x, n = nu * nv;
    int32_t* D = fields + (size_t)blockIdx.x * n;
    const int pitch = LDS ? nu + 1 : nu;
    typename std::conditional<LDS, nav_lds_ptr, nav_hbm_ptr>::type E;
    if constexpr (LDS) E = (nav_lds_ptr)s_E; else E = reinterpret_cast<uint32_t*>(D);
    const int gu = goals[2 * blockIdx.x], gv = goals[2 * blockIdx.x + 1];
    const bool goal_in = gu >= 0 && gu < nu && gv >= 0 && gv < nv;
    const bool goal_ok = goal_in && (cm[goal_in ? gv * nu + gu : 0] & 0xFFFFu) != NAV_BLOCKED;
    if (!goal_ok) {                                                      // the same for every lane: no barrier is skipped
        for (int c = t; c < n; c += NAV_BLOCK) D[c] = (int32_t)NAV_INF;
        if (t == 0) rounds[blockIdx.x] = 0;
        return;
    }
    for (int c = t; c < n; c += NAV_BLOCK) E[(c / nu) * pitch + c % nu] = NAV_INF;
    __syncthreads();
    if (t == 0) {
        E[gv * pitch + gu] = cm[gv * nu + gu] & 0xFFFFu;                 // D(g) = 0
        s_changed[0] = s_changed[1] = s_changed[2] = 0;
    }
    __syncthreads();
    int r = 0;
    bool settled = false;
    while (r < max_rounds) {
        bool changed = false;
        if (plain) {
            for (int c = t; c < n; c += NAV_BLOCK) changed |= nav_relax(E, cm, c, (c / nu) * pitch + c % nu, pitch);
        } else {
            for (int v = t; v < nv; v += NAV_BLOCK) {
                for (int u = 0; u < nu; u++) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                for (int u = nu - 2; u >= 0; u--) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
            }
            __syncthreads();
            for (int u = t; u < nu; u += NAV_BLOCK) {
                for (int v = 0; v < nv; v++) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
                for (int v = nv - 2; v >= 0; v--) changed |= nav_relax(E, cm, v * nu + u, v * pitch + u, pitch);
            }
        }
        // one barrier a round: the word of round r + 2 is cleared behind barrier r and raised in front of barrier r + 2 only
        if (changed) s_changed[r % 3] = 1;
        __syncthreads();
        const int any = s_changed[r % 3];
        if (t == 0) s_changed[(r + 2) % 3] = 0;
        r++;
        if (!any) { settled = true; break; }
    }
    for (int c = t; c < n; c += NAV_BLOCK) {
        const uint32_t e = E[(c / nu) * pitch + c % nu];
        D[c] = e >= NAV_INF ? (int32_t)NAV_INF : (int32_t)(e - (cm[c] & 0xFFFFu));
    }
    if (t == 0) {
        rounds[blockIdx.x] = r;
        if (!settled) atomicOr(err, ERRBIT_NAV_FIELD);
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_nav_s : StageHandle {
    aria_nav_config cfg{};
    NavParams P{};
    int n = 0;                                                 // cells
    bool lds = false;                                          // the field of one goal fits the LDS of a CU
    size_t lds_bytes = 0;
    int plain = 0;                                             // variants build: ARIA_NAV_SCHEDULE=plain
    bool stale = true;                                         // the map changed since the last solve (or there was none)
    int n_goals = 0;
    DeviceBuffer<uint8_t> d_cells, d_span;
    DeviceBuffer<uint16_t> d_d2, d_cost;
    DeviceBuffer<uint32_t> d_cm;
    DeviceBuffer<int32_t> d_fields;                            // max_goals x nv x nu
    DeviceBuffer<int32_t> d_goals;                             // 2 x max_goals: the goals of the last solve
    DeviceBuffer<int> d_rounds;                                // max_goals
    DeviceBuffer<int> d_bad;                                   // the refusal word of a set_cells call
    // host-form staging (grow-only)
    DeviceBuffer<uint8_t> d_in;
    DeviceBuffer<int32_t> d_queries, d_paths;
    DeviceBuffer<aria_nav_record> d_records;
};

namespace {

bool nav_bad_dims(int nx, int ny, int nz) {
    for (int n : {nx, ny, nz})
        if (n < 8 || n > NAV_MAX_DIM || n % 8) return true;
    return false;
}

bool nav_bad_config(const aria_nav_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_nav_config)) return true;
    if (nav_bad_dims(c->nx, c->ny, c->nz) || c->up_axis < 0 || c->up_axis > 2) return true;
    const int n_up = c->up_axis == 0 ? c->nx : c->up_axis == 1 ? c->ny : c->nz;
    if (c->band0 < 0 || c->band0 >= c->band1 || c->band1 > n_up) return true;
    if (c->min_weight < 1 || c->min_weight > 65535 || !std::isfinite(c->occ_tsdf)) return true;
    if (c->occ_count < 1 || c->occ_count > NAV_MAX_DIM || c->free_count < 1 || c->free_count > NAV_MAX_DIM) return true;
    if (c->clear_radius < 0 || c->clear_radius > NAV_MAX_RADIUS) return true;
    const int cap = (c->clear_radius + 1) * (c->clear_radius + 1);
    if (c->block_d2 < 0 || c->block_d2 > c->soft_d2 || c->soft_d2 > cap || c->soft_d2 < 1) return true;
    if (c->penalty < 0 || c->penalty > NAV_MAX_PENALTY || c->unknown_penalty < 0 || c->unknown_penalty > NAV_MAX_PENALTY) return true;
    if (c->allow_unknown < 0 || c->allow_unknown > 1 || c->max_goals < 1 || c->max_goals > NAV_MAX_GOALS) return true;
    if (!(c->voxel > 0) || !std::isfinite(c->voxel)) return true;
    for (float v : c->origin)
        if (!std::isfinite(v)) return true;
    return false;
}

unsigned nav_blocks(int n) { return (unsigned)((n + NAV_BLOCK - 1) / NAV_BLOCK); }

// Rules 3-5 on the cells the handle holds; enqueued.
int nav_rebuild(aria_nav_s* h) {
    const dim3 grid(nav_blocks(h->n)), block(NAV_BLOCK);
    hipLaunchKernelGGL(k_nav_span, grid, block, 0, h->stream, h->P, (const uint8_t*)h->d_cells, h->d_span);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nav_clearance, grid, block, 0, h->stream, h->P, (const uint8_t*)h->d_span, h->d_d2);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nav_cost, grid, block, 0, h->stream, h->P, (const uint8_t*)h->d_cells, (const uint16_t*)h->d_d2, h->d_cost);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nav_moves, grid, block, 0, h->stream, h->P.nu, h->P.nv, (const uint16_t*)h->d_cost, h->d_cm);
    ARIA_HIP(hipGetLastError());
    h->stale = true;
    return ARIA_OK;
}

int nav_read(aria_nav_s* h, void* out, const void* src, size_t bytes) {
    if (!h || !out) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(memcpy_on(h->stream, out, src, bytes, hipMemcpyDeviceToHost));
    return ARIA_OK;
}

}  // namespace

extern "C" {

void aria_nav_default_config(aria_nav_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_nav_config);
    c->nx = 256; c->ny = 256; c->nz = 128;                               // the TSDF defaults
    c->up_axis = 1;
    c->band0 = c->ny / 2 - 8; c->band1 = c->ny / 2 + 16;
    c->min_weight = 2; c->occ_tsdf = 0.0f; c->occ_count = 1; c->free_count = 1;
    c->clear_radius = 8; c->block_d2 = 16; c->soft_d2 = 64; c->penalty = 20; c->unknown_penalty = 10; c->allow_unknown = 1;
    c->max_goals = 256;
    c->voxel = 0.05f;
    c->origin[0] = -6.4f; c->origin[1] = -6.4f; c->origin[2] = 0.0f;
}

int64_t aria_nav_field_bytes(int nu, int nv, int max_goals) {
    if (nav_bad_dims(nu, nv, 8) || max_goals < 1 || max_goals > NAV_MAX_GOALS) return ARIA_E_INVALID;
    return (int64_t)4 * nu * nv * max_goals;
}

int aria_nav_create(const aria_nav_config* c, aria_nav_t* out) {
    if (!out || nav_bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_nav_create", [](aria_nav_s* h) {
        const aria_nav_config& c = h->cfg;
        const char* what = "aria_nav_create";
        NavParams& P = h->P;
        P.nx = c.nx; P.ny = c.ny; P.nz = c.nz; P.up_axis = c.up_axis; P.band0 = c.band0; P.band1 = c.band1;
        P.nu = c.up_axis == 0 ? c.ny : c.nx;
        P.nv = c.up_axis == 2 ? c.ny : c.nz;
        P.min_weight = c.min_weight; P.occ_count = c.occ_count; P.free_count = c.free_count; P.occ_tsdf = c.occ_tsdf;
        P.radius = c.clear_radius; P.block_d2 = c.block_d2; P.soft_d2 = c.soft_d2; P.penalty = c.penalty;
        P.unknown_penalty = c.unknown_penalty; P.allow_unknown = c.allow_unknown;
        h->n = P.nu * P.nv;
        h->lds_bytes = (size_t)4 * (P.nu + 1) * P.nv;
        h->lds = h->lds_bytes + 64 <= (size_t)NAV_LDS_BYTES;             // 64: the changed words and alignment
        if (const char* s = aria_getenv("ARIA_NAV_SCHEDULE")) h->plain = !std::strcmp(s, "plain");   // variants build: A/B
        if (h->plain) h->lds = false;
        const size_t n = (size_t)h->n, goals = (size_t)c.max_goals;
        int rc;
        if ((rc = h->d_cells.reserve(h->stream, n, what)) != ARIA_OK) return rc;
        if ((rc = h->d_span.reserve(h->stream, n, what)) != ARIA_OK) return rc;
        if ((rc = h->d_d2.reserve(h->stream, n, what)) != ARIA_OK) return rc;
        if ((rc = h->d_cost.reserve(h->stream, n, what)) != ARIA_OK) return rc;
        if ((rc = h->d_cm.reserve(h->stream, n, what)) != ARIA_OK) return rc;
        if ((rc = h->d_fields.reserve(h->stream, n * goals, what)) != ARIA_OK) return rc;
        if ((rc = h->d_goals.reserve(h->stream, 2 * goals, what)) != ARIA_OK) return rc;
        if ((rc = h->d_rounds.reserve(h->stream, goals, what)) != ARIA_OK) return rc;
        if ((rc = h->d_bad.reserve(h->stream, 1, what)) != ARIA_OK) return rc;
        // a property of the function, not of the handle: always the most the stage uses, so that handles of different planes
        // cannot lower it under one another
        hipError_t e = hipSuccess;
        if (h->lds)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nav_field<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    NAV_LDS_BYTES - 64);
        if (e == hipSuccess) e = hipMemsetAsync(h->d_cells, 2, n, h->stream);                // a new handle: every cell UNKNOWN
        if (e == hipSuccess) e = hipMemsetAsync(h->d_rounds, 0, sizeof(int) * goals, h->stream);
        if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
        return nav_rebuild(h);
    });
}

void aria_nav_destroy(aria_nav_t h) { stage_destroy(h); }

void* aria_nav_stream(aria_nav_t h) { return stage_stream(h); }

int aria_nav_check(aria_nav_t h) {
    return stage_check(h, {{ERRBIT_NAV_INPUT, ARIA_E_INVALID}, {ERRBIT_NAV_FIELD, ARIA_E_OVERFLOW}, {ERRBIT_NAV_CAP, ARIA_E_OUTPUT_TOO_SMALL}});
}

int aria_nav_update_from_volume_device(aria_nav_t h, const aria_tsdf_voxel* d_voxels) {
    if (!h || !d_voxels) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_nav_columns, dim3(nav_blocks(h->n)), dim3(NAV_BLOCK), 0, h->stream, h->P,
                       reinterpret_cast<const unsigned long long*>(d_voxels), h->d_cells);
    ARIA_HIP(hipGetLastError());
    return nav_rebuild(h);
}

int aria_nav_set_cells_device(aria_nav_t h, const uint8_t* d_cells) {
    if (!h || !d_cells) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(hipMemsetAsync(h->d_bad, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_nav_validate, dim3(nav_blocks(h->n)), dim3(NAV_BLOCK), 0, h->stream, d_cells, h->n, h->d_bad, h->d_err);
    ARIA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nav_adopt, dim3(nav_blocks(h->n)), dim3(NAV_BLOCK), 0, h->stream, d_cells, h->n, (const int*)h->d_bad, h->d_cells);
    ARIA_HIP(hipGetLastError());
    return nav_rebuild(h);
}

int aria_nav_set_cells(aria_nav_t h, const uint8_t* cells) {
    if (!h || !cells) return ARIA_E_INVALID;
    for (int c = 0; c < h->n; c++)
        if (cells[c] > 2) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_in.reserve(h->stream, (size_t)h->n)) != ARIA_OK) return rc;
    ARIA_HIP(memcpy_on(h->stream, h->d_in, cells, (size_t)h->n, hipMemcpyHostToDevice));
    if ((rc = aria_nav_set_cells_device(h, h->d_in)) != ARIA_OK) return rc;
    return aria_nav_check(h);
}

int aria_nav_read_cells(aria_nav_t h, uint8_t* out) { return nav_read(h, out, h ? h->d_cells.p : nullptr, h ? (size_t)h->n : 0); }
int aria_nav_read_clearance(aria_nav_t h, uint16_t* out) { return nav_read(h, out, h ? h->d_d2.p : nullptr, h ? (size_t)h->n * 2 : 0); }
int aria_nav_read_costs(aria_nav_t h, uint16_t* out) { return nav_read(h, out, h ? h->d_cost.p : nullptr, h ? (size_t)h->n * 2 : 0); }

int aria_nav_solve_device(aria_nav_t h, const int32_t* d_goals, int n_goals) {
    if (!h || n_goals < 0 || n_goals > h->cfg.max_goals || (n_goals > 0 && !d_goals)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    if (n_goals > 0) {
        ARIA_HIP(hipMemcpyAsync(h->d_goals, d_goals, sizeof(int32_t) * 2 * (size_t)n_goals, hipMemcpyDeviceToDevice, h->stream));
        const int max_rounds = h->n + 1;
        if (h->lds)
            hipLaunchKernelGGL(k_nav_field<true>, dim3((unsigned)n_goals), dim3(NAV_BLOCK), h->lds_bytes, h->stream, h->P.nu, h->P.nv,
                               (const uint32_t*)h->d_cm, (const int32_t*)h->d_goals, h->d_fields, h->d_rounds, max_rounds, 0, h->d_err);
        else
            hipLaunchKernelGGL(k_nav_field<false>, dim3((unsigned)n_goals), dim3(NAV_BLOCK), 0, h->stream, h->P.nu, h->P.nv,
                               (const uint32_t*)h->d_cm, (const int32_t*)h->d_goals, h->d_fields, h->d_rounds, max_rounds, h->plain, h->d_err);
        ARIA_HIP(hipGetLastError());
    }
    h->n_goals = n_goals;
    h->stale = false;
    return ARIA_OK;
}

int aria_nav_trace_device(aria_nav_t h, const int32_t* d_queries, int n_queries, aria_nav_record* d_records, int32_t* d_paths, int path_cap) {
    if (!h || n_queries < 0 || path_cap < 0 || (n_queries > 0 && (!d_queries || !d_records)) || (path_cap > 0 && n_queries > 0 && !d_paths))
        return ARIA_E_INVALID;
    if (h->stale) return ARIA_E_INVALID;                                 // the fields are not of this map
    if (n_queries == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_nav_trace, dim3(nav_blocks(n_queries)), dim3(NAV_BLOCK), 0, h->stream, h->P.nu, h->P.nv, (const uint32_t*)h->d_cm,
                       (const uint16_t*)h->d_d2, (const int32_t*)h->d_fields, (const int32_t*)h->d_goals, h->n_goals, d_queries, n_queries,
                       d_records, d_paths, path_cap, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_nav_plan(aria_nav_t h, const int32_t* goals, int n_goals, const int32_t* queries, int n_queries, aria_nav_record* records,
                  int32_t* paths, int path_cap) {
    if (!h || n_goals < 0 || n_goals > h->cfg.max_goals || n_queries < 0 || path_cap < 0 || (n_goals > 0 && !goals) ||
        (n_queries > 0 && (!queries || !records)) || (path_cap > 0 && n_queries > 0 && !paths))
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    const size_t n_paths = (size_t)n_queries * (size_t)path_cap;
    // the goals are staged in the query buffer, in front of the queries
    if ((rc = h->d_queries.reserve(h->stream, 2 * (size_t)n_goals + 3 * (size_t)n_queries + 1)) != ARIA_OK) return rc;
    if ((rc = h->d_records.reserve(h->stream, (size_t)n_queries + 1)) != ARIA_OK) return rc;
    if ((rc = h->d_paths.reserve(h->stream, n_paths + 1)) != ARIA_OK) return rc;
    int32_t* d_g = h->d_queries;
    int32_t* d_q = d_g + 2 * (size_t)n_goals;
    if (n_goals) ARIA_HIP(hipMemcpyAsync(d_g, goals, sizeof(int32_t) * 2 * (size_t)n_goals, hipMemcpyHostToDevice, h->stream));
    if (n_queries) ARIA_HIP(hipMemcpyAsync(d_q, queries, sizeof(int32_t) * 3 * (size_t)n_queries, hipMemcpyHostToDevice, h->stream));
    if (n_paths) ARIA_HIP(hipMemcpyAsync(h->d_paths, paths, sizeof(int32_t) * n_paths, hipMemcpyHostToDevice, h->stream));   // what is not written keeps its bytes
    ARIA_HIP(hipStreamSynchronize(h->stream));                           // the host arrays are free again
    if ((rc = aria_nav_solve_device(h, d_g, n_goals)) != ARIA_OK) return rc;
    if ((rc = aria_nav_trace_device(h, d_q, n_queries, h->d_records, h->d_paths, path_cap)) != ARIA_OK) return rc;
    if (n_queries) ARIA_HIP(hipMemcpyAsync(records, h->d_records, sizeof(aria_nav_record) * (size_t)n_queries, hipMemcpyDeviceToHost, h->stream));
    if (n_paths) ARIA_HIP(hipMemcpyAsync(paths, h->d_paths, sizeof(int32_t) * n_paths, hipMemcpyDeviceToHost, h->stream));
    return aria_nav_check(h);
}

int32_t* aria_nav_device_fields(aria_nav_t h) { return h ? h->d_fields.p : nullptr; }

int aria_nav_read_field(aria_nav_t h, int g, int32_t* out) {
    if (!h || !out || h->stale || g < 0 || g >= h->n_goals) return ARIA_E_INVALID;
    return nav_read(h, out, h->d_fields + (size_t)g * h->n, (size_t)h->n * 4);
}

int aria_nav_read_rounds(aria_nav_t h, int32_t* out, int n_goals) {
    if (!h || !out || h->stale || n_goals < 0 || n_goals > h->n_goals) return ARIA_E_INVALID;
    if (n_goals == 0) return ARIA_OK;
    return nav_read(h, out, h->d_rounds, sizeof(int32_t) * (size_t)n_goals);
}

}  // extern "C"
