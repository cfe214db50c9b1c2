// Sim(3) pose-graph optimisation and the map correction after a loop (include/aria_orb_hip.h, "Sim(3) pose-graph
// optimisation"): the roles of ORB-SLAM's OptimizeEssentialGraph and CorrectLoop. The reference has no code for either;
// aria_slam_amd/sgraph_ref.py is the specification, DESIGN.md section 32 the record.
//
// k_sgraph_lm: the schedule, its pieces and the host calls around the kernel are those of graph_lm_device.h (one workgroup per
// graph, persistent over every LM iteration), instantiated with 7 x 7 blocks and 13-double vertices (R, t, s). Specific to this
// stage, and written here:
//   validation    an edge's scale and every vertex's scale must be positive and finite (checked after the indices).
//   edge_blocks   e and the 7 x 7 Jacobians of a Sim(3) edge; only their non-zero entries enter a sum (ji_nz, jj_nz), and W has
//                 31 entries that are not structurally zero (w_nz). fix_scale pins the scale column and the scale error to 0.
//   vertex_update S <- S * D(d), the scale through scale_of.
//   the solve     ONE form, pcg_solve of the shared header, which holds for any size. The register and LDS forms of k_graph_lm
//                 (pcg_small) are not built (DESIGN.md section 32 says what they would take).
//   FRESH         the scratch strides go through lm_stride's opaque copy: without it this kernel spills (tests/test_sgraph_host.py).
// The kernel body itself is written out here and in graph_optimize.hip: graph_lm_device.h records why.
//
// k_sgraph_correct moves the arena's points, k_sgraph_from_pose and k_sgraph_to_pose copy between pose rows and vertices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "graph_lm_device.h"
#include "solver_device.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int SG_BLOCK = 512;             // 8 waves: 2 per SIMD, 256 VGPRs each
constexpr int SG_WAVES = SG_BLOCK / 64;
constexpr int ERRBIT_SG_INPUT = 1;        // counts, fixed index, an edge or a scale out of range (graph skipped); a refused point
constexpr int ERRBIT_SG_LARGE = 2;        // more vertices or edges than the handle was created for (graph skipped)
constexpr int NB = 7, NB2 = 49;           // block size
constexpr int VDBL = 13;                  // doubles of an aria_sgraph_vertex
constexpr int CORRECT_BLOCK = 256;

static_assert(sizeof(aria_sgraph_vertex) == VDBL * sizeof(double), "aria_sgraph_vertex is 13 doubles");
static_assert(sizeof(aria_sgraph_edge) == 120 && sizeof(aria_sgraph_correct_stats) == 16 && sizeof(aria_sgraph_result) == 48, "layouts");

// vertex (R[9], t[3], s) -> R[9], t[3]; returns s
__device__ inline double load_vertex(const double* S, double* R, double* t) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = S[c];
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = S[9 + c];
    return S[12];
}

// ---- the sparsity of the 7 x 7 Jacobians (sgraph_ref.py, "Jacobians") ------------------------------------------------------------
// Ji = [[-Rz^T / sz, (2 / sz) Rz^T [tm]x, -Rz^T tm / sz], [0, -(w I - [v]x) Rz^T, 0], [0, 0, -c]]
// Jj = [[se Re, 0, 0], [0, w I + [v]x, 0], [0, 0, c]]
__device__ constexpr bool ji_nz(int r, int a) { return r < 3 ? true : (r < 6 ? (a >= 3 && a < 6) : a == 6); }
__device__ constexpr bool jj_nz(int r, int c) { return r < 3 ? c < 3 : (r < 6 ? (c >= 3 && c < 6) : c == 6); }

// ---- the stage, as the pieces of graph_lm_device.h ask for it ---------------------------------------------------------------
struct Sim3Lm {
    static constexpr int NB = ::NB, VDBL = ::VDBL, BLOCK = SG_BLOCK;
    static constexpr bool FRESH = true, FULL_BLOCKS = false;
    using Edge = aria_sgraph_edge;
    using Scratch = GraphScratch<NB, VDBL>;
    struct Params {
        bool fix_scale;
    };

    // W = w Ji^T Jj: 31 entries are not structurally zero
    __device__ static constexpr bool w_nz(int a, int c) {
        bool nz = false;
        for (int r = 0; r < NB; r++) nz = nz || (ji_nz(r, a) && jj_nz(r, c));
        return nz;
    }

    // One edge: error, Jacobians and its blocks. Returns w * e.e. Stores A = w Ji^T Ji, B = w Jj^T Jj, W = w Ji^T Jj,
    // gi = w Ji^T e, gj = w Jj^T e at edge slot k. Only the non-zero entries of Ji and Jj enter a sum (ji_nz, jj_nz).
    __device__ static double edge_blocks(const double* verts, const Edge& ed, const Scratch& S, double* W, int k, const Params& prm) {
        const bool fix_scale = prm.fix_scale;
        double Ri[9], ti[3], Rj[9], tj[3], Rz[9], tz[3];
        const double si = load_vertex(verts + VDBL * (size_t)ed.from, Ri, ti);
        const double sj = load_vertex(verts + VDBL * (size_t)ed.to, Rj, tj);
        load_pose(ed.Z, Rz, tz);
        const double sz = ed.s;
        double Rm[9], tm[3], d[3], Re[9], te[3];
        mul_tn(Ri, Rj, Rm);
        d[0] = tj[0] - ti[0];  d[1] = tj[1] - ti[1];  d[2] = tj[2] - ti[2];
        mulv_t(Ri, d, tm);
        tm[0] /= si;  tm[1] /= si;  tm[2] /= si;
        mul_tn(Rz, Rm, Re);
        d[0] = tm[0] - tz[0];  d[1] = tm[1] - tz[1];  d[2] = tm[2] - tz[2];
        mulv_t(Rz, d, te);
        te[0] /= sz;  te[1] /= sz;  te[2] /= sz;
        const double se = (sj / si) / sz;
        double qx, qy, qz, qw;
        unit_quat_from_rot(Re, qx, qy, qz, qw);
        const double ise = 1.0 / se;
        const double e[NB] = {te[0], te[1], te[2], qx, qy, qz, fix_scale ? 0.0 : (se - ise) / 2};
        const double ch = fix_scale ? 0.0 : (se + ise) / 2;
        const double w = ed.info_scale;

        const double Tx[9] = {0, -tm[2], tm[1], tm[2], 0, -tm[0], -tm[1], tm[0], 0};
        const double Qm[9] = {qw, qz, -qy, -qz, qw, qx, qy, -qx, qw};     // w I - [v]x
        const double Qp[9] = {qw, -qz, qy, qz, qw, -qx, -qy, qx, qw};     // w I + [v]x
        double RzT[9], U[9], Lr[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) RzT[3 * i + j] = Rz[3 * j + i];
        mul_nn(RzT, Tx, U);
        mul_nn(Qm, RzT, Lr);
        double Ji[NB2], Jj[NB2];
#pragma unroll
        for (int c = 0; c < NB2; c++) Ji[c] = Jj[c] = 0.0;      // the structural zeros are never read (ji_nz, jj_nz)
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Ji[NB * i + j] = -RzT[3 * i + j] / sz;     Ji[NB * i + 3 + j] = (2 * U[3 * i + j]) / sz;
                Ji[NB * (i + 3) + 3 + j] = -Lr[3 * i + j];
                Jj[NB * i + j] = se * Re[3 * i + j];
                Jj[NB * (i + 3) + 3 + j] = Qp[3 * i + j];
            }
            const double rt = RzT[3 * i] * tm[0] + RzT[3 * i + 1] * tm[1] + RzT[3 * i + 2] * tm[2];
            Ji[NB * i + 6] = fix_scale ? 0.0 : -rt / sz;
        }
        Ji[NB * 6 + 6] = -ch;
        Jj[NB * 6 + 6] = ch;
        const size_t Ec = lm_stride<FRESH>(S.Ec);
#pragma unroll
        for (int a = 0; a < NB; a++) {
            double ga = 0.0, gb = 0.0;
#pragma unroll
            for (int r = 0; r < NB; r++) {
                if (ji_nz(r, a)) ga += Ji[NB * r + a] * e[r];
                if (jj_nz(r, a)) gb += Jj[NB * r + a] * e[r];
            }
            S.gi[a * Ec + k] = w * ga;
            S.gj[a * Ec + k] = w * gb;
#pragma unroll
            for (int c = 0; c < NB; c++) {
                double aa = 0.0, bb = 0.0, ww = 0.0;
#pragma unroll
                for (int r = 0; r < NB; r++) {
                    if (ji_nz(r, a) && ji_nz(r, c)) aa += Ji[NB * r + a] * Ji[NB * r + c];
                    if (jj_nz(r, a) && jj_nz(r, c)) bb += Jj[NB * r + a] * Jj[NB * r + c];
                    if (ji_nz(r, a) && jj_nz(r, c)) ww += Ji[NB * r + a] * Jj[NB * r + c];
                }
                S.A[(NB * a + c) * Ec + k] = w * aa;
                S.B[(NB * a + c) * Ec + k] = w * bb;
                W[(NB * a + c) * Ec + k] = w * ww;
            }
        }
        double ee = 0.0;
#pragma unroll
        for (int r = 0; r < NB; r++) ee += e[r] * e[r];
        return w * ee;
    }
};

// the inverse of the scale error (s - 1/s) / 2: always positive, no cancellation
__device__ inline double scale_of(double x) {
    const double r = sqrt(x * x + 1.0);
    return x >= 0.0 ? x + r : 1.0 / (-x + r);
}

// S <- S * D(d), rotation re-orthonormalised through its unit quaternion
__device__ inline void vertex_update(double* P, const double* d) {
    double R[9], t[3];
    const double s = load_vertex(P, R, t);
    double Rn[9];
    rotation_update(R, d, Rn);
#pragma unroll
    for (int c = 0; c < 9; c++) P[c] = Rn[c];
#pragma unroll
    for (int r = 0; r < 3; r++) P[9 + r] = t[r] + s * (R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
    P[12] = s * scale_of(d[6]);
}

// ---- the kernel: the schedule of graph_lm_device.h, written out (that header says why) ----------------------------------------
// mode 0: optimise. mode 1 (aria_sgraph_debug_linearize): linearise once; chi2 to results[g].chi2_initial, D, b and W stay in
// slot 0 of the scratch for the host to read.
__global__ __launch_bounds__(SG_BLOCK) void k_sgraph_lm(double* verts_all, const int* __restrict__ voff,
                                                        const aria_sgraph_edge* __restrict__ edges_all,
                                                        const int* __restrict__ eoff, const int* __restrict__ fixed_all,
                                                        int graph_base, int iterations, int max_vertices, int max_edges,
                                                        int pcg_max_iters, double pcg_rel_tol, double* vbase, double* ebase,
                                                        int* ibase, aria_sgraph_result* __restrict__ results, int* err,
                                                        int mode, int fix_scale_i) {
    __shared__ double red_lds[2 * 2 * SG_WAVES];
    __shared__ int scan[SG_BLOCK];
    const int g = graph_base + blockIdx.x;
    const int tid = threadIdx.x;
    const Sim3Lm::Params prm{fix_scale_i != 0};
    LmRed R{red_lds, 0};

    aria_sgraph_result res;
    res.chi2_initial = res.chi2_final = res.lambda = 0.0;
    res.iterations_done = res.trials = res.pcg_iterations = 0;
    res.valid = 0;
    res.stop_reason = STOP_INVALID;
    res.reserved = 0;

    // ---- validate before anything else is read: counts, then the edges, then (indices now known good) the vertex scales
    const int v0 = voff[g], e0 = eoff[g];
    const int nv = voff[g + 1] - v0, ne = eoff[g + 1] - e0;
    const int fixed = fixed_all[g];
    int bad = 0;
    if (v0 < 0 || e0 < 0 || nv < 0 || ne < 0 || (nv > 0 && (fixed < 0 || fixed >= nv)) || (nv == 0 && ne > 0))
        bad = ERRBIT_SG_INPUT;
    else if (nv > max_vertices || ne > max_edges)
        bad = ERRBIT_SG_LARGE;
    const aria_sgraph_edge* edges = edges_all + (bad ? 0 : e0);
    double* verts = verts_all + (bad ? 0 : VDBL * (size_t)v0);
    int ebad = 0;
    if (!bad) {
        for (int k = tid; k < ne; k += SG_BLOCK) {
            const int a = edges[k].from, b = edges[k].to;
            const double w = edges[k].info_scale, s = edges[k].s;
            if (a < 0 || a >= nv || b < 0 || b >= nv || a == b || !(w >= 0.0) || !(w < INFINITY) || !(s > 0.0) || !(s < INFINITY))
                ebad = 1;
        }
        for (int v = tid; v < nv; v += SG_BLOCK) {
            const double s = verts[VDBL * (size_t)v + 12];
            if (!(s > 0.0) || !(s < INFINITY)) ebad = 1;
        }
    }
    if (__syncthreads_or(ebad)) bad = ERRBIT_SG_INPUT;
    if (bad) {
        if (tid == 0) {
            atomicOr(err, bad);
            results[g] = res;
        }
        return;
    }
    res.valid = 1;
    res.stop_reason = STOP_ITERATIONS;
    if (nv == 0) {
        if (tid == 0) results[g] = res;
        return;
    }
    const Sim3Lm::Scratch S = Sim3Lm::Scratch::of(vbase, ebase, ibase, blockIdx.x, max_vertices, max_edges);
    build_adjacency<Sim3Lm>(S, edges, nv, ne, scan);

    // ---- linearise at the input vertices
    int curW = 0;
    double chi2 = edge_pass<Sim3Lm>(R, verts, edges, ne, S, S.W0, prm);
    const double maxdiag = vertex_gather<Sim3Lm>(R, nv, fixed, S);
    res.chi2_initial = res.chi2_final = chi2;
    if (mode == 1) {
        if (tid == 0) results[g] = res;
        return;
    }
    LmDamping lm;
    lm.start(maxdiag);

    for (int it = 0; it < iterations; it++) {
        bool accepted = false;
        for (int trial = 0; trial < LM_MAX_TRIALS; trial++) {
            res.trials++;
            double* Wc = curW ? S.W1 : S.W0;
            double* Wn = curW ? S.W0 : S.W1;
            precond_build<Sim3Lm>(nv, lm.lambda, S);       // each lane builds and later reads its own vertices' blocks
            res.pcg_iterations += pcg_solve<Sim3Lm>(R, nv, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol);
            // update (with a backup) and the gain's denominator dx.(lambda dx + b)
            double den = 0.0;
            for (int v = tid; v < nv; v += SG_BLOCK) {
                if (v == fixed) continue;
                const size_t Vc = lm_stride<true>(S.Vc);
                double P[VDBL], d[NB];
#pragma unroll
                for (int c = 0; c < VDBL; c++) {
                    P[c] = verts[VDBL * (size_t)v + c];
                    S.bak[c * Vc + v] = P[c];
                }
#pragma unroll
                for (int c = 0; c < NB; c++) {
                    d[c] = S.x[c * Vc + v];
                    den += d[c] * (lm.lambda * d[c] + S.b[c * Vc + v]);
                }
                vertex_update(P, d);
#pragma unroll
                for (int c = 0; c < VDBL; c++) verts[VDBL * (size_t)v + c] = P[c];
            }
            den = block_sum<SG_WAVES>(R.lds, R.phase, den) + 1e-3;   // barrier: the new vertices are visible
            const double chi2_new = edge_pass<Sim3Lm>(R, verts, edges, ne, S, Wn, prm);
            const double rho = (chi2 - chi2_new) / den;
            if (rho > 0.0 && chi2_new < INFINITY && chi2_new == chi2_new) {
                curW ^= 1;
                vertex_gather<Sim3Lm>(R, nv, fixed, S);
                chi2 = chi2_new;
                lm.accept(rho);
                accepted = true;
                break;
            }
            for (int v = tid; v < nv; v += SG_BLOCK) {
                if (v == fixed) continue;
                const size_t Vc = lm_stride<true>(S.Vc);
#pragma unroll
                for (int c = 0; c < VDBL; c++) verts[VDBL * (size_t)v + c] = S.bak[c * Vc + v];
            }
            __syncthreads();
            lm.reject();
        }
        if (!accepted) {
            res.stop_reason = STOP_TRIALS;
            break;
        }
        res.iterations_done++;
    }
    res.chi2_final = chi2;
    res.lambda = lm.lambda;
    if (tid == 0) results[g] = res;
}

// ---- the map after a loop (sgraph_ref.correct_points) ------------------------------------------------------------------------
// One lane per arena point. X' = S_new S_old^-1 X in the restatement's operation order (-ffp-contract=off: no FMA; fp64
// division is correctly rounded), three 8-byte stores, every other byte of the record untouched.
__device__ inline bool good_scale(double s) { return s > 0.0 && s < INFINITY; }

__global__ __launch_bounds__(CORRECT_BLOCK) void k_sgraph_correct(aria_map_point* __restrict__ pts, const long long* __restrict__ d_size,
                                                                  long long limit, const int* __restrict__ table, int n_table,
                                                                  int pair_base, const aria_sgraph_vertex* __restrict__ old_v,
                                                                  const aria_sgraph_vertex* __restrict__ new_v, int n_vertices,
                                                                  int* __restrict__ stats, int* err) {
    long long size = d_size ? *d_size : limit;
    size = size < 0 ? 0 : (size > limit ? limit : size);
    int moved = 0, left = 0, refused = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < size; i += (long long)gridDim.x * blockDim.x) {
        const long long slot = (long long)pts[i].pair - (long long)pair_base;
        int v = -1;
        if (slot >= 0 && slot < (long long)n_table) v = table[slot];
        if (v < 0) { left++;  continue; }
        if (v >= n_vertices) { refused++;  continue; }
        const double X0 = pts[i].X[0], X1 = pts[i].X[1], X2 = pts[i].X[2];
        const aria_sgraph_vertex& o = old_v[v];
        const aria_sgraph_vertex& n = new_v[v];
        const double so = o.s, sn = n.s;
        const bool finite = (X0 - X0 == 0.0) && (X1 - X1 == 0.0) && (X2 - X2 == 0.0);
        if (!good_scale(so) || !good_scale(sn) || !finite) { refused++;  continue; }
        const double d0 = X0 - o.t[0], d1 = X1 - o.t[1], d2 = X2 - o.t[2];
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = ((o.R[k] * d0 + o.R[3 + k] * d1) + o.R[6 + k] * d2) / so;
#pragma unroll
        for (int k = 0; k < 3; k++) pts[i].X[k] = sn * ((n.R[3 * k] * c[0] + n.R[3 * k + 1] * c[1]) + n.R[3 * k + 2] * c[2]) + n.t[k];
        moved++;
    }
    // integer counts: a wave sum, then one integer atomic per wave and counter
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        moved += __shfl_xor(moved, m, 64);
        left += __shfl_xor(left, m, 64);
        refused += __shfl_xor(refused, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (stats) {
            if (moved) atomicAdd(&stats[0], moved);
            if (left) atomicAdd(&stats[1], left);
            if (refused) atomicAdd(&stats[2], refused);
        }
        if (refused) atomicOr(err, ERRBIT_SG_INPUT);
    }
}

// pose rows [R t] (12 doubles) <-> vertices (R[9], t[3], s): 64-bit integer copies, no arithmetic
__global__ __launch_bounds__(256) void k_sgraph_from_pose(const unsigned long long* __restrict__ poses, unsigned long long* __restrict__ verts,
                                                          int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long* P = poses + 12 * (size_t)i;
    unsigned long long* S = verts + VDBL * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        S[3 * r] = P[4 * r];  S[3 * r + 1] = P[4 * r + 1];  S[3 * r + 2] = P[4 * r + 2];  S[9 + r] = P[4 * r + 3];
    }
    S[12] = 0x3FF0000000000000ull;          // 1.0
}

__global__ __launch_bounds__(256) void k_sgraph_to_pose(const unsigned long long* __restrict__ verts, unsigned long long* __restrict__ poses,
                                                        int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long* S = verts + VDBL * (size_t)i;
    unsigned long long* P = poses + 12 * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        P[4 * r] = S[3 * r];  P[4 * r + 1] = S[3 * r + 1];  P[4 * r + 2] = S[3 * r + 2];  P[4 * r + 3] = S[9 + r];
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_sgraph_s : StageHandle {
    aria_sgraph_config cfg{};
    DeviceBuffer<double> d_v;  // [max_graphs] vertex scratch
    DeviceBuffer<double> d_e;  // [max_graphs] edge scratch
    DeviceBuffer<int> d_i;     // [max_graphs] adjacency
    // single-graph staging (aria_sgraph_optimize, aria_sgraph_debug_linearize)
    DeviceBuffer<double> d_verts;
    DeviceBuffer<aria_sgraph_edge> d_edges;
    DeviceBuffer<int> d_off;   // [0..1] vertex offsets, [2..3] edge offsets, [4] fixed
    DeviceBuffer<aria_sgraph_result> d_res;
};

namespace {

bool bad_scale(double s) { return !(s > 0.0) || !std::isfinite(s); }

struct Sim3Host : Sim3Lm {
    using Handle = aria_sgraph_s;
    using Result = aria_sgraph_result;
    static constexpr auto kernel = k_sgraph_lm;
    static size_t lds_bytes(Handle*) { return 0; }
    static int last_arg(Handle* h) { return h->cfg.fix_scale; }
    static DeviceBuffer<double>& verts(Handle* h) { return h->d_verts; }
    static int check(Handle* h) { return aria_sgraph_check(h); }
    static bool edge_bad(const Edge& e) { return bad_scale(e.s); }
    static bool vertex_bad(const double* v) { return bad_scale(v[12]); }
};

int sgraph_correct(aria_sgraph_t h, aria_map_point* d_points, const long long* d_size, int64_t limit, const int* d_pair_vertex,
                   int n_table, int pair_base, const aria_sgraph_vertex* d_old, const aria_sgraph_vertex* d_new, int n_vertices,
                   aria_sgraph_correct_stats* d_stats) {
    if (d_stats) ARIA_HIP(hipMemsetAsync(d_stats, 0, sizeof(aria_sgraph_correct_stats), h->stream));
    if (!d_points || limit <= 0) return ARIA_OK;
    const int blocks = (int)std::min<int64_t>((limit + CORRECT_BLOCK - 1) / CORRECT_BLOCK, 4096);
    hipLaunchKernelGGL(k_sgraph_correct, dim3(blocks), dim3(CORRECT_BLOCK), 0, h->stream, d_points, d_size, (long long)limit,
                       d_pair_vertex, n_table, pair_base, d_old, d_new, n_vertices, reinterpret_cast<int*>(d_stats), h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

}  // namespace

extern "C" {

void aria_sgraph_default_config(aria_sgraph_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_sgraph_config);
    c->device = 0;
    c->stream = nullptr;
    c->max_graphs = 1;
    c->max_vertices = 4096;
    c->max_edges = 8192;
    c->pcg_max_iters = 1000;
    c->pcg_rel_tol = 1e-8;
    c->fix_scale = 0;
}

int aria_sgraph_create(const aria_sgraph_config* c, aria_sgraph_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_sgraph_config)) return ARIA_E_INVALID;
    if (c->max_graphs < 1 || c->max_graphs > 65535 || c->max_vertices < 1 || c->max_vertices > (1 << 20) || c->max_edges < 1 ||
        c->max_edges > (1 << 22) || c->pcg_max_iters < 1 || c->pcg_max_iters > 100000 || !(c->pcg_rel_tol > 0) ||
        !(c->pcg_rel_tol < 1) || (c->fix_scale != 0 && c->fix_scale != 1) || c->reserved != 0)
        return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_sgraph_create", [](aria_sgraph_s* h) { return graph_lm_reserve<Sim3Host>(h, "aria_sgraph_create"); });
}

void aria_sgraph_destroy(aria_sgraph_t h) { stage_destroy(h); }

void* aria_sgraph_stream(aria_sgraph_t h) { return stage_stream(h); }

int aria_sgraph_check(aria_sgraph_t h) {
    return stage_check(h, {{ERRBIT_SG_INPUT, ARIA_E_INVALID}, {ERRBIT_SG_LARGE, ARIA_E_TOO_LARGE}});
}

int aria_sgraph_optimize_batch_device(aria_sgraph_t h, aria_sgraph_vertex* d_vertices, const int* d_vertex_offset,
                                      const aria_sgraph_edge* d_edges, const int* d_edge_offset, const int* d_fixed, int n_graphs,
                                      int iterations, aria_sgraph_result* d_results) {
    return graph_lm_optimize_batch_device<Sim3Host>(h, reinterpret_cast<double*>(d_vertices), d_vertex_offset, d_edges, d_edge_offset,
                                                    d_fixed, n_graphs, iterations, d_results);
}

int aria_sgraph_optimize(aria_sgraph_t h, aria_sgraph_vertex* vertices_inout, int n_vertices, int fixed_index,
                         const aria_sgraph_edge* edges, int n_edges, int iterations, aria_sgraph_result* result) {
    return graph_lm_optimize<Sim3Host>(h, reinterpret_cast<double*>(vertices_inout), n_vertices, fixed_index, edges, n_edges, iterations,
                                       result);
}

int aria_sgraph_debug_linearize(aria_sgraph_t h, const aria_sgraph_vertex* vertices, int n_vertices, int fixed_index,
                                const aria_sgraph_edge* edges, int n_edges, double* chi2, double* b, double* H_diag, double* H_off) {
    return graph_lm_debug_linearize<Sim3Host>(h, reinterpret_cast<const double*>(vertices), n_vertices, fixed_index, edges, n_edges, chi2,
                                              b, H_diag, H_off);
}

int aria_sgraph_vertices_from_pose_device(aria_sgraph_t h, const double* d_poses, aria_sgraph_vertex* d_vertices, int n) {
    if (!h || n < 0 || (n && (!d_poses || !d_vertices))) return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_sgraph_from_pose, dim3((n + 255) / 256), dim3(256), 0, h->stream,
                       reinterpret_cast<const unsigned long long*>(d_poses), reinterpret_cast<unsigned long long*>(d_vertices), n);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_sgraph_poses_from_vertices_device(aria_sgraph_t h, const aria_sgraph_vertex* d_vertices, double* d_poses, int n) {
    if (!h || n < 0 || (n && (!d_poses || !d_vertices))) return ARIA_E_INVALID;
    if (n == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_sgraph_to_pose, dim3((n + 255) / 256), dim3(256), 0, h->stream,
                       reinterpret_cast<const unsigned long long*>(d_vertices), reinterpret_cast<unsigned long long*>(d_poses), n);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_sgraph_correct_map_device(aria_sgraph_t h, aria_map_t map, const int* d_pair_vertex, int n_table, int pair_base,
                                   const aria_sgraph_vertex* d_old, const aria_sgraph_vertex* d_new, int n_vertices,
                                   aria_sgraph_correct_stats* d_stats) {
    if (!h || !map || n_table < 0 || n_vertices < 0 || (n_table && !d_pair_vertex) || (n_vertices && (!d_old || !d_new)))
        return ARIA_E_INVALID;
    const aria_map_point* arena = nullptr;
    const long long* d_size = nullptr;
    int64_t capacity = 0;
    int map_device = -1;
    map_device_view(map, &arena, &d_size, &capacity, &map_device);
    if (map_device != h->device) return ARIA_E_INVALID;          // the correction writes the map's arena where it lies
    ARIA_HIP(hipSetDevice(h->device));
    // the one place that writes the arena from outside the map stage: the const of the view is cast away here
    return sgraph_correct(h, const_cast<aria_map_point*>(arena), d_size, capacity, d_pair_vertex, n_table, pair_base, d_old, d_new,
                          n_vertices, d_stats);
}

int aria_sgraph_correct_points_device(aria_sgraph_t h, aria_map_point* d_points, int64_t n_points, const int* d_pair_vertex,
                                      int n_table, int pair_base, const aria_sgraph_vertex* d_old, const aria_sgraph_vertex* d_new,
                                      int n_vertices, aria_sgraph_correct_stats* d_stats) {
    if (!h || n_points < 0 || (n_points && !d_points) || n_table < 0 || n_vertices < 0 || (n_table && !d_pair_vertex) ||
        (n_vertices && (!d_old || !d_new)))
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    return sgraph_correct(h, d_points, nullptr, n_points, d_pair_vertex, n_table, pair_base, d_old, d_new, n_vertices, d_stats);
}

}  // extern "C"
