// SE(3) pose-graph optimisation, batched over graphs (include/aria_orb_hip.h, "SE(3) pose-graph optimisation"): what the
// reference's PoseGraphOptimizer (src/legacy/LoopClosure.cpp:197-312) asks of g2o -- VertexSE3 / EdgeSE3 under
// Levenberg-Marquardt, first vertex fixed. aria_slam_amd/graph_ref.py is the specification; DESIGN.md section 13 the record.
//
// One kernel, k_graph_lm: the schedule, its pieces and the host calls around the kernel are those of graph_lm_device.h (one
// workgroup per graph, persistent over every LM iteration), instantiated with 6 x 6 blocks and 12-double pose rows [R t].
// Specific to this stage, and written here:
//   edge_blocks  e and the 6 x 6 Jacobians of an SE(3) edge. Their explicit zeros enter every sum.
//   pose_update  X <- X * fromMQT(d).
//   the solve    three forms of the one solve, the same arithmetic in the same order (the choice changes no bit): pcg_solve of
//                the shared header, any size; pcg_small<false>, up to 512 vertices: one vertex per lane, its diagonal and
//                preconditioner blocks, r and p in registers; pcg_small<true>, also at most 544 edges: W and p in LDS (142 KB
//                of dynamic LDS, asked for at create), so an iteration reads HBM for the adjacency only.
// The kernel body itself is written out here and in sim3_graph.hip: graph_lm_device.h records why.
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

constexpr int GRAPH_BLOCK = 512;          // 8 waves: 2 per SIMD, 256 VGPRs each
constexpr int GRAPH_WAVES = GRAPH_BLOCK / 64;
constexpr int ERRBIT_GRAPH_INPUT = 1;     // counts, fixed index or an edge out of range (graph skipped)
constexpr int ERRBIT_GRAPH_LARGE = 2;     // more vertices or edges than the handle was created for (graph skipped)
constexpr int GRAPH_LDS_EDGES = 544;      // edges whose W fits the LDS beside p: 27 * 544 * 8 + 6 * 512 * 8 = 142080 bytes of 160 KiB

__host__ __device__ inline size_t graph_lds_bytes(int wlds_edges) {
    return wlds_edges > 0 ? (27 * (size_t)wlds_edges + 6 * (size_t)GRAPH_BLOCK) * sizeof(double) : 0;
}

// W = s Ji^T Jj has a zero block: rows 0..2 x columns 3..5 (Ji's lower-left and Jj's off-diagonal blocks are zero)
__device__ constexpr bool w_zero(int r, int c) { return r < 3 && c >= 3; }
__device__ constexpr int w27(int r, int c) { return r < 3 ? 3 * r + c : 9 + 6 * (r - 3) + c; }    // index among the 27 others

// The solve of pcg_solve for a graph of at most GRAPH_BLOCK vertices: one vertex per lane, so its diagonal block, its preconditioner
// block (upper triangles) and its r and p stay in registers over the whole solve; only p (for the neighbours) and W go through memory. The
// arithmetic and its order are those of pcg_solve: both give the same bits.
// ONCHIP: the graph's W (its 27 entries per edge that are not structurally zero) and p live in LDS for the solve, so an
// iteration touches HBM for the adjacency only.
template <bool ONCHIP>
__device__ inline int pcg_small(LmRed& R, int nv, int ne, int fixed, double lambda, const double* W, const GraphScratch<6, 12>& S,
                                int max_iters, double rel_tol, double* wl, int wcap) {
    const size_t Vc = (size_t)S.Vc, Ec = (size_t)S.Ec;
    // The lane's vertex index goes through an opaque copy, here and in every iteration: threadIdx.x is invariant over the
    // whole kernel, and the 60-odd component addresses derived from it would otherwise be hoisted out of the LM loops and
    // held (and spilled) across everything else. Formed where they are used they cost a 64-bit add each.
    int v_lane = threadIdx.x;
    asm volatile("" : "+v"(v_lane));
    const int v = v_lane;
    const bool own = v < nv, act = own && v != fixed;
    double Dr[21], Mr[21], r[6], p[6], z[6];      // x is only ever added to: it stays in the scratch
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = a; c < 6; c++) {
            Dr[tri6(a, c)] = act ? S.D[(6 * a + c) * Vc + v] : 0.0;
            Mr[tri6(a, c)] = act ? S.Mi[(6 * a + c) * Vc + v] : 0.0;
        }
    const int a0 = act ? S.aoff[v] : 0, a1 = act ? S.aoff[v + 1] : 0;
    double* pl = wl + 27 * (size_t)wcap;             // p behind W: [6][GRAPH_BLOCK]
    if (ONCHIP) {
#pragma unroll 1
        for (int j = 0; j < 27; j++) {
            const int full = j < 9 ? (j / 3) * 6 + j % 3 : 9 + j;
            for (int k = threadIdx.x; k < ne; k += GRAPH_BLOCK) wl[j * wcap + k] = W[full * Ec + k];
        }
    }
    double rz = 0.0, bb = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) r[c] = act ? S.b[c * Vc + v] : 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) t += Mr[tri6(a, c)] * r[c];
        z[a] = t;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
        p[c] = z[c];
        if (own) S.x[c * Vc + v] = 0.0;
        if (ONCHIP) pl[c * GRAPH_BLOCK + v] = p[c];
        else if (own) S.p[c * Vc + v] = p[c];
        rz += r[c] * z[c];
        bb += r[c] * r[c];
    }
    block_sum2<GRAPH_WAVES>(R.lds, R.phase, rz, bb);
    int iters = 0;
    if (bb > 0.0) {
        const double stop = rel_tol * rel_tol * bb;
        for (int it = 1; it <= max_iters; it++) {
            int v = v_lane;
            asm volatile("" : "+v"(v));
            double y[6], pAp = 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double t = lambda * p[a];
#pragma unroll
                for (int c = 0; c < 6; c++) t += Dr[tri6(a, c)] * p[c];
                y[a] = t;
            }
            for (int a = a0; a < a1; a++) {
                const int code = S.adj[a];
                const size_t k = (size_t)(code >> 1);
                const int other = S.nbr[a];
                double q[6];
#pragma unroll
                for (int c = 0; c < 6; c++) q[c] = ONCHIP ? pl[c * GRAPH_BLOCK + other] : S.p[c * Vc + other];
                if (code & 1) {
#pragma unroll
                    for (int c = 0; c < 6; c++)
#pragma unroll
                        for (int r2 = 0; r2 < 6; r2++)
                            if (!w_zero(r2, c)) y[c] += (ONCHIP ? wl[w27(r2, c) * wcap + k] : W[(6 * r2 + c) * Ec + k]) * q[r2];
                } else {
#pragma unroll
                    for (int r2 = 0; r2 < 6; r2++)
#pragma unroll
                        for (int c = 0; c < 6; c++)
                            if (!w_zero(r2, c)) y[r2] += (ONCHIP ? wl[w27(r2, c) * wcap + k] : W[(6 * r2 + c) * Ec + k]) * q[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c++) pAp += p[c] * y[c];
            pAp = block_sum<GRAPH_WAVES>(R.lds, R.phase, pAp);   // barrier: every lane has read its neighbours' p
            if (!(pAp > 0.0)) break;
            const double alpha = rz / pAp;
            double rr = 0.0, rzn = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                if (act) S.x[c * Vc + v] += alpha * p[c];
                r[c] = r[c] - alpha * y[c];
            }
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double t = 0.0;
#pragma unroll
                for (int c = 0; c < 6; c++) t += Mr[tri6(a, c)] * r[c];
                z[a] = t;
            }
#pragma unroll
            for (int c = 0; c < 6; c++) {
                rr += r[c] * r[c];
                rzn += r[c] * z[c];
            }
            block_sum2<GRAPH_WAVES>(R.lds, R.phase, rr, rzn);
            iters = it;
            if (rr <= stop) break;
            const double beta = rzn / rz;
            rz = rzn;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                p[c] = z[c] + beta * p[c];
                if (ONCHIP) pl[c * GRAPH_BLOCK + v] = p[c];
                else if (act) S.p[c * Vc + v] = p[c];
            }
            __syncthreads();                         // p is visible before the next product gathers it
        }
    }
    return iters;
}

// ---- the stage, as the pieces of graph_lm_device.h ask for it ---------------------------------------------------------------
struct Se3Lm {
    static constexpr int NB = 6, VDBL = 12, BLOCK = GRAPH_BLOCK;
    static constexpr bool FRESH = false, FULL_BLOCKS = true;
    using Edge = aria_graph_edge;
    using Scratch = GraphScratch<NB, VDBL>;
    struct Params {};

    __device__ static constexpr bool w_nz(int r, int c) { return !w_zero(r, c); }

    // One edge: error, Jacobians and its blocks. Returns s * e.e. Stores A = s Ji^T Ji, B = s Jj^T Jj, W = s Ji^T Jj,
    // gi = s Ji^T e, gj = s Jj^T e at edge slot k. The explicit zeros of Ji and Jj enter every sum.
    __device__ static double edge_blocks(const double* poses, const Edge& ed, const Scratch& S, double* W, int k, const Params&) {
        double Ri[9], ti[3], Rj[9], tj[3], Rz[9], tz[3];
        load_pose(poses + 12 * (size_t)ed.from, Ri, ti);
        load_pose(poses + 12 * (size_t)ed.to, Rj, tj);
        load_pose(ed.Z, Rz, tz);
        double Rm[9], tm[3], d[3], Re[9], te[3];
        mul_tn(Ri, Rj, Rm);
        d[0] = tj[0] - ti[0];  d[1] = tj[1] - ti[1];  d[2] = tj[2] - ti[2];
        mulv_t(Ri, d, tm);
        mul_tn(Rz, Rm, Re);
        d[0] = tm[0] - tz[0];  d[1] = tm[1] - tz[1];  d[2] = tm[2] - tz[2];
        mulv_t(Rz, d, te);
        double qx, qy, qz, qw;
        unit_quat_from_rot(Re, qx, qy, qz, qw);
        const double e[6] = {te[0], te[1], te[2], qx, qy, qz};
        const double s = ed.info_scale;

        // Ji = [[-Rz^T, 2 Rz^T [tm]x], [0, -(w I - [v]x) Rz^T]],  Jj = [[Re, 0], [0, w I + [v]x]]
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
        double Ji[36], Jj[36];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Ji[6 * i + j] = -RzT[3 * i + j];       Ji[6 * i + 3 + j] = 2 * U[3 * i + j];
                Ji[6 * (i + 3) + j] = 0.0;             Ji[6 * (i + 3) + 3 + j] = -Lr[3 * i + j];
                Jj[6 * i + j] = Re[3 * i + j];         Jj[6 * i + 3 + j] = 0.0;
                Jj[6 * (i + 3) + j] = 0.0;             Jj[6 * (i + 3) + 3 + j] = Qp[3 * i + j];
            }
        const size_t Ec = (size_t)S.Ec;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double ga = 0.0, gb = 0.0;
#pragma unroll
            for (int r = 0; r < 6; r++) { ga += Ji[6 * r + a] * e[r];  gb += Jj[6 * r + a] * e[r]; }
            S.gi[a * Ec + k] = s * ga;
            S.gj[a * Ec + k] = s * gb;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double aa = 0.0, bb = 0.0, ww = 0.0;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    aa += Ji[6 * r + a] * Ji[6 * r + c];
                    bb += Jj[6 * r + a] * Jj[6 * r + c];
                    ww += Ji[6 * r + a] * Jj[6 * r + c];
                }
                S.A[(6 * a + c) * Ec + k] = s * aa;
                S.B[(6 * a + c) * Ec + k] = s * bb;
                W[(6 * a + c) * Ec + k] = s * ww;
            }
        }
        double ee = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) ee += e[r] * e[r];
        return s * ee;
    }
};

// X <- X * fromMQT(d), rotation re-orthonormalised through its unit quaternion
__device__ inline void pose_update(double* P, const double* d) {
    double R[9], t[3], Rn[9];
    load_pose(P, R, t);
    rotation_update(R, d, Rn);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        P[4 * r] = Rn[3 * r];  P[4 * r + 1] = Rn[3 * r + 1];  P[4 * r + 2] = Rn[3 * r + 2];
        P[4 * r + 3] = t[r] + (R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
    }
}

// ---- the kernel: the schedule of graph_lm_device.h, written out (that header says why) ----------------------------------------
// mode 0: optimise. mode 1 (aria_graph_debug_linearize): linearise once; chi2 to results[g].chi2_initial, D, b and W stay in
// slot 0 of the scratch for the host to read.
__global__ __launch_bounds__(GRAPH_BLOCK) void k_graph_lm(double* poses_all, const int* __restrict__ voff,
                                                          const aria_graph_edge* __restrict__ edges_all,
                                                          const int* __restrict__ eoff, const int* __restrict__ fixed_all,
                                                          int graph_base, int iterations, int max_vertices, int max_edges,
                                                          int pcg_max_iters, double pcg_rel_tol, double* vbase, double* ebase,
                                                          int* ibase, aria_graph_result* __restrict__ results, int* err,
                                                          int mode, int wlds_edges) {
    extern __shared__ double wlds[];                 // graph_lds_bytes(wlds_edges): W and p of a graph that fits (pcg_small)
    __shared__ double red_lds[2 * 2 * GRAPH_WAVES];
    __shared__ int scan[GRAPH_BLOCK];
    const int g = graph_base + blockIdx.x;
    const int tid = threadIdx.x;
    LmRed R{red_lds, 0};

    aria_graph_result res;
    res.chi2_initial = res.chi2_final = res.lambda = 0.0;
    res.iterations_done = res.trials = res.pcg_iterations = 0;
    res.valid = 0;
    res.stop_reason = STOP_INVALID;
    res.reserved = 0;

    // ---- validate before anything else is read
    const int v0 = voff[g], e0 = eoff[g];
    const int nv = voff[g + 1] - v0, ne = eoff[g + 1] - e0;
    const int fixed = fixed_all[g];
    int bad = 0;
    if (v0 < 0 || e0 < 0 || nv < 0 || ne < 0 || (nv > 0 && (fixed < 0 || fixed >= nv)) || (nv == 0 && ne > 0))
        bad = ERRBIT_GRAPH_INPUT;
    else if (nv > max_vertices || ne > max_edges)
        bad = ERRBIT_GRAPH_LARGE;
    const aria_graph_edge* edges = edges_all + (bad ? 0 : e0);
    int ebad = 0;
    if (!bad)
        for (int k = tid; k < ne; k += GRAPH_BLOCK) {
            const int a = edges[k].from, b = edges[k].to;
            const double s = edges[k].info_scale;
            if (a < 0 || a >= nv || b < 0 || b >= nv || a == b || !(s >= 0.0) || !(s < INFINITY)) ebad = 1;
        }
    if (__syncthreads_or(ebad)) bad = ERRBIT_GRAPH_INPUT;
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
    double* poses = poses_all + 12 * (size_t)v0;
    const Se3Lm::Scratch S = Se3Lm::Scratch::of(vbase, ebase, ibase, blockIdx.x, max_vertices, max_edges);

    build_adjacency<Se3Lm>(S, edges, nv, ne, scan);

    // ---- linearise at the input poses
    int curW = 0;
    double chi2 = edge_pass<Se3Lm>(R, poses, edges, ne, S, S.W0, {});
    const double maxdiag = vertex_gather<Se3Lm>(R, nv, fixed, S);
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
            precond_build<Se3Lm>(nv, lm.lambda, S);           // each lane builds and later reads its own vertices' blocks
            // three forms of one solve, the same arithmetic in the same order (the choice changes no bit of the result)
            if (nv <= GRAPH_BLOCK && ne <= wlds_edges)
                res.pcg_iterations += pcg_small<true>(R, nv, ne, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol, wlds, wlds_edges);
            else if (nv <= GRAPH_BLOCK)
                res.pcg_iterations += pcg_small<false>(R, nv, ne, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol, wlds, 0);
            else
                res.pcg_iterations += pcg_solve<Se3Lm>(R, nv, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol);
            // update (with a backup) and the gain's denominator dx.(lambda dx + b)
            double den = 0.0;
            const size_t Vc = (size_t)S.Vc;
            for (int v = tid; v < nv; v += GRAPH_BLOCK) {
                if (v == fixed) continue;
                double P[12], d[6];
#pragma unroll
                for (int c = 0; c < 12; c++) {
                    P[c] = poses[12 * (size_t)v + c];
                    S.bak[c * Vc + v] = P[c];
                }
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    d[c] = S.x[c * Vc + v];
                    den += d[c] * (lm.lambda * d[c] + S.b[c * Vc + v]);
                }
                pose_update(P, d);
#pragma unroll
                for (int c = 0; c < 12; c++) poses[12 * (size_t)v + c] = P[c];
            }
            den = block_sum<GRAPH_WAVES>(R.lds, R.phase, den) + 1e-3;   // barrier: the new poses are visible
            const double chi2_new = edge_pass<Se3Lm>(R, poses, edges, ne, S, Wn, {});
            const double rho = (chi2 - chi2_new) / den;
            if (rho > 0.0 && chi2_new < INFINITY && chi2_new == chi2_new) {
                curW ^= 1;
                vertex_gather<Se3Lm>(R, nv, fixed, S);
                chi2 = chi2_new;
                lm.accept(rho);
                accepted = true;
                break;
            }
            for (int v = tid; v < nv; v += GRAPH_BLOCK) {
                if (v == fixed) continue;
#pragma unroll
                for (int c = 0; c < 12; c++) poses[12 * (size_t)v + c] = S.bak[c * Vc + v];
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

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_graph_s : StageHandle {
    aria_graph_config cfg{};
    DeviceBuffer<double> d_v;  // [max_graphs] vertex scratch
    DeviceBuffer<double> d_e;  // [max_graphs] edge scratch
    DeviceBuffer<int> d_i;     // [max_graphs] adjacency
    // single-graph staging (aria_graph_optimize, aria_graph_debug_linearize)
    DeviceBuffer<double> d_poses;
    DeviceBuffer<aria_graph_edge> d_edges;
    DeviceBuffer<int> d_off;   // [0..1] vertex offsets, [2..3] edge offsets, [4] fixed
    DeviceBuffer<aria_graph_result> d_res;
    int wlds_edges = 0;        // edges of the on-chip solve (0: the device refused the LDS size, W and p stay in HBM)
};

namespace {

struct Se3Host : Se3Lm {
    using Handle = aria_graph_s;
    using Result = aria_graph_result;
    static constexpr auto kernel = k_graph_lm;
    static size_t lds_bytes(Handle* h) { return graph_lds_bytes(h->wlds_edges); }
    static int last_arg(Handle* h) { return h->wlds_edges; }
    static DeviceBuffer<double>& verts(Handle* h) { return h->d_poses; }
    static int check(Handle* h) { return aria_graph_check(h); }
    static bool edge_bad(const Edge&) { return false; }        // nothing beyond what graph_lm_stage_single asks of every edge
    static bool vertex_bad(const double*) { return false; }
};

}  // namespace

extern "C" {

void aria_graph_default_config(aria_graph_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_graph_config);
    c->device = 0;
    c->stream = nullptr;
    c->max_graphs = 1;
    c->max_vertices = 4096;
    c->max_edges = 8192;
    c->pcg_max_iters = 1000;
    c->pcg_rel_tol = 1e-8;
}

int aria_graph_create(const aria_graph_config* c, aria_graph_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_graph_config)) return ARIA_E_INVALID;
    if (c->max_graphs < 1 || c->max_graphs > 65535 || c->max_vertices < 1 || c->max_vertices > (1 << 20) || c->max_edges < 1 ||
        c->max_edges > (1 << 22) || c->pcg_max_iters < 1 || c->pcg_max_iters > 100000 || !(c->pcg_rel_tol > 0) ||
        !(c->pcg_rel_tol < 1))
        return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_graph_create", [](aria_graph_s* h) {
        // more than 64 KiB of dynamic LDS has to be asked for; where that is refused the solve keeps W and p in HBM
        h->wlds_edges = std::min(h->cfg.max_edges, GRAPH_LDS_EDGES);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_graph_lm), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)graph_lds_bytes(h->wlds_edges)) != hipSuccess) {
            (void)hipGetLastError();
            h->wlds_edges = 0;
        }
        return graph_lm_reserve<Se3Host>(h, "aria_graph_create");
    });
}

void aria_graph_destroy(aria_graph_t h) { stage_destroy(h); }

void* aria_graph_stream(aria_graph_t h) { return stage_stream(h); }

int aria_graph_check(aria_graph_t h) {
    return stage_check(h, {{ERRBIT_GRAPH_INPUT, ARIA_E_INVALID}, {ERRBIT_GRAPH_LARGE, ARIA_E_TOO_LARGE}});
}

int aria_graph_optimize_batch_device(aria_graph_t h, double* d_poses, const int* d_vertex_offset, const aria_graph_edge* d_edges,
                                     const int* d_edge_offset, const int* d_fixed, int n_graphs, int iterations,
                                     aria_graph_result* d_results) {
    return graph_lm_optimize_batch_device<Se3Host>(h, d_poses, d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs,
                                                   iterations, d_results);
}

int aria_graph_optimize(aria_graph_t h, double* poses_inout, int n_vertices, int fixed_index, const aria_graph_edge* edges,
                        int n_edges, int iterations, aria_graph_result* result) {
    return graph_lm_optimize<Se3Host>(h, poses_inout, n_vertices, fixed_index, edges, n_edges, iterations, result);
}

int aria_graph_debug_linearize(aria_graph_t h, const double* poses, int n_vertices, int fixed_index, const aria_graph_edge* edges,
                               int n_edges, double* chi2, double* b, double* H_diag, double* H_off) {
    return graph_lm_debug_linearize<Se3Host>(h, poses, n_vertices, fixed_index, edges, n_edges, chi2, b, H_diag, H_off);
}

}  // extern "C"
