// The pose-graph Levenberg-Marquardt solver of the SE(3) and Sim(3) stages (k_graph_lm of graph_optimize.hip, k_sgraph_lm of
// sim3_graph.hip): one definition of the scratch layout, of the device pieces of the schedule and of the host calls around
// the kernel. Not part of the public interface. Every device function is inlined into the including file's kernel.
//
// The schedule both kernels follow: ONE WORKGROUP PER GRAPH, persistent over every LM iteration of its graph, workgroup
// barriers only. Nothing waits on another workgroup, so a stage makes progress whatever else shares the device.
//   stage     validate the counts, the edges (before any vertex is read) and, where the stage has some, the vertex scales; build
//             the vertex -> incident-edge adjacency (build_adjacency: CSR by integer atomics, each list then sorted by edge index
//             and direction: the fixed gather order).
//   linearise one lane per edge (edge_pass over the stage's edge_blocks): e, Ji, Jj in registers, stores w Ji^T Ji, w Jj^T Jj,
//             W = w Ji^T Jj, w Ji^T e, w Jj^T e; then one lane per vertex gathers its diagonal block and its b over its incident
//             edges (vertex_gather). H is never scattered.
//   PCG       block-Jacobi (precond_build, precond_apply) preconditioned conjugate gradients on (H + lambda I) dx = b. The row of
//             H p is a gather over the vertex's edges, reading the entries of W that are not structurally zero; dot products are a
//             per-lane sum in vertex order, a wave butterfly and a fixed 8-way sum through LDS (solver_device.h). pcg_solve is the
//             form for any size: the five vectors in the handle's HBM scratch (structure of arrays, L2-resident), every lane owns
//             the vertices v = lane + k * BLOCK. graph_optimize.hip has two more forms of the same arithmetic (pcg_small).
//   trial     update the vertices, evaluate chi2_new with the pass that linearises (into the other W buffer, so a rejected trial
//             restores nothing but the vertices and an accepted one has paid for its edges once).
// fp64 throughout, no float atomics, no grid-wide barrier; every result is bitwise reproducible and independent of where the
// graph sits in a batch.
//
// A stage is a traits struct T:
//   NB, VDBL, BLOCK       block size (6 / 7), doubles of a vertex record (12 / 13), lanes of the workgroup (512)
//   FRESH                 the scratch strides go through an opaque scalar copy wherever addresses are formed (lm_stride)
//   FULL_BLOCKS           precond_build reads all of D and writes all of Minv (else the triangles the solver reads)
//   Edge, Params, Scratch = GraphScratch<NB, VDBL>
//   w_nz(r, c)            the entries of W that are not structurally zero (27 / 31)
//   edge_blocks(verts, edge, S, W, k, params)   one edge: error, Jacobians, its blocks stored at edge slot k; returns w e.e
// and for the host calls, which come after the kernel, a struct derived from it that adds
//   Handle, Result, kernel, lds_bytes, last_arg, verts, check   the launch, the staging of one graph, the deferred error
//   edge_bad, vertex_bad  what the stage rejects beyond the indices and the information scale
//
// The rule is that of solver_device.h: a piece lives here only if every kernel of the two files passes tools/isa_compare.py
// against the parent with the code written out -- the same instruction count, opcode histogram, registers, scratch, LDS and
// occupancy, in the product and the variants build (profiles/graph_lm_isa_compare.txt). k_graph_lm (17845 instructions, 224
// VGPRs, 2856 scalar-register moves to and from vector lanes) is the kernel that decides: its register allocation answers
// to any change in the order of its intermediate code. Tried, failed the rule in k_graph_lm, and therefore still written out
// in both files:
//   the kernel body as one `template <typename T> __device__` function (result, validation, early exits, adjacency,
//     linearisation, the LM trial loop; the predicates, the vertex step and the solve as trait hooks): 17845 -> 17992. Its
//     changes one at a time, each in the otherwise written-out kernel:
//       the vertex pointer formed before the validation, as k_sgraph_lm needs it: 17813 (17836 without the select on `bad`);
//       the edge predicate through a __host__ __device__ helper and a vertex loop that is empty for SE(3): 17822; the
//         predicate written out with only the stage's part a hook: 17844; the whole predicate as the stage's hook, the
//         vertex loop under `if constexpr`, together with the solve hook below: 17855 and 226 VGPRs;
//       the three-way solver choice as a hook T::solve (early returns, one return, __forceinline__: all the same): 17876;
//       the vertex step with its backup and the restore of a rejected trial as two helpers: 17845, but seven opcode counts
//         differ; either one alone: 226 VGPRs.
//   the tail of edge_blocks (w Ji^T Ji, w Jj^T Jj, w Ji^T Jj, the two gradients and their stores) as one helper over
//     T::ji_nz / T::jj_nz, constant `true` for SE(3): 17866, also __forceinline__, with __restrict__ and without predicates.
//   precond_build in k_sgraph_lm's form alone (lower triangle read through sym_idx, no zero-fill of Li): 18406 and 12 bytes
//     of scratch. It is here with FULL_BLOCKS, which reproduces each kernel's own read form.
// Nothing was tried on k_sgraph_lm that had failed in k_graph_lm.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "solver_device.h"
#include "stage_handle.h"

namespace aria {

// per-graph slice of the handle's scratch; vertex arrays are [component][Vc], edge arrays [component][Ec]
template <int NB, int VDBL>
struct GraphScratch {
    static constexpr int NB2 = NB * NB;
    static constexpr int EDGE_DOUBLES = NB2 * 4 + 2 * NB;            // A, B, W[2], gi, gj per edge
    static constexpr int VERT_DOUBLES = VDBL + NB2 + NB2 + NB * 5;   // backup, D, Minv, b, x, r, p, Ap per vertex
    static constexpr int D_AT = VDBL, B_AT = VDBL + 2 * NB2;         // D and b in the vertex slice, in units of Vc
    static constexpr int W0_AT = 2 * NB2;                            // W0 in the edge slice, in units of Ec
    double *bak, *D, *Mi, *b, *x, *r, *p, *Ap;
    double *A, *B, *W0, *W1, *gi, *gj;
    int *aoff, *cur, *adj, *nbr;   // CSR offsets, fill cursors, (2 * edge + direction) per entry, its neighbour vertex
    int Vc, Ec;

    __host__ __device__ static size_t int_words(int Vc, int Ec) { return 2 * ((size_t)Vc + 1) + 4 * (size_t)Ec; }

    __device__ static GraphScratch of(double* vbase, double* ebase, int* ibase, int slot, int Vc, int Ec) {
        GraphScratch s;
        double* v = vbase + (size_t)slot * VERT_DOUBLES * Vc;
        s.bak = v;            s.D = s.bak + VDBL * (size_t)Vc;  s.Mi = s.D + NB2 * (size_t)Vc;  s.b = s.Mi + NB2 * (size_t)Vc;
        s.x = s.b + NB * (size_t)Vc;  s.r = s.x + NB * (size_t)Vc;  s.p = s.r + NB * (size_t)Vc;  s.Ap = s.p + NB * (size_t)Vc;
        double* e = ebase + (size_t)slot * EDGE_DOUBLES * Ec;
        s.A = e;              s.B = s.A + NB2 * (size_t)Ec;     s.W0 = s.B + NB2 * (size_t)Ec;  s.W1 = s.W0 + NB2 * (size_t)Ec;
        s.gi = s.W1 + NB2 * (size_t)Ec;  s.gj = s.gi + NB * (size_t)Ec;
        int* i = ibase + (size_t)slot * int_words(Vc, Ec);
        s.aoff = i;           s.cur = i + Vc + 1;               s.adj = s.cur + Vc + 1;         s.nbr = s.adj + 2 * (size_t)Ec;
        s.Vc = Vc;            s.Ec = Ec;
        return s;
    }
};

// ---- reductions: per-lane partial (vertex order), then block_sum2 / block_sum / block_max of solver_device.h
struct LmRed {
    double* lds;      // [2][2][BLOCK / 64]
    int phase;
};

// A scratch stride. FRESH: through an opaque copy, taken inside every loop body that forms component addresses from it. The
// strides are invariant over the whole kernel, and the few hundred scalar addresses derived from them (49 per block array of
// k_sgraph_lm) would otherwise be hoisted out of the LM loops and held -- spilled -- across everything else. Formed where they
// are used they cost a scalar multiply each.
template <bool FRESH>
__device__ inline size_t lm_stride(int stride) {
    if constexpr (FRESH) asm volatile("" : "+s"(stride));
    return (size_t)stride;
}

// D and Minv are symmetric bit for bit (each entry is the same sum of commuting products), so the solver reads their upper
// triangles only
template <int N>
__device__ constexpr int sym_idx(int a, int c) { return a <= c ? N * a + c : N * c + a; }

// ---- SE(3) pieces (graph_ref.py: quat_from_rot, rot_from_quat, oplus) ---------------------------------------------------
// q = (x, y, z, w), unit, w >= 0
__device__ inline void unit_quat_from_rot(const double* R, double& qx, double& qy, double& qz, double& qw) {
    const double tr = R[0] + R[4] + R[8];
    double x, y, z, w;
    if (tr > 0) {
        const double s = sqrt(tr + 1.0) * 2;
        x = (R[7] - R[5]) / s;  y = (R[2] - R[6]) / s;  z = (R[3] - R[1]) / s;  w = 0.25 * s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2;
        x = 0.25 * s;  y = (R[1] + R[3]) / s;  z = (R[2] + R[6]) / s;  w = (R[7] - R[5]) / s;
    } else if (R[4] >= R[8]) {
        const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2;
        x = (R[1] + R[3]) / s;  y = 0.25 * s;  z = (R[5] + R[7]) / s;  w = (R[2] - R[6]) / s;
    } else {
        const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2;
        x = (R[2] + R[6]) / s;  y = (R[5] + R[7]) / s;  z = 0.25 * s;  w = (R[3] - R[1]) / s;
    }
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x /= n;  y /= n;  z /= n;  w /= n;
    if (w < 0) { x = -x;  y = -y;  z = -z;  w = -w; }
    qx = x;  qy = y;  qz = z;  qw = w;
}

__device__ inline void rot_from_quat(double x, double y, double z, double w, double* R) {
    R[0] = 1 - 2 * (y * y + z * z);  R[1] = 2 * (x * y - z * w);      R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);      R[4] = 1 - 2 * (x * x + z * z);  R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);      R[7] = 2 * (y * z + x * w);      R[8] = 1 - 2 * (x * x + y * y);
}

// pose rows [R t] (12 doubles) -> R[9], t[3]
__device__ inline void load_pose(const double* P, double* R, double* t) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        R[3 * r] = P[4 * r];  R[3 * r + 1] = P[4 * r + 1];  R[3 * r + 2] = P[4 * r + 2];  t[r] = P[4 * r + 3];
    }
}

// C = A^T B (3x3)
__device__ inline void mul_tn(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ inline void mul_nn(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// y = A^T v
__device__ inline void mulv_t(const double* A, const double* v, double* y) {
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}

// the rotation part of a vertex step: R <- R * R(d[3..5]), re-orthonormalised through its unit quaternion (Rn)
__device__ inline void rotation_update(const double* R, const double* d, double* Rn) {
    const double n2 = d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    double qx, qy, qz, qw;
    if (n2 > 1.0) {
        const double n = sqrt(n2);
        qx = -d[3] / n;  qy = -d[4] / n;  qz = -d[5] / n;  qw = 0.0;
    } else {
        qx = d[3];  qy = d[4];  qz = d[5];  qw = sqrt(1.0 - n2);
    }
    double Rd[9];
    rot_from_quat(qx, qy, qz, qw, Rd);
    mul_nn(R, Rd, Rn);
    unit_quat_from_rot(Rn, qx, qy, qz, qw);
    rot_from_quat(qx, qy, qz, qw, Rn);
}

// every edge of the graph; returns chi2 (identical in every lane)
template <typename T>
__device__ inline double edge_pass(LmRed& R, const double* verts, const typename T::Edge* __restrict__ edges, int ne,
                                   const typename T::Scratch& S, double* W, const typename T::Params& prm) {
    double part = 0.0;
    for (int k = threadIdx.x; k < ne; k += T::BLOCK) part += T::edge_blocks(verts, edges[k], S, W, k, prm);
    return block_sum<T::BLOCK / 64>(R.lds, R.phase, part);   // its barrier also publishes the blocks to the workgroup
}

// ---- adjacency: counts (integer atomics), block scan, fill, then every list sorted -> a fixed gather order ------------------
template <typename T>
__device__ inline void build_adjacency(const typename T::Scratch& S, const typename T::Edge* edges, int nv, int ne, int* scan) {
    constexpr int BLOCK = T::BLOCK;
    const int tid = threadIdx.x;
    for (int v = tid; v <= nv; v += BLOCK) S.aoff[v] = 0;
    __syncthreads();
    for (int k = tid; k < ne; k += BLOCK) {
        atomicAdd(&S.aoff[edges[k].from], 1);
        atomicAdd(&S.aoff[edges[k].to], 1);
    }
    __syncthreads();
    {
        const int chunk = (nv + BLOCK - 1) / BLOCK;
        const int lo = min(tid * chunk, nv), hi = min(lo + chunk, nv);
        int sum = 0;
        for (int v = lo; v < hi; v++) sum += S.aoff[v];
        scan[tid] = sum;
        __syncthreads();
        for (int off = 1; off < BLOCK; off <<= 1) {
            const int add = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        int run = scan[tid] - sum;              // exclusive prefix of this lane's chunk
        for (int v = lo; v < hi; v++) {
            const int dgr = S.aoff[v];
            S.aoff[v] = run;
            S.cur[v] = run;
            run += dgr;
        }
        if (tid == BLOCK - 1) S.aoff[nv] = scan[BLOCK - 1];
        __syncthreads();
    }
    for (int k = tid; k < ne; k += BLOCK) {
        S.adj[atomicAdd(&S.cur[edges[k].from], 1)] = 2 * k;
        S.adj[atomicAdd(&S.cur[edges[k].to], 1)] = 2 * k + 1;
    }
    __syncthreads();
    for (int v = tid; v < nv; v += BLOCK) {
        const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
        for (int a = a0 + 1; a < a1; a++) {
            const int key = S.adj[a];
            int c = a - 1;
            while (c >= a0 && S.adj[c] > key) { S.adj[c + 1] = S.adj[c];  c--; }
            S.adj[c + 1] = key;
        }
    }
    __syncthreads();
    for (int a = tid; a < 2 * ne; a += BLOCK) {
        const int code = S.adj[a];
        S.nbr[a] = (code & 1) ? edges[code >> 1].from : edges[code >> 1].to;
    }
    __syncthreads();
}

// every vertex gathers D and b over its incident edges in adjacency order; returns max diag(D) over the free vertices
template <typename T>
__device__ inline double vertex_gather(LmRed& R, int nv, int fixed, const typename T::Scratch& S) {
    constexpr int NB = T::NB, NB2 = NB * NB;
    double mx = 0.0;
    for (int v = threadIdx.x; v < nv; v += T::BLOCK) {
        const size_t Vc = lm_stride<T::FRESH>(S.Vc), Ec = lm_stride<T::FRESH>(S.Ec);
        double D[NB2], b[NB];
#pragma unroll
        for (int c = 0; c < NB2; c++) D[c] = 0.0;
#pragma unroll
        for (int c = 0; c < NB; c++) b[c] = 0.0;
        const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
        for (int a = a0; a < a1; a++) {
            const int code = S.adj[a];
            const size_t k = (size_t)(code >> 1);
            const double* blk = (code & 1) ? S.B : S.A;
            const double* g = (code & 1) ? S.gj : S.gi;
#pragma unroll
            for (int c = 0; c < NB2; c++) D[c] += blk[c * Ec + k];
#pragma unroll
            for (int c = 0; c < NB; c++) b[c] -= g[c * Ec + k];
        }
#pragma unroll
        for (int c = 0; c < NB2; c++) S.D[c * Vc + v] = D[c];
#pragma unroll
        for (int c = 0; c < NB; c++) S.b[c * Vc + v] = b[c];
        if (v != fixed) {
#pragma unroll
            for (int c = 0; c < NB; c++) mx = fmax(mx, D[(NB + 1) * c]);
        }
    }
    return block_max<T::BLOCK / 64>(R.lds, R.phase, mx);
}

// ---- preconditioner: inverse of the damped diagonal blocks (the separable step: swap this and precond_apply) ------------
// Cholesky in registers, one vertex per lane. A block that is not positive definite preconditions with 0.
// FULL_BLOCKS: every entry of D is read, Li is zero-filled and every entry of Minv written; else the lower triangle of D is
// read through its upper one and the upper triangle of Minv written, which is all the solver reads.
template <typename T>
__device__ inline void precond_build(int nv, double lambda, const typename T::Scratch& S) {
    constexpr int NB = T::NB, NB2 = NB * NB;
    constexpr bool FULL = T::FULL_BLOCKS;
    for (int v = threadIdx.x; v < nv; v += T::BLOCK) {
        const size_t Vc = lm_stride<T::FRESH>(S.Vc);
        double L[NB2];
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int j = 0; j <= (FULL ? NB - 1 : i); j++) L[NB * i + j] = S.D[(FULL ? NB * i + j : sym_idx<NB>(i, j)) * Vc + v];
#pragma unroll
        for (int c = 0; c < NB; c++) L[(NB + 1) * c] += lambda;
        bool ok = true;
#pragma unroll
        for (int j = 0; j < NB; j++) {
            double d = L[(NB + 1) * j];
#pragma unroll
            for (int k = 0; k < j; k++) d -= L[NB * j + k] * L[NB * j + k];
            ok = ok && (d > 0.0) && (d < INFINITY);
            const double l = sqrt(ok ? d : 1.0);
            L[(NB + 1) * j] = l;
#pragma unroll
            for (int i = j + 1; i < NB; i++) {
                double t = L[NB * i + j];
#pragma unroll
                for (int k = 0; k < j; k++) t -= L[NB * i + k] * L[NB * j + k];
                L[NB * i + j] = t / l;
            }
        }
        // Li = L^-1 (lower), Minv = Li^T Li
        double Li[NB2];
        if (FULL) {
#pragma unroll
            for (int c = 0; c < NB2; c++) Li[c] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < NB; j++) {
            Li[(NB + 1) * j] = 1.0 / L[(NB + 1) * j];
#pragma unroll
            for (int i = j + 1; i < NB; i++) {
                double t = 0.0;
#pragma unroll
                for (int k = j; k < i; k++) t -= L[NB * i + k] * Li[NB * k + j];
                Li[NB * i + j] = t / L[(NB + 1) * i];
            }
        }
#pragma unroll
        for (int a = 0; a < NB; a++)
#pragma unroll
            for (int c = (FULL ? 0 : a); c < NB; c++) {
                double t = 0.0;
#pragma unroll
                for (int k = (a > c ? a : c); k < NB; k++) t += Li[NB * k + a] * Li[NB * k + c];
                S.Mi[(NB * a + c) * Vc + v] = ok ? t : 0.0;
            }
    }
}

template <typename T>
__device__ inline void precond_apply(const typename T::Scratch& S, size_t Vc, int v, const double* r, double* z) {
    constexpr int NB = T::NB;
#pragma unroll
    for (int a = 0; a < NB; a++) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < NB; c++) t += S.Mi[sym_idx<NB>(a, c) * Vc + v] * r[c];    // symmetric: the upper triangle is read
        z[a] = t;
    }
}

// ---- PCG on (H + lambda I) x = b, the fixed vertex removed. Returns the iterations; x in S.x ------------------------------
template <typename T>
__device__ inline int pcg_solve(LmRed& R, int nv, int fixed, double lambda, const double* W, const typename T::Scratch& S,
                                int max_iters, double rel_tol) {
    constexpr int NB = T::NB, BLOCK = T::BLOCK, WAVES = BLOCK / 64;
    constexpr bool FRESH = T::FRESH;
    double rz = 0.0, bb = 0.0;
    for (int v = threadIdx.x; v < nv; v += BLOCK) {
        const size_t Vc = lm_stride<FRESH>(S.Vc);
        double r[NB], z[NB];
#pragma unroll
        for (int c = 0; c < NB; c++) r[c] = (v == fixed) ? 0.0 : S.b[c * Vc + v];
        precond_apply<T>(S, Vc, v, r, z);
#pragma unroll
        for (int c = 0; c < NB; c++) {
            if (v == fixed) z[c] = 0.0;
            S.x[c * Vc + v] = 0.0;
            S.r[c * Vc + v] = r[c];
            S.p[c * Vc + v] = z[c];
            rz += r[c] * z[c];
            bb += r[c] * r[c];
        }
    }
    block_sum2<WAVES>(R.lds, R.phase, rz, bb);   // barrier: p is visible to the workgroup
    if (!(bb > 0.0)) return 0;
    const double stop = rel_tol * rel_tol * bb;
    int iters = 0;
    for (int it = 1; it <= max_iters; it++) {
        // Ap = (H + lambda I) p: the vertex's row, gathered over its incident edges
        double pAp = 0.0;
        for (int v = threadIdx.x; v < nv; v += BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = lm_stride<FRESH>(S.Vc), Ec = lm_stride<FRESH>(S.Ec);
            double p[NB], y[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) p[c] = S.p[c * Vc + v];
#pragma unroll
            for (int a = 0; a < NB; a++) {
                double t = lambda * p[a];
#pragma unroll
                for (int c = 0; c < NB; c++) t += S.D[sym_idx<NB>(a, c) * Vc + v] * p[c];
                y[a] = t;
            }
            const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
            for (int a = a0; a < a1; a++) {
                const int code = S.adj[a];
                const size_t k = (size_t)(code >> 1);
                const int other = S.nbr[a];
                double q[NB];
#pragma unroll
                for (int c = 0; c < NB; c++) q[c] = S.p[c * Vc + other];
                if (code & 1) {                      // v is the edge's `to`: W^T p_from
#pragma unroll
                    for (int c = 0; c < NB; c++)
#pragma unroll
                        for (int r2 = 0; r2 < NB; r2++)
                            if (T::w_nz(r2, c)) y[c] += W[(NB * r2 + c) * Ec + k] * q[r2];
                } else {                             // v is the edge's `from`: W p_to
#pragma unroll
                    for (int r2 = 0; r2 < NB; r2++)
#pragma unroll
                        for (int c = 0; c < NB; c++)
                            if (T::w_nz(r2, c)) y[r2] += W[(NB * r2 + c) * Ec + k] * q[c];
                }
            }
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.Ap[c * Vc + v] = y[c];
                pAp += p[c] * y[c];
            }
        }
        pAp = block_sum<WAVES>(R.lds, R.phase, pAp);
        if (!(pAp > 0.0)) break;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        for (int v = threadIdx.x; v < nv; v += BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = lm_stride<FRESH>(S.Vc);
            double r[NB], z[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.x[c * Vc + v] += alpha * S.p[c * Vc + v];
                r[c] = S.r[c * Vc + v] - alpha * S.Ap[c * Vc + v];
                S.r[c * Vc + v] = r[c];
            }
            precond_apply<T>(S, Vc, v, r, z);
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.Ap[c * Vc + v] = z[c];             // Ap is free until the next product: it carries z to the p update
                rr += r[c] * r[c];
                rzn += r[c] * z[c];
            }
        }
        block_sum2<WAVES>(R.lds, R.phase, rr, rzn);
        iters = it;
        if (rr <= stop) break;
        const double beta = rzn / rz;
        rz = rzn;
        for (int v = threadIdx.x; v < nv; v += BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = lm_stride<FRESH>(S.Vc);
#pragma unroll
            for (int c = 0; c < NB; c++) S.p[c * Vc + v] = S.Ap[c * Vc + v] + beta * S.p[c * Vc + v];
        }
        __syncthreads();                             // p is visible before the next product gathers it
    }
    return iters;
}

// ---- the host calls around the kernel ---------------------------------------------------------------------------------------
// More graphs than the handle has scratch for run as consecutive launches on the stream; a graph's result does not depend on
// which launch or which slot it gets.
template <typename T>
void graph_lm_launch(typename T::Handle* h, double* d_verts, const int* d_voff, const typename T::Edge* d_edges, const int* d_eoff,
                     const int* d_fixed, int n_graphs, int iterations, typename T::Result* d_results, int mode) {
    const auto& c = h->cfg;
    for (int base = 0; base < n_graphs; base += c.max_graphs) {
        const int n = std::min(c.max_graphs, n_graphs - base);
        hipLaunchKernelGGL(T::kernel, dim3(n), dim3(T::BLOCK), T::lds_bytes(h), h->stream, d_verts, d_voff, d_edges, d_eoff,
                           d_fixed, base, iterations, c.max_vertices, c.max_edges, c.pcg_max_iters, c.pcg_rel_tol, h->d_v, h->d_e,
                           h->d_i, d_results, h->d_err, mode, T::last_arg(h));
    }
}

// uploads one graph (host buffers) into the single-graph staging; rejects what the kernel would on the host
template <typename T>
int graph_lm_stage_single(typename T::Handle* h, const double* verts, int nv, int fixed, const typename T::Edge* edges, int ne) {
    if (nv < 0 || ne < 0 || (nv && !verts) || (ne && !edges)) return ARIA_E_INVALID;
    if (nv > h->cfg.max_vertices || ne > h->cfg.max_edges) return ARIA_E_TOO_LARGE;
    if ((nv > 0 && (fixed < 0 || fixed >= nv)) || (nv == 0 && ne > 0)) return ARIA_E_INVALID;
    for (int k = 0; k < ne; k++)
        if (edges[k].from < 0 || edges[k].from >= nv || edges[k].to < 0 || edges[k].to >= nv || edges[k].from == edges[k].to ||
            !(edges[k].info_scale >= 0.0) || !std::isfinite(edges[k].info_scale) || T::edge_bad(edges[k]))
            return ARIA_E_INVALID;
    for (int v = 0; v < nv; v++)
        if (T::vertex_bad(verts + T::VDBL * (size_t)v)) return ARIA_E_INVALID;
    const int off[5] = {0, nv, 0, ne, fixed};
    if (nv) ARIA_HIP(hipMemcpyAsync(T::verts(h), verts, sizeof(double) * T::VDBL * (size_t)nv, hipMemcpyHostToDevice, h->stream));
    if (ne) ARIA_HIP(hipMemcpyAsync(h->d_edges, edges, sizeof(typename T::Edge) * (size_t)ne, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_off, off, sizeof(off), hipMemcpyHostToDevice));
    return ARIA_OK;
}

// the device memory of a handle: the scratch of max_graphs graphs and the staging of one
template <typename T>
int graph_lm_reserve(typename T::Handle* h, const char* what) {
    using Sc = typename T::Scratch;
    const auto& c = h->cfg;
    const size_t G = (size_t)c.max_graphs, V = (size_t)c.max_vertices, E = (size_t)c.max_edges;
    int rc;
    if ((rc = h->d_v.reserve(h->stream, G * V * Sc::VERT_DOUBLES, what)) != ARIA_OK) return rc;
    if ((rc = h->d_e.reserve(h->stream, G * E * Sc::EDGE_DOUBLES, what)) != ARIA_OK) return rc;
    if ((rc = h->d_i.reserve(h->stream, G * Sc::int_words(c.max_vertices, c.max_edges), what)) != ARIA_OK) return rc;
    if ((rc = T::verts(h).reserve(h->stream, V * T::VDBL, what)) != ARIA_OK) return rc;
    if ((rc = h->d_edges.reserve(h->stream, E, what)) != ARIA_OK) return rc;
    if ((rc = h->d_off.reserve(h->stream, 8, what)) != ARIA_OK) return rc;
    return h->d_res.reserve(h->stream, 1, what);
}

template <typename T>
int graph_lm_optimize_batch_device(typename T::Handle* h, double* d_verts, const int* d_vertex_offset, const typename T::Edge* d_edges,
                                   const int* d_edge_offset, const int* d_fixed, int n_graphs, int iterations,
                                   typename T::Result* d_results) {
    if (!h || !d_verts || !d_vertex_offset || !d_edges || !d_edge_offset || !d_fixed || !d_results || n_graphs < 0 ||
        iterations < 0)
        return ARIA_E_INVALID;
    if (n_graphs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    graph_lm_launch<T>(h, d_verts, d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs, iterations, d_results, 0);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

template <typename T>
int graph_lm_optimize(typename T::Handle* h, double* verts_inout, int n_vertices, int fixed_index, const typename T::Edge* edges,
                      int n_edges, int iterations, typename T::Result* result) {
    if (!h || !result || iterations < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = graph_lm_stage_single<T>(h, verts_inout, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    graph_lm_launch<T>(h, T::verts(h), h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, iterations, h->d_res, 0);
    ARIA_HIP(hipGetLastError());
    if (n_vertices)
        ARIA_HIP(hipMemcpyAsync(verts_inout, T::verts(h), sizeof(double) * T::VDBL * (size_t)n_vertices, hipMemcpyDeviceToHost,
                                h->stream));
    ARIA_HIP(hipMemcpyAsync(result, h->d_res, sizeof(typename T::Result), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return T::check(h);
}

template <typename T>
int graph_lm_debug_linearize(typename T::Handle* h, const double* verts, int n_vertices, int fixed_index, const typename T::Edge* edges,
                             int n_edges, double* chi2, double* b, double* H_diag, double* H_off) {
    using Sc = typename T::Scratch;
    constexpr int NB = T::NB, NB2 = Sc::NB2;
    if (!h || !chi2 || !b || !H_diag || !H_off) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = graph_lm_stage_single<T>(h, verts, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    graph_lm_launch<T>(h, T::verts(h), h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, 0, h->d_res, 1);
    ARIA_HIP(hipGetLastError());
    const size_t Vc = (size_t)h->cfg.max_vertices, Ec = (size_t)h->cfg.max_edges;
    std::vector<double> D(NB2 * Vc), bb(NB * Vc), W(NB2 * Ec);
    typename T::Result res;
    // slot 0 of the scratch, at the offsets of GraphScratch::of
    ARIA_HIP(hipMemcpyAsync(D.data(), h->d_v + Sc::D_AT * Vc, sizeof(double) * NB2 * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(bb.data(), h->d_v + Sc::B_AT * Vc, sizeof(double) * NB * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(W.data(), h->d_e + Sc::W0_AT * Ec, sizeof(double) * NB2 * Ec, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(&res, h->d_res, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    *chi2 = res.chi2_initial;
    for (int v = 0; v < n_vertices; v++) {
        for (int c = 0; c < NB2; c++) H_diag[NB2 * (size_t)v + c] = D[c * Vc + v];
        for (int c = 0; c < NB; c++) b[NB * (size_t)v + c] = bb[c * Vc + v];
    }
    for (int k = 0; k < n_edges; k++)
        for (int c = 0; c < NB2; c++) H_off[NB2 * (size_t)k + c] = W[c * Ec + k];
    return T::check(h);
}

}  // namespace aria
