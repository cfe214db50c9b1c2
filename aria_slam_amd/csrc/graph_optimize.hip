// SE(3) pose-graph optimisation, batched over graphs (include/aria_orb_hip.h, "SE(3) pose-graph optimisation"): what the
// reference's PoseGraphOptimizer (src/legacy/LoopClosure.cpp:197-312) asks of g2o -- VertexSE3 / EdgeSE3 under
// Levenberg-Marquardt, first vertex fixed. aria_slam_amd/graph_ref.py is the specification; DESIGN.md section 13 the record.
//
// One kernel, k_graph_lm: ONE WORKGROUP PER GRAPH, persistent over every LM iteration of its graph, workgroup barriers
// only. Nothing waits on another workgroup, so the stage makes progress whatever else shares the device.
//   stage     validate the counts and the edges (before any pose is read), build the vertex -> incident-edge adjacency (CSR,
//             each list sorted by edge index and direction: the fixed gather order).
//   linearise one lane per edge: e, Ji, Jj in registers, stores s Ji^T Ji, s Jj^T Jj, W = s Ji^T Jj, s Ji^T e, s Jj^T e;
//             then one lane per vertex gathers its diagonal block and its b over its incident edges. H is never scattered.
//   PCG       block-Jacobi preconditioned conjugate gradients on (H + lambda I) dx = b. The row of H p is a gather over the
//             vertex's edges; dot products are a per-lane sum in vertex order, a wave butterfly and a fixed 8-way sum
//             through LDS. Three forms of the one solve, the same arithmetic in the same order (the choice changes no bit):
//             pcg_solve, any size: the five vectors in the handle's HBM scratch (structure of arrays, L2-resident), every
//             lane owns the vertices v = lane + k * 512; pcg_small<false>, up to 512 vertices: one vertex per lane, its
//             diagonal and preconditioner blocks, r and p in registers; pcg_small<true>, also at most 544 edges: W and p in
//             LDS (142 KB), so an iteration reads HBM for the adjacency only.
//   trial     update the poses, evaluate chi2_new with the pass that linearises (into the other W buffer, so a rejected
//             trial restores nothing but the poses and an accepted one has paid for its edges once).
// fp64 throughout, no float atomics (the adjacency counts are integer atomics followed by a sort), every result bitwise
// reproducible and independent of where the graph sits in a batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "solver_device.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int GRAPH_BLOCK = 512;          // 8 waves: 2 per SIMD, 256 VGPRs each
constexpr int GRAPH_WAVES = GRAPH_BLOCK / 64;
constexpr int ERRBIT_GRAPH_INPUT = 1;     // counts, fixed index or an edge out of range (graph skipped)
constexpr int ERRBIT_GRAPH_LARGE = 2;     // more vertices or edges than the handle was created for (graph skipped)
constexpr int GRAPH_LDS_EDGES = 544;      // edges whose W fits the LDS beside p: 27 * 544 * 8 + 6 * 512 * 8 = 142080 bytes of 160 KiB
constexpr int EDGE_DOUBLES = 36 * 4 + 12; // A, B, W[2], gi, gj per edge
constexpr int VERT_DOUBLES = 12 + 36 + 36 + 6 * 5;   // backup, D, Minv, b, x, r, p, Ap per vertex

// per-graph slice of the handle's scratch; vertex arrays are [component][Vc], edge arrays [component][Ec]
struct Scratch {
    double *bak, *D, *Mi, *b, *x, *r, *p, *Ap;
    double *A, *B, *W0, *W1, *gi, *gj;
    int *aoff, *cur, *adj, *nbr;   // CSR offsets, fill cursors, (2 * edge + direction) per entry, its neighbour vertex
    int Vc, Ec;
};

__host__ __device__ inline size_t graph_lds_bytes(int wlds_edges) {
    return wlds_edges > 0 ? (27 * (size_t)wlds_edges + 6 * (size_t)GRAPH_BLOCK) * sizeof(double) : 0;
}
__host__ __device__ inline size_t graph_int_words(int Vc, int Ec) { return 2 * ((size_t)Vc + 1) + 4 * (size_t)Ec; }

__device__ inline Scratch scratch_of(double* vbase, double* ebase, int* ibase, int slot, int Vc, int Ec) {
    Scratch s;
    double* v = vbase + (size_t)slot * VERT_DOUBLES * Vc;
    s.bak = v;            s.D = s.bak + 12 * (size_t)Vc;  s.Mi = s.D + 36 * (size_t)Vc;  s.b = s.Mi + 36 * (size_t)Vc;
    s.x = s.b + 6 * (size_t)Vc;  s.r = s.x + 6 * (size_t)Vc;  s.p = s.r + 6 * (size_t)Vc;  s.Ap = s.p + 6 * (size_t)Vc;
    double* e = ebase + (size_t)slot * EDGE_DOUBLES * Ec;
    s.A = e;              s.B = s.A + 36 * (size_t)Ec;    s.W0 = s.B + 36 * (size_t)Ec;  s.W1 = s.W0 + 36 * (size_t)Ec;
    s.gi = s.W1 + 36 * (size_t)Ec;  s.gj = s.gi + 6 * (size_t)Ec;
    int* i = ibase + (size_t)slot * graph_int_words(Vc, Ec);
    s.aoff = i;           s.cur = i + Vc + 1;             s.adj = s.cur + Vc + 1;        s.nbr = s.adj + 2 * (size_t)Ec;
    s.Vc = Vc;            s.Ec = Ec;
    return s;
}

// ---- reductions: per-lane partial (vertex order), then block_sum2 / block_sum / block_max<GRAPH_WAVES> of solver_device.h
struct Red {
    double* lds;      // [2][2][GRAPH_WAVES]
    int phase;
};

// ---- SE(3) pieces (graph_ref.py: quat_from_rot, rot_from_quat, oplus) ---------------------------------------------------
// q = (x, y, z, w), unit, w >= 0
__device__ inline void quat_from_rot(const double* R, double& qx, double& qy, double& qz, double& qw) {
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

// ---- one edge: error, Jacobians and its blocks ------------------------------------------------------------------------
// Returns s * e.e. Stores A = s Ji^T Ji, B = s Jj^T Jj, W = s Ji^T Jj, gi = s Ji^T e, gj = s Jj^T e at edge slot k.
__device__ inline double edge_blocks(const double* poses, const aria_graph_edge& ed, const Scratch& S, double* W,
                                     int k) {
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
    quat_from_rot(Re, qx, qy, qz, qw);
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

// every edge of the graph; returns chi2 (identical in every lane)
__device__ inline double edge_pass(Red& R, const double* poses, const aria_graph_edge* __restrict__ edges, int ne,
                                   const Scratch& S, double* W) {
    double part = 0.0;
    for (int k = threadIdx.x; k < ne; k += GRAPH_BLOCK) part += edge_blocks(poses, edges[k], S, W, k);
    return block_sum<GRAPH_WAVES>(R.lds, R.phase, part);   // its barrier also publishes the blocks to the workgroup
}

// every vertex gathers D and b over its incident edges in adjacency order; returns max diag(D) over the free vertices
__device__ inline double vertex_gather(Red& R, int nv, int fixed, const Scratch& S) {
    const size_t Vc = (size_t)S.Vc, Ec = (size_t)S.Ec;
    double mx = 0.0;
    for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
        double D[36], b[6];
#pragma unroll
        for (int c = 0; c < 36; c++) D[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) b[c] = 0.0;
        const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
        for (int a = a0; a < a1; a++) {
            const int code = S.adj[a];
            const size_t k = (size_t)(code >> 1);
            const double* blk = (code & 1) ? S.B : S.A;
            const double* g = (code & 1) ? S.gj : S.gi;
#pragma unroll
            for (int c = 0; c < 36; c++) D[c] += blk[c * Ec + k];
#pragma unroll
            for (int c = 0; c < 6; c++) b[c] -= g[c * Ec + k];
        }
#pragma unroll
        for (int c = 0; c < 36; c++) S.D[c * Vc + v] = D[c];
#pragma unroll
        for (int c = 0; c < 6; c++) S.b[c * Vc + v] = b[c];
        if (v != fixed) {
#pragma unroll
            for (int c = 0; c < 6; c++) mx = fmax(mx, D[7 * c]);
        }
    }
    return block_max<GRAPH_WAVES>(R.lds, R.phase, mx);
}

// ---- preconditioner: inverse of the damped diagonal blocks (the separable step: swap this and precond_apply) ------------
// Cholesky in registers, one vertex per lane. A block that is not positive definite preconditions with 0.
__device__ inline void precond_build(int nv, double lambda, const Scratch& S) {
    const size_t Vc = (size_t)S.Vc;
    for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
        double L[36];
#pragma unroll
        for (int c = 0; c < 36; c++) L[c] = S.D[c * Vc + v];
#pragma unroll
        for (int c = 0; c < 6; c++) L[7 * c] += lambda;
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double d = L[7 * j];
#pragma unroll
            for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k];
            ok = ok && (d > 0.0) && (d < INFINITY);
            const double l = sqrt(ok ? d : 1.0);
            L[7 * j] = l;
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double t = L[6 * i + j];
#pragma unroll
                for (int k = 0; k < j; k++) t -= L[6 * i + k] * L[6 * j + k];
                L[6 * i + j] = t / l;
            }
        }
        // Li = L^-1 (lower), Minv = Li^T Li
        double Li[36];
#pragma unroll
        for (int c = 0; c < 36; c++) Li[c] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            Li[7 * j] = 1.0 / L[7 * j];
#pragma unroll
            for (int i = j + 1; i < 6; i++) {
                double t = 0.0;
#pragma unroll
                for (int k = j; k < i; k++) t -= L[6 * i + k] * Li[6 * k + j];
                Li[6 * i + j] = t / L[7 * i];
            }
        }
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double t = 0.0;
#pragma unroll
                for (int k = (a > c ? a : c); k < 6; k++) t += Li[6 * k + a] * Li[6 * k + c];
                S.Mi[(6 * a + c) * Vc + v] = ok ? t : 0.0;
            }
    }
}

// D and Minv are symmetric bit for bit (each entry is the same sum of commuting products), so the solver reads their upper
// triangles only: 21 of 36 entries
__device__ constexpr int sym6(int a, int c) { return a <= c ? 6 * a + c : 6 * c + a; }
// W = s Ji^T Jj has a zero block: rows 0..2 x columns 3..5 (Ji's lower-left and Jj's off-diagonal blocks are zero)
__device__ constexpr bool w_zero(int r, int c) { return r < 3 && c >= 3; }
__device__ constexpr int w27(int r, int c) { return r < 3 ? 3 * r + c : 9 + 6 * (r - 3) + c; }    // index among the 27 others

__device__ inline void precond_apply(const Scratch& S, int v, const double* r, double* z) {
    const size_t Vc = (size_t)S.Vc;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) t += S.Mi[sym6(a, c) * Vc + v] * r[c];    // symmetric: the upper triangle is read
        z[a] = t;
    }
}

// ---- PCG on (H + lambda I) x = b, the fixed vertex removed. Returns the iterations; x in S.x ------------------------------
__device__ inline int pcg_solve(Red& R, int nv, int fixed, double lambda, const double* W, const Scratch& S,
                                int max_iters, double rel_tol) {
    const size_t Vc = (size_t)S.Vc, Ec = (size_t)S.Ec;
    double rz = 0.0, bb = 0.0;
    for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
        double r[6], z[6];
#pragma unroll
        for (int c = 0; c < 6; c++) r[c] = (v == fixed) ? 0.0 : S.b[c * Vc + v];
        precond_apply(S, v, r, z);
#pragma unroll
        for (int c = 0; c < 6; c++) {
            if (v == fixed) z[c] = 0.0;
            S.x[c * Vc + v] = 0.0;
            S.r[c * Vc + v] = r[c];
            S.p[c * Vc + v] = z[c];
            rz += r[c] * z[c];
            bb += r[c] * r[c];
        }
    }
    block_sum2<GRAPH_WAVES>(R.lds, R.phase, rz, bb);   // barrier: p is visible to the workgroup
    if (!(bb > 0.0)) return 0;
    const double stop = rel_tol * rel_tol * bb;
    int iters = 0;
    for (int it = 1; it <= max_iters; it++) {
        // Ap = (H + lambda I) p: the vertex's row, gathered over its incident edges
        double pAp = 0.0;
        for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
            if (v == fixed) continue;
            double p[6], y[6];
#pragma unroll
            for (int c = 0; c < 6; c++) p[c] = S.p[c * Vc + v];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double t = lambda * p[a];
#pragma unroll
                for (int c = 0; c < 6; c++) t += S.D[sym6(a, c) * Vc + v] * p[c];
                y[a] = t;
            }
            const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
            for (int a = a0; a < a1; a++) {
                const int code = S.adj[a];
                const size_t k = (size_t)(code >> 1);
                const int other = S.nbr[a];
                double q[6];
#pragma unroll
                for (int c = 0; c < 6; c++) q[c] = S.p[c * Vc + other];
                if (code & 1) {                      // v is the edge's `to`: W^T p_from
#pragma unroll
                    for (int c = 0; c < 6; c++)
#pragma unroll
                        for (int r2 = 0; r2 < 6; r2++)
                            if (!w_zero(r2, c)) y[c] += W[(6 * r2 + c) * Ec + k] * q[r2];
                } else {                             // v is the edge's `from`: W p_to
#pragma unroll
                    for (int r2 = 0; r2 < 6; r2++)
#pragma unroll
                        for (int c = 0; c < 6; c++)
                            if (!w_zero(r2, c)) y[r2] += W[(6 * r2 + c) * Ec + k] * q[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c++) {
                S.Ap[c * Vc + v] = y[c];
                pAp += p[c] * y[c];
            }
        }
        pAp = block_sum<GRAPH_WAVES>(R.lds, R.phase, pAp);
        if (!(pAp > 0.0)) break;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
            if (v == fixed) continue;
            double r[6], z[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                S.x[c * Vc + v] += alpha * S.p[c * Vc + v];
                r[c] = S.r[c * Vc + v] - alpha * S.Ap[c * Vc + v];
                S.r[c * Vc + v] = r[c];
            }
            precond_apply(S, v, r, z);
#pragma unroll
            for (int c = 0; c < 6; c++) {
                S.Ap[c * Vc + v] = z[c];             // Ap is free until the next product: it carries z to the p update
                rr += r[c] * r[c];
                rzn += r[c] * z[c];
            }
        }
        block_sum2<GRAPH_WAVES>(R.lds, R.phase, rr, rzn);
        iters = it;
        if (rr <= stop) break;
        const double beta = rzn / rz;
        rz = rzn;
        for (int v = threadIdx.x; v < nv; v += GRAPH_BLOCK) {
            if (v == fixed) continue;
#pragma unroll
            for (int c = 0; c < 6; c++) S.p[c * Vc + v] = S.Ap[c * Vc + v] + beta * S.p[c * Vc + v];
        }
        __syncthreads();                             // p is visible before the next product gathers it
    }
    return iters;
}

// The same solve for a graph of at most GRAPH_BLOCK vertices: one vertex per lane, so its diagonal block, its preconditioner
// block (upper triangles) and its r and p stay in registers over the whole solve; only p (for the neighbours) and W go through memory. The
// arithmetic and its order are those of pcg_solve: both give the same bits.
// ONCHIP: the graph's W (its 27 entries per edge that are not structurally zero) and p live in LDS for the solve, so an
// iteration touches HBM for the adjacency only.
template <bool ONCHIP>
__device__ inline int pcg_small(Red& R, int nv, int ne, int fixed, double lambda, const double* W, const Scratch& S,
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

// X <- X * fromMQT(d), rotation re-orthonormalised through its unit quaternion
__device__ inline void pose_update(double* P, const double* d) {
    double R[9], t[3];
    load_pose(P, R, t);
    const double n2 = d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    double qx, qy, qz, qw;
    if (n2 > 1.0) {
        const double n = sqrt(n2);
        qx = -d[3] / n;  qy = -d[4] / n;  qz = -d[5] / n;  qw = 0.0;
    } else {
        qx = d[3];  qy = d[4];  qz = d[5];  qw = sqrt(1.0 - n2);
    }
    double Rd[9], Rn[9];
    rot_from_quat(qx, qy, qz, qw, Rd);
    mul_nn(R, Rd, Rn);
    quat_from_rot(Rn, qx, qy, qz, qw);
    rot_from_quat(qx, qy, qz, qw, Rn);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        P[4 * r] = Rn[3 * r];  P[4 * r + 1] = Rn[3 * r + 1];  P[4 * r + 2] = Rn[3 * r + 2];
        P[4 * r + 3] = t[r] + (R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
    }
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------
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
    Red R{red_lds, 0};

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
    const Scratch S = scratch_of(vbase, ebase, ibase, blockIdx.x, max_vertices, max_edges);

    // ---- adjacency: counts (integer atomics), block scan, fill, then every list sorted -> a fixed gather order
    for (int v = tid; v <= nv; v += GRAPH_BLOCK) S.aoff[v] = 0;
    __syncthreads();
    for (int k = tid; k < ne; k += GRAPH_BLOCK) {
        atomicAdd(&S.aoff[edges[k].from], 1);
        atomicAdd(&S.aoff[edges[k].to], 1);
    }
    __syncthreads();
    {
        const int chunk = (nv + GRAPH_BLOCK - 1) / GRAPH_BLOCK;
        const int lo = min(tid * chunk, nv), hi = min(lo + chunk, nv);
        int sum = 0;
        for (int v = lo; v < hi; v++) sum += S.aoff[v];
        scan[tid] = sum;
        __syncthreads();
        for (int off = 1; off < GRAPH_BLOCK; off <<= 1) {
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
        if (tid == GRAPH_BLOCK - 1) S.aoff[nv] = scan[GRAPH_BLOCK - 1];
        __syncthreads();
    }
    for (int k = tid; k < ne; k += GRAPH_BLOCK) {
        S.adj[atomicAdd(&S.cur[edges[k].from], 1)] = 2 * k;
        S.adj[atomicAdd(&S.cur[edges[k].to], 1)] = 2 * k + 1;
    }
    __syncthreads();
    for (int v = tid; v < nv; v += GRAPH_BLOCK) {
        const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
        for (int a = a0 + 1; a < a1; a++) {
            const int key = S.adj[a];
            int c = a - 1;
            while (c >= a0 && S.adj[c] > key) { S.adj[c + 1] = S.adj[c];  c--; }
            S.adj[c + 1] = key;
        }
    }
    __syncthreads();
    for (int a = tid; a < 2 * ne; a += GRAPH_BLOCK) {
        const int code = S.adj[a];
        S.nbr[a] = (code & 1) ? edges[code >> 1].from : edges[code >> 1].to;
    }
    __syncthreads();

    // ---- linearise at the input poses
    int curW = 0;
    double chi2 = edge_pass(R, poses, edges, ne, S, S.W0);
    const double maxdiag = vertex_gather(R, nv, fixed, S);
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
            precond_build(nv, lm.lambda, S);           // each lane builds and later reads its own vertices' blocks
            // three forms of one solve, the same arithmetic in the same order (the choice changes no bit of the result)
            if (nv <= GRAPH_BLOCK && ne <= wlds_edges)
                res.pcg_iterations += pcg_small<true>(R, nv, ne, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol, wlds, wlds_edges);
            else if (nv <= GRAPH_BLOCK)
                res.pcg_iterations += pcg_small<false>(R, nv, ne, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol, wlds, 0);
            else
                res.pcg_iterations += pcg_solve(R, nv, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol);
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
            const double chi2_new = edge_pass(R, poses, edges, ne, S, Wn);
            const double rho = (chi2 - chi2_new) / den;
            if (rho > 0.0 && chi2_new < INFINITY && chi2_new == chi2_new) {
                curW ^= 1;
                vertex_gather(R, nv, fixed, S);
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

void graph_launch(aria_graph_t h, double* d_poses, const int* d_voff, const aria_graph_edge* d_edges, const int* d_eoff,
                  const int* d_fixed, int n_graphs, int iterations, aria_graph_result* d_results, int mode) {
    const aria_graph_config& c = h->cfg;
    // more graphs than the handle has scratch for run as consecutive launches on the stream; a graph's result does not
    // depend on which launch or which slot it gets
    for (int base = 0; base < n_graphs; base += c.max_graphs) {
        const int n = std::min(c.max_graphs, n_graphs - base);
        hipLaunchKernelGGL(k_graph_lm, dim3(n), dim3(GRAPH_BLOCK), graph_lds_bytes(h->wlds_edges), h->stream, d_poses, d_voff, d_edges, d_eoff, d_fixed, base,
                           iterations, c.max_vertices, c.max_edges, c.pcg_max_iters, c.pcg_rel_tol, h->d_v, h->d_e, h->d_i,
                           d_results, h->d_err, mode, h->wlds_edges);
    }
}

// uploads one graph (host buffers) into the single-graph staging; rejects what the kernel would on the host
int graph_stage_single(aria_graph_t h, const double* poses, int nv, int fixed, const aria_graph_edge* edges, int ne) {
    if (nv < 0 || ne < 0 || (nv && !poses) || (ne && !edges)) return ARIA_E_INVALID;
    if (nv > h->cfg.max_vertices || ne > h->cfg.max_edges) return ARIA_E_TOO_LARGE;
    if ((nv > 0 && (fixed < 0 || fixed >= nv)) || (nv == 0 && ne > 0)) return ARIA_E_INVALID;
    for (int k = 0; k < ne; k++)
        if (edges[k].from < 0 || edges[k].from >= nv || edges[k].to < 0 || edges[k].to >= nv || edges[k].from == edges[k].to ||
            !(edges[k].info_scale >= 0.0) || !std::isfinite(edges[k].info_scale))
            return ARIA_E_INVALID;
    const int off[5] = {0, nv, 0, ne, fixed};
    if (nv) ARIA_HIP(hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 12 * (size_t)nv, hipMemcpyHostToDevice, h->stream));
    if (ne) ARIA_HIP(hipMemcpyAsync(h->d_edges, edges, sizeof(aria_graph_edge) * (size_t)ne, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_off, off, sizeof(off), hipMemcpyHostToDevice));
    return ARIA_OK;
}

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
        const aria_graph_config& c = h->cfg;
        // more than 64 KiB of dynamic LDS has to be asked for; where that is refused the solve keeps W and p in HBM
        h->wlds_edges = std::min(c.max_edges, GRAPH_LDS_EDGES);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_graph_lm), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)graph_lds_bytes(h->wlds_edges)) != hipSuccess) {
            (void)hipGetLastError();
            h->wlds_edges = 0;
        }
        const size_t G = (size_t)c.max_graphs, V = (size_t)c.max_vertices, E = (size_t)c.max_edges;
        const char* what = "aria_graph_create";
        int rc;
        if ((rc = h->d_v.reserve(h->stream, G * V * VERT_DOUBLES, what)) != ARIA_OK) return rc;
        if ((rc = h->d_e.reserve(h->stream, G * E * EDGE_DOUBLES, what)) != ARIA_OK) return rc;
        if ((rc = h->d_i.reserve(h->stream, G * graph_int_words(c.max_vertices, c.max_edges), what)) != ARIA_OK) return rc;
        if ((rc = h->d_poses.reserve(h->stream, V * 12, what)) != ARIA_OK) return rc;
        if ((rc = h->d_edges.reserve(h->stream, E, what)) != ARIA_OK) return rc;
        if ((rc = h->d_off.reserve(h->stream, 8, what)) != ARIA_OK) return rc;
        return h->d_res.reserve(h->stream, 1, what);
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
    if (!h || !d_poses || !d_vertex_offset || !d_edges || !d_edge_offset || !d_fixed || !d_results || n_graphs < 0 ||
        iterations < 0)
        return ARIA_E_INVALID;
    if (n_graphs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    graph_launch(h, d_poses, d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs, iterations, d_results, 0);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_graph_optimize(aria_graph_t h, double* poses_inout, int n_vertices, int fixed_index, const aria_graph_edge* edges,
                        int n_edges, int iterations, aria_graph_result* result) {
    if (!h || !result || iterations < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = graph_stage_single(h, poses_inout, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    graph_launch(h, h->d_poses, h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, iterations, h->d_res, 0);
    ARIA_HIP(hipGetLastError());
    if (n_vertices)
        ARIA_HIP(hipMemcpyAsync(poses_inout, h->d_poses, sizeof(double) * 12 * (size_t)n_vertices, hipMemcpyDeviceToHost,
                                h->stream));
    ARIA_HIP(hipMemcpyAsync(result, h->d_res, sizeof(aria_graph_result), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_graph_check(h);
}

int aria_graph_debug_linearize(aria_graph_t h, const double* poses, int n_vertices, int fixed_index, const aria_graph_edge* edges,
                               int n_edges, double* chi2, double* b, double* H_diag, double* H_off) {
    if (!h || !chi2 || !b || !H_diag || !H_off) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = graph_stage_single(h, poses, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    graph_launch(h, h->d_poses, h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, 0, h->d_res, 1);
    ARIA_HIP(hipGetLastError());
    const size_t Vc = (size_t)h->cfg.max_vertices, Ec = (size_t)h->cfg.max_edges;
    std::vector<double> D(36 * Vc), bb(6 * Vc), W(36 * Ec);
    aria_graph_result res;
    // slot 0 of the scratch: D behind the 12 backup rows, b behind D and Minv, W0 behind A and B (scratch_of)
    ARIA_HIP(hipMemcpyAsync(D.data(), h->d_v + 12 * Vc, sizeof(double) * 36 * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(bb.data(), h->d_v + (12 + 72) * Vc, sizeof(double) * 6 * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(W.data(), h->d_e + 72 * Ec, sizeof(double) * 36 * Ec, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(&res, h->d_res, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    *chi2 = res.chi2_initial;
    for (int v = 0; v < n_vertices; v++) {
        for (int c = 0; c < 36; c++) H_diag[36 * (size_t)v + c] = D[c * Vc + v];
        for (int c = 0; c < 6; c++) b[6 * (size_t)v + c] = bb[c * Vc + v];
    }
    for (int k = 0; k < n_edges; k++)
        for (int c = 0; c < 36; c++) H_off[36 * (size_t)k + c] = W[c * Ec + k];
    return aria_graph_check(h);
}

}  // extern "C"
