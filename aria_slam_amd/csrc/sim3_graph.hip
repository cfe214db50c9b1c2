// Sim(3) pose-graph optimisation and the map correction after a loop (include/aria_orb_hip.h, "Sim(3) pose-graph
// optimisation"): the roles of ORB-SLAM's OptimizeEssentialGraph and CorrectLoop. The reference has no code for either;
// aria_slam_amd/sgraph_ref.py is the specification, DESIGN.md section 32 the record.
//
// k_sgraph_lm follows the schedule of k_graph_lm (graph_optimize.hip) with 7 x 7 blocks: ONE WORKGROUP PER GRAPH, persistent
// over every LM iteration of its graph, workgroup barriers only. Nothing waits on another workgroup.
//   stage     validate the counts, the edges (before any vertex is read) and then the vertex scales; build the vertex ->
//             incident-edge adjacency (CSR by integer atomics, each list then sorted by edge index and direction: the fixed
//             gather order).
//   linearise one lane per edge: e, Ji, Jj in registers -- only their non-zero entries enter a sum (ji_nz, jj_nz) -- stores
//             w Ji^T Ji, w Jj^T Jj, W = w Ji^T Jj, w Ji^T e, w Jj^T e; then one lane per vertex gathers its diagonal block and
//             its b over its incident edges. H is never scattered.
//   PCG       block-Jacobi preconditioned conjugate gradients on (H + lambda I) dx = b. The row of H p is a gather over the
//             vertex's edges, reading the 31 entries of W that are not structurally zero; dot products are a per-lane sum in
//             vertex order, a wave butterfly and a fixed 8-way sum through LDS (solver_device.h). ONE form of the solve is
//             built, the strided one of k_graph_lm (pcg_solve): the five vectors in the handle's HBM scratch (structure of
//             arrays, L2-resident), every lane owns the vertices v = lane + k * 512. It holds for any size. The register
//             and LDS forms of k_graph_lm are not built (DESIGN.md section 32 says what they would take).
//   trial     update the vertices, evaluate chi2_new with the pass that linearises (into the other W buffer, so a rejected
//             trial restores nothing but the vertices and an accepted one has paid for its edges once).
// fp64 throughout, no float atomics, no grid-wide barrier; every result is bitwise reproducible and independent of where the
// graph sits in a batch. The SE(3) pieces (quat_from_rot, rot_from_quat, the 3 x 3 products) are written out here as they are
// in graph_optimize.hip: sharing them means moving them into solver_device.h under that header's rule, a follow-up.
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
constexpr int EDGE_DOUBLES = NB2 * 4 + 2 * NB;            // A, B, W[2], gi, gj per edge
constexpr int VERT_DOUBLES = VDBL + NB2 + NB2 + NB * 5;   // backup, D, Minv, b, x, r, p, Ap per vertex
constexpr int CORRECT_BLOCK = 256;

static_assert(sizeof(aria_sgraph_vertex) == VDBL * sizeof(double), "aria_sgraph_vertex is 13 doubles");
static_assert(sizeof(aria_sgraph_edge) == 120 && sizeof(aria_sgraph_correct_stats) == 16 && sizeof(aria_sgraph_result) == 48, "layouts");

// per-graph slice of the handle's scratch; vertex arrays are [component][Vc], edge arrays [component][Ec]
struct Scratch {
    double *bak, *D, *Mi, *b, *x, *r, *p, *Ap;
    double *A, *B, *W0, *W1, *gi, *gj;
    int *aoff, *cur, *adj, *nbr;   // CSR offsets, fill cursors, (2 * edge + direction) per entry, its neighbour vertex
    int Vc, Ec;
};

__host__ __device__ inline size_t sg_int_words(int Vc, int Ec) { return 2 * ((size_t)Vc + 1) + 4 * (size_t)Ec; }

__device__ inline Scratch scratch_of(double* vbase, double* ebase, int* ibase, int slot, int Vc, int Ec) {
    Scratch s;
    double* v = vbase + (size_t)slot * VERT_DOUBLES * Vc;
    s.bak = v;            s.D = s.bak + VDBL * (size_t)Vc;  s.Mi = s.D + NB2 * (size_t)Vc;  s.b = s.Mi + NB2 * (size_t)Vc;
    s.x = s.b + NB * (size_t)Vc;  s.r = s.x + NB * (size_t)Vc;  s.p = s.r + NB * (size_t)Vc;  s.Ap = s.p + NB * (size_t)Vc;
    double* e = ebase + (size_t)slot * EDGE_DOUBLES * Ec;
    s.A = e;              s.B = s.A + NB2 * (size_t)Ec;     s.W0 = s.B + NB2 * (size_t)Ec;  s.W1 = s.W0 + NB2 * (size_t)Ec;
    s.gi = s.W1 + NB2 * (size_t)Ec;  s.gj = s.gi + NB * (size_t)Ec;
    int* i = ibase + (size_t)slot * sg_int_words(Vc, Ec);
    s.aoff = i;           s.cur = i + Vc + 1;               s.adj = s.cur + Vc + 1;         s.nbr = s.adj + 2 * (size_t)Ec;
    s.Vc = Vc;            s.Ec = Ec;
    return s;
}

struct Red {
    double* lds;      // [2][2][SG_WAVES]
    int phase;
};

// A scratch stride through an opaque copy, taken inside every loop body that forms component addresses from it. The strides
// are invariant over the whole kernel, and the few hundred scalar addresses derived from them (49 per block array) would
// otherwise be hoisted out of the LM loops and held -- spilled -- across everything else. Formed where they are used they cost
// a scalar multiply each.
__device__ inline size_t fresh(int stride) {
    asm volatile("" : "+s"(stride));
    return (size_t)stride;
}

// ---- SE(3) pieces (graph_ref.py: quat_from_rot, rot_from_quat), as in graph_optimize.hip ------------------------------------
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

// vertex (R[9], t[3], s) -> R[9], t[3]; returns s
__device__ inline double load_vertex(const double* S, double* R, double* t) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = S[c];
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = S[9 + c];
    return S[12];
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

// ---- the sparsity of the 7 x 7 Jacobians (sgraph_ref.py, "Jacobians") ------------------------------------------------------------
// Ji = [[-Rz^T / sz, (2 / sz) Rz^T [tm]x, -Rz^T tm / sz], [0, -(w I - [v]x) Rz^T, 0], [0, 0, -c]]
// Jj = [[se Re, 0, 0], [0, w I + [v]x, 0], [0, 0, c]]
__device__ constexpr bool ji_nz(int r, int a) { return r < 3 ? true : (r < 6 ? (a >= 3 && a < 6) : a == 6); }
__device__ constexpr bool jj_nz(int r, int c) { return r < 3 ? c < 3 : (r < 6 ? (c >= 3 && c < 6) : c == 6); }
// W = w Ji^T Jj: 31 entries are not structurally zero
__device__ constexpr bool w_nz(int a, int c) {
    bool nz = false;
    for (int r = 0; r < NB; r++) nz = nz || (ji_nz(r, a) && jj_nz(r, c));
    return nz;
}
// D and Minv are symmetric bit for bit (each entry is the same sum of commuting products): the solver reads the upper triangle
__device__ constexpr int sym7(int a, int c) { return a <= c ? NB * a + c : NB * c + a; }

// ---- one edge: error, Jacobians and its blocks ------------------------------------------------------------------------
// Returns w * e.e. Stores A = w Ji^T Ji, B = w Jj^T Jj, W = w Ji^T Jj, gi = w Ji^T e, gj = w Jj^T e at edge slot k.
__device__ inline double edge_blocks(const double* verts, const aria_sgraph_edge& ed, const Scratch& S, double* W, int k,
                                     bool fix_scale) {
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
    quat_from_rot(Re, qx, qy, qz, qw);
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
    const size_t Ec = fresh(S.Ec);
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

// every edge of the graph; returns chi2 (identical in every lane)
__device__ inline double edge_pass(Red& R, const double* verts, const aria_sgraph_edge* __restrict__ edges, int ne,
                                   const Scratch& S, double* W, bool fix_scale) {
    double part = 0.0;
    for (int k = threadIdx.x; k < ne; k += SG_BLOCK) part += edge_blocks(verts, edges[k], S, W, k, fix_scale);
    return block_sum<SG_WAVES>(R.lds, R.phase, part);   // its barrier also publishes the blocks to the workgroup
}

// every vertex gathers D and b over its incident edges in adjacency order; returns max diag(D) over the free vertices
__device__ inline double vertex_gather(Red& R, int nv, int fixed, const Scratch& S) {
    double mx = 0.0;
    for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
        const size_t Vc = fresh(S.Vc), Ec = fresh(S.Ec);
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
    return block_max<SG_WAVES>(R.lds, R.phase, mx);
}

// ---- preconditioner: inverse of the damped diagonal blocks -------------------------------------------------------------------
// Cholesky in registers, one vertex per lane. A block that is not positive definite preconditions with 0.
__device__ inline void precond_build(int nv, double lambda, const Scratch& S) {
    for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
        const size_t Vc = fresh(S.Vc);
        double L[NB2];
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) L[NB * i + j] = S.D[sym7(i, j) * Vc + v];
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
            for (int c = a; c < NB; c++) {
                double t = 0.0;
#pragma unroll
                for (int k = c; k < NB; k++) t += Li[NB * k + a] * Li[NB * k + c];
                S.Mi[(NB * a + c) * Vc + v] = ok ? t : 0.0;       // the upper triangle is all the solver reads
            }
    }
}

__device__ inline void precond_apply(const Scratch& S, size_t Vc, int v, const double* r, double* z) {
#pragma unroll
    for (int a = 0; a < NB; a++) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < NB; c++) t += S.Mi[sym7(a, c) * Vc + v] * r[c];
        z[a] = t;
    }
}

// ---- PCG on (H + lambda I) x = b, the fixed vertex removed. Returns the iterations; x in S.x ------------------------------
__device__ inline int pcg_solve(Red& R, int nv, int fixed, double lambda, const double* W, const Scratch& S,
                                int max_iters, double rel_tol) {
    double rz = 0.0, bb = 0.0;
    for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
        const size_t Vc = fresh(S.Vc);
        double r[NB], z[NB];
#pragma unroll
        for (int c = 0; c < NB; c++) r[c] = (v == fixed) ? 0.0 : S.b[c * Vc + v];
        precond_apply(S, Vc, v, r, z);
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
    block_sum2<SG_WAVES>(R.lds, R.phase, rz, bb);   // barrier: p is visible to the workgroup
    if (!(bb > 0.0)) return 0;
    const double stop = rel_tol * rel_tol * bb;
    int iters = 0;
    for (int it = 1; it <= max_iters; it++) {
        // Ap = (H + lambda I) p: the vertex's row, gathered over its incident edges
        double pAp = 0.0;
        for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = fresh(S.Vc), Ec = fresh(S.Ec);
            double p[NB], y[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) p[c] = S.p[c * Vc + v];
#pragma unroll
            for (int a = 0; a < NB; a++) {
                double t = lambda * p[a];
#pragma unroll
                for (int c = 0; c < NB; c++) t += S.D[sym7(a, c) * Vc + v] * p[c];
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
                            if (w_nz(r2, c)) y[c] += W[(NB * r2 + c) * Ec + k] * q[r2];
                } else {                             // v is the edge's `from`: W p_to
#pragma unroll
                    for (int r2 = 0; r2 < NB; r2++)
#pragma unroll
                        for (int c = 0; c < NB; c++)
                            if (w_nz(r2, c)) y[r2] += W[(NB * r2 + c) * Ec + k] * q[c];
                }
            }
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.Ap[c * Vc + v] = y[c];
                pAp += p[c] * y[c];
            }
        }
        pAp = block_sum<SG_WAVES>(R.lds, R.phase, pAp);
        if (!(pAp > 0.0)) break;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = fresh(S.Vc);
            double r[NB], z[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.x[c * Vc + v] += alpha * S.p[c * Vc + v];
                r[c] = S.r[c * Vc + v] - alpha * S.Ap[c * Vc + v];
                S.r[c * Vc + v] = r[c];
            }
            precond_apply(S, Vc, v, r, z);
#pragma unroll
            for (int c = 0; c < NB; c++) {
                S.Ap[c * Vc + v] = z[c];             // Ap is free until the next product: it carries z to the p update
                rr += r[c] * r[c];
                rzn += r[c] * z[c];
            }
        }
        block_sum2<SG_WAVES>(R.lds, R.phase, rr, rzn);
        iters = it;
        if (rr <= stop) break;
        const double beta = rzn / rz;
        rz = rzn;
        for (int v = threadIdx.x; v < nv; v += SG_BLOCK) {
            if (v == fixed) continue;
            const size_t Vc = fresh(S.Vc);
#pragma unroll
            for (int c = 0; c < NB; c++) S.p[c * Vc + v] = S.Ap[c * Vc + v] + beta * S.p[c * Vc + v];
        }
        __syncthreads();                             // p is visible before the next product gathers it
    }
    return iters;
}

// the inverse of the scale error (s - 1/s) / 2: always positive, no cancellation
__device__ inline double scale_of(double x) {
    const double r = sqrt(x * x + 1.0);
    return x >= 0.0 ? x + r : 1.0 / (-x + r);
}

// S <- S * D(d), rotation re-orthonormalised through its unit quaternion
__device__ inline void vertex_update(double* P, const double* d) {
    double R[9], t[3];
    const double s = load_vertex(P, R, t);
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
    for (int c = 0; c < 9; c++) P[c] = Rn[c];
#pragma unroll
    for (int r = 0; r < 3; r++) P[9 + r] = t[r] + s * (R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2]);
    P[12] = s * scale_of(d[6]);
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------
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
    const bool fix_scale = fix_scale_i != 0;
    Red R{red_lds, 0};

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
    const Scratch S = scratch_of(vbase, ebase, ibase, blockIdx.x, max_vertices, max_edges);

    // ---- adjacency: counts (integer atomics), block scan, fill, then every list sorted -> a fixed gather order
    for (int v = tid; v <= nv; v += SG_BLOCK) S.aoff[v] = 0;
    __syncthreads();
    for (int k = tid; k < ne; k += SG_BLOCK) {
        atomicAdd(&S.aoff[edges[k].from], 1);
        atomicAdd(&S.aoff[edges[k].to], 1);
    }
    __syncthreads();
    {
        const int chunk = (nv + SG_BLOCK - 1) / SG_BLOCK;
        const int lo = min(tid * chunk, nv), hi = min(lo + chunk, nv);
        int sum = 0;
        for (int v = lo; v < hi; v++) sum += S.aoff[v];
        scan[tid] = sum;
        __syncthreads();
        for (int off = 1; off < SG_BLOCK; off <<= 1) {
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
        if (tid == SG_BLOCK - 1) S.aoff[nv] = scan[SG_BLOCK - 1];
        __syncthreads();
    }
    for (int k = tid; k < ne; k += SG_BLOCK) {
        S.adj[atomicAdd(&S.cur[edges[k].from], 1)] = 2 * k;
        S.adj[atomicAdd(&S.cur[edges[k].to], 1)] = 2 * k + 1;
    }
    __syncthreads();
    for (int v = tid; v < nv; v += SG_BLOCK) {
        const int a0 = S.aoff[v], a1 = S.aoff[v + 1];
        for (int a = a0 + 1; a < a1; a++) {
            const int key = S.adj[a];
            int c = a - 1;
            while (c >= a0 && S.adj[c] > key) { S.adj[c + 1] = S.adj[c];  c--; }
            S.adj[c + 1] = key;
        }
    }
    __syncthreads();
    for (int a = tid; a < 2 * ne; a += SG_BLOCK) {
        const int code = S.adj[a];
        S.nbr[a] = (code & 1) ? edges[code >> 1].from : edges[code >> 1].to;
    }
    __syncthreads();

    // ---- linearise at the input vertices
    int curW = 0;
    double chi2 = edge_pass(R, verts, edges, ne, S, S.W0, fix_scale);
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
            res.pcg_iterations += pcg_solve(R, nv, fixed, lm.lambda, Wc, S, pcg_max_iters, pcg_rel_tol);
            // update (with a backup) and the gain's denominator dx.(lambda dx + b)
            double den = 0.0;
            for (int v = tid; v < nv; v += SG_BLOCK) {
                if (v == fixed) continue;
                const size_t Vc = fresh(S.Vc);
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
            const double chi2_new = edge_pass(R, verts, edges, ne, S, Wn, fix_scale);
            const double rho = (chi2 - chi2_new) / den;
            if (rho > 0.0 && chi2_new < INFINITY && chi2_new == chi2_new) {
                curW ^= 1;
                vertex_gather(R, nv, fixed, S);
                chi2 = chi2_new;
                lm.accept(rho);
                accepted = true;
                break;
            }
            for (int v = tid; v < nv; v += SG_BLOCK) {
                if (v == fixed) continue;
                const size_t Vc = fresh(S.Vc);
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

void sgraph_launch(aria_sgraph_t h, double* d_verts, const int* d_voff, const aria_sgraph_edge* d_edges, const int* d_eoff,
                   const int* d_fixed, int n_graphs, int iterations, aria_sgraph_result* d_results, int mode) {
    const aria_sgraph_config& c = h->cfg;
    // more graphs than the handle has scratch for run as consecutive launches on the stream; a graph's result does not
    // depend on which launch or which slot it gets
    for (int base = 0; base < n_graphs; base += c.max_graphs) {
        const int n = std::min(c.max_graphs, n_graphs - base);
        hipLaunchKernelGGL(k_sgraph_lm, dim3(n), dim3(SG_BLOCK), 0, h->stream, d_verts, d_voff, d_edges, d_eoff, d_fixed, base,
                           iterations, c.max_vertices, c.max_edges, c.pcg_max_iters, c.pcg_rel_tol, h->d_v, h->d_e, h->d_i,
                           d_results, h->d_err, mode, c.fix_scale);
    }
}

bool bad_scale(double s) { return !(s > 0.0) || !std::isfinite(s); }

// uploads one graph (host buffers) into the single-graph staging; rejects what the kernel would on the host
int sgraph_stage_single(aria_sgraph_t h, const aria_sgraph_vertex* verts, int nv, int fixed, const aria_sgraph_edge* edges, int ne) {
    if (nv < 0 || ne < 0 || (nv && !verts) || (ne && !edges)) return ARIA_E_INVALID;
    if (nv > h->cfg.max_vertices || ne > h->cfg.max_edges) return ARIA_E_TOO_LARGE;
    if ((nv > 0 && (fixed < 0 || fixed >= nv)) || (nv == 0 && ne > 0)) return ARIA_E_INVALID;
    for (int k = 0; k < ne; k++)
        if (edges[k].from < 0 || edges[k].from >= nv || edges[k].to < 0 || edges[k].to >= nv || edges[k].from == edges[k].to ||
            !(edges[k].info_scale >= 0.0) || !std::isfinite(edges[k].info_scale) || bad_scale(edges[k].s))
            return ARIA_E_INVALID;
    for (int v = 0; v < nv; v++)
        if (bad_scale(verts[v].s)) return ARIA_E_INVALID;
    const int off[5] = {0, nv, 0, ne, fixed};
    if (nv) ARIA_HIP(hipMemcpyAsync(h->d_verts, verts, sizeof(aria_sgraph_vertex) * (size_t)nv, hipMemcpyHostToDevice, h->stream));
    if (ne) ARIA_HIP(hipMemcpyAsync(h->d_edges, edges, sizeof(aria_sgraph_edge) * (size_t)ne, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_off, off, sizeof(off), hipMemcpyHostToDevice));
    return ARIA_OK;
}

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
    return stage_create(c, out, 1, "aria_sgraph_create", [](aria_sgraph_s* h) {
        const aria_sgraph_config& c = h->cfg;
        const size_t G = (size_t)c.max_graphs, V = (size_t)c.max_vertices, E = (size_t)c.max_edges;
        const char* what = "aria_sgraph_create";
        int rc;
        if ((rc = h->d_v.reserve(h->stream, G * V * VERT_DOUBLES, what)) != ARIA_OK) return rc;
        if ((rc = h->d_e.reserve(h->stream, G * E * EDGE_DOUBLES, what)) != ARIA_OK) return rc;
        if ((rc = h->d_i.reserve(h->stream, G * sg_int_words(c.max_vertices, c.max_edges), what)) != ARIA_OK) return rc;
        if ((rc = h->d_verts.reserve(h->stream, V * VDBL, what)) != ARIA_OK) return rc;
        if ((rc = h->d_edges.reserve(h->stream, E, what)) != ARIA_OK) return rc;
        if ((rc = h->d_off.reserve(h->stream, 8, what)) != ARIA_OK) return rc;
        return h->d_res.reserve(h->stream, 1, what);
    });
}

void aria_sgraph_destroy(aria_sgraph_t h) { stage_destroy(h); }

void* aria_sgraph_stream(aria_sgraph_t h) { return stage_stream(h); }

int aria_sgraph_check(aria_sgraph_t h) {
    return stage_check(h, {{ERRBIT_SG_INPUT, ARIA_E_INVALID}, {ERRBIT_SG_LARGE, ARIA_E_TOO_LARGE}});
}

int aria_sgraph_optimize_batch_device(aria_sgraph_t h, aria_sgraph_vertex* d_vertices, const int* d_vertex_offset,
                                      const aria_sgraph_edge* d_edges, const int* d_edge_offset, const int* d_fixed, int n_graphs,
                                      int iterations, aria_sgraph_result* d_results) {
    if (!h || !d_vertices || !d_vertex_offset || !d_edges || !d_edge_offset || !d_fixed || !d_results || n_graphs < 0 ||
        iterations < 0)
        return ARIA_E_INVALID;
    if (n_graphs == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    sgraph_launch(h, reinterpret_cast<double*>(d_vertices), d_vertex_offset, d_edges, d_edge_offset, d_fixed, n_graphs, iterations,
                  d_results, 0);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_sgraph_optimize(aria_sgraph_t h, aria_sgraph_vertex* vertices_inout, int n_vertices, int fixed_index,
                         const aria_sgraph_edge* edges, int n_edges, int iterations, aria_sgraph_result* result) {
    if (!h || !result || iterations < 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = sgraph_stage_single(h, vertices_inout, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    sgraph_launch(h, h->d_verts, h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, iterations, h->d_res, 0);
    ARIA_HIP(hipGetLastError());
    if (n_vertices)
        ARIA_HIP(hipMemcpyAsync(vertices_inout, h->d_verts, sizeof(aria_sgraph_vertex) * (size_t)n_vertices, hipMemcpyDeviceToHost,
                                h->stream));
    ARIA_HIP(hipMemcpyAsync(result, h->d_res, sizeof(aria_sgraph_result), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    return aria_sgraph_check(h);
}

int aria_sgraph_debug_linearize(aria_sgraph_t h, const aria_sgraph_vertex* vertices, int n_vertices, int fixed_index,
                                const aria_sgraph_edge* edges, int n_edges, double* chi2, double* b, double* H_diag, double* H_off) {
    if (!h || !chi2 || !b || !H_diag || !H_off) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = sgraph_stage_single(h, vertices, n_vertices, fixed_index, edges, n_edges);
    if (rc != ARIA_OK) return rc;
    sgraph_launch(h, h->d_verts, h->d_off, h->d_edges, h->d_off + 2, h->d_off + 4, 1, 0, h->d_res, 1);
    ARIA_HIP(hipGetLastError());
    const size_t Vc = (size_t)h->cfg.max_vertices, Ec = (size_t)h->cfg.max_edges;
    std::vector<double> D(NB2 * Vc), bb(NB * Vc), W(NB2 * Ec);
    aria_sgraph_result res;
    // slot 0 of the scratch: D behind the backup, b behind D and Minv, W0 behind A and B (scratch_of)
    ARIA_HIP(hipMemcpyAsync(D.data(), h->d_v + VDBL * Vc, sizeof(double) * NB2 * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(bb.data(), h->d_v + (VDBL + 2 * NB2) * Vc, sizeof(double) * NB * Vc, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(W.data(), h->d_e + 2 * NB2 * Ec, sizeof(double) * NB2 * Ec, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipMemcpyAsync(&res, h->d_res, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    *chi2 = res.chi2_initial;
    for (int v = 0; v < n_vertices; v++) {
        for (int c = 0; c < NB2; c++) H_diag[NB2 * (size_t)v + c] = D[c * Vc + v];
        for (int c = 0; c < NB; c++) b[NB * (size_t)v + c] = bb[c * Vc + v];
    }
    for (int k = 0; k < n_edges; k++)
        for (int c = 0; c < NB2; c++) H_off[NB2 * (size_t)k + c] = W[c * Ec + k];
    return aria_sgraph_check(h);
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
