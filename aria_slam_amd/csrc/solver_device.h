// Device helpers shared by the solver kernels: the Jacobi eigen-solver of the two RANSAC stages with a 3x3 in registers
// (pose_ransac.hip, pnp_ransac.hip), the fixed-order workgroup reductions and the packed 6x6 index of the two persistent
// Levenberg-Marquardt kernels (k_graph_lm, k_ba_lm), their damping rule and stop codes, and Exp on so(3) (k_ba_lm,
// k_pnp_finish). Not part of the public interface. Every function is inlined into the including file's kernels.
// The rule is that of ransac_device.h: a helper lives here only if every kernel that uses it passes tools/isa_compare.py
// against the parent with the code written out -- the same instruction count, opcode histogram, registers, scratch, LDS
// and occupancy (profiles/solver_device_isa_compare.txt). Tried, failed that, and therefore still written out:
//   the sorted eigen block of project_essential and pnp_rotation (jacobi3, then the three-select sort network), as one
//     helper with the nine outputs by reference and as a struct returned by value, both the same: k_pose_hyp 4240 -> 4296
//     instructions, k_pose_finish 6401 -> 6516, k_pnp_hyp 5047 -> 5112, k_pnp_finish 4610 -> 4647;
//   the reductions taking a struct {double* lds; int phase;} by reference in k_ba_lm: 11998 -> 11992 and other metadata.
//     They take the LDS pointer and the phase as plain arguments.
#pragma once
#include <hip/hip_runtime.h>

namespace aria {

// One Jacobi rotation zeroing A[p][q] of a symmetric N x N matrix (row-major), accumulated into V's columns.
template <int N, typename P>
__device__ __forceinline__ void jacobi_rotate(P A, P V, int p, int q) {
    const double apq = A[p * N + q];
    if (apq == 0.0) return;
    const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < N; k++) {            // A <- A J
        const double akp = A[k * N + p], akq = A[k * N + q];
        A[k * N + p] = c * akp - s * akq;
        A[k * N + q] = s * akp + c * akq;
    }
    for (int k = 0; k < N; k++) {            // A <- J^T A
        const double apk = A[p * N + k], aqk = A[q * N + k];
        A[p * N + k] = c * apk - s * aqk;
        A[q * N + k] = s * apk + c * aqk;
    }
    A[p * N + q] = 0.0;
    A[q * N + p] = 0.0;
    for (int k = 0; k < N; k++) {            // V <- V J
        const double vkp = V[k * N + p], vkq = V[k * N + q];
        V[k * N + p] = c * vkp - s * vkq;
        V[k * N + q] = s * vkp + c * vkq;
    }
}

// 3 x 3 symmetric eigen-decomposition in registers: eigenvalues on A's diagonal, eigenvectors in V's columns
__device__ __forceinline__ void jacobi3(double A[9], double V[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 10; sweep++) {
        jacobi_rotate<3>(A, V, 0, 1);
        jacobi_rotate<3>(A, V, 0, 2);
        jacobi_rotate<3>(A, V, 1, 2);
    }
}

// ---- reductions over a workgroup of WAVES waves: per-lane partial, wave butterfly, the waves summed in wave order ----------
// lds is [2][2][WAVES] doubles, phase starts at 0.
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int WAVES>
__device__ inline void block_sum2(double* lds, int& phase, double& a, double& b) {
    a = wave_sum(a);
    b = wave_sum(b);
    double* slot = lds + phase * 2 * WAVES;
    if ((threadIdx.x & 63) == 0) {
        slot[threadIdx.x >> 6] = a;
        slot[WAVES + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { sa += slot[w]; sb += slot[WAVES + w]; }
    a = sa;
    b = sb;
    phase ^= 1;      // the next reduction uses the other slot: one barrier per reduction is enough
}

template <int WAVES>
__device__ inline double block_sum(double* lds, int& phase, double a) {
    double b = 0.0;
    block_sum2<WAVES>(lds, phase, a, b);
    return a;
}

template <int WAVES>
__device__ inline double block_max(double* lds, int& phase, double a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a = fmax(a, __shfl_xor(a, m, 64));
    double* slot = lds + phase * 2 * WAVES;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = slot[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) s = fmax(s, slot[w]);
    phase ^= 1;
    return s;
}

// index of (a, c) in the 21 entries of a symmetric 6 x 6 stored as its upper triangle, row by row
__device__ constexpr int tri6(int a, int c) { return a <= c ? 6 * a - a * (a - 1) / 2 + (c - a) : 6 * c - c * (c - 1) / 2 + (a - c); }

// E = Exp(w) = I + a K + b K^2 (row-major), K = [w]x, a = sin(th) / th, b = (1 - cos(th)) / th^2; their series below th^2 = 1e-16
__device__ inline void exp_so3(const double* w, double* E) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b;
    if (th2 < 1e-16) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double k2 = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
            E[r * 3 + c] = ((r == c) ? 1.0 : 0.0) + a * K[r * 3 + c] + b * k2;
        }
}

// ---- Levenberg-Marquardt control of k_graph_lm and k_ba_lm (include/aria_orb_hip.h, "LM" and "LM control") ---------------
// The stop_reason fields of aria_graph_result and aria_ba_result, and the rejected trials that end a call with STOP_TRIALS.
constexpr int LM_MAX_TRIALS = 10;
constexpr int STOP_ITERATIONS = 0, STOP_TRIALS = 1, STOP_INVALID = 2;

// The damping. rho = (chi2 - chi2_new) / (dx.(lambda dx + b) + 1e-3) is the caller's: the 1e-3 belongs to the gain.
struct LmDamping {
    double lambda, ni;
    __device__ void start(double maxdiag) { lambda = 1e-5 * maxdiag;  ni = 2.0; }
    __device__ void accept(double rho) {
        const double a = 2.0 * rho - 1.0;
        lambda *= fmax(1.0 / 3.0, 1.0 - a * a * a);
        ni = 2.0;
    }
    __device__ void reject() { lambda *= ni;  ni *= 2.0; }
};

}  // namespace aria
