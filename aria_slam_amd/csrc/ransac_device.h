// Device helpers shared by the stages that work on match lists: the counter-based sample hash of the two RANSAC stages
// (aria_orb_hip.h "Hypotheses") and the wave-ordered compaction of the map and stereo stages. Every function is inlined
// into the including file's kernels; only code that was identical in them lives here, the per-stage arithmetic stays with
// its stage. A helper belongs here only if every kernel that uses it compiles to the instructions it had with the code
// written out (tools/isa_compare.py): the pair validation of the stage kernels and the argmax tree of the finish kernels
// did not, in any of the forms tried, and stay written out in pose_ransac.hip and fund_ransac.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aria {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// sample slot j (0..7) of the hypothesis keyed hkey, draw number `retry`: an index in [0, n)
__device__ __forceinline__ int ransac_draw(uint64_t hkey, uint32_t j, uint32_t retry, uint32_t n) {
    const uint64_t r = splitmix64(hkey ^ (uint64_t)(retry * 8u + j));
    return (int)(((r >> 32) * (uint64_t)n) >> 32);
}

// K distinct indices in [0, n) for hypothesis h of pair `pair`: slot j redraws until it differs from slots 0..j-1, at most
// MAX_RETRY times. A slot that exhausts them stays -1 and the sample is invalid (returns false).
template <int K, int MAX_RETRY>
__device__ __forceinline__ bool draw_sample(uint64_t seed, uint32_t pair, int h, int n, int idx[K]) {
    bool ok = true;
    const uint64_t hkey = splitmix64(splitmix64(splitmix64(seed) ^ (uint64_t)pair) ^ (uint64_t)h);
#pragma unroll
    for (int j = 0; j < K; j++) {
        int v = -1;
        for (int retry = 0; retry < MAX_RETRY; retry++) {
            const int c = ransac_draw(hkey, (uint32_t)j, (uint32_t)retry, (uint32_t)n);
            bool dup = false;
#pragma unroll
            for (int k = 0; k < j; k++) dup |= idx[k] == c;
            if (!dup) { v = c; break; }
        }
        idx[j] = v;
        ok &= v >= 0;
    }
    return ok;
}

__device__ __forceinline__ void swap_if(bool c, double& a, double& b) {
    const double x = a, y = b;
    a = c ? y : x;
    b = c ? x : y;
}

// wave-ordered stable compaction of one BLOCK-thread round: returns this lane's slot (valid when keep) and the round's total
template <int BLOCK>
__device__ __forceinline__ int block_compact(bool keep, int* wsum, int& total) {
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        before += (w < wave) ? wsum[w] : 0;
        total += wsum[w];
    }
    __syncthreads();                                     // wsum is reused by the next round
    return before + rank;
}

}  // namespace aria
