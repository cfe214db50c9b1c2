// Place recognition: a flat binary bag-of-words vocabulary, the bags of frames, a ring database of bags and its scored top-K
// query. Semantics in include/aria_orb_hip.h ("place recognition"); aria_slam_amd/bow_ref.py is the definition and this file
// equals it bit for bit. Everything is integer arithmetic except one correctly rounded fp64 division per score.
//
// Quantising is the matcher's kNN-2 kernel (launch_knn2_mfma, mode 0) with the vocabulary as the train set every frame shares
// (t_stride = 0, nt_fixed = V): its key is distance << 16 | word, so the best key is the nearest word, ties to the lowest.
//
// k_bow_counts    frame counts outside [0, limit] become 0 and a deferred error, before the kNN kernel reads a descriptor.
// k_bow_hist      one 256-thread workgroup per frame: an LDS histogram of V counters from the keys' low 16 bits (integer LDS
//                 atomics). Transform form: the uint16 row and the norm by a fixed-order integer reduction. Training form: the
//                 frame's counts are added to the words' member counts (one integer global atomic per word the frame holds,
//                 not one per descriptor) and one presence bit per word is written by ballot. LDS 4 V bytes.
// k_bow_scan      one workgroup: where each word's member list starts (exclusive scan of the member counts).
// k_bow_scatter   one workgroup per frame: the LDS histogram again, one integer global atomic per word of the frame reserves
//                 the frame's span in the word's list, LDS atomics rank the descriptors inside it. LDS 8 V bytes.
// k_bow_majority  one wave per word, no atomics on the counts at all: lane l keeps the four bit counters 4l .. 4l+3 in
//                 registers over the word's member list, the wave assembles the new word by shuffles, compares it with the old
//                 one and ORs the changed flag the host reads once per iteration. The order inside a list is free: sums.
// k_bow_idf       a lane per word: frames holding it from the presence bits, the weight by the integer logarithm.
// k_bow_store     one workgroup per added bag: the row into its ring slot (rows padded to 8 words for 16-byte loads), the norm
//                 recomputed and held to the caller's.
// k_bow_check_query one workgroup per query bag: the norm recomputed and held to the caller's (a bag that fails is an empty query).
// k_bow_score     grid (tiles of 64 entries, tiles of 4 queries): the queries' weighted bags as V x uint32 each and the weights
//                 as V x uint16 in LDS (18 V bytes: 72 KiB at V = 4096, two workgroups per CU); a wave per entry streams the
//                 row once per query tile in 16-byte loads, min on 64-bit products, 64-bit integer sums, shuffle reduction.
// k_bow_topk      one workgroup per query: gate and score (the one fp64 division), then K rounds of "the best key after the
//                 previous one" over (score bits descending, index ascending).
// No float atomics, no scratch, no grid-wide barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "match_kernels.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_bow_hit) == 32, "aria_bow_hit is 32 bytes");
static_assert(sizeof(aria_bow_config) == 40, "aria_bow_config is 40 bytes");

#define BOW_HD __host__ __device__ __forceinline__

namespace {

// ---- the plain arithmetic of the stage (compiles for the host too: no LDS, no barrier, no cross-lane operation) ----
constexpr int BW_MAX_WORDS = 4096;
constexpr int BW_MAX_ROWS = 4096;
constexpr int BW_MAX_FRAMES = 65535;
constexpr int BW_MAX_K = 32;
constexpr int BW_MAX_NORM = 1 << 24;

// rule 3: a bit of the new word; a tie gives 0
BOW_HD unsigned bow_majority_bit(unsigned ones, unsigned members) { return 2u * ones > members ? 1u : 0u; }

// rule 4: log2(num / den) in Q8 for 1 <= den <= num < 2^16, by shift and square on 64-bit integers (bow_ref.ilog2_q8)
BOW_HD unsigned bow_ilog2_q8(unsigned num, unsigned den) {
    unsigned e = 0;
    while (((unsigned long long)den << (e + 1)) <= (unsigned long long)num) e++;
    unsigned long long m = ((unsigned long long)num << 30) / ((unsigned long long)den << e);
    unsigned r = e;
    for (int k = 0; k < 8; k++) {
        m = (m * m) >> 30;
        r <<= 1;
        if (m >= (1ull << 31)) {
            r |= 1u;
            m >>= 1;
        }
    }
    return r;
}

BOW_HD unsigned bow_idf(unsigned n_frames, unsigned n_w) { return (n_w == 0 || n_w >= n_frames) ? 0u : bow_ilog2_q8(n_frames, n_w); }

// rule 5: a word's weighted count
BOW_HD unsigned bow_weighted(unsigned tf, unsigned idf_q) { return tf * idf_q; }

// rule 6: a word's term of the numerator, and the score. Weighted counts and norms are below 2^24 (rule 5; the store and query
// kernels refuse bags that are not), so the masks change nothing and let the compiler take the 24-bit multiplier for both
// halves of each 48-bit product instead of the quarter-rate 64-bit multiply-add.
BOW_HD unsigned long long bow_term(unsigned v, unsigned n_d, unsigned u, unsigned n_q) {
    const unsigned long long a = (unsigned long long)(v & 0xFFFFFFu) * (n_d & 0xFFFFFFu), b = (unsigned long long)(u & 0xFFFFFFu) * (n_q & 0xFFFFFFu);
    return a < b ? a : b;
}

BOW_HD double bow_score(long long S, int n_q, int n_d) { return (double)S / (double)((long long)n_q * (long long)n_d); }

// rule 8: does (score bits a, index a) rank before (score bits b, index b)? Positive doubles order as their bit patterns.
BOW_HD bool bow_hit_before(unsigned long long bits_a, int idx_a, unsigned long long bits_b, int idx_b) {
    return bits_a > bits_b || (bits_a == bits_b && idx_a < idx_b);
}
// ---- end of the plain arithmetic ----

constexpr int BW_BLOCK = 256;
constexpr int BW_QT = 4;            // queries per tile of the score kernel
constexpr int BW_EPB = 64;          // entries per workgroup of the score kernel
constexpr int BW_IDS = 256;         // ids travel as kernel arguments, this many per launch: nothing of the caller's is read later
constexpr int ERRBIT_BOW_INPUT = 1;

struct BowIds {
    long long v[BW_IDS];
};

__global__ __launch_bounds__(BW_BLOCK) void k_bow_counts(const int* __restrict__ counts, int fixed, int n_frames, int limit,
                                                         int* __restrict__ cnt, int* __restrict__ err) {
    const int f = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (f >= n_frames) return;
    int c = counts ? counts[f] : fixed;
    if (c < 0 || c > limit) {
        c = 0;
        atomicOr(err, ERRBIT_BOW_INPUT);
    }
    cnt[f] = c;
}

__global__ __launch_bounds__(BW_BLOCK) void k_bow_init_words(const uint8_t* __restrict__ desc, const long long* __restrict__ src, int V,
                                                             uint32_t* __restrict__ words) {
    const int t = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (t >= V * 8) return;
    words[t] = reinterpret_cast<const uint32_t*>(desc + src[t >> 3] * 32)[t & 7];
}

// the frame's histogram of words in LDS; ends with a barrier
__device__ __forceinline__ void bow_lds_hist(uint32_t* s_h, const uint2* __restrict__ keys, int n, int V) {
    for (int w = threadIdx.x; w < V; w += BW_BLOCK) s_h[w] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += BW_BLOCK) {
        const unsigned w = keys[i].x & 0xFFFFu;
        if (w < (unsigned)V) atomicAdd(&s_h[w], 1u);
    }
    __syncthreads();
}

template <bool TRAIN>
__global__ __launch_bounds__(BW_BLOCK) void k_bow_hist(const uint2* __restrict__ keys, const int* __restrict__ cnt, int64_t maxq, int V,
                                                       const uint16_t* __restrict__ idf, uint16_t* __restrict__ tf,
                                                       int* __restrict__ norm, uint32_t* __restrict__ members,
                                                       uint32_t* __restrict__ present, int present_stride) {
    extern __shared__ uint32_t s_dyn[];
    __shared__ uint32_t s_red[BW_BLOCK / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    bow_lds_hist(s_dyn, keys + (int64_t)f * maxq, cnt[f], V);
    if (TRAIN) {
        for (int base = 0; base < V; base += BW_BLOCK) {
            const int w = base + tid;
            const uint32_t c = w < V ? s_dyn[w] : 0u;
            if (c) atomicAdd(&members[w], c);
            const unsigned long long b = __ballot(c != 0);
            if ((tid & 63) == 0) {
                uint32_t* row = present + (int64_t)f * present_stride + ((base + tid) >> 5);
                row[0] = (uint32_t)b;
                row[1] = (uint32_t)(b >> 32);
            }
        }
    } else {
        uint32_t part = 0;
        for (int w = tid; w < V; w += BW_BLOCK) {
            const uint32_t c = s_dyn[w];
            tf[(int64_t)f * V + w] = (uint16_t)c;
            part += bow_weighted(c, idf[w]);
        }
        for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
        if ((tid & 63) == 0) s_red[tid >> 6] = part;
        __syncthreads();
        if (tid == 0) norm[f] = (int)(s_red[0] + s_red[1] + s_red[2] + s_red[3]);
    }
}

// base[w] = members[0] + ... + members[w - 1]; cursor[w] = base[w]
__global__ __launch_bounds__(BW_BLOCK) void k_bow_scan(const uint32_t* __restrict__ members, int V, uint32_t* __restrict__ base,
                                                       uint32_t* __restrict__ cursor) {
    __shared__ uint32_t s_part[BW_BLOCK];
    const int tid = threadIdx.x, per = (V + BW_BLOCK - 1) / BW_BLOCK, w0 = tid * per;
    uint32_t sum = 0;
    for (int k = 0; k < per; k++)
        if (w0 + k < V) sum += members[w0 + k];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < BW_BLOCK; k++) {
            const uint32_t p = s_part[k];
            s_part[k] = run;
            run += p;
        }
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (int k = 0; k < per; k++)
        if (w0 + k < V) {
            base[w0 + k] = run;
            cursor[w0 + k] = run;
            run += members[w0 + k];
        }
}

__global__ __launch_bounds__(BW_BLOCK) void k_bow_scatter(const uint2* __restrict__ keys, const int* __restrict__ cnt, int64_t maxq, int V,
                                                          int64_t desc_stride, uint32_t* __restrict__ cursor, int* __restrict__ list,
                                                          uint32_t n_total) {
    extern __shared__ uint32_t s_dyn[];
    uint32_t* s_h = s_dyn;
    uint32_t* s_b = s_dyn + V;
    const int f = blockIdx.x, tid = threadIdx.x, n = cnt[f];
    const uint2* kf = keys + (int64_t)f * maxq;
    bow_lds_hist(s_h, kf, n, V);
    for (int w = tid; w < V; w += BW_BLOCK) {
        const uint32_t c = s_h[w];
        s_b[w] = c ? atomicAdd(&cursor[w], c) : 0u;
        s_h[w] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += BW_BLOCK) {
        const unsigned w = kf[i].x & 0xFFFFu;
        if (w >= (unsigned)V) continue;
        const uint32_t at = s_b[w] + atomicAdd(&s_h[w], 1u);
        if (at < n_total) list[at] = (int)((int64_t)f * desc_stride + i);
    }
}

__global__ __launch_bounds__(64) void k_bow_majority(const uint8_t* __restrict__ desc, const int* __restrict__ list,
                                                     const uint32_t* __restrict__ base, const uint32_t* __restrict__ members,
                                                     uint32_t* __restrict__ words, int* __restrict__ changed) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const uint32_t m = members[w];
    if (m == 0) return;                                           // a word without members keeps its bits
    const int* mine = list + base[w];
    const int byte = lane >> 1, shift = (lane & 1) * 4;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t nib = ((uint32_t)desc[(int64_t)mine[k] * 32 + byte] >> shift) & 15u;
        c0 += nib & 1u;
        c1 += (nib >> 1) & 1u;
        c2 += (nib >> 2) & 1u;
        c3 += (nib >> 3) & 1u;
    }
    uint32_t v = bow_majority_bit(c0, m) | (bow_majority_bit(c1, m) << 1) | (bow_majority_bit(c2, m) << 2) | (bow_majority_bit(c3, m) << 3);
    v <<= (lane & 7) * 4;                                         // lanes 8g .. 8g+7 hold bits 32g .. 32g+31
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    v |= __shfl_xor(v, 4);
    if ((lane & 7) == 0) {
        uint32_t* out = words + (int64_t)w * 8 + (lane >> 3);
        if (*out != v) {
            *out = v;
            atomicOr(changed, 1);
        }
    }
}

__global__ __launch_bounds__(BW_BLOCK) void k_bow_idf(const uint32_t* __restrict__ present, int present_stride, int n_frames, int V,
                                                      uint16_t* __restrict__ idf) {
    const int w = blockIdx.x * BW_BLOCK + threadIdx.x;
    if (w >= V) return;
    unsigned n_w = 0;
    for (int f = 0; f < n_frames; f++) n_w += (present[(int64_t)f * present_stride + (w >> 5)] >> (w & 31)) & 1u;
    idf[w] = (uint16_t)bow_idf((unsigned)n_frames, n_w);
}

// bag j of the call goes to ring slot (first + j) % cap. A norm that is not the sum of the weighted counts, or not below 2^24:
// the bag is stored empty and the error deferred.
__global__ __launch_bounds__(BW_BLOCK) void k_bow_store(const uint16_t* __restrict__ tf, const int* __restrict__ norm, BowIds ids, int V, int Vp,
                                                        const uint16_t* __restrict__ idf, long long first, long long cap,
                                                        uint16_t* __restrict__ db_tf, int* __restrict__ db_norm,
                                                        long long* __restrict__ db_ids, int* __restrict__ err) {
    __shared__ unsigned long long s_red[BW_BLOCK / 64];
    const int j = blockIdx.x, tid = threadIdx.x;
    const long long slot = (first + j) % cap;
    unsigned long long part = 0;
    for (int w = tid; w < Vp; w += BW_BLOCK) {
        const uint16_t c = w < V ? tf[(int64_t)j * V + w] : (uint16_t)0;
        db_tf[slot * Vp + w] = c;
        if (w < V) part += (unsigned long long)bow_weighted(c, idf[w]);
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long N = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        const int given = norm[j];
        const bool ok = N < (unsigned long long)BW_MAX_NORM && given >= 0 && (unsigned long long)given == N;
        if (!ok) atomicOr(err, ERRBIT_BOW_INPUT);
        db_norm[slot] = ok ? given : 0;
        db_ids[slot] = ids.v[j];
    }
}

// one workgroup per query bag: its norm recomputed and held to the caller's, as k_bow_store does for entries; a bag that fails
// is an empty query (norm 0) and a deferred error
__global__ __launch_bounds__(BW_BLOCK) void k_bow_check_query(const uint16_t* __restrict__ tf, const int* __restrict__ norm, int V,
                                                              const uint16_t* __restrict__ idf, int* __restrict__ out_norm,
                                                              int* __restrict__ err) {
    __shared__ unsigned long long s_red[BW_BLOCK / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    unsigned long long part = 0;
    for (int w = tid; w < V; w += BW_BLOCK) part += (unsigned long long)bow_weighted(tf[(int64_t)q * V + w], idf[w]);
    for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long N = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        const int given = norm[q];
        const bool ok = N < (unsigned long long)BW_MAX_NORM && given >= 0 && (unsigned long long)given == N;
        if (!ok) atomicOr(err, ERRBIT_BOW_INPUT);
        out_norm[q] = ok ? given : 0;
    }
}

__global__ __launch_bounds__(BW_BLOCK) void k_bow_score(const uint16_t* __restrict__ q_tf, const int* __restrict__ q_norm, int nq, int V, int Vp,
                                                        const uint16_t* __restrict__ idf, const uint16_t* __restrict__ db_tf,
                                                        const int* __restrict__ db_norm, long long head, int size, long long cap,
                                                        long long* __restrict__ out_S) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t* s_v = s_dyn;                                                     // [BW_QT][Vp]
    uint16_t* s_idf = reinterpret_cast<uint16_t*>(s_dyn + BW_QT * Vp);         // [Vp]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int q0 = blockIdx.y * BW_QT;
    uint32_t nqv[BW_QT];
#pragma unroll
    for (int k = 0; k < BW_QT; k++) {
        const int n = q0 + k < nq ? q_norm[q0 + k] : 0;
        nqv[k] = n > 0 ? (uint32_t)n : 0u;
    }
    for (int w = tid; w < Vp; w += BW_BLOCK) {
        const uint32_t wt = w < V ? idf[w] : 0u;
        s_idf[w] = (uint16_t)wt;
#pragma unroll
        for (int k = 0; k < BW_QT; k++) s_v[k * Vp + w] = (nqv[k] && w < V) ? bow_weighted(q_tf[(int64_t)(q0 + k) * V + w], wt) : 0u;
    }
    __syncthreads();
    const int e_end = min(size, ((int)blockIdx.x + 1) * BW_EPB);
    for (int e = blockIdx.x * BW_EPB + wv; e < e_end; e += BW_BLOCK / 64) {
        const long long slot = (head + e) % cap;
        const int nd_i = db_norm[slot];
        const uint32_t nd = nd_i > 0 ? (uint32_t)nd_i : 0u;
        unsigned long long S[BW_QT];
#pragma unroll
        for (int k = 0; k < BW_QT; k++) S[k] = 0;
        if (nd) {
            const uint4* row = reinterpret_cast<const uint4*>(db_tf + slot * Vp);
            // four 16-byte loads of the row in flight per lane before the first is used
            for (int cb = lane * 8; cb < Vp; cb += 4 * 64 * 8) {
            uint4 tq[4];
#pragma unroll
            for (int j = 0; j < 4; j++) tq[j] = cb + j * 512 < Vp ? row[(cb + j * 512) >> 3] : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = cb + j * 512;
                const uint4 t = tq[j];
                if ((t.x | t.y | t.z | t.w) == 0) continue;                    // bags are sparse (and nothing lies beyond Vp)
                const uint4 wq = *reinterpret_cast<const uint4*>(s_idf + c);
                const uint32_t tw[4] = {t.x, t.y, t.z, t.w}, iw[4] = {wq.x, wq.y, wq.z, wq.w};
                uint32_t u[8];
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    u[2 * p] = bow_weighted(tw[p] & 0xFFFFu, iw[p] & 0xFFFFu);
                    u[2 * p + 1] = bow_weighted(tw[p] >> 16, iw[p] >> 16);
                }
#pragma unroll
                for (int k = 0; k < BW_QT; k++) {
                    const uint4 a = *reinterpret_cast<const uint4*>(s_v + k * Vp + c), b = *reinterpret_cast<const uint4*>(s_v + k * Vp + c + 4);
                    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int p = 0; p < 8; p++) S[k] += bow_term(v[p], nd, u[p], nqv[k]);
                }
            }
            }
        }
#pragma unroll
        for (int k = 0; k < BW_QT; k++) {
            unsigned long long s = S[k];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
            if (lane == 0 && q0 + k < nq) out_S[(int64_t)(q0 + k) * size + e] = (long long)s;
        }
    }
}

__global__ __launch_bounds__(BW_BLOCK) void k_bow_topk(const long long* __restrict__ S, unsigned long long* __restrict__ bits,
                                                       const int* __restrict__ q_norm, BowIds qids, const int* __restrict__ db_norm,
                                                       const long long* __restrict__ db_ids, long long head, int size, long long cap,
                                                       int mfb, int K, aria_bow_hit* __restrict__ hits, int* __restrict__ counts) {
    __shared__ unsigned long long s_bits[BW_BLOCK / 64];
    __shared__ int s_idx[BW_BLOCK / 64];
    __shared__ unsigned long long s_best_bits;
    __shared__ int s_best_idx;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n_q = q_norm[q];
    const long long qid = qids.v[q];
    const long long* Sq = S + (int64_t)q * size;
    unsigned long long* bq = bits + (int64_t)q * size;
    for (int e = tid; e < size; e += BW_BLOCK) {
        const long long slot = (head + e) % cap;
        const int n_d = db_norm[slot];
        const long long s = Sq[e];
        const bool ok = n_q > 0 && n_d > 0 && qid - db_ids[slot] >= (long long)mfb && s > 0;
        bq[e] = ok ? (unsigned long long)__double_as_longlong(bow_score(s, n_q, n_d)) : 0ull;     // every thread rereads only its own
    }
    unsigned long long prev_bits = ~0ull;
    int prev_idx = -1, found = 0;
    for (int k = 0; k < K; k++) {
        unsigned long long best_bits = 0;
        int best_idx = INT_MAX;
        for (int e = tid; e < size; e += BW_BLOCK) {
            const unsigned long long b = bq[e];
            if (b && bow_hit_before(prev_bits, prev_idx, b, e) && bow_hit_before(b, e, best_bits, best_idx)) {
                best_bits = b;
                best_idx = e;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_down(best_bits, o);
            const int oi = __shfl_down(best_idx, o);
            if (bow_hit_before(ob, oi, best_bits, best_idx)) {
                best_bits = ob;
                best_idx = oi;
            }
        }
        if ((tid & 63) == 0) {
            s_bits[tid >> 6] = best_bits;
            s_idx[tid >> 6] = best_idx;
        }
        __syncthreads();
        if (tid == 0) {
            for (int p = 1; p < BW_BLOCK / 64; p++)
                if (bow_hit_before(s_bits[p], s_idx[p], best_bits, best_idx)) {
                    best_bits = s_bits[p];
                    best_idx = s_idx[p];
                }
            s_best_bits = best_bits;
            s_best_idx = best_idx;
            aria_bow_hit h;
            h.index = -1; h.reserved = 0; h.id = -1; h.S = 0; h.score = 0.0;
            if (best_bits) {
                h.index = best_idx;
                h.id = db_ids[(head + best_idx) % cap];
                h.S = Sq[best_idx];
                h.score = __longlong_as_double((long long)best_bits);
            }
            hits[(int64_t)q * K + k] = h;
        }
        __syncthreads();
        prev_bits = s_best_bits;
        prev_idx = s_best_idx;
        if (prev_bits) found++;
        __syncthreads();
    }
    if (tid == 0) counts[q] = found;
}

int score_lds_bytes(int Vp) { return BW_QT * Vp * 4 + Vp * 2; }

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_bow_s : StageHandle {
    aria_bow_config cfg{};
    int V = 0, Vp = 0;                       // words of the vocabulary (0: none yet) and the ring's row stride
    DeviceBuffer<uint32_t> d_words;          // [BW_MAX_WORDS][8]
    DeviceBuffer<uint16_t> d_idf;            // [BW_MAX_WORDS]
    // the database: a ring of `capacity` slots, oldest at head
    DeviceBuffer<uint16_t> d_db_tf;          // [capacity][Vp]
    DeviceBuffer<int> d_db_norm;             // [capacity]
    DeviceBuffer<long long> d_db_ids;        // [capacity]
    std::vector<long long> ids;              // the ids again, by slot, for aria_bow_info
    long long head = 0;
    int size = 0;
    // grow-only workspace
    DeviceBuffer<uint2> d_keys;              // [frames][maxq]
    DeviceBuffer<int> d_cnt;                 // [frames]
    DeviceBuffer<long long> d_S;             // [queries of a chunk][size]
    DeviceBuffer<unsigned long long> d_bits;
    DeviceBuffer<int> d_qnorm;               // [queries of a chunk]: the norms the query kernels trust
    DeviceBuffer<uint32_t> d_members, d_present;   // training: [3][V] members, base, cursor; presence bits
    DeviceBuffer<int> d_list;
    DeviceBuffer<long long> d_src;
    DeviceBuffer<uint8_t> d_train_desc;      // host-buffer training
    DeviceBuffer<int> d_train_counts;
    DeviceBuffer<int> d_flag;                // the changed flag of an iteration
    // single-frame staging of the host forms
    DeviceBuffer<uint8_t> d_desc1;           // [rows][32]
    DeviceBuffer<uint16_t> d_tf1;            // [BW_MAX_WORDS]
    DeviceBuffer<int> d_norm1;               // norm, count
    DeviceBuffer<aria_bow_hit> d_hits1;      // [BW_MAX_K]
};

namespace {

bool bad_config(const aria_bow_config* c) {
    return !c || c->struct_size != (int)sizeof(aria_bow_config) || c->words < 1 || c->words > BW_MAX_WORDS || c->rows < 1 ||
           c->rows > BW_MAX_ROWS || c->capacity < 1 || c->top_k < 1 || c->top_k > BW_MAX_K || c->train_iters < 0;
}

// a vocabulary of V words now lies in d_words / d_idf: size the ring for it and empty the database
int adopt_vocabulary(aria_bow_s* h, int V) {
    const int Vp = (V + 7) & ~7;
    const int rc = h->d_db_tf.reserve(h->stream, (size_t)h->cfg.capacity * (size_t)Vp);
    if (rc != ARIA_OK) {
        h->V = h->Vp = 0;
        return rc;
    }
    h->V = V;
    h->Vp = Vp;
    h->head = 0;
    h->size = 0;
    return ARIA_OK;
}

// counts -> kNN-2 against the vocabulary -> keys of every frame at h->d_keys (maxq per frame), clamped counts at h->d_cnt
int quantise_frames(aria_bow_s* h, const uint8_t* d_desc, const int* d_counts, int fixed, int n_frames, int64_t desc_stride, int limit,
                    int maxq) {
    int rc;
    if ((rc = h->d_keys.reserve(h->stream, (size_t)n_frames * (size_t)maxq)) != ARIA_OK) return rc;
    if ((rc = h->d_cnt.reserve(h->stream, (size_t)n_frames)) != ARIA_OK) return rc;
    hipLaunchKernelGGL(k_bow_counts, dim3((n_frames + BW_BLOCK - 1) / BW_BLOCK), dim3(BW_BLOCK), 0, h->stream, d_counts, fixed, n_frames,
                       limit, h->d_cnt.p, h->d_err);
    launch_knn2_mfma(0, maxq, n_frames, h->stream, d_desc, h->d_cnt.p, 0, reinterpret_cast<const uint8_t*>(h->d_words.p), nullptr, h->V,
                     desc_stride * 32, 0, h->d_keys.p, maxq, 0.0, nullptr, h->V, nullptr);
    return ARIA_OK;
}

int transform_impl(aria_bow_s* h, const uint8_t* d_desc, const int* d_counts, int fixed, int n_frames, int64_t desc_stride, uint16_t* d_tf,
                   int32_t* d_norm) {
    const int limit = (int)std::min<int64_t>(desc_stride, h->cfg.rows);
    const int rc = quantise_frames(h, d_desc, d_counts, fixed, n_frames, desc_stride, limit, limit);
    if (rc != ARIA_OK) return rc;
    hipLaunchKernelGGL((k_bow_hist<false>), dim3(n_frames), dim3(BW_BLOCK), (size_t)h->V * 4, h->stream, h->d_keys.p, h->d_cnt.p,
                       (int64_t)limit, h->V, h->d_idf, d_tf, d_norm, (uint32_t*)nullptr, (uint32_t*)nullptr, 0);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int read_exact(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n ? 0 : -1; }

uint32_t le32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }

const uint8_t kMagic[8] = {'A', 'R', 'I', 'A', 'B', 'O', 'W', 0};
constexpr uint32_t kFileVersion = 1;

}  // namespace

extern "C" {

void aria_bow_default_config(aria_bow_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_bow_config);
    c->words = BW_MAX_WORDS;
    c->rows = BW_MAX_ROWS;
    c->capacity = 65536;
    c->top_k = 10;
    c->min_frames_between = 30;      // HipLoopDetector's
    c->train_iters = 10;
}

int aria_bow_create(const aria_bow_config* c, aria_bow_t* out) {
    if (!out || bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 1, "aria_bow_create", [](aria_bow_s* h) {
        const char* what = "aria_bow_create";
        const size_t capacity = (size_t)h->cfg.capacity;
        h->ids.assign(capacity, -1);
        int rc;
        if ((rc = h->d_words.reserve(h->stream, BW_MAX_WORDS * 8, what)) != ARIA_OK) return rc;
        if ((rc = h->d_idf.reserve(h->stream, BW_MAX_WORDS, what)) != ARIA_OK) return rc;
        if ((rc = h->d_db_norm.reserve(h->stream, capacity, what)) != ARIA_OK) return rc;
        if ((rc = h->d_db_ids.reserve(h->stream, capacity, what)) != ARIA_OK) return rc;
        if ((rc = h->d_flag.reserve(h->stream, 1, what)) != ARIA_OK) return rc;
        if ((rc = h->d_desc1.reserve(h->stream, (size_t)h->cfg.rows * 32, what)) != ARIA_OK) return rc;
        if ((rc = h->d_tf1.reserve(h->stream, BW_MAX_WORDS, what)) != ARIA_OK) return rc;
        if ((rc = h->d_norm1.reserve(h->stream, 2, what)) != ARIA_OK) return rc;
        if ((rc = h->d_hits1.reserve(h->stream, BW_MAX_K, what)) != ARIA_OK) return rc;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bow_score), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 score_lds_bytes(BW_MAX_WORDS));
        return e == hipSuccess ? (int)ARIA_OK : hip_fail(e, what, __FILE__, __LINE__);
    });
}

void aria_bow_destroy(aria_bow_t h) { stage_destroy(h); }

void* aria_bow_stream(aria_bow_t h) { return stage_stream(h); }

int aria_bow_check(aria_bow_t h) { return stage_check(h, {{ERRBIT_BOW_INPUT, ARIA_E_INVALID}}); }

int aria_bow_words(aria_bow_t h) { return h ? h->V : 0; }

int aria_bow_train_device(aria_bow_t h, const uint8_t* d_desc, const int* d_counts, int n_frames, int64_t desc_stride, int* iters_run) {
    if (iters_run) *iters_run = 0;
    if (!h || !d_desc || !d_counts || n_frames < 1 || n_frames > BW_MAX_FRAMES || desc_stride < 1 || desc_stride > (int64_t)INT_MAX / 64)
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const int V = h->cfg.words;
    std::vector<int> counts((size_t)n_frames);
    ARIA_HIP(memcpy_on(h->stream, counts.data(), d_counts, sizeof(int) * (size_t)n_frames, hipMemcpyDeviceToHost));
    long long n = 0;
    for (int c : counts) {
        if (c < 0 || c > desc_stride) return ARIA_E_INVALID;
        n += c;
    }
    if (n < V || n >= (long long)INT_MAX) return ARIA_E_INVALID;
    // initial word j: training descriptor floor(j * n / V) of the frames in order
    std::vector<long long> src((size_t)V);
    {
        long long before = 0;
        int f = 0;
        for (int j = 0; j < V; j++) {
            const long long at = ((long long)j * n) / V;
            while (at >= before + counts[f]) before += counts[f++];
            src[j] = (long long)f * desc_stride + (at - before);
        }
    }
    const int ps = ((V + BW_BLOCK - 1) / BW_BLOCK) * (BW_BLOCK / 32);
    int rc;
    if ((rc = h->d_src.reserve(h->stream, (size_t)V)) != ARIA_OK) return rc;
    if ((rc = h->d_members.reserve(h->stream, (size_t)3 * V)) != ARIA_OK) return rc;
    if ((rc = h->d_present.reserve(h->stream, (size_t)n_frames * ps)) != ARIA_OK) return rc;
    if ((rc = h->d_list.reserve(h->stream, (size_t)n)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemsetAsync(h->d_list.p, 0, sizeof(int) * (size_t)n, h->stream));      // every position a valid row, whatever happens
    ARIA_HIP(memcpy_on(h->stream, h->d_src.p, src.data(), sizeof(long long) * (size_t)V, hipMemcpyHostToDevice));
    h->V = V;                                // the kNN call reads it; adopt_vocabulary settles the rest
    hipLaunchKernelGGL(k_bow_init_words, dim3((V * 8 + BW_BLOCK - 1) / BW_BLOCK), dim3(BW_BLOCK), 0, h->stream, d_desc, h->d_src.p, V,
                       h->d_words);
    uint32_t* members = h->d_members.p;
    uint32_t* base = members + V;
    uint32_t* cursor = members + 2 * V;
    const int maxq = (int)desc_stride;
    int run = 0;
    auto quantise_and_count = [&]() -> int {
        const int r = quantise_frames(h, d_desc, d_counts, 0, n_frames, desc_stride, maxq, maxq);
        if (r != ARIA_OK) return r;
        ARIA_HIP(hipMemsetAsync(members, 0, sizeof(uint32_t) * (size_t)V, h->stream));
        hipLaunchKernelGGL((k_bow_hist<true>), dim3(n_frames), dim3(BW_BLOCK), (size_t)V * 4, h->stream, h->d_keys.p, h->d_cnt.p,
                           (int64_t)maxq, V, (const uint16_t*)nullptr, (uint16_t*)nullptr, (int*)nullptr, members, h->d_present.p, ps);
        return ARIA_OK;
    };
    rc = ARIA_OK;
    while (run < h->cfg.train_iters) {
        if ((rc = quantise_and_count()) != ARIA_OK) break;
        hipLaunchKernelGGL(k_bow_scan, dim3(1), dim3(BW_BLOCK), 0, h->stream, members, V, base, cursor);
        hipLaunchKernelGGL(k_bow_scatter, dim3(n_frames), dim3(BW_BLOCK), (size_t)V * 8, h->stream, h->d_keys.p, h->d_cnt.p, (int64_t)maxq,
                           V, desc_stride, cursor, h->d_list.p, (uint32_t)n);
        hipError_t e = hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream);
        if (e != hipSuccess) { rc = hip_fail(e, "aria_bow_train_device", __FILE__, __LINE__); break; }
        hipLaunchKernelGGL(k_bow_majority, dim3(V), dim3(64), 0, h->stream, d_desc, h->d_list.p, base, members, h->d_words, h->d_flag);
        int changed = 0;
        e = memcpy_on(h->stream, &changed, h->d_flag, sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { rc = hip_fail(e, "aria_bow_train_device", __FILE__, __LINE__); break; }
        run++;
        if (!changed) break;
    }
    if (rc == ARIA_OK) rc = quantise_and_count();
    if (rc == ARIA_OK) {
        hipLaunchKernelGGL(k_bow_idf, dim3((V + BW_BLOCK - 1) / BW_BLOCK), dim3(BW_BLOCK), 0, h->stream, h->d_present.p, ps, n_frames, V,
                           h->d_idf);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "aria_bow_train_device", __FILE__, __LINE__);
    }
    if (rc != ARIA_OK) {
        h->V = h->Vp = 0;
        return rc;
    }
    if (iters_run) *iters_run = run;
    return adopt_vocabulary(h, V);
}

int aria_bow_train(aria_bow_t h, const uint8_t* desc, const int* counts, int n_frames, int64_t desc_stride, int* iters_run) {
    if (iters_run) *iters_run = 0;
    if (!h || !desc || !counts || n_frames < 1 || n_frames > BW_MAX_FRAMES || desc_stride < 1 || desc_stride > (int64_t)INT_MAX / 64)
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const size_t bytes = (size_t)n_frames * (size_t)desc_stride * 32;
    int rc;
    if ((rc = h->d_train_desc.reserve(h->stream, bytes)) != ARIA_OK) return rc;
    if ((rc = h->d_train_counts.reserve(h->stream, (size_t)n_frames)) != ARIA_OK) return rc;
    ARIA_HIP(hipMemcpyAsync(h->d_train_desc.p, desc, bytes, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_train_counts.p, counts, sizeof(int) * (size_t)n_frames, hipMemcpyHostToDevice));
    return aria_bow_train_device(h, h->d_train_desc.p, h->d_train_counts.p, n_frames, desc_stride, iters_run);
}

int aria_bow_set_vocabulary(aria_bow_t h, const uint8_t* words, const uint16_t* idf_q, int V) {
    if (!h || !words || !idf_q || V < 1 || V > BW_MAX_WORDS) return ARIA_E_INVALID;
    for (int w = 0; w < V; w++)
        if (idf_q[w] >= 4096) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    ARIA_HIP(hipMemcpyAsync(h->d_words, words, (size_t)V * 32, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(memcpy_on(h->stream, h->d_idf, idf_q, (size_t)V * sizeof(uint16_t), hipMemcpyHostToDevice));
    return adopt_vocabulary(h, V);
}

int aria_bow_get_vocabulary(aria_bow_t h, uint8_t* words, uint16_t* idf_q, int* V) {
    if (!h || !V) return ARIA_E_INVALID;
    *V = h->V;
    if (h->V == 0) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    if (words) ARIA_HIP(memcpy_on(h->stream, words, h->d_words, (size_t)h->V * 32, hipMemcpyDeviceToHost));
    if (idf_q) ARIA_HIP(memcpy_on(h->stream, idf_q, h->d_idf, (size_t)h->V * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return ARIA_OK;
}

int aria_bow_save(aria_bow_t h, const char* path) {
    if (!h || !path || h->V == 0) return ARIA_E_INVALID;
    std::vector<uint8_t> words((size_t)h->V * 32);
    std::vector<uint16_t> idf((size_t)h->V);
    int V = 0;
    const int rc = aria_bow_get_vocabulary(h, words.data(), idf.data(), &V);
    if (rc != ARIA_OK) return rc;
    std::vector<uint8_t> blob;
    blob.insert(blob.end(), kMagic, kMagic + 8);
    for (uint32_t x : {kFileVersion, (uint32_t)V})
        for (int k = 0; k < 4; k++) blob.push_back((uint8_t)(x >> (8 * k)));
    blob.insert(blob.end(), words.begin(), words.end());
    for (uint16_t x : idf) {
        blob.push_back((uint8_t)(x & 0xFF));
        blob.push_back((uint8_t)(x >> 8));
    }
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return ARIA_E_INVALID;
    const bool ok = std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
    return (std::fclose(f) == 0 && ok) ? ARIA_OK : ARIA_E_INVALID;
}

int aria_bow_load(aria_bow_t h, const char* path) {
    if (!h || !path) return ARIA_E_INVALID;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return ARIA_E_INVALID;
    uint8_t head[16];
    std::vector<uint8_t> words, idf_b;
    bool ok = read_exact(f, head, 16) == 0 && std::memcmp(head, kMagic, 8) == 0 && le32(head + 8) == kFileVersion;
    const uint32_t V = ok ? le32(head + 12) : 0;
    ok = ok && V >= 1 && V <= (uint32_t)BW_MAX_WORDS;
    if (ok) {
        words.resize((size_t)V * 32);
        idf_b.resize((size_t)V * 2);
        uint8_t extra;
        ok = read_exact(f, words.data(), words.size()) == 0 && read_exact(f, idf_b.data(), idf_b.size()) == 0 &&
             std::fread(&extra, 1, 1, f) == 0;                      // nothing may follow
    }
    std::fclose(f);
    if (!ok) return ARIA_E_INVALID;
    std::vector<uint16_t> idf((size_t)V);
    for (uint32_t w = 0; w < V; w++) idf[w] = (uint16_t)(idf_b[2 * w] | (idf_b[2 * w + 1] << 8));
    return aria_bow_set_vocabulary(h, words.data(), idf.data(), (int)V);
}

int aria_bow_transform_batch_device(aria_bow_t h, const uint8_t* d_desc, const int* d_counts, int n_frames, int64_t desc_stride,
                                    uint16_t* d_tf, int32_t* d_norm) {
    if (!h || h->V == 0 || !d_desc || !d_counts || !d_tf || !d_norm || n_frames < 0 || desc_stride < 1 ||
        desc_stride > (int64_t)INT_MAX / 64)
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    return transform_impl(h, d_desc, d_counts, 0, n_frames, desc_stride, d_tf, d_norm);
}

int aria_bow_add_batch_device(aria_bow_t h, const uint16_t* d_tf, const int32_t* d_norm, const long long* ids, int n) {
    if (!h || h->V == 0 || n < 0 || (n && (!d_tf || !d_norm || !ids))) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const long long cap = h->cfg.capacity;
    for (int at = 0; at < n;) {
        const int m = (int)std::min<long long>(std::min<long long>(n - at, BW_IDS), cap);
        BowIds arg;
        for (int j = 0; j < m; j++) arg.v[j] = ids[at + j];
        // make room: what the chunk pushes out leaves at the head
        const long long drop = std::max<long long>(0, (long long)h->size + m - cap);
        h->head = (h->head + drop) % cap;
        h->size -= (int)drop;
        const long long first = (h->head + h->size) % cap;
        hipLaunchKernelGGL(k_bow_store, dim3(m), dim3(BW_BLOCK), 0, h->stream, d_tf + (int64_t)at * h->V, d_norm + at, arg, h->V, h->Vp,
                           h->d_idf, first, cap, h->d_db_tf.p, h->d_db_norm, h->d_db_ids, h->d_err);
        for (int j = 0; j < m; j++) h->ids[(size_t)((first + j) % cap)] = ids[at + j];
        h->size += m;
        at += m;
    }
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_bow_add_device(aria_bow_t h, long long id, const uint8_t* d_desc, int n) {
    if (!h || h->V == 0 || n < 0 || n > h->cfg.rows || (n && !d_desc)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const int rc = transform_impl(h, n ? d_desc : h->d_desc1.p, nullptr, n, 1, h->cfg.rows, h->d_tf1, h->d_norm1);
    return rc != ARIA_OK ? rc : aria_bow_add_batch_device(h, h->d_tf1, h->d_norm1, &id, 1);
}

int aria_bow_add(aria_bow_t h, long long id, const uint8_t* desc_host, int n) {
    if (!h || h->V == 0 || n < 0 || n > h->cfg.rows || (n && !desc_host)) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    if (n) ARIA_HIP(memcpy_on(h->stream, h->d_desc1, desc_host, (size_t)n * 32, hipMemcpyHostToDevice));
    return aria_bow_add_device(h, id, h->d_desc1, n);
}

int aria_bow_size(aria_bow_t h) { return h ? h->size : 0; }

int aria_bow_info(aria_bow_t h, int index, long long* id, int* norm) {
    if (!h || index < 0 || index >= h->size) return ARIA_E_INVALID;
    const long long slot = (h->head + index) % h->cfg.capacity;
    if (id) *id = h->ids[(size_t)slot];
    if (norm) {
        ARIA_HIP(hipSetDevice(h->device));
        ARIA_HIP(memcpy_on(h->stream, norm, h->d_db_norm + slot, sizeof(int), hipMemcpyDeviceToHost));
    }
    return ARIA_OK;
}

int aria_bow_query_batch_device(aria_bow_t h, const uint16_t* d_tf, const int32_t* d_norm, const long long* query_ids, int n_queries,
                                aria_bow_hit* d_hits, int* d_counts) {
    if (!h || h->V == 0 || n_queries < 0 || (n_queries && (!d_tf || !d_norm || !query_ids || !d_hits || !d_counts))) return ARIA_E_INVALID;
    if (n_queries == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const int K = h->cfg.top_k, size = h->size;
    // the numerators of a chunk of queries against every entry: at most 2^25 of them (256 MiB) at a time
    const int chunk = (int)std::max<long long>(1, std::min<long long>(BW_IDS, (1ll << 25) / std::max(size, 1)));
    int rc;
    if ((rc = h->d_S.reserve(h->stream, (size_t)std::min(chunk, n_queries) * (size_t)std::max(size, 1))) != ARIA_OK) return rc;
    if ((rc = h->d_bits.reserve(h->stream, (size_t)std::min(chunk, n_queries) * (size_t)std::max(size, 1))) != ARIA_OK) return rc;
    if ((rc = h->d_qnorm.reserve(h->stream, (size_t)std::min(chunk, n_queries))) != ARIA_OK) return rc;
    for (int at = 0; at < n_queries; at += chunk) {
        const int m = std::min(chunk, n_queries - at);
        BowIds arg;
        for (int j = 0; j < m; j++) arg.v[j] = query_ids[at + j];
        hipLaunchKernelGGL(k_bow_check_query, dim3(m), dim3(BW_BLOCK), 0, h->stream, d_tf + (int64_t)at * h->V, d_norm + at, h->V, h->d_idf,
                           h->d_qnorm.p, h->d_err);
        if (size > 0)
            hipLaunchKernelGGL(k_bow_score, dim3((size + BW_EPB - 1) / BW_EPB, (m + BW_QT - 1) / BW_QT), dim3(BW_BLOCK),
                               (size_t)score_lds_bytes(h->Vp), h->stream, d_tf + (int64_t)at * h->V, h->d_qnorm.p, m, h->V, h->Vp, h->d_idf,
                               h->d_db_tf.p, h->d_db_norm, h->head, size, (long long)h->cfg.capacity, h->d_S.p);
        hipLaunchKernelGGL(k_bow_topk, dim3(m), dim3(BW_BLOCK), 0, h->stream, h->d_S.p, h->d_bits.p, h->d_qnorm.p, arg, h->d_db_norm,
                           h->d_db_ids, h->head, size, (long long)h->cfg.capacity, h->cfg.min_frames_between, K, d_hits + (int64_t)at * K,
                           d_counts + at);
    }
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_bow_query_device(aria_bow_t h, long long query_id, const uint8_t* d_desc, int n, aria_bow_hit* hits, int* n_out) {
    if (n_out) *n_out = 0;
    if (!h || h->V == 0 || n < 0 || n > h->cfg.rows || (n && !d_desc) || !hits) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = transform_impl(h, n ? d_desc : h->d_desc1.p, nullptr, n, 1, h->cfg.rows, h->d_tf1, h->d_norm1);
    if (rc != ARIA_OK) return rc;
    if ((rc = aria_bow_query_batch_device(h, h->d_tf1, h->d_norm1, &query_id, 1, h->d_hits1, h->d_norm1 + 1)) != ARIA_OK) return rc;
    int count = 0;
    ARIA_HIP(hipMemcpyAsync(hits, h->d_hits1, sizeof(aria_bow_hit) * (size_t)h->cfg.top_k, hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(memcpy_on(h->stream, &count, h->d_norm1 + 1, sizeof(int), hipMemcpyDeviceToHost));
    if (n_out) *n_out = count;
    return aria_bow_check(h);
}

int aria_bow_query(aria_bow_t h, long long query_id, const uint8_t* desc_host, int n, aria_bow_hit* hits, int* n_out) {
    if (n_out) *n_out = 0;
    if (!h || h->V == 0 || n < 0 || n > h->cfg.rows || (n && !desc_host) || !hits) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    if (n) ARIA_HIP(memcpy_on(h->stream, h->d_desc1, desc_host, (size_t)n * 32, hipMemcpyHostToDevice));
    return aria_bow_query_device(h, query_id, h->d_desc1, n, hits, n_out);
}

}  // extern "C"
