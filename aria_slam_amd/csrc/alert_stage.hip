// Obstacle alerts: an exact order statistic of the valid fp32 depths inside three image zones and every detection box of a
// frame, and the arbitration of the candidates they give into a short, prioritised, non-repeating list of events per track.
// Semantics in include/aria_orb_hip.h ("obstacle alerts"); aria_slam_amd/alert_ref.py is the definition and this file equals
// it bit for bit. Integer arithmetic and fp32 compares; no float atomics.
//
// k_alert_measure    one workgroup of 1024 lanes per (frame, source). Exact selection on the uint32 bit patterns of the valid
//                    depths (positive floats order as their bits): three radix passes of 11 + 11 + 10 bits, each a walk of the
//                    rectangle into an LDS histogram (four copies) filled by integer LDS atomics, a workgroup scan to the bin that holds rank
//                    k, and the rank inside that bin for the next pass. The first pass also counts n. A row is walked by
//                    min(64, pow2 >= w) consecutive lanes along x (coalesced, any left edge, any pitch), the other lanes of
//                    the wave take the rows below. Empty rectangles and n < min_valid take one pass or none.
// k_alert_measure_plain  (variants build only) the plainest exact form: a bitwise bisection of 32 counting passes, each
//                    re-reading the rectangle. The yardstick of tools/alert_rate.py.
// k_alert_arbitrate  one wave per track, persistent over the track's frames; the cooldown state sits in LDS and is stored
//                    once. A lane holds each of the 64 source slots; a lane's rank under rule 4 by comparison against the other
//                    lanes (the pattern of detect_stage.hip), then the walk in rank order, wave-uniform, bounded by 64 a frame.
// Plain HIP C++. The text between "// ---- rules" and "// ---- kernels" also compiles for the host
// (tests/test_alert_kernel_emulation.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

static_assert(sizeof(aria_alert_meas) == 16, "aria_alert_meas is 16 bytes");
static_assert(sizeof(aria_alert_event) == 32, "aria_alert_event is 32 bytes");
static_assert(sizeof(aria_alert_state) == 2320, "aria_alert_state is 2320 bytes");
static_assert(sizeof(aria_alert_config) == 264, "aria_alert_config is 264 bytes");
static_assert(sizeof(aria_detection) == 24, "aria_detection is 24 bytes");

namespace {

// ---- rules (plain functions, no cross-lane operation) ---------------------------------------------------------------------
constexpr int ALERT_SOURCES = 64;
constexpr int ERRBIT_ALERT_INPUT = 1, ERRBIT_ALERT_CAP = 2;

// What the kernels take by value.
struct AlertParams {
    int width, height, zone_top, zone_bottom, bound0, bound1;
    int max_dets, min_valid;
    float min_depth, max_depth;
    int zone_num, zone_den, det_num, det_den;
    float zone_alert_m, default_depth, crit_m, high_m, medium_m, beep_m;
    int obstacle_dangerous, n_dangerous;
    int dangerous[32];
    int max_events;
    long long cooldown_ns[4];
};

struct AlertRect { int x0, y0, x1, y1; };      // columns [x0, x1), rows [y0, y1); empty when either range is

struct AlertCand {
    int cand, class_id, direction, priority, flags;
    float distance;
};

// rule 1: 0 CENTER, 1 LEFT, 2 RIGHT from a normalised abscissa, as the compares fall (a NaN is CENTER)
__host__ __device__ inline int alert_direction(float nrm) { return nrm < 0.35f ? 1 : nrm > 0.65f ? 2 : 0; }

__host__ __device__ inline int alert_column_zone(int x, int width) { return alert_direction(((float)x + 0.5f) / (float)width); }

// rule 1: the detections of a frame that are sources; *bad when the count is outside [0, det_cap]
__host__ __device__ inline int alert_det_count(int count, int det_cap, int max_dets, bool* bad) {
    *bad = count < 0 || count > det_cap;
    return *bad ? 0 : (count < max_dets ? count : max_dets);
}

__host__ __device__ inline bool alert_corner_ok(float v) { return v >= -1048576.0f && v <= 1048576.0f; }   // false for NaN and Inf

__host__ __device__ inline AlertRect alert_source_rect(const AlertParams& P, int source, const aria_detection& d) {
    AlertRect r;
    if (source < 3) {
        r.y0 = P.zone_top; r.y1 = P.zone_bottom;
        r.x0 = source == 1 ? 0 : source == 0 ? P.bound0 : P.bound1;
        r.x1 = source == 1 ? P.bound0 : source == 0 ? P.bound1 : P.width;
        return r;
    }
    r.x0 = r.y0 = r.x1 = r.y1 = 0;
    if (!(alert_corner_ok(d.x1) && alert_corner_ok(d.y1) && alert_corner_ok(d.x2) && alert_corner_ok(d.y2))) return r;
    const int ax = (int)d.x1, ay = (int)d.y1, bx = (int)d.x2, by = (int)d.y2;
    r.x0 = ax > 0 ? ax : 0; r.x1 = bx < P.width ? bx : P.width;
    r.y0 = ay > 0 ? ay : 0; r.y1 = by < P.height ? by : P.height;
    return r;
}

__host__ __device__ inline bool alert_rect_empty(const AlertRect& r) { return r.x0 >= r.x1 || r.y0 >= r.y1; }

__host__ __device__ inline bool alert_valid_depth(const AlertParams& P, float d) { return d >= P.min_depth && d <= P.max_depth; }

// rule 2: the index taken among n valid depths
__host__ __device__ inline long long alert_rank(long long n, int num, int den) { return n * (long long)num / (long long)den; }

__host__ __device__ inline bool alert_dangerous(const AlertParams& P, int class_id) {
    if (class_id == -1) return P.obstacle_dangerous != 0;
    bool hit = false;
    for (int i = 0; i < P.n_dangerous; i++) hit = hit || P.dangerous[i] == class_id;
    return hit;
}

__host__ __device__ inline int alert_priority(const AlertParams& P, int class_id, float distance) {
    if (distance < P.crit_m) return 3;
    if (distance < P.high_m && alert_dangerous(P, class_id)) return 2;
    if (distance < P.medium_m) return 1;
    return 0;
}

// rule 3 for one source slot; is_source: the slot is a zone or one of the frame's detections
__host__ __device__ inline AlertCand alert_classify(const AlertParams& P, int source, bool is_source, const aria_alert_meas& m,
                                           const aria_detection& d) {
    AlertCand c;
    c.cand = 0; c.class_id = -1; c.direction = 0; c.priority = 0; c.flags = 0; c.distance = 0.0f;
    if (!is_source) return c;
    const bool measured = (m.flags & ARIA_ALERT_MEAS_OK) != 0;
    if (source < 3) {
        if (!measured || !(m.distance < P.zone_alert_m)) return c;
        c.direction = source;
        c.distance = m.distance;
    } else {
        c.class_id = d.class_id;
        const float cx = (d.x1 + d.x2) / 2.0f;
        const float nrm = cx / (float)P.width;
        c.direction = alert_direction(nrm);
        c.distance = measured ? m.distance : P.default_depth;
        c.flags = measured ? 0 : ARIA_ALERT_NO_DEPTH;
    }
    c.cand = 1;
    c.priority = alert_priority(P, c.class_id, c.distance);
    if (c.distance < P.beep_m) c.flags |= ARIA_ALERT_BEEP;
    if (c.priority == 3) c.flags |= ARIA_ALERT_CRITICAL_ALERT | ARIA_ALERT_INTERRUPT;
    return c;
}

// rule 4: a strictly before b
__host__ __device__ inline bool alert_precedes(int a_prio, float a_dist, int a_dir, int a_src, int b_prio, float b_dist, int b_dir, int b_src) {
    if (a_prio != b_prio) return a_prio > b_prio;
    if (a_dist < b_dist) return true;
    if (b_dist < a_dist) return false;
    if (a_dir != b_dir) return a_dir < b_dir;
    return a_src < b_src;
}

// rule 5
__host__ __device__ inline int alert_key(int class_id, int direction) {
    const int ck = class_id == -1 ? 0 : 1 + (class_id < 0 ? 0 : class_id > 83 ? 83 : class_id);
    return ck * 3 + direction;
}

__host__ __device__ inline bool alert_may_announce(int last_prio1, long long last_ns, int priority, long long t, long long cooldown_ns) {
    return last_prio1 == 0 || priority + 1 > last_prio1 || t - last_ns >= cooldown_ns;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
constexpr int AM_BLOCK = 1024, AM_WAVES = AM_BLOCK / 64, AM_BINS = 2048;
// The histogram is kept in four copies, lane l counting into copy l & 3: neighbouring pixels hold neighbouring depths, so the lanes
// of a wave would otherwise queue on a handful of words. A copy starts 8 words past a multiple of 32, so that the same bin of the
// four copies lies on four different banks.
constexpr int AM_COPIES = 4, AM_COPY_STRIDE = AM_BINS + 8;

// The valid bit patterns of a rectangle, each handed to `visit` once. lpr = min(64, pow2 >= w) consecutive lanes walk a row
// along x; a wave takes 64 / lpr rows a step and the workgroup's 16 waves take consecutive groups of rows. A lane loads the pixels
// of four such steps before it looks at any of them (four loads in flight); a row beyond the rectangle counts as 0.0f, which is
// never valid (min_depth > 0).
template <typename F>
__device__ __forceinline__ void alert_walk(const AlertParams& P, const AlertRect& r, const float* __restrict__ depth, int pitch, F visit) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int w = r.x1 - r.x0;
    int lg = 0;
    while (lg < 6 && (1 << lg) < w) lg++;
    const int lpr = 1 << lg, rows_per_wave = 64 >> lg;
    const int col = lane & (lpr - 1), sub = lane >> lg;
    const int step = AM_WAVES * rows_per_wave;
    for (int y = r.y0 + wave * rows_per_wave + sub; y < r.y1; y += 4 * step) {
        for (int x = r.x0 + col; x < r.x1; x += lpr) {
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int yy = y + j * step;
                d[j] = yy < r.y1 ? depth[(size_t)yy * (size_t)pitch + x] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (alert_valid_depth(P, d[j])) visit(__float_as_uint(d[j]));
        }
    }
}

// Inclusive scan of one value per lane over the workgroup; *total = the sum. Two barriers; s_wave is free again on return.
__device__ __forceinline__ unsigned alert_block_scan(unsigned v, unsigned* s_wave, unsigned* total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    unsigned off = 0, tot = 0;
    for (int i = 0; i < AM_WAVES; i++) {
        const unsigned x = s_wave[i];
        off += i < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return v + off;
}

// The frame and source of a workgroup, what rule 1 makes of it, and the "none" record. Returns false when the workgroup is
// done (the slot is no source, or its rectangle is empty); the same for every lane.
__device__ __forceinline__ bool alert_measure_setup(const AlertParams& P, const aria_detection* __restrict__ dets, const int* __restrict__ ndets,
                                                    int det_cap, aria_alert_meas* __restrict__ meas, int* err, AlertRect* r, size_t* slot,
                                                    int* f_out) {
    const int f = (int)(blockIdx.x >> 6), s = (int)(blockIdx.x & 63), t = (int)threadIdx.x;
    *f_out = f;
    *slot = (size_t)f * ALERT_SOURCES + s;
    int n_det = 0;
    if (ndets) {
        const int count = ndets[f];
        bool bad;
        n_det = alert_det_count(count, det_cap, P.max_dets, &bad);
        if (s == 0 && t == 0) {
            if (bad) atomicOr(err, ERRBIT_ALERT_INPUT);
            else if (count > P.max_dets) atomicMax(err + 1, count);
        }
    }
    aria_alert_meas m;
    m.distance = -1.0f; m.n_valid = 0; m.k = 0; m.flags = 0;
    if (s >= 3 + n_det) {
        if (t == 0) meas[*slot] = m;
        return false;
    }
    aria_detection d;
    d.x1 = d.y1 = d.x2 = d.y2 = d.confidence = 0.0f; d.class_id = 0;
    if (s >= 3) d = dets[(size_t)f * det_cap + (s - 3)];
    *r = alert_source_rect(P, s, d);
    if (alert_rect_empty(*r)) {
        m.flags = ARIA_ALERT_MEAS_SOURCE;
        if (t == 0) meas[*slot] = m;
        return false;
    }
    return true;
}

// grid: n_frames * 64
__global__ __launch_bounds__(AM_BLOCK) void k_alert_measure(AlertParams P, const float* __restrict__ depth, long long depth_stride, int pitch,
                                                            const aria_detection* __restrict__ dets, const int* __restrict__ ndets, int det_cap,
                                                            aria_alert_meas* __restrict__ meas, int* err) {
    __shared__ unsigned s_hist[AM_COPIES * AM_COPY_STRIDE];
    __shared__ unsigned s_wave[AM_WAVES];
    __shared__ unsigned s_sel[2];                                        // the bin of rank k, and k's rank inside it
    const int t = (int)threadIdx.x;
    AlertRect r;
    size_t slot;
    int f;
    if (!alert_measure_setup(P, dets, ndets, det_cap, meas, err, &r, &slot, &f)) return;
    const float* __restrict__ D = depth + (size_t)f * (size_t)depth_stride;
    const bool zone = (blockIdx.x & 63) < 3;
    unsigned prefix = 0, k = 0, n = 0;
    for (int pass = 0; pass < 3; pass++) {
        for (int c = 0; c < AM_COPIES; c++) { s_hist[c * AM_COPY_STRIDE + 2 * t] = 0; s_hist[c * AM_COPY_STRIDE + 2 * t + 1] = 0; }
        __syncthreads();
        unsigned* hist = s_hist + (t & (AM_COPIES - 1)) * AM_COPY_STRIDE;
        if (pass == 0) alert_walk(P, r, D, pitch, [&](unsigned u) { atomicAdd(&hist[u >> 21], 1u); });
        else if (pass == 1) alert_walk(P, r, D, pitch, [&](unsigned u) { if ((u >> 21) == prefix) atomicAdd(&hist[(u >> 10) & 0x7FFu], 1u); });
        else alert_walk(P, r, D, pitch, [&](unsigned u) { if ((u >> 10) == prefix) atomicAdd(&hist[u & 0x3FFu], 1u); });
        __syncthreads();
        unsigned c0 = 0, c1 = 0;
        for (int c = 0; c < AM_COPIES; c++) { c0 += s_hist[c * AM_COPY_STRIDE + 2 * t]; c1 += s_hist[c * AM_COPY_STRIDE + 2 * t + 1]; }
        unsigned total;
        const unsigned incl = alert_block_scan(c0 + c1, s_wave, &total);
        if (pass == 0) {
            n = total;
            if ((long long)n < (long long)P.min_valid) {                 // the same for every lane
                if (t == 0) {
                    aria_alert_meas m;
                    m.distance = -1.0f; m.n_valid = (int)n; m.k = 0; m.flags = ARIA_ALERT_MEAS_SOURCE;
                    meas[slot] = m;
                }
                return;
            }
            k = (unsigned)alert_rank((long long)n, zone ? P.zone_num : P.det_num, zone ? P.zone_den : P.det_den);
        }
        const unsigned rank = pass == 0 ? k : s_sel[1];
        __syncthreads();                                                 // everyone has read s_sel before it is written again
        const unsigned excl = incl - c0 - c1;
        if (rank >= excl && rank < excl + c0) { s_sel[0] = 2u * t; s_sel[1] = rank - excl; }
        else if (rank >= excl + c0 && rank < incl) { s_sel[0] = 2u * t + 1u; s_sel[1] = rank - excl - c0; }
        __syncthreads();
        prefix = pass == 0 ? s_sel[0] : pass == 1 ? (prefix << 11) | s_sel[0] : (prefix << 10) | s_sel[0];
    }
    if (t == 0) {
        aria_alert_meas m;
        m.distance = __uint_as_float(prefix); m.n_valid = (int)n; m.k = (int)k; m.flags = ARIA_ALERT_MEAS_SOURCE | ARIA_ALERT_MEAS_OK;
        meas[slot] = m;
    }
}

#ifdef ARIA_VARIANTS
// The yardstick: the largest pattern v with |{valid u < v}| <= k is the value of rank k; one counting pass per bit.
__global__ __launch_bounds__(AM_BLOCK) void k_alert_measure_plain(AlertParams P, const float* __restrict__ depth, long long depth_stride, int pitch,
                                                                  const aria_detection* __restrict__ dets, const int* __restrict__ ndets,
                                                                  int det_cap, aria_alert_meas* __restrict__ meas, int* err) {
    __shared__ unsigned s_wave[AM_WAVES];
    const int t = (int)threadIdx.x;
    AlertRect r;
    size_t slot;
    int f;
    if (!alert_measure_setup(P, dets, ndets, det_cap, meas, err, &r, &slot, &f)) return;
    const float* __restrict__ D = depth + (size_t)f * (size_t)depth_stride;
    const bool zone = (blockIdx.x & 63) < 3;
    unsigned mine = 0, n;
    alert_walk(P, r, D, pitch, [&](unsigned) { mine++; });
    alert_block_scan(mine, s_wave, &n);
    aria_alert_meas m;
    m.distance = -1.0f; m.n_valid = (int)n; m.k = 0; m.flags = ARIA_ALERT_MEAS_SOURCE;
    if ((long long)n >= (long long)P.min_valid) {
        const unsigned k = (unsigned)alert_rank((long long)n, zone ? P.zone_num : P.det_num, zone ? P.zone_den : P.det_den);
        unsigned ans = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const unsigned cand = ans | (1u << bit);
            unsigned below;
            mine = 0;
            alert_walk(P, r, D, pitch, [&](unsigned u) { mine += u < cand ? 1u : 0u; });
            alert_block_scan(mine, s_wave, &below);
            if (below <= k) ans = cand;
        }
        m.distance = __uint_as_float(ans); m.k = (int)k; m.flags |= ARIA_ALERT_MEAS_OK;
    }
    if (t == 0) meas[slot] = m;
}
#endif

// grid: n_tracks, one wave each
__global__ __launch_bounds__(64) void k_alert_arbitrate(AlertParams P, const int* __restrict__ track_offset, const long long* __restrict__ timestamps,
                                                        int n_frames, const aria_alert_meas* __restrict__ meas,
                                                        const aria_detection* __restrict__ dets, const int* __restrict__ ndets, int det_cap,
                                                        aria_alert_state* __restrict__ states, aria_alert_event* __restrict__ events,
                                                        int event_cap, int* __restrict__ nevents, int* err) {
    __shared__ long long s_last[256];
    __shared__ unsigned char s_prio1[256];
    const int lane = (int)threadIdx.x, track = (int)blockIdx.x;
    const int f0 = track_offset[track], f1 = track_offset[track + 1];
    if (f0 < 0 || f1 < f0 || f1 > n_frames) {                            // the same for every lane
        if (lane == 0) { nevents[track] = 0; atomicOr(err, ERRBIT_ALERT_INPUT); }
        return;
    }
    aria_alert_state* st = states + track;
    for (int i = lane; i < 256; i += 64) { s_last[i] = st->last_ns[i]; s_prio1[i] = st->last_prio1[i]; }
    __syncthreads();
    long long total = 0, prev = 0;
    bool have_prev = false;
    for (int f = f0; f < f1; f++) {
        const long long ts = timestamps[f];
        if (have_prev && ts < prev) {
            if (lane == 0) atomicOr(err, ERRBIT_ALERT_INPUT);
            continue;
        }
        prev = ts; have_prev = true;
        int n_det = 0;
        if (ndets) {
            bool bad;
            n_det = alert_det_count(ndets[f], det_cap, P.max_dets, &bad);
            if (bad && lane == 0) atomicOr(err, ERRBIT_ALERT_INPUT);
        }
        const bool is_source = lane < 3 + n_det;
        const aria_alert_meas m = meas[(size_t)f * ALERT_SOURCES + lane];
        aria_detection d;
        d.x1 = d.y1 = d.x2 = d.y2 = d.confidence = 0.0f; d.class_id = 0;
        if (is_source && lane >= 3) d = dets[(size_t)f * det_cap + (lane - 3)];
        const AlertCand c = alert_classify(P, lane, is_source, m, d);
        const unsigned long long cands = __ballot(c.cand);
        const int n_cand = __popcll(cands);
        if (n_cand == 0) continue;
        int rank = 0;
        for (int j = 0; j < 64; j++) {
            if (!((cands >> j) & 1ull)) continue;                        // wave-uniform
            const int o_prio = __shfl(c.priority, j, 64), o_dir = __shfl(c.direction, j, 64);
            const float o_dist = __shfl(c.distance, j, 64);
            rank += alert_precedes(o_prio, o_dist, o_dir, j, c.priority, c.distance, c.direction, lane) ? 1 : 0;
        }
        int announced = 0;
        for (int r = 0; r < n_cand && announced < P.max_events; r++) {
            const unsigned long long who = __ballot(c.cand && rank == r);
            if (who == 0) break;                                         // cannot happen under a strict total order
            const int src = __ffsll((long long)who) - 1;
            const int cls = __shfl(c.class_id, src, 64), dir = __shfl(c.direction, src, 64), prio = __shfl(c.priority, src, 64);
            const int flags = __shfl(c.flags, src, 64);
            const float dist = __shfl(c.distance, src, 64);
            const int key = alert_key(cls, dir);
            const bool go = alert_may_announce(s_prio1[key], s_last[key], prio, ts, P.cooldown_ns[prio]);
            __syncthreads();                                             // the key's words are read before lane 0 replaces them
            if (!go) continue;
            if (lane == 0) {
                s_prio1[key] = (unsigned char)(prio + 1);
                s_last[key] = ts;
                if (total < (long long)event_cap) {
                    aria_alert_event e;
                    e.frame = f; e.source = src; e.class_id = cls; e.direction = dir; e.priority = prio; e.distance = dist;
                    e.flags = flags; e.reserved = 0;
                    events[(size_t)track * event_cap + (size_t)total] = e;
                }
            }
            total++;
            announced++;
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = lane; i < 256; i += 64) { st->last_ns[i] = s_last[i]; st->last_prio1[i] = s_prio1[i]; }
    if (lane == 0) {
        st->events_total += total;
        nevents[track] = (int)total;
        if (total > (long long)event_cap) atomicOr(err, ERRBIT_ALERT_CAP);
    }
}

}  // namespace

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct aria_alert_s : StageHandle {
    aria_alert_config cfg{};
    AlertParams P{};
    int plain = 0;                                             // variants build: ARIA_ALERT_SELECT=plain
    int dets_seen = 0;
    DeviceBuffer<aria_alert_meas> d_meas;                      // run_batch_device, and the host forms
    // host-form staging (grow-only)
    DeviceBuffer<float> d_depth;
    DeviceBuffer<aria_detection> d_dets;
    DeviceBuffer<int> d_ints;                                  // ndets, track offsets, nevents
    DeviceBuffer<long long> d_ts;
    DeviceBuffer<aria_alert_state> d_states;
    DeviceBuffer<aria_alert_event> d_events;
};

namespace {

constexpr int ALERT_MAX_DIM = 8192, ALERT_MAX_FRAMES = 1 << 24;

bool alert_bad_config(const aria_alert_config* c) {
    if (!c || c->struct_size != (int)sizeof(aria_alert_config)) return true;
    if (c->width < 1 || c->width > ALERT_MAX_DIM || c->height < 1 || c->height > ALERT_MAX_DIM) return true;
    if (c->zone_top < 0 || c->zone_top >= c->zone_bottom || c->zone_bottom > c->height) return true;
    if (c->max_dets < 0 || c->max_dets > ARIA_ALERT_MAX_DETS || c->min_valid < 1) return true;
    if (!std::isfinite(c->min_depth) || !std::isfinite(c->max_depth) || !(c->min_depth > 0.0f) || !(c->min_depth <= c->max_depth)) return true;
    if (c->zone_pct_num < 0 || c->zone_pct_num >= c->zone_pct_den || c->det_pct_num < 0 || c->det_pct_num >= c->det_pct_den) return true;
    for (float v : {c->zone_alert_m, c->default_depth, c->crit_m, c->high_m, c->medium_m, c->beep_m})
        if (!std::isfinite(v)) return true;
    if (c->n_dangerous < 0 || c->n_dangerous > 32 || c->max_events_per_frame < 0 || c->max_events_per_frame > ALERT_SOURCES) return true;
    for (long long v : c->cooldown_ns)
        if (v < 0) return true;
    return false;
}

bool alert_bad_frames(const aria_alert_s* h, int64_t depth_stride, int depth_pitch, int n_frames, const void* dets, const void* ndets, int det_cap) {
    if (n_frames < 0 || n_frames > ALERT_MAX_FRAMES || depth_pitch < h->cfg.width || depth_stride < 0) return true;
    if ((dets == nullptr) != (ndets == nullptr)) return true;
    return dets && (det_cap < 0 || det_cap > (1 << 20));
}

}  // namespace

extern "C" {

int aria_alert_zone_bounds(int width, int out[2]) {
    if (width < 1 || width > ALERT_MAX_DIM || !out) return ARIA_E_INVALID;
    int b0 = width, b1 = width;
    for (int x = width - 1; x >= 0; x--) {
        const int z = alert_column_zone(x, width);
        if (z == 2) b1 = x;
        if (z != 1) b0 = x;
    }
    out[0] = b0; out[1] = b1;
    return ARIA_OK;
}

int64_t aria_alert_algorithmic_bytes(int width, int zone_top, int zone_bottom, int n_frames) {
    if (width < 1 || width > ALERT_MAX_DIM || zone_top < 0 || zone_top >= zone_bottom || zone_bottom > ALERT_MAX_DIM || n_frames < 0 ||
        n_frames > ALERT_MAX_FRAMES)
        return ARIA_E_INVALID;
    return (int64_t)n_frames * ((int64_t)4 * width * (zone_bottom - zone_top) + 16 * ALERT_SOURCES);
}

void aria_alert_default_config(aria_alert_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_alert_config);
    c->width = 752; c->height = 480; c->zone_top = 120; c->zone_bottom = 480;
    c->max_dets = 32; c->min_valid = 16; c->min_depth = 0.1f; c->max_depth = 20.0f;
    c->zone_pct_num = 5; c->zone_pct_den = 100; c->det_pct_num = 1; c->det_pct_den = 2;
    c->zone_alert_m = 3.0f; c->default_depth = 5.0f; c->crit_m = 1.0f; c->high_m = 2.0f; c->medium_m = 3.0f; c->beep_m = 1.5f;
    c->obstacle_dangerous = 1; c->n_dangerous = 6;
    const int dangerous[6] = {0, 1, 2, 3, 5, 7};                         // H16:472
    for (int i = 0; i < 6; i++) c->dangerous[i] = dangerous[i];
    c->max_events_per_frame = 2;
    c->cooldown_ns[0] = 2000000000ll; c->cooldown_ns[1] = 800000000ll; c->cooldown_ns[2] = 500000000ll; c->cooldown_ns[3] = 0;
}

int aria_alert_create(const aria_alert_config* c, aria_alert_t* out) {
    if (!out || alert_bad_config(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 2, "aria_alert_create", [](aria_alert_s* h) {
        const aria_alert_config& c = h->cfg;
        AlertParams& P = h->P;
        P.width = c.width; P.height = c.height; P.zone_top = c.zone_top; P.zone_bottom = c.zone_bottom;
        int b[2];
        (void)aria_alert_zone_bounds(c.width, b);
        P.bound0 = b[0]; P.bound1 = b[1];
        P.max_dets = c.max_dets; P.min_valid = c.min_valid; P.min_depth = c.min_depth; P.max_depth = c.max_depth;
        P.zone_num = c.zone_pct_num; P.zone_den = c.zone_pct_den; P.det_num = c.det_pct_num; P.det_den = c.det_pct_den;
        P.zone_alert_m = c.zone_alert_m; P.default_depth = c.default_depth; P.crit_m = c.crit_m; P.high_m = c.high_m;
        P.medium_m = c.medium_m; P.beep_m = c.beep_m;
        P.obstacle_dangerous = c.obstacle_dangerous; P.n_dangerous = c.n_dangerous;
        for (int i = 0; i < 32; i++) P.dangerous[i] = c.dangerous[i];
        P.max_events = c.max_events_per_frame;
        for (int i = 0; i < 4; i++) P.cooldown_ns[i] = c.cooldown_ns[i];
        if (const char* s = aria_getenv("ARIA_ALERT_SELECT")) h->plain = !std::strcmp(s, "plain");   // variants build: A/B
        return (int)ARIA_OK;
    });
}

void aria_alert_destroy(aria_alert_t h) { stage_destroy(h); }

void* aria_alert_stream(aria_alert_t h) { return stage_stream(h); }

int aria_alert_check(aria_alert_t h) {
    if (!h) return ARIA_E_INVALID;
    int words[2] = {0, 0};
    const int rc = stage_read_errors(h, words, 2);
    if (rc != ARIA_OK) return rc;
    h->dets_seen = words[1];
    if (words[0] & ERRBIT_ALERT_INPUT) return ARIA_E_INVALID;
    return (words[0] & ERRBIT_ALERT_CAP) ? ARIA_E_OUTPUT_TOO_SMALL : ARIA_OK;
}

int aria_alert_dets_seen(aria_alert_t h) { return h ? h->dets_seen : ARIA_E_INVALID; }

int aria_alert_measure_batch_device(aria_alert_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int n_frames,
                                    const aria_detection* d_dets, const int* d_ndets, int det_cap, aria_alert_meas* d_meas) {
    if (!h || alert_bad_frames(h, depth_stride, depth_pitch, n_frames, d_dets, d_ndets, det_cap) || (n_frames > 0 && (!d_depth || !d_meas)))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const dim3 grid((unsigned)n_frames * ALERT_SOURCES), block(AM_BLOCK);
#ifdef ARIA_VARIANTS
    if (h->plain)
        hipLaunchKernelGGL(k_alert_measure_plain, grid, block, 0, h->stream, h->P, d_depth, (long long)depth_stride, depth_pitch, d_dets, d_ndets,
                           det_cap, d_meas, h->d_err);
    else
#endif
        hipLaunchKernelGGL(k_alert_measure, grid, block, 0, h->stream, h->P, d_depth, (long long)depth_stride, depth_pitch, d_dets, d_ndets,
                           det_cap, d_meas, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_alert_arbitrate_batch_device(aria_alert_t h, const int* d_track_offset, int n_tracks, const int64_t* d_timestamps, int n_frames,
                                      const aria_alert_meas* d_meas, const aria_detection* d_dets, const int* d_ndets, int det_cap,
                                      aria_alert_state* d_states, aria_alert_event* d_events, int event_cap, int* d_nevents) {
    if (!h || alert_bad_frames(h, 0, h->cfg.width, n_frames, d_dets, d_ndets, det_cap) || n_tracks < 0 || n_tracks > ALERT_MAX_FRAMES ||
        event_cap < 0 || (n_tracks > 0 && (!d_track_offset || !d_states || !d_nevents || (event_cap > 0 && !d_events))) ||
        (n_frames > 0 && (!d_timestamps || !d_meas)))
        return ARIA_E_INVALID;
    if (n_tracks == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_alert_arbitrate, dim3((unsigned)n_tracks), dim3(64), 0, h->stream, h->P, d_track_offset,
                       reinterpret_cast<const long long*>(d_timestamps), n_frames, d_meas, d_dets, d_ndets, det_cap, d_states, d_events, event_cap,
                       d_nevents, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_alert_run_batch_device(aria_alert_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int n_frames,
                                const aria_detection* d_dets, const int* d_ndets, int det_cap, const int* d_track_offset, int n_tracks,
                                const int64_t* d_timestamps, aria_alert_state* d_states, aria_alert_event* d_events, int event_cap,
                                int* d_nevents) {
    if (!h || n_frames < 0 || n_frames > ALERT_MAX_FRAMES) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_meas.reserve(h->stream, (size_t)n_frames * ALERT_SOURCES + 1)) != ARIA_OK) return rc;
    if ((rc = aria_alert_measure_batch_device(h, d_depth, depth_stride, depth_pitch, n_frames, d_dets, d_ndets, det_cap, h->d_meas)) != ARIA_OK)
        return rc;
    return aria_alert_arbitrate_batch_device(h, d_track_offset, n_tracks, d_timestamps, n_frames, h->d_meas, d_dets, d_ndets, det_cap, d_states,
                                             d_events, event_cap, d_nevents);
}

}  // extern "C"

namespace {

size_t alert_depth_elems(const aria_alert_s* h, int64_t depth_stride, int depth_pitch, int n_frames) {
    return n_frames == 0 ? 0 : (size_t)(n_frames - 1) * (size_t)depth_stride + (size_t)(h->cfg.height - 1) * (size_t)depth_pitch + (size_t)h->cfg.width;
}

// Uploads of the host forms; each leaves the stream synchronised by the caller's last blocking copy.
int alert_stage_frames(aria_alert_s* h, const float* depth, int64_t depth_stride, int depth_pitch, int n_frames, const aria_detection* dets,
                       const int* ndets, int det_cap) {
    int rc;
    if (depth) {
        const size_t n = alert_depth_elems(h, depth_stride, depth_pitch, n_frames);
        if ((rc = h->d_depth.reserve(h->stream, n + 1)) != ARIA_OK) return rc;
        if (n) ARIA_HIP(hipMemcpyAsync(h->d_depth, depth, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    if (dets) {
        const size_t n = (size_t)n_frames * (size_t)det_cap;
        if ((rc = h->d_dets.reserve(h->stream, n + 1)) != ARIA_OK) return rc;
        if (n) ARIA_HIP(hipMemcpyAsync(h->d_dets, dets, n * sizeof(aria_detection), hipMemcpyHostToDevice, h->stream));
    }
    return ARIA_OK;
}

// d_ints: [0, n_frames) ndets, then n_tracks + 1 offsets, then n_tracks event counts
int alert_stage_ints(aria_alert_s* h, const int* ndets, int n_frames, const int* track_offset, int n_tracks) {
    int rc;
    if ((rc = h->d_ints.reserve(h->stream, (size_t)n_frames + 2 * (size_t)n_tracks + 2)) != ARIA_OK) return rc;
    if (ndets && n_frames) ARIA_HIP(hipMemcpyAsync(h->d_ints, ndets, sizeof(int) * (size_t)n_frames, hipMemcpyHostToDevice, h->stream));
    if (track_offset)
        ARIA_HIP(hipMemcpyAsync(h->d_ints.p + n_frames, track_offset, sizeof(int) * ((size_t)n_tracks + 1), hipMemcpyHostToDevice, h->stream));
    return ARIA_OK;
}

int alert_stage_tracks(aria_alert_s* h, const int64_t* timestamps, int n_frames, const aria_alert_state* states, int n_tracks,
                       const aria_alert_event* events, int event_cap) {
    int rc;
    const size_t n_events = (size_t)n_tracks * (size_t)event_cap;
    if ((rc = h->d_ts.reserve(h->stream, (size_t)n_frames + 1)) != ARIA_OK) return rc;
    if ((rc = h->d_states.reserve(h->stream, (size_t)n_tracks + 1)) != ARIA_OK) return rc;
    if ((rc = h->d_events.reserve(h->stream, n_events + 1)) != ARIA_OK) return rc;
    if (n_frames) ARIA_HIP(hipMemcpyAsync(h->d_ts, timestamps, sizeof(int64_t) * (size_t)n_frames, hipMemcpyHostToDevice, h->stream));
    if (n_tracks) ARIA_HIP(hipMemcpyAsync(h->d_states, states, sizeof(aria_alert_state) * (size_t)n_tracks, hipMemcpyHostToDevice, h->stream));
    if (n_events) ARIA_HIP(hipMemcpyAsync(h->d_events, events, sizeof(aria_alert_event) * n_events, hipMemcpyHostToDevice, h->stream));   // what is not written keeps its bytes
    return ARIA_OK;
}

int alert_fetch_tracks(aria_alert_s* h, int n_frames, aria_alert_state* states, int n_tracks, aria_alert_event* events, int event_cap, int* nevents) {
    const size_t n_events = (size_t)n_tracks * (size_t)event_cap;
    if (n_tracks) {
        ARIA_HIP(hipMemcpyAsync(states, h->d_states, sizeof(aria_alert_state) * (size_t)n_tracks, hipMemcpyDeviceToHost, h->stream));
        ARIA_HIP(hipMemcpyAsync(nevents, h->d_ints.p + n_frames + n_tracks + 1, sizeof(int) * (size_t)n_tracks, hipMemcpyDeviceToHost, h->stream));
    }
    if (n_events) ARIA_HIP(hipMemcpyAsync(events, h->d_events, sizeof(aria_alert_event) * n_events, hipMemcpyDeviceToHost, h->stream));
    return ARIA_OK;
}

bool alert_bad_host_tracks(const int* track_offset, int n_tracks, const int64_t* timestamps, int n_frames, const aria_alert_state* states,
                           const aria_alert_event* events, int event_cap, const int* nevents) {
    if (n_tracks < 0 || n_tracks > ALERT_MAX_FRAMES || event_cap < 0) return true;
    if (n_tracks > 0 && (!track_offset || !states || !nevents || (event_cap > 0 && !events))) return true;
    return n_frames > 0 && !timestamps;
}

}  // namespace

extern "C" {

int aria_alert_measure(aria_alert_t h, const float* depth, int64_t depth_stride, int depth_pitch, int n_frames, const aria_detection* dets,
                       const int* ndets, int det_cap, aria_alert_meas* meas) {
    if (!h || alert_bad_frames(h, depth_stride, depth_pitch, n_frames, dets, ndets, det_cap) || (n_frames > 0 && (!depth || !meas)))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    const size_t n_meas = (size_t)n_frames * ALERT_SOURCES;
    if ((rc = h->d_meas.reserve(h->stream, n_meas + 1)) != ARIA_OK) return rc;
    if ((rc = alert_stage_frames(h, depth, depth_stride, depth_pitch, n_frames, dets, ndets, det_cap)) != ARIA_OK) return rc;
    if ((rc = alert_stage_ints(h, ndets, n_frames, nullptr, 0)) != ARIA_OK) return rc;
    ARIA_HIP(hipStreamSynchronize(h->stream));                           // the host arrays are free again
    if ((rc = aria_alert_measure_batch_device(h, h->d_depth, depth_stride, depth_pitch, n_frames, dets ? (const aria_detection*)h->d_dets : nullptr,
                                              ndets ? (const int*)h->d_ints : nullptr, det_cap, h->d_meas)) != ARIA_OK)
        return rc;
    ARIA_HIP(hipMemcpyAsync(meas, h->d_meas, sizeof(aria_alert_meas) * n_meas, hipMemcpyDeviceToHost, h->stream));
    return aria_alert_check(h);
}

int aria_alert_arbitrate(aria_alert_t h, const int* track_offset, int n_tracks, const int64_t* timestamps, int n_frames,
                         const aria_alert_meas* meas, const aria_detection* dets, const int* ndets, int det_cap, aria_alert_state* states,
                         aria_alert_event* events, int event_cap, int* nevents) {
    if (!h || alert_bad_frames(h, 0, h->cfg.width, n_frames, dets, ndets, det_cap) || (n_frames > 0 && !meas) ||
        alert_bad_host_tracks(track_offset, n_tracks, timestamps, n_frames, states, events, event_cap, nevents))
        return ARIA_E_INVALID;
    if (n_tracks == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    const size_t n_meas = (size_t)n_frames * ALERT_SOURCES;
    if ((rc = h->d_meas.reserve(h->stream, n_meas + 1)) != ARIA_OK) return rc;
    if ((rc = alert_stage_frames(h, nullptr, 0, 0, n_frames, dets, ndets, det_cap)) != ARIA_OK) return rc;
    if ((rc = alert_stage_ints(h, ndets, n_frames, track_offset, n_tracks)) != ARIA_OK) return rc;
    if ((rc = alert_stage_tracks(h, timestamps, n_frames, states, n_tracks, events, event_cap)) != ARIA_OK) return rc;
    if (n_meas) ARIA_HIP(hipMemcpyAsync(h->d_meas, meas, sizeof(aria_alert_meas) * n_meas, hipMemcpyHostToDevice, h->stream));
    ARIA_HIP(hipStreamSynchronize(h->stream));
    if ((rc = aria_alert_arbitrate_batch_device(h, h->d_ints.p + n_frames, n_tracks, reinterpret_cast<const int64_t*>(h->d_ts.p), n_frames, h->d_meas,
                                                dets ? (const aria_detection*)h->d_dets : nullptr, ndets ? (const int*)h->d_ints : nullptr, det_cap,
                                                h->d_states, h->d_events, event_cap, h->d_ints.p + n_frames + n_tracks + 1)) != ARIA_OK)
        return rc;
    if ((rc = alert_fetch_tracks(h, n_frames, states, n_tracks, events, event_cap, nevents)) != ARIA_OK) return rc;
    return aria_alert_check(h);
}

int aria_alert_run(aria_alert_t h, const float* depth, int64_t depth_stride, int depth_pitch, int n_frames, const aria_detection* dets,
                   const int* ndets, int det_cap, const int* track_offset, int n_tracks, const int64_t* timestamps, aria_alert_state* states,
                   aria_alert_event* events, int event_cap, int* nevents) {
    if (!h || alert_bad_frames(h, depth_stride, depth_pitch, n_frames, dets, ndets, det_cap) || (n_frames > 0 && !depth) ||
        alert_bad_host_tracks(track_offset, n_tracks, timestamps, n_frames, states, events, event_cap, nevents))
        return ARIA_E_INVALID;
    if (n_tracks == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = alert_stage_frames(h, n_frames ? depth : nullptr, depth_stride, depth_pitch, n_frames, dets, ndets, det_cap)) != ARIA_OK) return rc;
    if ((rc = alert_stage_ints(h, ndets, n_frames, track_offset, n_tracks)) != ARIA_OK) return rc;
    if ((rc = alert_stage_tracks(h, timestamps, n_frames, states, n_tracks, events, event_cap)) != ARIA_OK) return rc;
    ARIA_HIP(hipStreamSynchronize(h->stream));
    if ((rc = aria_alert_run_batch_device(h, h->d_depth, depth_stride, depth_pitch, n_frames, dets ? (const aria_detection*)h->d_dets : nullptr,
                                          ndets ? (const int*)h->d_ints : nullptr, det_cap, h->d_ints.p + n_frames, n_tracks,
                                          reinterpret_cast<const int64_t*>(h->d_ts.p), h->d_states, h->d_events, event_cap,
                                          h->d_ints.p + n_frames + n_tracks + 1)) != ARIA_OK)
        return rc;
    if ((rc = alert_fetch_tracks(h, n_frames, states, n_tracks, events, event_cap, nevents)) != ARIA_OK) return rc;
    return aria_alert_check(h);
}

}  // extern "C"
