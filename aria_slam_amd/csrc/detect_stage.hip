// Object-detector stage around the network (include/aria_orb_hip.h, "object detector"): TRTInference::preprocess
// (reference src/legacy/TRTInference.cpp:68-93) and TRTInference::postprocess (:95-142, with cv::dnn::NMSBoxes) as two
// kernels, batched over frames. aria_slam_amd/detect_ref.py restates both in NumPy and is the definition: integer arithmetic,
// single correctly rounded fp32 / fp64 operations and copies, so the comparison is bitwise.
//
// k_det_preprocess   one lane per four adjacent output pixels of one row: 2 x 2 source bytes per pixel and channel through the
//                    per-column / per-row tables (built on the host in fp32 exactly as the restatement builds them), the
//                    fixed-point bilinear value, one fp32 multiply, and ONE 16-byte store per plane (8 bytes for fp16). A lane
//                    whose four pixels are not 16-byte aligned (rows of an input width that is no multiple of 4) or that holds
//                    the 1..3 pixels of a row's tail stores scalars. Gray input computes the pixel once and stores it thrice.
//                    Memory-bound: W * H * C bytes in, 3 * in_w * in_h * 4 out per frame; the stores are 6.5x the loads at
//                    752 x 480 gray -> 640 x 640.
// k_det_postprocess  one workgroup per frame, candidates in LDS: threshold + scale + cast, rank sort by (score desc, index
//                    asc), then NMSBoxes' greedy rule walked serially over the sorted order with a wave-uniform loop -- for
//                    every box that is still alive when its turn comes, all lanes test the boxes after it in parallel (fp64
//                    division) and mark the ones it suppresses. A suppressed box is skipped when its turn comes, so it
//                    suppresses nothing. No float atomics; the rows depend on the frame's own candidates only.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "stage_handle.h"

using namespace aria;

namespace {

constexpr int DET_BLOCK = 256;
constexpr int DET_MAX_DIM = 16384;           // image and network-input sides; keeps every table entry in 16 bits
constexpr int DET_COEF_ONE = 2048;           // INTER_RESIZE_COEF_SCALE
constexpr int ERRBIT_DET_CAP = 1;            // d_err[0]; d_err[1] / d_err[2] = largest det / box rows any frame needed

struct DetClasses {
    int n;                                   // < 0: every class
    int ids[ARIA_DET_MAX_CLASS_IDS];
};

// ---- preprocess -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void det_store4(float* p, const float* v, int n) {
    if (n == 4 && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) p[k] = v[k];
    }
}

__device__ __forceinline__ void det_store4(__half* p, const float* v, int n) {
    __half h[4];
#pragma unroll
    for (int k = 0; k < 4; k++) h[k] = __float2half_rn(v[k]);
    if (n == 4 && ((uintptr_t)p & 7) == 0) {
        uint2 w;
        w.x = (uint32_t)__half_as_ushort(h[0]) | ((uint32_t)__half_as_ushort(h[1]) << 16);
        w.y = (uint32_t)__half_as_ushort(h[2]) | ((uint32_t)__half_as_ushort(h[3]) << 16);
        *reinterpret_cast<uint2*>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n) p[k] = h[k];
    }
}

template <typename OutT, int C>
__global__ __launch_bounds__(DET_BLOCK) void k_det_preprocess(const uint8_t* __restrict__ img, int W, int H, int row_stride,
                                                              int64_t frame_stride, int swap_rb, const uint32_t* __restrict__ xtab,
                                                              const uint32_t* __restrict__ ytab, int in_w, int in_h,
                                                              OutT* __restrict__ out) {
    const int qpr = (in_w + 3) >> 2;                       // lanes per output row
    const int q = blockIdx.x * DET_BLOCK + threadIdx.x;
    if (q >= qpr * in_h) return;
    const int dy = q / qpr, dx0 = (q - dy * qpr) * 4;
    const int n = min(4, in_w - dx0);
    const uint32_t ey = ytab[dy];
    const int y0 = (int)(ey & 0xffffu), b1 = (int)(ey >> 16), b0 = DET_COEF_ONE - b1;
    const int y1 = min(y0 + 1, H - 1);
    const uint8_t* f0 = img + (int64_t)blockIdx.y * frame_stride;
    const uint8_t* r0 = f0 + (int64_t)y0 * row_stride;
    const uint8_t* r1 = f0 + (int64_t)y1 * row_stride;
    const float k255 = (float)(1.0 / 255.0);
    float v[C][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t ex = xtab[dx0 + min(k, n - 1)];       // (a tail lane repeats its last pixel; never stored)
        const int x0 = (int)(ex & 0xffffu), a1 = (int)(ex >> 16), a0 = DET_COEF_ONE - a1;
        const int x1 = min(x0 + 1, W - 1);
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int S0 = (int)r0[x0 * C + c] * a0 + (int)r0[x1 * C + c] * a1;
            const int S1 = (int)r1[x0 * C + c] * a0 + (int)r1[x1 * C + c] * a1;
            const int val = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
            v[c][k] = (float)val * k255;
        }
    }
    const int64_t plane = (int64_t)in_w * in_h;
    OutT* base = out + (int64_t)blockIdx.y * 3 * plane + (int64_t)dy * in_w + dx0;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        if (C == 1) {
            det_store4(base + p * plane, v[0], n);
        } else {
            // (selected by value, not by a runtime index into v: keeps v in registers)
            const int c = swap_rb ? 2 - p : p;
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; k++) t[k] = c == 0 ? v[0][k] : c == 1 ? v[1 % C][k] : v[2 % C][k];
            det_store4(base + p * plane, t, n);
        }
    }
}

// ---- postprocess ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int det_class_id(float v) {       // (int)raw[5]; saturating, 0 for a NaN
    if (v != v) return 0;
    if (v >= 2147483648.f) return INT_MAX;
    if (v <= -2147483648.f) return INT_MIN;
    return (int)v;
}

// threshold (TRTInference.cpp:116 and NMSBoxes' strict one), scale and cast (:118-121) of one candidate row
__device__ __forceinline__ bool det_decode(const float* __restrict__ r, float sx, float sy, float conf, int* b) {
    const float sc = r[4];
    if (!(sc >= conf && sc > conf)) return false;
    const float s[4] = {sx, sy, sx, sy};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float x = r[k];
        const float p = x * s[k];
        ok = ok && (fabsf(x) <= FLT_MAX) && (fabsf(p) <= 1048576.f);     // finite, and the product inside +-2^20
        b[k] = ok ? (int)p : 0;
    }
    return ok;
}

// 1.f - (float)jaccardDistance(a, b) on integer rectangles, areas exact
__device__ __forceinline__ float det_overlap(int ax1, int ay1, int ax2, int ay2, long long Aa, int bx1, int by1, int bx2, int by2,
                                             long long Ab) {
    const double dAa = (double)Aa, dAb = (double)Ab;
    double jd;
    if (dAa + dAb <= DBL_EPSILON) {
        jd = 0.0;
    } else {
        const long long iw = (long long)min(ax2, bx2) - max(ax1, bx1), ih = (long long)min(ay2, by2) - max(ay1, by1);
        const double Aab = (iw <= 0 || ih <= 0) ? 0.0 : (double)(iw * ih);
        jd = 1.0 - Aab / (dAa + dAb - Aab);
    }
    return 1.f - (float)jd;
}

__global__ __launch_bounds__(DET_BLOCK) void k_det_postprocess(const float* __restrict__ raw, int n_cand, float sx, float sy, float conf,
                                                               float nms, DetClasses cls, aria_detection* __restrict__ dets,
                                                               int* __restrict__ ndets, int det_cap, aria_box* __restrict__ boxes,
                                                               int* __restrict__ nboxes, int box_cap, int* __restrict__ err) {
    constexpr int N = ARIA_DET_MAX_CANDIDATES;
    __shared__ float s_key[N];            // by candidate: the score, NaN when the candidate takes no part
    __shared__ int s_x1[N], s_y1[N], s_x2[N], s_y2[N], s_cls[N];   // by rank from here on
    __shared__ float s_conf[N];
    __shared__ long long s_area[N];
    __shared__ int s_sdet[N], s_sbox[N];  // output slot, -1 = not written
    __shared__ unsigned char s_supp[N];
    __shared__ int s_m;
    const int tid = threadIdx.x, f = blockIdx.x;
    const float* fr = raw + (int64_t)f * n_cand * 6;
    if (tid == 0) s_m = 0;
    for (int i = tid; i < N; i += DET_BLOCK) {
        int b[4];
        s_key[i] = (i < n_cand && det_decode(fr + (int64_t)i * 6, sx, sy, conf, b)) ? fr[(int64_t)i * 6 + 4] : __int_as_float(0x7fc00000);
        s_supp[i] = 0;
        s_sdet[i] = -1;
        s_sbox[i] = -1;
    }
    __syncthreads();
    // rank sort: (score descending, candidate index ascending) -- std::stable_sort's order
    for (int i = tid; i < n_cand; i += DET_BLOCK) {
        const float si = s_key[i];
        if (si != si) continue;
        int r = 0;
        for (int j = 0; j < n_cand; j++) {
            const float sj = s_key[j];              // (a NaN compares false both times)
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        int b[4];
        det_decode(fr + (int64_t)i * 6, sx, sy, conf, b);
        s_x1[r] = b[0]; s_y1[r] = b[1]; s_x2[r] = b[2]; s_y2[r] = b[3];
        s_area[r] = (long long)(b[2] - b[0]) * (long long)(b[3] - b[1]);
        s_conf[r] = si;
        s_cls[r] = det_class_id(fr[(int64_t)i * 6 + 5]);
        atomicAdd(&s_m, 1);
    }
    __syncthreads();
    const int m = s_m;
    // NMSBoxes' greedy pass. i, s_supp[i] and the counters are the same in every lane (wave- and block-uniform): the flag of
    // box i is final when its turn comes, because every box kept before it has finished marking behind a barrier.
    int nk = 0, nb = 0;
    for (int i = 0; i < m; i++) {
        if (s_supp[i]) continue;
        const int ax1 = s_x1[i], ay1 = s_y1[i], ax2 = s_x2[i], ay2 = s_y2[i], c = s_cls[i];
        const long long Aa = s_area[i];
        bool dyn = cls.n < 0;
        for (int k = 0; k < cls.n; k++) dyn = dyn || cls.ids[k] == c;
        if (tid == 0) {
            s_sdet[i] = nk;
            s_sbox[i] = dyn ? nb : -1;
        }
        nk++;
        nb += dyn ? 1 : 0;
        for (int j = i + 1 + tid; j < m; j += DET_BLOCK) {
            if (s_supp[j]) continue;
            const float ov = det_overlap(ax1, ay1, ax2, ay2, Aa, s_x1[j], s_y1[j], s_x2[j], s_y2[j], s_area[j]);
            if (!(ov <= nms)) s_supp[j] = 1;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int p = tid; p < m; p += DET_BLOCK) {
        const int sd = s_sdet[p], sb = s_sbox[p];
        const float x1 = (float)s_x1[p], y1 = (float)s_y1[p], x2 = (float)s_x2[p], y2 = (float)s_y2[p];
        if (sd >= 0 && sd < det_cap) {
            aria_detection d;
            d.x1 = x1; d.y1 = y1; d.x2 = x2; d.y2 = y2; d.confidence = s_conf[p]; d.class_id = s_cls[p];
            dets[(int64_t)f * det_cap + sd] = d;
        }
        if (boxes && sb >= 0 && sb < box_cap) {
            aria_box b;
            b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2;
            boxes[(int64_t)f * box_cap + sb] = b;
        }
    }
    if (tid == 0) {
        ndets[f] = min(nk, det_cap);
        if (nk > det_cap) {
            atomicOr(err, ERRBIT_DET_CAP);
            atomicMax(err + 1, nk);
        }
        if (boxes) {
            nboxes[f] = min(nb, box_cap);
            if (nb > box_cap) {
                atomicOr(err, ERRBIT_DET_CAP);
                atomicMax(err + 2, nb);
            }
        }
    }
}

// Per-axis table of the resize, in fp32 exactly as detect_ref.resize_table: first tap | weight of the second tap << 16
void det_build_table(int src, int dst, uint32_t* out) {
    const float scale = (float)src / (float)dst;
    for (int d = 0; d < dst; d++) {
        const float t = ((float)d + 0.5f) * scale;
        float f = t - 0.5f;
        const float fl = std::floor(f);
        int s = (int)fl;
        f = f - fl;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        const int a1 = (int)std::nearbyint(f * (float)DET_COEF_ONE);      // cvRound: half to even (default rounding mode)
        out[d] = (uint32_t)s | ((uint32_t)a1 << 16);
    }
}

}  // namespace

// ---- C-ABI ------------------------------------------------------------------------------------------------------------------
struct aria_det_s : StageHandle {          // d_err: [0] bits, [1] det rows needed, [2] box rows needed
    aria_det_config cfg{};
    DeviceBuffer<uint32_t> d_tab;          // x table at 0, y table at DET_MAX_DIM
    std::vector<uint32_t> h_tab;           // host copy (kept while the upload may be in flight)
    int tab_key[4] = {0, 0, 0, 0};         // W, H, in_w, in_h of the tables on the device
    // the handle's own buffers (aria_det_device_buffers, host forms), allocated on first use
    DeviceBuffer<uint8_t> d_input;         // bytes: floats or halves, cfg.out_half
    DeviceBuffer<float> d_raw;
    DeviceBuffer<aria_detection> d_dets;
    DeviceBuffer<aria_box> d_boxes;
    DeviceBuffer<int> d_counts;            // ndets at 0, nboxes at max_batch
    DeviceBuffer<uint8_t> d_img;           // staging of aria_det_preprocess
};

namespace {

size_t det_elem(const aria_det_s* h) { return h->cfg.out_half ? 2 : 4; }

int det_ensure_buffers(aria_det_t h) {
    const size_t B = (size_t)h->cfg.max_batch, NC = (size_t)h->cfg.max_candidates;
    int rc;
    if ((rc = h->d_input.reserve(h->stream, B * 3 * (size_t)h->cfg.input_w * h->cfg.input_h * det_elem(h))) != ARIA_OK) return rc;
    if ((rc = h->d_raw.reserve(h->stream, B * NC * 6)) != ARIA_OK) return rc;
    if ((rc = h->d_dets.reserve(h->stream, B * NC)) != ARIA_OK) return rc;
    if ((rc = h->d_boxes.reserve(h->stream, B * NC)) != ARIA_OK) return rc;
    return h->d_counts.reserve(h->stream, 2 * B);
}

int det_tables(aria_det_t h, int W, int H) {
    const int key[4] = {W, H, h->cfg.input_w, h->cfg.input_h};
    if (!std::memcmp(key, h->tab_key, sizeof(key))) return ARIA_OK;
    ARIA_HIP(hipStreamSynchronize(h->stream));           // launches that still read the old tables
    h->h_tab.assign(2 * DET_MAX_DIM, 0);
    det_build_table(W, h->cfg.input_w, h->h_tab.data());
    det_build_table(H, h->cfg.input_h, h->h_tab.data() + DET_MAX_DIM);
    ARIA_HIP(memcpy_on(h->stream, h->d_tab, h->h_tab.data(), 2 * DET_MAX_DIM * sizeof(uint32_t), hipMemcpyHostToDevice));
    std::memcpy(h->tab_key, key, sizeof(key));
    return ARIA_OK;
}

template <typename OutT>
void det_launch_pre(aria_det_t h, const uint8_t* d_images, int n_frames, int W, int H, int row_stride, int64_t frame_stride,
                    int channels, int swap_rb, void* d_input) {
    const int in_w = h->cfg.input_w, in_h = h->cfg.input_h;
    const int lanes = ((in_w + 3) / 4) * in_h;
    const dim3 grid((lanes + DET_BLOCK - 1) / DET_BLOCK, n_frames);
    if (channels == 1)
        hipLaunchKernelGGL((k_det_preprocess<OutT, 1>), grid, dim3(DET_BLOCK), 0, h->stream, d_images, W, H, row_stride, frame_stride,
                           swap_rb, h->d_tab, h->d_tab + DET_MAX_DIM, in_w, in_h, (OutT*)d_input);
    else
        hipLaunchKernelGGL((k_det_preprocess<OutT, 3>), grid, dim3(DET_BLOCK), 0, h->stream, d_images, W, H, row_stride, frame_stride,
                           swap_rb, h->d_tab, h->d_tab + DET_MAX_DIM, in_w, in_h, (OutT*)d_input);
}

bool det_config_ok(const aria_det_config* c) {
    return c->input_w >= 1 && c->input_h >= 1 && c->input_w <= DET_MAX_DIM && c->input_h <= DET_MAX_DIM && c->max_batch >= 1 &&
           c->max_batch <= 65535 && c->max_candidates >= 1 && c->max_candidates <= ARIA_DET_MAX_CANDIDATES &&
           (c->out_half == 0 || c->out_half == 1);
}

}  // namespace

extern "C" {

void aria_det_default_config(aria_det_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int)sizeof(aria_det_config);
    c->device = 0;
    c->stream = nullptr;
    c->input_w = 640;                    // TRTInference.cpp:38-40: the engine's NCHW input
    c->input_h = 640;
    c->max_batch = 1;
    c->max_candidates = 300;             // TRTInference.cpp:105
    c->out_half = 0;
}

int aria_det_create(const aria_det_config* c, aria_det_t* out) {
    if (!c || !out || c->struct_size != (int)sizeof(aria_det_config)) return ARIA_E_INVALID;
    *out = nullptr;
    if (!det_config_ok(c)) return ARIA_E_INVALID;
    return stage_create(c, out, 4, "aria_det_create",
                        [](aria_det_s* h) { return h->d_tab.reserve(h->stream, 2 * DET_MAX_DIM, "aria_det_create"); });
}

void aria_det_destroy(aria_det_t h) { stage_destroy(h); }

void* aria_det_stream(aria_det_t h) { return stage_stream(h); }

int aria_det_check(aria_det_t h, int* det_rows_needed, int* box_rows_needed) {
    if (!h) return ARIA_E_INVALID;
    if (det_rows_needed) *det_rows_needed = 0;
    if (box_rows_needed) *box_rows_needed = 0;
    int w[3] = {0, 0, 0};
    const int rc = stage_read_errors(h, w, 3);
    if (rc != ARIA_OK) return rc;
    if (!w[0]) return ARIA_OK;
    if (det_rows_needed) *det_rows_needed = w[1];
    if (box_rows_needed) *box_rows_needed = w[2];
    return ARIA_E_OUTPUT_TOO_SMALL;
}

int aria_det_device_buffers(aria_det_t h, void** d_input, float** d_raw, aria_detection** d_dets, int** d_ndets, aria_box** d_boxes,
                            int** d_nboxes) {
    if (!h) return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    const int rc = det_ensure_buffers(h);
    if (rc != ARIA_OK) return rc;
    if (d_input) *d_input = h->d_input;
    if (d_raw) *d_raw = h->d_raw;
    if (d_dets) *d_dets = h->d_dets;
    if (d_ndets) *d_ndets = h->d_counts;
    if (d_boxes) *d_boxes = h->d_boxes;
    if (d_nboxes) *d_nboxes = h->d_counts + h->cfg.max_batch;
    return ARIA_OK;
}

int aria_det_preprocess_batch_device(aria_det_t h, const uint8_t* d_images, int n_frames, int width, int height, int row_stride,
                                     int64_t frame_stride, int channels, int swap_rb, void* d_input) {
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch || (channels != 1 && channels != 3) || width < 1 || height < 1 ||
        width > DET_MAX_DIM || height > DET_MAX_DIM || (int64_t)row_stride < (int64_t)width * channels ||
        (n_frames > 1 && frame_stride < (int64_t)(height - 1) * row_stride + (int64_t)width * channels) ||
        (n_frames && (!d_images || !d_input)))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    ARIA_HIP(hipSetDevice(h->device));
    const int rc = det_tables(h, width, height);
    if (rc != ARIA_OK) return rc;
    if (h->cfg.out_half) det_launch_pre<__half>(h, d_images, n_frames, width, height, row_stride, frame_stride, channels, swap_rb, d_input);
    else det_launch_pre<float>(h, d_images, n_frames, width, height, row_stride, frame_stride, channels, swap_rb, d_input);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_det_postprocess_batch_device(aria_det_t h, const float* d_raw, int n_frames, int n_candidates, int src_width, int src_height,
                                      float conf, float nms, const int* class_ids, int n_class_ids, aria_detection* d_dets,
                                      int* d_ndets, int det_cap, aria_box* d_boxes, int* d_nboxes, int box_cap) {
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch || n_candidates < 0 || n_candidates > h->cfg.max_candidates ||
        src_width < 1 || src_height < 1 || det_cap < 0 || (det_cap && !d_dets) || !d_ndets || (n_frames && n_candidates && !d_raw) ||
        (d_boxes && (!d_nboxes || box_cap < 0)) || n_class_ids > ARIA_DET_MAX_CLASS_IDS || (class_ids == nullptr && n_class_ids > 0))
        return ARIA_E_INVALID;
    if (n_frames == 0) return ARIA_OK;
    DetClasses cls{};
    if (n_class_ids < 0) {
        cls.n = -1;
    } else if (!class_ids) {
        static const int kDynamic[10] = {0, 1, 2, 3, 5, 6, 7, 14, 15, 16};      // src/main.cpp:29-40
        cls.n = 10;
        std::memcpy(cls.ids, kDynamic, sizeof(kDynamic));
    } else {
        cls.n = n_class_ids;
        std::memcpy(cls.ids, class_ids, (size_t)n_class_ids * sizeof(int));
    }
    ARIA_HIP(hipSetDevice(h->device));
    const float sx = (float)src_width / (float)h->cfg.input_w, sy = (float)src_height / (float)h->cfg.input_h;   // :164-165
    hipLaunchKernelGGL(k_det_postprocess, dim3(n_frames), dim3(DET_BLOCK), 0, h->stream, d_raw, n_candidates, sx, sy, conf, nms, cls,
                       d_dets, d_ndets, det_cap, d_boxes, d_nboxes, box_cap, h->d_err);
    ARIA_HIP(hipGetLastError());
    return ARIA_OK;
}

int aria_det_preprocess(aria_det_t h, const uint8_t* image, int width, int height, int row_stride, int channels, int swap_rb,
                        void* input) {
    if (!h || !image || !input || width < 1 || height < 1 || width > DET_MAX_DIM || height > DET_MAX_DIM ||
        (channels != 1 && channels != 3) || (int64_t)row_stride < (int64_t)width * channels)
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = det_ensure_buffers(h);
    if (rc != ARIA_OK) return rc;
    const size_t bytes = (size_t)row_stride * height;
    if ((rc = h->d_img.reserve(h->stream, bytes)) != ARIA_OK) return rc;
    // (the last row may be shorter than row_stride in the caller's buffer)
    const size_t used = (size_t)row_stride * (height - 1) + (size_t)width * channels;
    ARIA_HIP(memcpy_on(h->stream, h->d_img, image, used, hipMemcpyHostToDevice));
    rc = aria_det_preprocess_batch_device(h, h->d_img, 1, width, height, row_stride, (int64_t)bytes, channels, swap_rb,
                                          h->d_input);
    if (rc != ARIA_OK) return rc;
    ARIA_HIP(memcpy_on(h->stream, input, h->d_input, 3 * (size_t)h->cfg.input_w * h->cfg.input_h * det_elem(h), hipMemcpyDeviceToHost));
    return ARIA_OK;
}

int aria_det_postprocess(aria_det_t h, const float* raw, int n_candidates, int src_width, int src_height, float conf, float nms,
                         const int* class_ids, int n_class_ids, aria_detection* dets, int det_cap, int* n_dets, aria_box* boxes,
                         int box_cap, int* n_boxes) {
    if (!h || n_candidates < 0 || n_candidates > h->cfg.max_candidates || (n_candidates && !raw) || !n_dets || det_cap < 0 ||
        (det_cap && !dets) || (boxes && (!n_boxes || box_cap < 0)))
        return ARIA_E_INVALID;
    ARIA_HIP(hipSetDevice(h->device));
    int rc = det_ensure_buffers(h);
    if (rc != ARIA_OK) return rc;
    const int NC = h->cfg.max_candidates;
    int* d_nd = h->d_counts;
    int* d_nb = h->d_counts + h->cfg.max_batch;
    if (n_candidates)
        ARIA_HIP(memcpy_on(h->stream, h->d_raw, raw, (size_t)n_candidates * 6 * sizeof(float), hipMemcpyHostToDevice));
    rc = aria_det_postprocess_batch_device(h, h->d_raw, 1, n_candidates, src_width, src_height, conf, nms, class_ids, n_class_ids,
                                           h->d_dets, d_nd, NC, h->d_boxes, d_nb, NC);
    if (rc != ARIA_OK) return rc;
    int nd = 0, nb = 0;
    ARIA_HIP(hipMemcpyAsync(&nd, d_nd, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ARIA_HIP(memcpy_on(h->stream, &nb, d_nb, sizeof(int), hipMemcpyDeviceToHost));
    *n_dets = nd;
    if (n_boxes) *n_boxes = nb;
    const int wd = std::min(nd, det_cap), wb = boxes ? std::min(nb, box_cap) : 0;
    if (wd) ARIA_HIP(memcpy_on(h->stream, dets, h->d_dets, (size_t)wd * sizeof(aria_detection), hipMemcpyDeviceToHost));
    if (wb) ARIA_HIP(memcpy_on(h->stream, boxes, h->d_boxes, (size_t)wb * sizeof(aria_box), hipMemcpyDeviceToHost));
    return (nd > det_cap || (boxes && nb > box_cap)) ? ARIA_E_OUTPUT_TOO_SMALL : ARIA_OK;
}

int aria_det_resize_table(int src, int dst, uint32_t* out, int cap) {
    if (!out || src < 1 || dst < 1 || src > DET_MAX_DIM || dst > DET_MAX_DIM || cap < dst) return ARIA_E_INVALID;
    det_build_table(src, dst, out);
    return dst;
}

int64_t aria_det_algorithmic_bytes(int width, int height, int channels, int input_w, int input_h, int out_half) {
    return (int64_t)width * height * channels + 3 * (int64_t)input_w * input_h * (out_half ? 2 : 4);
}

}  // extern "C"
