/*
 * aria_orb_hip.h -- C-ABI of the MI355X-native ORB extractor + brute-force Hamming matcher.
 *
 * This is the drop-in boundary for aria-slam's feature front-end. Each entry point names
 * the reference interface it replaces; paths are relative to the reference tree (robertteleng/aria-slam).
 * Plain pointers and sizes only: no C++ types, no torch types, never throws. All functions return an
 * aria_status (0 = OK, negative = error); aria_status_string() explains a code.
 *
 * Conventions
 *  - Images are 8-bit grayscale, row-major (include/interfaces/IFeatureExtractor.hpp:14).
 *  - aria_keypoint / aria_match are byte-for-byte aria::core::KeyPoint / aria::core::Match
 *    (include/core/Types.hpp:9-15, :97-101); descriptors are N x 32 bytes, row-major (Types.hpp:25,29).
 *  - The ORB configuration is the one the reference hard-codes (src/adapters/gpu/OrbCudaExtractor.cpp:35-45):
 *    scaleFactor 1.2f, 8 levels, edgeThreshold 31, firstLevel 0, WTA_K 2, HARRIS_SCORE, patchSize 31,
 *    fastThreshold 20; only nfeatures is settable, as in the reference (setMaxFeatures, :212-216).
 *  - Results follow CPU cv::ORB::detectAndCompute (src/legacy/Frame.cpp:45-49), not cv::cuda::ORB.
 *    Keypoint order is canonical: level ascending; within a level response (Harris) descending, then y, then
 *    x ascending. A level may return more than its quota when responses tie at the cut (OpenCV keeps ties),
 *    so a frame can yield slightly more than max_features keypoints; size outputs with aria_orb_kp_capacity().
 *  - A handle is single-owner (not thread-safe), like the reference adapters
 *    (include/adapters/gpu/OrbCudaExtractor.hpp:38-50). Independent handles on different devices/streams
 *    may run concurrently. The library never returns memory it owns; callers allocate every output.
 *  - "device" pointers are HIP device pointers on the handle's device; "stream" is a hipStream_t passed as
 *    void* (borrowed; NULL = the handle creates and owns one: OrbCudaExtractor.cpp:24-29,48-52).
 */
#ifndef ARIA_ORB_HIP_H
#define ARIA_ORB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARIA_ORB_HIP_ABI_VERSION 4

typedef enum {
    ARIA_OK = 0,
    ARIA_E_INVALID = -1,          /* bad argument (null pointer, size out of range, bad struct_size)        */
    ARIA_E_NO_DEVICE = -2,        /* no usable HIP device (none present, bad ordinal, driver/runtime not initialised) */
    ARIA_E_OOM = -3,              /* device or host allocation failed                                       */
    ARIA_E_TOO_LARGE = -4,        /* image larger than the handle was created for                           */
    ARIA_E_OUTPUT_TOO_SMALL = -5, /* caller's keypoint/match capacity is smaller than the result            */
    ARIA_E_OVERFLOW = -6,         /* an internal buffer overflowed; results are NOT valid. Either a FAST candidate
                                     list (only possible with cand_cap_scale > 0: raise it or use 0), or the
                                     tie-storm arenas: selection ties beyond the on-chip capacities are handled
                                     in global memory (k_select_ovf), whose arenas hold the worst case of four
                                     whole frames per internal pass -- a batch with more all-tied frames than
                                     that needs a smaller max_batch.                                         */
    ARIA_E_BUSY = -7,             /* extract_async called while another async extract is pending            */
    ARIA_E_NOT_PENDING = -8,      /* sync called with nothing pending (treated as a no-op by the adapter)   */
    ARIA_E_HIP = -9,              /* a HIP runtime call failed (bad pointer, bad stream, ...): aria_last_hip_error() */
    ARIA_E_KERNEL = -10           /* a kernel launch failed or faulted on the device: aria_last_hip_error()  */
} aria_status;

/* == aria::core::KeyPoint (include/core/Types.hpp:9-15), 24 bytes */
typedef struct { float x, y, size, angle, response; int octave; } aria_keypoint;
/* == aria::core::Match (include/core/Types.hpp:97-101), 12 bytes */
typedef struct { int query_idx, train_idx; float distance; } aria_match;

typedef struct aria_orb_s* aria_orb_t;
typedef struct aria_matcher_s* aria_matcher_t;

/* Replaces the constructor arguments of OrbCudaExtractor (OrbCudaExtractor.cpp:21-46) and
 * FactoryConfig{cuda_device, max_features} (include/factory/PipelineFactory.hpp:16-28). */
typedef struct {
    int   struct_size;     /* = sizeof(aria_orb_config)                                                     */
    int   device;          /* HIP device ordinal                                                            */
    void* stream;          /* borrowed hipStream_t, or NULL = the handle creates (and owns) a stream. The legacy
                            * default stream has handle 0 and therefore cannot be borrowed: two handles that must run
                            * in order (extract, then match on its descriptors) need one real stream between them,
                            * or a sync (aria_orb_check) in between.                                            */
    int   max_width;       /* largest image the handle must accept                                          */
    int   max_height;
    int   max_features;    /* nfeatures (OrbCudaExtractor.hpp:12 default 1000)                              */
    int   max_batch;       /* frames processed per internal pass of the batch entry point (>= 1)            */
    int   blur_tie_mode;   /* rounding of exact ties in the 7x7 blur's column filter, which in OpenCV depends on the SIMD
                            * width its dispatcher picks: 1 (default) ties to even for columns x < (w & ~3) and up in the
                            * scalar tail; 2 / 3: the vector body ends at w & ~7 / w & ~15; 0: ties up everywhere       */
    int   cand_cap_scale;  /* 0 (default): FAST candidate lists sized for the worst case, cannot overflow;
                              > 0: cap each level's list at cand_cap_scale * quota entries to save HBM          */
    int   level_size_mode; /* pyramid level size: 0 (default) cvRound(dim * (1.0f / scale)), 1 cvRound(dim / scale) -- the
                              two readings of cv::ORB's sizing; they differ for few sizes (tools/level_size_sweep.py,
                              profiles/level_size_sweep.txt: none of the BASELINE sizes)                            */
} aria_orb_config;

const char* aria_status_string(int status);
int         aria_abi_version(void);
/* Last HIP runtime error text seen by this thread's most recent failing call ("" if none). */
const char* aria_last_hip_error(void);

void aria_orb_default_config(aria_orb_config* cfg);
int  aria_orb_create(const aria_orb_config* cfg, aria_orb_t* out);
void aria_orb_destroy(aria_orb_t h);

/* IFeatureExtractor::setMaxFeatures / getMaxFeatures (include/interfaces/IFeatureExtractor.hpp:38-39,
 * OrbCudaExtractor.cpp:212-216). All other ORB parameters keep the reference's values. */
int aria_orb_set_max_features(aria_orb_t h, int n);
int aria_orb_get_max_features(aria_orb_t h);
/* Rows to allocate per frame for keypoints/descriptors: sum over levels of (quota + 64 rows of tie slack). OpenCV's
 * retainBest keeps EVERY keypoint tying with the last kept one, so a tie storm (checkerboards, synthetic
 * patterns) can return more: the host entry points then report ARIA_E_OUTPUT_TOO_SMALL with *n_out = rows required
 * (retry with that capacity, or call aria_orb_fetch_last), the batch entry point makes aria_orb_check return
 * ARIA_E_OUTPUT_TOO_SMALL and aria_orb_rows_needed() tell the rows its largest frame needs. */
int aria_orb_kp_capacity(aria_orb_t h);
int aria_orb_rows_needed(aria_orb_t h);
/* Copies the result of the last completed aria_orb_extract / aria_orb_sync out again (it stays in the handle until the
 * next extraction): what a caller uses after ARIA_E_OUTPUT_TOO_SMALL instead of extracting again. */
int aria_orb_fetch_last(aria_orb_t h, aria_keypoint* keypoints, uint8_t* descriptors, int cap, int* n_out);

/* IFeatureExtractor::extract (IFeatureExtractor.hpp:18-23; OrbCudaExtractor.cpp:64-128). Host buffers.
 * image is borrowed and never written; stride = bytes between rows (width for the reference's packed Mat,
 * OrbCudaExtractor.cpp:72). Writes up to cap keypoints (24 B each) and cap*32 descriptor bytes; *n_out = count.
 * Returns ARIA_E_OUTPUT_TOO_SMALL (with *n_out = required) if cap is too small. Blocks until done. */
int aria_orb_extract(aria_orb_t h, const uint8_t* image, int width, int height, int stride,
                     aria_keypoint* keypoints, uint8_t* descriptors, int cap, int* n_out);

/* IFeatureExtractor::extractAsync + sync (IFeatureExtractor.hpp:27-35; OrbCudaExtractor.cpp:136-210).
 * One pending operation per handle, as in the reference. The image buffer must stay valid until
 * aria_orb_sync returns (the upload is asynchronous, :158). */
int aria_orb_extract_async(aria_orb_t h, const uint8_t* image, int width, int height, int stride);
int aria_orb_sync(aria_orb_t h, aria_keypoint* keypoints, uint8_t* descriptors, int cap, int* n_out);

/* OrbCudaExtractor::getGpuDescriptors() (include/adapters/gpu/OrbCudaExtractor.hpp:34-35, "get descriptors without
 * download (for GPU matching)"): device pointers to the result of the single-frame entry points, for a matcher on the same
 * device (aria_matcher_match_device*). The block belongs to the handle: the pointers stay the same from call to call
 * (until a tie storm makes the handle grow it, or aria_orb_set_max_features) and the CONTENT is that of the most recent
 * aria_orb_extract / aria_orb_extract_async, complete once that call / aria_orb_sync has returned -- or, for work queued
 * behind it on the handle's stream, as soon as the extraction's kernels have run. *d_count is the device copy of the
 * keypoint count (clamped to *rows = the block's row capacity), *n the host copy (-1 while an async extract is pending,
 * or before the first extraction). Any output pointer may be NULL. */
int aria_orb_last_device(aria_orb_t h, const aria_keypoint** d_keypoints, const uint8_t** d_descriptors, const int** d_count,
                         int* n, int* rows);

/* Device-resident batch form: the role OrbCudaExtractor::getGpuDescriptors() was meant to play
 * (include/adapters/gpu/OrbCudaExtractor.hpp:35) -- results stay in HBM for the matcher.
 *   d_images     : n_frames images, frame f at d_images + f*frame_stride, rows row_stride bytes apart
 *   d_keypoints  : n_frames * kp_cap records (frame f at index f*kp_cap)
 *   d_descriptors: n_frames * kp_cap * 32 bytes
 *   d_counts     : n_frames ints, keypoints found per frame
 * Enqueued on the handle's stream; returns without synchronising. Call aria_orb_check() after a stream
 * sync to learn whether any frame overflowed an internal buffer or kp_cap. */
int aria_orb_extract_batch_device(aria_orb_t h, const uint8_t* d_images, int n_frames, int width, int height,
                                  int64_t frame_stride, int row_stride,
                                  aria_keypoint* d_keypoints, uint8_t* d_descriptors, int* d_counts, int kp_cap);
/* Synchronises the handle's stream and returns ARIA_OK or the first deferred error (overflow flags). */
int aria_orb_check(aria_orb_t h);
void* aria_orb_stream(aria_orb_t h);
/* Diagnostics: FAST+blur workgroups whose survivor queue overflowed (corner-dense image regions) and that therefore
 * took the slower dense-rescoring path -- results are identical either way. Counted when aria_orb_extract /
 * aria_orb_sync / aria_orb_check read the device state; the handle enlarges the queue for later calls by itself. */
long long aria_orb_slow_path_blocks(aria_orb_t h, int reset);

/* Diagnostics: name of the FAST/blur kernel the handle's most recent pass launched ("k_fast_blur_stream" for batches whose
 * plan and source alignment allow the streaming kernel, "k_fast_blur_band" for the single-frame schedule and the rest). */
const char* aria_orb_fast_blur_kernel(aria_orb_t h);

/* Per-stage device timing for bench.py's roofline figure (no reference counterpart): when enabled, HIP events
 * are recorded on the handle's stream around each stage of every internal pass.
 * Stages: 0 pyramid resize (7 launches per pass), 1 FAST+NMS+blur, 2 select (retainBest+Harris), 3 describe
 * (IC angle + rBRIEF). get_profile synchronises the stream; times are summed milliseconds since the last reset.
 * `enable`: 0 off; 1 every stage; any other even value brackets only the stages s whose bit (s + 1) is set (each
 * bracket drains the stream before and after the stage, ~20 us of idle GPU, so a throughput run times only what it
 * reports). The matcher's aria_matcher_set_profiling takes the same encoding over its 2 stages. */
#define ARIA_ORB_STAGES 4
int aria_orb_set_profiling(aria_orb_t h, int enable);
int aria_orb_get_profile(aria_orb_t h, int reset, double* stage_ms /*[4]*/, int64_t* stage_launches /*[4]*/,
                         int64_t* frames);

/* Stream-ordering hook for callers that pipeline other work beside a batch extraction (no reference counterpart):
 * `event` (a hipEvent_t, or NULL to clear) is recorded on the handle's stream right BEFORE stage `stage` (numbering as
 * above) of the last internal pass of every aria_orb_extract_batch_device call. A second stream that waits on it starts
 * when the FAST/blur launches are done -- bench.py lets the matcher of the previous step run beside select + describe
 * rather than beside the FAST/blur kernel. Only stage 2 (select) is accepted so far (ARIA_E_INVALID otherwise). The
 * event stays owned by the caller and must outlive the calls that record it. */
int aria_orb_set_stage_event(aria_orb_t h, int stage, void* event);

/* Introspection for parity tests and benchmarks (no reference counterpart).
 * Host-only geometry (no handle, no GPU needed): size, quota and scale of pyramid level `level` in [0, 8) for
 * a width x height image, as CPU cv::ORB lays it out; and the fixed-point INTER_LINEAR_EXACT coefficient table
 * of level >= 1 along axis 0 (x) or 1 (y): entry d = source offset | (weight_of_next_pixel_in_1/256 << 16).
 * aria_orb_resize_table returns the number of entries written (or a negative status). */
int aria_orb_level_info(int max_features, int width, int height, int level, int* lw, int* lh, int* quota, float* scale);
int aria_orb_resize_table(int width, int height, int level, int axis, uint32_t* out, int cap);
/* Row schedule of the fused pyramid kernel (host-only, for tests): per band of level-0 rows and per level, four ints
 * {first row computed, rows computed, first row owned, rows owned}. Returns the number of ints written. */
int aria_orb_pyramid_bands(int width, int height, int* out, int cap, int* band_rows, int* lds_bytes);
/* Algorithmic bytes of one frame: b_extract = 5P - p0 - p7 + 56N, b_fused = 2P + 56N. */
int aria_orb_algorithmic_bytes(int width, int height, int n_keypoints, int64_t* b_extract, int64_t* b_fused);
/* Copies level `level` (raw or blurred) of frame 0 of the most recent call to host memory (lw*lh bytes, packed). */
int aria_orb_debug_read_level(aria_orb_t h, int level, int blurred, uint8_t* host_out);

/* ---- matcher: replaces CudaMatcher (include/adapters/gpu/CudaMatcher.hpp, src/adapters/gpu/CudaMatcher.cpp) -- */
typedef struct {
    int   struct_size;
    int   device;
    void* stream;      /* borrowed hipStream_t or NULL (CudaMatcher.cpp:9-17,22-26) */
    int   max_query;   /* rows per descriptor set the host entry points must accept */
    int   max_train;
} aria_matcher_config;

void aria_matcher_default_config(aria_matcher_config* cfg);
int  aria_matcher_create(const aria_matcher_config* cfg, aria_matcher_t* out);
void aria_matcher_destroy(aria_matcher_t m);

/* IMatcher::match (include/interfaces/IMatcher.hpp:19-24; CudaMatcher.cpp:28-68). Host buffers.
 * Brute-force Hamming kNN (k = 2) of every query row against every train row (ties: lower train index
 * first, as CPU cv::BFMatcher), then Lowe's test d0 < ratio*d1 in fp32 (CudaMatcher.cpp:60). Matches are
 * written in query order. nq == 0 or nt == 0 -> *n_out = 0 (CudaMatcher.cpp:35-37). nt == 1 -> no matches
 * (knn.size() >= 2 fails, :60). ratio == 0 means "ratio test disabled" as IMatcher.hpp:18 documents:
 * the best match of every query is returned (the reference adapter would return nothing).
 * Frame-to-frame use: the handle keeps the query set of the previous call on the device; when train_desc holds the
 * same bytes (frame i matched against frame i-1) it is not uploaded again. Purely an optimisation -- the result never
 * depends on it -- but it means a handle serves one caller at a time, like every other entry point here. */
int aria_matcher_match(aria_matcher_t m, const uint8_t* query_desc, int nq, const uint8_t* train_desc, int nt,
               float ratio, aria_match* matches, int cap, int* n_out);

/* CudaMatcher::matchGpu (include/adapters/gpu/CudaMatcher.hpp:22-28, "GPU-to-GPU matching, zero-copy when used with
 * OrbCudaExtractor"): the descriptor sets are device pointers (e.g. aria_orb_last_device), the matches come back to the
 * host; same results as aria_matcher_match on the same rows. The handle keeps ONE descriptor set resident between calls
 * (device copy): a NULL d_query or d_train stands for that resident set, whose row count must then equal nq / nt. After
 * the call the resident set is the one passed as a non-NULL pointer (the query when both are given) -- frame i against
 * frame i-1 is match_device(d_cur, n_cur, NULL, n_prev) in SlamPipeline's order (query = current) or
 * match_device(NULL, n_prev, d_cur, n_cur) in the legacy executables' order (query = previous, src/euroc_eval.cpp:168-169).
 * aria_matcher_retain_device makes a set resident without matching (first frame); aria_matcher_resident_rows tells its
 * rows (-1: none). aria_matcher_match (host buffers) also replaces the resident set, by its query. */
int aria_matcher_match_device(aria_matcher_t m, const uint8_t* d_query, int nq, const uint8_t* d_train, int nt, float ratio,
                              aria_match* matches, int cap, int* n_out);
int aria_matcher_retain_device(aria_matcher_t m, const uint8_t* d_desc, int n);
int aria_matcher_resident_rows(aria_matcher_t m);
/* Pipelined form for a caller whose extractor and matcher share one stream (extractAsync ... sync, the shape of
 * SlamPipeline's async variant, docs/milestones/H12_CLEAN_ARCHITECTURE.md:711-716): the match of the NEW set (d_new, row count
 * read on the device from *d_n_new <= n_new_max, e.g. aria_orb_last_device's d_count) against the resident set is queued
 * on the matcher's stream without waiting -- behind the extraction when both handles were given the same stream -- and
 * aria_matcher_finish synchronises, is told the new set's row count (which the caller knows by then) and returns the
 * matches. new_is_query: 1 = query is the new set, 0 = query is the resident set. One pending operation per handle
 * (ARIA_E_BUSY); aria_matcher_finish without one returns ARIA_E_NOT_PENDING. The kernels read the new set where it lies
 * and the copy that keeps it resident is queued BEHIND the result copy (aria_matcher_finish does not wait for it): whatever
 * overwrites d_new next must be queued on the same stream -- true for the extractor handle that shares it. */
int aria_matcher_match_device_async(aria_matcher_t m, const uint8_t* d_new, const int* d_n_new, int n_new_max, int new_is_query,
                                    float ratio);
int aria_matcher_finish(aria_matcher_t m, int n_new, aria_match* matches, int cap, int* n_out);

/* Raw kNN-2 (cv::BFMatcher::knnMatch(k=2) itself), host buffers: idx/dist hold 2 ints per query
 * (nearest, second nearest); idx = -1 / dist = INT_MAX where the train set is too small. */
int aria_matcher_knn2(aria_matcher_t m, const uint8_t* query_desc, int nq, const uint8_t* train_desc, int nt,
                    int* idx, int* dist);

/* Device-resident batch form: the role CudaMatcher::matchGpu was declared for (CudaMatcher.hpp:23-28).
 * Pair p matches query block (d_query + p*desc_stride bytes, d_nq[p] rows) against train block
 * (d_train + p*desc_stride, d_nt[p] rows); writes up to match_cap matches at d_matches + p*match_cap and the
 * count at d_nmatches[p]. Enqueued on the matcher's stream; no synchronisation. */
int aria_matcher_match_batch_device(aria_matcher_t m, const uint8_t* d_query, const int* d_nq,
                            const uint8_t* d_train, const int* d_nt, int n_pairs, int64_t desc_stride,
                            float ratio, aria_match* d_matches, int* d_nmatches, int match_cap);

/* ---- dynamic-object filter: src/main.cpp:42-50 isInDynamicObject + :164-175, the hook
 * SlamPipeline::filterDynamicKeypoints was declared for (include/pipeline/SlamPipeline.hpp:96-99). The detector is out of
 * scope; its boxes are an input (the caller passes the boxes of dynamic classes, main.cpp:29-40). Step 1, between describe
 * and match: flags[f*kp_cap + i] = 1 when keypoint i of frame f lies in one of frame f's boxes (frame f's boxes at
 * d_boxes + f*box_cap, d_nboxes[f] of them). mode 0 = the legacy test, cv::Rect::contains of the keypoint rounded to an
 * integer point (half to even): x1 <= round(x) < x2, y1 <= round(y) < y2; mode 1 = core::Detection::contains
 * (include/core/Types.hpp:109-111): closed float intervals. Step 2: the batched matcher drops every ratio-test survivor
 * with a flagged endpoint and counts them (main.cpp's filtered_count) -- kNN-2 itself still sees every keypoint, as in the
 * reference. flag_stride = flags per frame block (>= desc_stride / 32); pair p's query / train flags at
 * d_qflags / d_tflags + p*flag_stride. */
typedef struct { float x1, y1, x2, y2; } aria_box;
int aria_flag_keypoints_device(void* stream, const aria_keypoint* d_keypoints, const int* d_counts, int n_frames, int kp_cap,
                               const aria_box* d_boxes, const int* d_nboxes, int box_cap, int mode, uint8_t* d_flags);
/* The reference's semantics for pairs of consecutive frames. main.cpp:164-175 tests BOTH endpoints of a match against the
 * detections of the CURRENT frame, so the train side of pair (f + 1, f) -- frame f's keypoints -- must be flagged against
 * frame f + 1's boxes, not its own (which is what the call above gives when one flag array serves as query flags of one pair
 * and train flags of the next). box_frame_offset = +1 produces exactly those train flags into a second array (frames whose
 * f + offset does not exist get no flag); offset 0 is the call above. Batched use with the reference's semantics:
 *   aria_flag_keypoints_device(...,          d_qflags);          // query flags: frame f vs boxes f
 *   aria_flag_keypoints_shifted_device(..., +1, d_tflags);       // train flags: frame f vs boxes f + 1
 *   aria_matcher_match_batch_filtered_device(m, desc + stride, cnt + 1, desc, cnt, B - 1, stride, ratio,
 *                                            d_qflags + kp_cap, d_tflags, kp_cap, ...);   // pair p: query f = p + 1, train f = p */
int aria_flag_keypoints_shifted_device(void* stream, const aria_keypoint* d_keypoints, const int* d_counts, int n_frames, int kp_cap,
                                       const aria_box* d_boxes, const int* d_nboxes, int box_cap, int mode, int box_frame_offset,
                                       uint8_t* d_flags);
int aria_matcher_match_batch_filtered_device(aria_matcher_t m, const uint8_t* d_query, const int* d_nq, const uint8_t* d_train,
                                             const int* d_nt, int n_pairs, int64_t desc_stride, float ratio,
                                             const uint8_t* d_qflags, const uint8_t* d_tflags, int64_t flag_stride,
                                             aria_match* d_matches, int* d_nmatches, int match_cap, int* d_nfiltered);

/* Loop-closure candidate scan, the semantic behind IMatcher::matchMultiple (IMatcher.hpp:27-37) as the
 * legacy code uses it (src/legacy/LoopClosure.cpp:72-114): one query descriptor set against n_kf keyframe
 * blocks resident in HBM (block k at d_db + k*desc_stride bytes, d_kf_counts[k] rows). For every keyframe:
 * kNN-2, ratio test in double (d0 < ratio*d1, LoopClosure.cpp:92), d_good[k] = number of passing queries.
 * Scoring/top-5 (LoopClosure.cpp:98-111) is host logic in the adapter. */
int aria_matcher_match_db_device(aria_matcher_t m, const uint8_t* d_query, int nq, const uint8_t* d_db,
                         const int* d_kf_counts, int n_kf, int64_t desc_stride, double ratio, int* d_good);
/* IMatcher::matchMultiple (include/interfaces/IMatcher.hpp:27-37) in one batch: the query is uploaded once, every
 * candidate's descriptors go to a device staging area back to back, ONE kNN-2 launch covers all candidates, one
 * download. Candidate c's matches are written at matches + c*cap_per_cand, its count at n_out[c]; per candidate the
 * result equals aria_matcher_match(query, candidate c). Host buffers. */
int aria_matcher_match_multi(aria_matcher_t m, const uint8_t* query_desc, int nq, const uint8_t* const* train_descs,
                             const int* nts, int n_cand, float ratio, aria_match* matches, int cap_per_cand, int* n_out);
/* The scan of LoopClosureDetector::findCandidates (src/legacy/LoopClosure.cpp:79-96) over host-resident candidates:
 * good[c] = number of queries whose two nearest neighbours in candidate c pass d0 < ratio*d1 in double. One launch. */
int aria_matcher_count_good_multi(aria_matcher_t m, const uint8_t* query_desc, int nq, const uint8_t* const* train_descs,
                                  const int* nts, int n_cand, double ratio, int* good);

/* ---- HBM-resident keyframe descriptor database: the deque of LoopClosureDetector (src/legacy/LoopClosure.cpp:24-31;
 * docs/milestones/H14_GPU_LOOPCLOSURE_AUDIT.md designs exactly this). Fixed-capacity slots of `rows` descriptors;
 * adding beyond `capacity` drops the oldest keyframe (pop_front, :28-30). Index i below = position in the deque,
 * oldest first. The scan is one kernel launch over the whole database. */
typedef struct aria_kfdb_s* aria_kfdb_t;
int  aria_kfdb_create(int device, void* stream, int capacity, int rows, aria_kfdb_t* out);
void aria_kfdb_destroy(aria_kfdb_t db);
int  aria_kfdb_size(aria_kfdb_t db);
int  aria_kfdb_add(aria_kfdb_t db, long long id, const uint8_t* desc_host, int n);
int  aria_kfdb_add_device(aria_kfdb_t db, long long id, const uint8_t* d_desc, int n);
int  aria_kfdb_info(aria_kfdb_t db, int index, long long* id, int* count);
int  aria_kfdb_fetch(aria_kfdb_t db, int index, uint8_t* desc_host, int cap_rows, int* n_out);
/* The ratio-test match list of the query against keyframe `index` (LoopClosure.cpp:120-131, the list verifyGeometry starts
 * from), matched where the keyframe lies in HBM; same result as aria_matcher_match(query, fetched keyframe). Host query. */
int  aria_kfdb_match(aria_kfdb_t db, aria_matcher_t m, int index, const uint8_t* query_desc, int nq, float ratio,
                     aria_match* matches, int cap, int* n_out);
/* good[i] for every keyframe i (ratio test in double, LoopClosure.cpp:92); *n_out = keyframes. Host query. */
int  aria_kfdb_scan(aria_kfdb_t db, aria_matcher_t m, const uint8_t* query_desc, int nq, double ratio, int* good, int cap,
                    int* n_out);

/* Same for the matcher: stage 0 = kNN-2 kernel, stage 1 = ratio test + ordered compaction. */
#define ARIA_MATCHER_STAGES 2
int aria_matcher_set_profiling(aria_matcher_t m, int enable);
int aria_matcher_get_profile(aria_matcher_t m, int reset, double* stage_ms /*[2]*/, int64_t* stage_launches /*[2]*/,
                             int64_t* pairs);
/* Diagnostics (like aria_orb_fast_blur_kernel): kernel form of the handle's most recent batch / database kNN-2 launch --
 * "k_knn2_fp4" (FP4 matrix path, train sets <= 4096 rows), "k_knn2_mfma" (int8, wider train sets), or
 * "k_knn2_fp4|k_knn2_mfma" when both were launched behind the device-side gate (the FP4 one does the batch unless some pair's
 * train count exceeds 4096). bench.py keys the label and the peak of roofline.matcher on it. */
const char* aria_matcher_knn_kernel(aria_matcher_t m);
void* aria_matcher_stream(aria_matcher_t m);
int   aria_matcher_sync(aria_matcher_t m);

/* cudaStreamCreate / cudaStreamDestroy as the reference adapters use them (OrbCudaExtractor.cpp:28,50; CudaMatcher.cpp:16,24)
 * for hosts that do not link the HIP runtime: a stream to pass as aria_orb_config.stream AND aria_matcher_config.stream,
 * which orders the two handles' work (needed by aria_matcher_match_device_async). Destroy it after the handles. */
int aria_stream_create(int device, void** stream);
int aria_stream_destroy(int device, void* stream);

/* ---- device memory, staging copies and events (ABI 4) for a host that drives the BATCH entry points from the reference's
 * language without linking the HIP runtime (aria_slam_amd/host BatchFrontEnd, euroc_frontend --batch). What the reference
 * does through cv::cuda::GpuMat / the CUDA runtime on this path: device allocation + upload per frame
 * (src/legacy/Frame.cpp:19, src/adapters/gpu/OrbCudaExtractor.cpp:83, :158 upload on the stream), download of the results
 * (OrbCudaExtractor.cpp:102-103, :186-187), cudaStreamSynchronize (src/euroc_eval.cpp:153-154). Plain pointers and sizes;
 * every call returns an aria_status (HIP failures as ARIA_E_HIP with the text in aria_last_hip_error()).
 * Pinned host memory is what makes the copies asynchronous (a pageable source is staged by the runtime, synchronously).
 * Events order two streams (the copy stream fills chunk c + 1 while the compute stream works on chunk c) and time them. */
int aria_device_count(int* n);
int aria_device_alloc(int device, size_t bytes, void** d_ptr);
int aria_device_free(int device, void* d_ptr);
int aria_host_alloc_pinned(size_t bytes, void** h_ptr);
int aria_host_free_pinned(void* h_ptr);
int aria_copy_h2d_async(int device, void* stream, void* d_dst, const void* h_src, size_t bytes);
int aria_copy_d2h_async(int device, void* stream, void* h_dst, const void* d_src, size_t bytes);
int aria_copy_d2d_async(int device, void* stream, void* d_dst, const void* d_src, size_t bytes);
int aria_fill_async(int device, void* stream, void* d_dst, int byte_value, size_t bytes);
int aria_stream_synchronize(int device, void* stream);
int aria_event_create(int device, void** event);
int aria_event_destroy(int device, void* event);
int aria_event_record(int device, void* event, void* stream);
int aria_stream_wait_event(int device, void* stream, void* event);
int aria_event_synchronize(int device, void* event);
int aria_event_elapsed_ms(void* start_event, void* stop_event, float* ms);

/* ---- two-view relative pose: cv::findEssentialMat(pts1, pts2, K, RANSAC, 0.999, 1.0) + cv::recoverPose, the step every
 * consumer of a match list takes next in the reference (src/euroc_eval.cpp:178-201, src/main.cpp:186-191,
 * src/legacy/LoopClosure.cpp:116-190), on the device and batched over pairs. Additive to ABI 4.
 *
 * Points. For match m, view 1 is the query keypoint and view 2 the train keypoint when query_is_first = 1 (the legacy
 *   executables' order, euroc_eval.cpp:181-182: query = previous frame), the other way round when 0. Coordinates are
 *   normalised by the config's intrinsics in fp64 and rounded to fp32: ((x - cx) / fx, (y - cy) / fy).
 * Pose. x2 ~ R x1 + t with |t| = 1 (recoverPose's convention); E satisfies x2^T E x1 = 0 and has unit Frobenius norm.
 *   R, E row-major.
 * Inliers. Squared Sampson distance in normalised coordinates against thr2 = (threshold_px / ((fx + fy) / 2))^2, as
 *   findEssentialMat sets it, evaluated in fp32 and division-free: with Ex1 = E x1, Etx2 = E^T x2, r = x2^T E x1,
 *   d = Ex1[0]^2 + Ex1[1]^2 + Etx2[0]^2 + Etx2[1]^2, a point is an inlier when d > 0 and r^2 <= thr2 * d.
 * Hypotheses. `hypotheses` per pair (multiple of 64, 64..16384). All arithmetic modulo 2^64 on uint64:
 *     splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                    x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)
 *     key(pair, h)          = splitmix64(splitmix64(splitmix64(seed) ^ pair) ^ h)     pair = pair_base + p (as uint32)
 *     draw(pair, h, j, r)   = ((splitmix64(key(pair, h) ^ (8 r + j)) >> 32) * n) >> 32  in [0, n)
 *   Sample j = 0..7 of hypothesis h is draw(pair, h, j, r) for the first r = 0, 1, ... whose value differs from samples
 *   0..j-1; a slot still duplicate after 256 draws makes the hypothesis invalid. Results therefore depend on (seed, pair
 *   id, points) only, not on how pairs are batched (aria_slam_amd/pose_ref.py restates this in Python).
 * Minimal solver. Normalised 8-point on the sample: rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] (fp64), Gaussian
 *   elimination with partial pivoting (first row of largest |a|); a pivot with |pivot| <= 1e-9 * max|A_ij| marks the sample
 *   rank-deficient: invalid. Back substitution with f8 = 1, scale to unit norm, then projection onto the essential manifold:
 *   E = (u1 v1^T + u2 v2^T) / sqrt(2) from the SVD of the solution (invalid if sigma2 <= 1e-9 sigma1). The points already
 *   are in normalised camera coordinates (|x| ~ 1), so Hartley's conditioning transform is not applied again.
 * Winner. Most inliers; ties to the lowest h; an invalid hypothesis scores -1. Integer counts, fixed reduction order.
 * Refit. When the winner has >= 8 inliers: one least-squares 8-point fit over them -- the 9x9 normal matrix summed in fp64
 *   in a fixed order (per thread over its strided share of the matches, then a fixed tree), its smallest eigenvector
 *   (cyclic Jacobi), projected onto the manifold and rescored; kept (refined = 1) when its inlier count is >= the winner's.
 * recoverPose. E is decomposed into (R1, t), (R2, t), (R1, -t), (R2, -t) (R1 = U W V^T, R2 = U W^T V^T, t = u3). Every
 *   RANSAC inlier is triangulated under each candidate -- least-squares depths (z1, z2) of z2 x2 = z1 R x1 + t, where
 *   OpenCV solves the equivalent DLT -- and counted when 0 < z1 < distance_thresh and 0 < z2 < distance_thresh. The
 *   candidate with the most points wins (recoverPose's order of preference on ties); n_pose_inliers is that count (its
 *   return value), the mask is the RANSAC mask AND that candidate's cheirality mask.
 * Validity. valid = 0 when a pair has fewer than 8 matches or no valid hypothesis: R = I, t = 0, E = 0, counts 0,
 *   best_hypothesis = -1, mask all zeros. No field is ever NaN or Inf. Acceptance thresholds stay with the caller (e.g.
 *   n_pose_inliers > 10, euroc_eval.cpp:191).
 * Determinism. No float atomics; every result is bitwise reproducible run to run and independent of the batch split. */
typedef struct aria_pose_s* aria_pose_t;
typedef struct {
    int      struct_size;      /* = sizeof(aria_pose_config)                                                    */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one. An owned stream is
                                * non-blocking: it is NOT ordered against the legacy default stream (where torch works
                                * by default), so a caller that fills inputs there must synchronise first or pass its
                                * own stream                                                                        */
    int      hypotheses;       /* per pair: multiple of 64, 64..16384 (default 1024)                            */
    double   fx, fy, cx, cy;   /* intrinsics (default EuRoC cam0, src/legacy/EuRoCReader.cpp:11-17)              */
    double   threshold_px;     /* findEssentialMat's threshold in pixels (default 1.0)                           */
    double   distance_thresh;  /* recoverPose's depth bound (default 50, OpenCV's)                               */
    uint64_t seed;             /* sample hash seed (default 0)                                                   */
} aria_pose_config;
typedef struct {
    double R[9], t[3], E[9];
    int    n_matches, n_inliers, n_pose_inliers, best_hypothesis, refined, valid;
} aria_pose_result;

void  aria_pose_default_config(aria_pose_config* cfg);
int   aria_pose_create(const aria_pose_config* cfg, aria_pose_t* out);
void  aria_pose_destroy(aria_pose_t h);
void* aria_pose_stream(aria_pose_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check:
 * ARIA_E_INVALID when some pair's counts (n_matches outside [0, match_cap], a keypoint count outside [0, kp_stride]) or
 * match indices were out of range. Such a pair is detected before any keypoint is read and skipped (valid = 0,
 * n_matches = 0, zero mask); the other pairs are unaffected. */
int   aria_pose_check(aria_pose_t h);
/* One pair, host buffers; blocks. pair_base is the pair id the sample hash uses (the batch call's pair_base + p gives
 * the same result). mask (optional): n_matches bytes, 1 = RANSAC inlier in front of both cameras. Out-of-range match
 * indices: ARIA_E_INVALID. */
int   aria_pose_estimate(aria_pose_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                         const aria_match* matches, int n_matches, int query_is_first, int pair_base, aria_pose_result* out,
                         uint8_t* mask);
/* Device-resident batch form over what aria_orb_extract_batch_device and aria_matcher_match_batch_device leave in HBM.
 * Pair p reads keypoints at d_kp_query + p*kp_stride (d_nq[p] of them) and d_kp_train + p*kp_stride (d_nt[p]), matches at
 * d_matches + p*match_cap (d_nmatches[p] of them); writes d_out[p] and, if d_mask is not NULL, match_cap bytes at
 * d_mask + p*match_cap (zero beyond the pair's matches). The sample hash sees pair id pair_base + p. Consecutive frames
 * of one batch (pair p: query f = p + 1, train f = p, as in the dynamic-filter example above) are
 *   aria_pose_estimate_batch_device(h, kps + kp_cap, cnt + 1, kps, cnt, kp_cap, matches, nmatches, B - 1, match_cap,
 *                                   0, pair_base, out, mask);      // view 1 = train = previous frame
 * Enqueued on the handle's stream; no synchronisation (the first call with a larger batch grows the workspace, which waits
 * for the stream). Errors in the data are deferred to aria_pose_check. */
int   aria_pose_estimate_batch_device(aria_pose_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                      const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                      const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                      int query_is_first, int pair_base, aria_pose_result* d_out, uint8_t* d_mask);
/* Test hook: for one pair (host buffers), every hypothesis's 8 sample indices (sample_idx[h*8 + j]; -1 when n < 8),
 * E (E[h*9 + k], fp32 as scored; zero when invalid) and inlier count (counts[h], -1 when invalid). Blocks. */
int   aria_pose_debug_hypotheses(aria_pose_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                                 const aria_match* matches, int n_matches, int query_is_first, int pair_base, int* sample_idx,
                                 float* E, int* counts);

/* ---- two-view triangulation and point map: the reference's Mapper::triangulate (src/legacy/Mapper.cpp:7-120, thresholds
 * include/legacy/Mapper.hpp:67-70), the step euroc_eval.cpp:218-222 takes after every accepted pose, with filterOutliers
 * (:126-158) and filterByDistance (:160-168), on the device and batched over pairs into a map that stays in HBM. Additive
 * to ABI 4.
 *
 * Points and poses. For match m, x1 / x2 are the view-1 / view-2 keypoint pixels (fp32 as stored, used in fp64); view 1 is
 *   the query side when query_is_first = 1 (as in the pose stage). Each view has world-to-camera extrinsics [R_i | t_i]
 *   (3x4 row-major fp64, x_cam = R X + t -- how Mapper::triangulate uses its Matrix4d arguments); P_i = K [R_i | t_i]
 *   with rows (fx r0 + cx r2, fy r1 + cy r2, r2) of [R_i | t_i].
 * DLT (cv::triangulatePoints). A is the 4x4 with rows x1 P1[2] - P1[0], y1 P1[2] - P1[1], x2 P2[2] - P2[0],
 *   y2 P2[2] - P2[1]; X is the right singular vector of its smallest singular value, by a one-sided (Hestenes) Jacobi SVD
 *   in fp64: columns a_0..a_3 of A, V = I; one sweep visits the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in that order;
 *   with alpha = |a_i|^2, beta = |a_j|^2, gamma = a_i.a_j a pair is skipped when |gamma| <= 10 DBL_EPSILON sqrt(alpha beta),
 *   else zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = +1),
 *   c = 1 / sqrt(1 + t^2), s = c t, and (a_i, a_j) <- (c a_i - s a_j, s a_i + c a_j), the same on V's columns. Sweeps stop
 *   after the first one that rotates no pair, or after 30. X = the column of V whose rotated a_k has the least |a_k|^2
 *   (ties: lowest k); it has unit norm up to rounding. The point is rejected when |X[3]| < 1e-10, else dehomogenised.
 * Tests, in the reference's order, in fp64; a NaN fails every test:
 *   depth       keep when min_depth <= z_cam_i <= max_depth in both views;
 *   parallax    C_i = -R_i^T t_i, ray_i = (X - C_i) / |X - C_i|, parallax = acos(min(1, |ray1.ray2|)) * 180 / pi;
 *               rejected when below min_parallax_deg;
 *   reprojection err_i = sqrt((fx Xc / Zc + cx - u)^2 + (fy Yc / Zc + cy - v)^2) per view; rejected when either exceeds
 *               max_reproj_px.
 *   A pair with fewer than 8 matches adds nothing (Mapper.cpp:13, on the pair's match count before any mask).
 * Colour and quality. gray = the view-1 image byte at (clamp((int)x1, 0, W-1), clamp((int)y1, 0, H-1)); 127 without an
 *   image (the reference's default colour 0.5 as its export writes it, (int)(0.5 * 255)). quality = 1 / (err1 + err2 + 0.1).
 * Candidates. Every match, or those with a nonzero byte in the optional per-match mask (e.g. the pose stage's).
 * Map. Kept points are appended in pair order, then match order; id is a map-wide sequence number (next_id_++) that
 *   clear() resets. An append whose points do not all fit the capacity appends whole pairs in order while they fit and
 *   drops the rest (deferred ARIA_E_OUTPUT_TOO_SMALL; aria_map_points_needed tells what to reserve).
 * Filters (both compact stably and keep ids).
 *   filter_outliers: nothing below 10 points (Mapper.cpp:136); else mean = sum p / n, sd = sqrt(sum |p - mean|^2 / n),
 *     each sum in fp64 over blocks of 1024 consecutive points (per thread in order, then a fixed tree) added in block
 *     order; points with |p - mean| > 3 sd are removed.
 *   filter_distance(d): points with |p| > d are removed.
 * Determinism. No float atomics; the map after a sequence of calls is bitwise reproducible run to run and independent of
 *   how the same pairs were split into batch calls.
 * Known reference defect, not reproduced: Mapper.cpp:52-58 reads cv::triangulatePoints' output with at<double> where
 *   OpenCV 4.9 creates it with the (float) type of the input points; the stage computes what that code intends. */
typedef struct aria_map_s* aria_map_t;
typedef struct {
    int      struct_size;      /* = sizeof(aria_map_config)                                                     */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking, as in
                                * aria_pose_config)                                                               */
    double   fx, fy, cx, cy;   /* intrinsics (default EuRoC cam0)                                                */
    double   min_depth;        /* default 0.1; depth units are those of the extrinsics (baseline units with pose
                                * records, |t| = 1)                                                               */
    double   max_depth;        /* default 50                                                                     */
    double   min_parallax_deg; /* default 1.0                                                                    */
    double   max_reproj_px;    /* default 2.0                                                                    */
    int64_t  capacity;         /* initial arena capacity in points (default 65536)                               */
    int      min_pose_inliers; /* pose-record gate of the batch form: n_pose_inliers <= this adds nothing (default 10) */
    int      reserved;
} aria_map_config;
typedef struct {
    uint64_t id;               /* map-wide sequence number                                                       */
    double   X[3];             /* world point                                                                    */
    double   quality;          /* 1 / (err1 + err2 + 0.1)                                                        */
    float    err[2];           /* reprojection errors in views 1, 2 (px)                                         */
    int      pair, match;      /* pair id, index in the pair's match list                                        */
    int      idx1, idx2;       /* view-1 / view-2 keypoint index                                                 */
    uint8_t  gray;             /* view-1 image byte, 127 without an image                                        */
    uint8_t  pad[7];
} aria_map_point;              /* 72 bytes                                                                       */

void  aria_map_default_config(aria_map_config* cfg);
int   aria_map_create(const aria_map_config* cfg, aria_map_t* out);
void  aria_map_destroy(aria_map_t h);
void* aria_map_stream(aria_map_t h);
/* Synchronises the handle's stream and returns the deferred error of the calls since the last check, once:
 * ARIA_E_INVALID when some pair's counts or match indices were out of range (that pair was skipped before any keypoint
 * was read, the others are unaffected), else ARIA_E_OUTPUT_TOO_SMALL when an append was cut at the capacity. */
int   aria_map_check(aria_map_t h);
/* One pair from host buffers; blocks, appends, and grows the arena itself when needed. pose1 / pose2: 12 doubles each,
 * [R | t] row-major. image1 (optional): view 1's gray image, W x H bytes with `pitch` bytes per row. mask (optional):
 * n_matches bytes, nonzero = candidate. *n_added = points appended. Out-of-range match indices: ARIA_E_INVALID. */
int   aria_map_triangulate(aria_map_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                           const aria_match* matches, int n_matches, int query_is_first, const double* pose1,
                           const double* pose2, const uint8_t* image1, int width, int height, int pitch, const uint8_t* mask,
                           int pair_id, int* n_added);
/* Device-resident batch form over what the batch extract, match and pose calls leave in HBM, with the pointer and stride
 * conventions of aria_pose_estimate_batch_device: pair p reads keypoints at d_kp_query + p*kp_stride (d_nq[p] of them)
 * and d_kp_train + p*kp_stride (d_nt[p]), matches at d_matches + p*match_cap (d_nmatches[p]); its points carry pair id
 * pair_base + p. Poses: d_extrinsics (24 doubles per pair: [R1|t1], [R2|t2]) or, when that is NULL, d_pose records used as
 * [I|0], [R|t]; a record with valid == 0 or n_pose_inliers <= min_pose_inliers adds nothing. Optional: d_mask (match_cap
 * bytes per pair), view-1 images at d_img + p*img_stride (W x H, `pitch` bytes per row), d_added[p] = points appended
 * (0 for a pair dropped at the capacity). Enqueued on the handle's stream; no synchronisation (the first call with a larger
 * batch grows the workspace, which waits for the stream). Errors in the data are deferred to aria_map_check. */
int   aria_map_triangulate_batch_device(aria_map_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                        const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                        const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                        int query_is_first, int pair_base, const double* d_extrinsics,
                                        const aria_pose_result* d_pose, const uint8_t* d_mask, const uint8_t* d_img,
                                        int64_t img_stride, int width, int height, int pitch, int* d_added);
/* The largest map size an append since create / the last clear asked for (what to reserve after a cut). Blocks. */
int   aria_map_points_needed(aria_map_t h, int64_t* needed);
int   aria_map_size(aria_map_t h, int64_t* size);                  /* blocks */
int64_t aria_map_capacity(aria_map_t h);
int   aria_map_clear(aria_map_t h);                                /* size 0, ids restart at 0 */
int   aria_map_reserve(aria_map_t h, int64_t capacity);            /* grows, keeps the contents; blocks */
int   aria_map_read(aria_map_t h, int64_t first, int64_t count, aria_map_point* out);   /* blocks */
/* The arena on the device: aria_map_size points. Valid until the next reserve, grow or filter. */
const aria_map_point* aria_map_device_points(aria_map_t h);
int   aria_map_filter_outliers(aria_map_t h);                      /* enqueued */
int   aria_map_filter_distance(aria_map_t h, double max_distance); /* enqueued */

/* ---- fundamental-matrix RANSAC: cv::findFundamentalMat(pts1, pts2, FM_RANSAC, 3.0, 0.99, mask), the geometric check of
 * a loop candidate in the reference (src/legacy/LoopClosure.cpp:116-155, verifyGeometry), on the device and batched over
 * pairs. The F inliers, compacted in match order, are exactly the match input of aria_pose_estimate_batch_device, so a
 * loop candidate is verified F -> E without a round trip to the host (computeRelativePose, :158-195). Additive to ABI 4.
 *
 * Points. As in the pose stage: for match m, view 1 is the query keypoint when query_is_first = 1, the train keypoint when
 *   0. Coordinates are the stored fp32 pixels. F satisfies x2^T F x1 = 0 in pixel coordinates, row-major, fp64.
 * Small inputs. A pair with fewer than 15 matches has valid = 0 and costs no work. OpenCV takes other branches there
 *   (n = 7: the 7-point solver alone, mask all ones; 8..14: LMeDS); they are not restated.
 * Hypotheses. `hypotheses` per pair (multiple of 64, 64..16384). Sample slots j = 0..6 are drawn with the pose stage's
 *   hash, formulas unchanged (draw(pair, h, j, r), 256 redraws per slot; a slot still duplicate makes the hypothesis invalid).
 * Sample check (FMEstimatorCallback::checkSubset). OpenCV's haveCollinearPoints in both views, in fp64 from the fp32
 *   points: slot 6 against every pair (j, k), k < j < 6, with d1 = p_j - p_6, d2 = p_k - p_6; collinear when
 *   |d2.x d1.y - d2.y d1.x| <= FLT_EPSILON (|d1.x| + |d1.y| + |d2.x| + |d2.y|). A collinear sample makes the hypothesis
 *   invalid where OpenCV draws again: the fixed budget shrinks a little on near-degenerate data.
 * Minimal solver (run7Point, fp64). Each view of the sample is normalised on its own: centroid c, mean distance m from it
 *   (invalid when m < FLT_EPSILON), u = (x - c) sqrt(2) / m. Rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of the
 *   normalised points; Gaussian elimination over columns 0..6 with partial pivoting (first row of largest |a|); a pivot
 *   with |pivot| <= 1e-9 * max|A_ij| makes the hypothesis invalid (x1 == x2 for every match has rank 6 and lands here).
 *   Back substitution gives the null-space basis g1 (f7 = 1, f8 = 0) and g2 (f7 = 0, f8 = 1). With f1 = g1 - g2, f2 = g2
 *   the cubic det(l f1 + f2) = c0 l^3 + c1 l^2 + c2 l + c3 has run7Point's coefficients; |c0| <= 1e-12 max|c_i| makes the
 *   hypothesis invalid (our rule). Real roots in closed form -- trigonometric for three (Q^3 - R^2 > 0), Cardano for one --
 *   sorted ascending as k = 0..2. Per root, as run7Point: s = f1[8] l + f2[8]; if |s| > DBL_EPSILON the model is
 *   (l f1 + f2) / s with F[8] = 1, else l f1 + f2 with F[8] = 0; F = T2^T F T1 (de-normalised); F /= F[8] when
 *   |F[8]| > FLT_EPSILON. A hypothesis with a non-finite model entry is invalid. The rank-2 members of the pencil do not
 *   depend on the basis, so the models equal run7Point's (SVD basis) up to rounding.
 * Inliers (computeError). With (a, b, c) = F x1, d2 = x2 . (a, b, c) and (a', b', c') = F^T x2, a point is an inlier when
 *   a^2 + b^2 > 0, a'^2 + b'^2 > 0 and max(d2^2 / (a^2 + b^2), d2^2 / (a'^2 + b'^2)) <= threshold_px^2. Evaluated in fp32,
 *   division-free, on points conditioned once per pair: per view the centroid c and RMS distance d of all the pair's
 *   matches (fp64 sums in a fixed order; d = 1 below 1 px), u = (x - c) / d, G = A2^T F A1 (A = [[d, 0, cx], [0, d, cy],
 *   [0, 0, 1]]) scaled to max|G_ij| = 1; with l = G u1, l' = G^T u2, r = u2 . l: inlier when D2 = l0^2 + l1^2 > 0,
 *   D1 = l'0^2 + l'1^2 > 0, r^2 <= (thr / d2)^2 D2 and r^2 <= (thr / d1)^2 D1. For every point whose fp64 pixel-space
 *   error lies more than a relative 1e-3 from thr^2 the decision equals the fp64 form's (aria_slam_amd/fund_ref.py).
 * Winner. Most inliers over all (h, k); ties to the lowest h, then the lowest k; an invalid model scores -1. A winner
 *   needs at least 7 inliers (OpenCV's count > max(best, 6)), else valid = 0. Integer counts, fixed reduction order, no
 *   refit: F is the winning minimal model, the mask its inliers.
 * Validity. valid = 0: F = 0, n_inliers = n_models = 0, best_hypothesis = best_root = -1, mask zero, compacted count 0.
 *   No field is ever NaN or Inf.
 * Determinism. No float atomics; every result is bitwise reproducible run to run and independent of the batch split.
 * Not restated: USAC, OpenCV's RNG sequence and its adaptive stop (the budget is fixed; the default 1024 covers the
 *   reference's 1000 iterations). Parity with a running OpenCV is not pinned by any test. */
typedef struct aria_fund_s* aria_fund_t;
typedef struct {
    int      struct_size;      /* = sizeof(aria_fund_config)                                                    */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one. An owned stream is
                                * non-blocking: it is NOT ordered against the legacy default stream (where torch works
                                * by default), so a caller that fills inputs there must synchronise first or pass its
                                * own stream                                                                        */
    int      hypotheses;       /* per pair: multiple of 64, 64..16384 (default 1024)                            */
    double   threshold_px;     /* findFundamentalMat's threshold in pixels (default 3.0, LoopClosure.cpp:143)    */
    uint64_t seed;             /* sample hash seed (default 0)                                                   */
} aria_fund_config;
typedef struct {
    double F[9];               /* row-major, pixel coordinates, x2^T F x1 = 0                                    */
    int    n_matches, n_inliers, n_models, best_hypothesis, best_root, valid;   /* n_models: valid models scored */
} aria_fund_result;            /* 96 bytes                                                                       */

void  aria_fund_default_config(aria_fund_config* cfg);
int   aria_fund_create(const aria_fund_config* cfg, aria_fund_t* out);
void  aria_fund_destroy(aria_fund_t h);
void* aria_fund_stream(aria_fund_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check, once:
 * ARIA_E_INVALID when some pair's counts or match indices were out of range. Such a pair is detected before any keypoint
 * is read and skipped (valid = 0, n_matches = 0, zero mask, compacted count 0); the other pairs are unaffected. */
int   aria_fund_check(aria_fund_t h);
/* One pair, host buffers; blocks. pair_base is the pair id of the sample hash. mask (optional): n_matches bytes,
 * 1 = inlier of F. Out-of-range match indices: ARIA_E_INVALID. */
int   aria_fund_estimate(aria_fund_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                         const aria_match* matches, int n_matches, int query_is_first, int pair_base, aria_fund_result* out,
                         uint8_t* mask);
/* Device-resident batch form with the conventions of aria_pose_estimate_batch_device (keypoints at p*kp_stride, matches
 * at p*match_cap, pair id pair_base + p). Writes d_out[p] and, each optional: d_mask (match_cap bytes at p*match_cap, zero
 * beyond the pair's matches); d_inliers (the F inliers' aria_match records in match order at p*match_cap, zero records
 * beyond the count) with d_ninliers[p] = their count -- pass both or neither; they are the (d_matches, d_nmatches) input
 * of aria_pose_estimate_batch_device with the same keypoints and match_cap. Enqueued on the handle's stream; no
 * synchronisation (a larger batch grows the workspace, which waits for the stream). Data errors: aria_fund_check. */
int   aria_fund_estimate_batch_device(aria_fund_t h, const aria_keypoint* d_kp_query, const int* d_nq,
                                      const aria_keypoint* d_kp_train, const int* d_nt, int64_t kp_stride,
                                      const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                      int query_is_first, int pair_base, aria_fund_result* d_out, uint8_t* d_mask,
                                      aria_match* d_inliers, int* d_ninliers);
/* Test hook: for one pair (host buffers), per hypothesis h: the 7 sample indices (sample_idx[h*7 + j]; -1 when n < 15 or
 * the slot stayed duplicate), the number of valid models n_models[h] (0, 1 or 3), the models F[h*27 + k*9 + e] (fp64, zero
 * for k >= n_models[h]) and their inlier counts counts[h*3 + k] (-1 for k >= n_models[h]). Blocks. */
int   aria_fund_debug_hypotheses(aria_fund_t h, const aria_keypoint* kp_query, int nq, const aria_keypoint* kp_train, int nt,
                                 const aria_match* matches, int n_matches, int query_is_first, int pair_base, int* sample_idx,
                                 int* n_models, double* F, int* counts);

/* ---- SE(3) pose-graph optimisation: the reference's PoseGraphOptimizer (include/legacy/LoopClosure.hpp:80-113,
 * src/legacy/LoopClosure.cpp:197-312), g2o's VertexSE3 / EdgeSE3 graph under Levenberg-Marquardt, batched over graphs.
 * Additive to ABI 4. aria_slam_amd/graph_ref.py restates the stage in NumPy and is its definition; parity with a running
 * g2o is not pinned by any test (g2o and Eigen are not available to this project).
 *
 * Pose. 12 doubles, the rows of [R t]. A graph's vertices are the dense indices 0..n-1 (the id -> index map, the dropping
 *   of edges that name an unknown id and the x10 of loop edges live in the adapters); one vertex is fixed.
 * Update. X <- X * fromMQT(d), d = (tx, ty, tz, qx, qy, qz), w = sqrt(1 - |q|^2), for |q|^2 > 1 the quaternion (0, -q)
 *   normalised; the rotation is then replaced by that of its unit quaternion.
 * Error. e = toMQT(Z^-1 Xi^-1 Xj) with the quaternion's w >= 0; chi2 = sum info_scale * e.e. Analytic Jacobians.
 * LM. lambda0 = 1e-5 max diag(H) per call; a trial solves (H + lambda I) dx = b; rho = (chi2 - chi2_new) / (dx.(lambda dx
 *   + b) + 1e-3); accepted when rho > 0 and chi2_new is finite, then lambda *= max(1/3, 1 - (2 rho - 1)^3), ni = 2;
 *   otherwise lambda *= ni, ni *= 2 and the poses are restored; at most 10 trials; an iteration whose trials all fail ends
 *   the call (stop_reason 1). No robust kernel.
 * Solver. Block-Jacobi preconditioned conjugate gradients in fp64, from x = 0, until |r| <= pcg_rel_tol |b| or
 *   pcg_max_iters; |b| = 0 gives dx = 0. One workgroup per graph, no communication between workgroups.
 * Invalid input. Counts below 0, a fixed index outside [0, n), an edge index outside [0, n), an edge from a vertex to
 *   itself or an info_scale that is negative or not finite: that graph gets valid = 0, stop_reason 2, before any of its
 *   poses is read, and its poses are not written; the other graphs of the batch are unaffected.
 * Determinism. No float atomics; H is gathered per vertex over its edges in edge order; sums are fixed trees. Every pose
 *   and result is bitwise reproducible run to run and independent of the graph's place in a batch and of the batch split.
 *   The fixed vertex is never written; with iterations = 0 no pose is written. */
typedef struct aria_graph_s* aria_graph_t;
typedef struct {
    int      struct_size;      /* = sizeof(aria_graph_config)                                                   */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking: not
                                * ordered against the legacy default stream, see aria_fund_config)               */
    int      max_graphs;       /* graphs in flight per launch (scratch slots), 1..65535 (default 1); a larger batch
                                * runs as consecutive launches                                                    */
    int      max_vertices;     /* per graph, 1..2^20 (default 4096)                                              */
    int      max_edges;        /* per graph, 1..2^22 (default 8192)                                              */
    int      pcg_max_iters;    /* cap of one solve (default 1000)                                                */
    double   pcg_rel_tol;      /* stop at |r| <= pcg_rel_tol |b| (default 1e-8)                                  */
} aria_graph_config;           /* 40 bytes                                                                       */
typedef struct {
    int32_t  from, to;         /* vertex indices of the graph                                                    */
    double   info_scale;       /* information = info_scale * I6                                                  */
    double   Z[12];            /* the measured pose of `to` in the frame of `from`, rows of [R t]                */
} aria_graph_edge;             /* 112 bytes                                                                      */
typedef struct {
    double   chi2_initial, chi2_final, lambda;
    int      iterations_done;  /* iterations with an accepted trial                                              */
    int      trials;           /* linear solves                                                                  */
    int      pcg_iterations;   /* over all solves                                                                */
    int      valid;
    int      stop_reason;      /* 0 = the iteration count, 1 = every trial of an iteration failed, 2 = invalid   */
    int      reserved;
} aria_graph_result;           /* 48 bytes                                                                       */

void  aria_graph_default_config(aria_graph_config* cfg);
int   aria_graph_create(const aria_graph_config* cfg, aria_graph_t* out);
void  aria_graph_destroy(aria_graph_t h);
void* aria_graph_stream(aria_graph_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check, once:
 * ARIA_E_INVALID when some graph was invalid (above), else ARIA_E_TOO_LARGE when some graph had more vertices or edges
 * than the handle was created for (that graph: valid = 0, nothing read, nothing written). */
int   aria_graph_check(aria_graph_t h);
/* One graph, host arrays; blocks. poses_inout: n_vertices * 12 doubles. Invalid input: ARIA_E_INVALID, larger than the
 * handle: ARIA_E_TOO_LARGE, in both cases nothing is written. */
int   aria_graph_optimize(aria_graph_t h, double* poses_inout, int n_vertices, int fixed_index, const aria_graph_edge* edges,
                          int n_edges, int iterations, aria_graph_result* result);
/* Device-resident batch: graph g owns the vertices d_vertex_offset[g] .. d_vertex_offset[g+1] of d_poses (12 doubles each)
 * and the edges d_edge_offset[g] .. d_edge_offset[g+1] of d_edges (indices relative to the graph), fixed vertex
 * d_fixed[g]; both offset arrays hold n_graphs + 1 entries. Writes d_poses in place and d_results[g]. Enqueued on the
 * handle's stream: every LM iteration of a graph runs inside one launch, there is no host synchronisation. Data errors:
 * aria_graph_check. */
int   aria_graph_optimize_batch_device(aria_graph_t h, double* d_poses, const int* d_vertex_offset,
                                       const aria_graph_edge* d_edges, const int* d_edge_offset, const int* d_fixed,
                                       int n_graphs, int iterations, aria_graph_result* d_results);
/* Test hook: one graph (host arrays) linearised at its poses. chi2; b (n_vertices * 6); H_diag (n_vertices * 36, row-major
 * 6x6 diagonal blocks); H_off (n_edges * 36, the block at (from, to) of every edge, row-major; its transpose sits at
 * (to, from)). Nothing of the fixed vertex is removed. Blocks. */
int   aria_graph_debug_linearize(aria_graph_t h, const double* poses, int n_vertices, int fixed_index,
                                 const aria_graph_edge* edges, int n_edges, double* chi2, double* b, double* H_diag,
                                 double* H_off);

/* ---- visual-inertial fusion: the reference's SensorFusion EKF (include/legacy/IMU.hpp:53-118, src/legacy/IMU.cpp:102-305)
 * and IMUPreintegrator (IMU.hpp:17-51, IMU.cpp:28-100), batched over tracks and over image intervals. Additive to ABI 4.
 * aria_slam_amd/fusion_ref.py restates both classes in NumPy and is their definition; parity with an Eigen build of the
 * reference is not pinned by any test (Eigen is not available to this project).
 *
 * State. p, v (world), q = (w, x, y, z) body -> world, accelerometer and gyro bias, P 15x15 row-major over the error state
 *   [p, v, theta, ba, bg]. fp64 throughout.
 * Events. Frame f of a track first consumes the IMU samples [imu_end[f-1], imu_end[f]) of the track (imu_end[-1] = 0), then
 *   its visual record when accept != 0 (src/euroc_eval.cpp:139-142, :209), then one aria_fuse_state is written.
 * IMU sample (addIMU + predictEKF, IMU.cpp:126-222). Ignored while the filter is not initialised. dt = t - last_imu_time;
 *   dt <= 0 or dt > 0.1 only moves last_imu_time (counted as skipped). Otherwise a = accel - ba, w = gyro - bg, R = R(q)
 *   of the orientation BEFORE the gyro step; q <- normalize(q * AngleAxis(|w dt|, w dt / |w dt|)) when |w dt| > 1e-10;
 *   a_w = R a + g; p += v dt + ((0.5 a_w) dt) dt; v += a_w dt; P <- F P F^T + G Q G^T with the reference's F (identity plus
 *   six 3x3 blocks) and G (five blocks), Q = diag(accel_noise^2, gyro_noise^2, accel_bias_walk^2, gyro_bias_walk^2) x I3;
 *   P <- 0.5 (P + P^T).
 * Visual record (addVisualPose + updateEKF, IMU.cpp:224-305). The first accepted record initialises p = p_meas, q = quat(R),
 *   v = 0, both times = t. Later ones: innovation [p_meas - p, log(normalize(quat(R) * q^-1))], S = P_hh + diag(pos_noise^2 x3,
 *   rot_noise^2 x3) over the rows / columns h = {0, 1, 2, 6, 7, 8}, K = P_:h S^-1, p, v, ba, bg += K innov,
 *   q <- normalize(exp(dx_theta) * q), Joseph form, P <- 0.5 (P + P^T), last_visual_time = t.
 * Ours by definition (Eigen internals written out). quat(R): trace > 0 branch, else the largest diagonal entry (first of
 *   equals), no sign forced on w. log(q): angle = 2 atan2(|vec|, |w|), axis = vec / |vec|, negated when w < 0, zero vector when
 *   |vec| = 0: independent of the sign of q. S^-1: Cholesky (lower, no pivoting), applied as two triangular solves; a pivot
 *   that is not > 0 skips the update (nothing changes but last_visual_time; n_updates stays 0).
 * Invalid input. A non-finite field of a sample or of a visual record, imu_end decreasing, negative or beyond the track's
 *   samples, an offset array that decreases or leaves [0, total]: the track is invalid, detected before anything else of it
 *   is read; its filter is not written, its states are zeroed (valid = 0; not written at all when its frame range itself is
 *   out of bounds), the other tracks are unaffected, and aria_fuse_check reports ARIA_E_INVALID. For valid input no output is
 *   ever NaN or Inf.
 * Determinism. No float atomics. A track's bits depend on its filter record and its events only: reproducible run to run,
 *   independent of the track's place in a batch, of its neighbours, of the batch split, and of feeding the track in chunks
 *   through the filter record (the counters of aria_fuse_state are per frame for that reason).
 * Preintegration (IMUPreintegrator::integrate). Interval i integrates the samples [begin[i], end[i]). The first sample only
 *   sets the time; dt <= 0 or dt > 0.5 is skipped; a_w = delta_q * a with delta_q BEFORE this sample's rotation, the
 *   covariance's F and G with delta_q AFTER it; noise 0.01 / 0.001; the 9x9 covariance [p, v, theta] is not symmetrised.
 *   begin > end, a range outside [0, n_imu] or a non-finite sample: valid = 0, the record zeroed, ARIA_E_INVALID deferred. */
typedef struct aria_fuse_s* aria_fuse_t;
typedef struct {
    double   t;                /* seconds                                                                        */
    double   accel[3];         /* m/s^2                                                                          */
    double   gyro[3];          /* rad/s                                                                          */
} aria_imu_sample;             /* 56 bytes (IMUMeasurement, IMU.hpp:6-10)                                        */
typedef struct {
    double   t;
    double   R[9];             /* row-major                                                                      */
    double   p[3];
    int      accept;           /* 0: the frame has no measurement (src/euroc_eval.cpp:191)                       */
    int      reserved;
} aria_fuse_visual;            /* 112 bytes                                                                      */
typedef struct {
    double   p[3], v[3], q[4], ba[3], bg[3];
    double   P[225];
    double   last_imu_time, last_visual_time;      /* -1 before the first event                                 */
    double   gravity[3];                           /* (0, 0, -9.81), IMU.hpp:105                                */
    double   accel_noise, gyro_noise, accel_bias_walk, gyro_bias_walk, pos_noise, rot_noise;   /* IMU.hpp:108-113 */
    int      initialized;
    int      reserved;
} aria_fuse_filter;            /* 2024 bytes: everything SensorFusion holds, so a sequence can be fed in chunks   */
typedef struct {
    double   t;                /* the frame's visual timestamp                                                   */
    double   p[3], v[3], q[4], ba[3], bg[3];
    double   P_diag[15];
    int      n_predicted;      /* this frame's IMU samples that propagated the state                            */
    int      n_skipped;        /* ... that only moved last_imu_time (dt <= 0 or dt > 0.1)                        */
    int      n_ignored;        /* ... that arrived before the filter was initialised                             */
    int      n_updates;        /* 1 when the frame's visual record updated the filter (the initialising one: 0)   */
    int      initialized;      /* after the frame                                                                */
    int      valid;
} aria_fuse_state;             /* 280 bytes                                                                      */
typedef struct {
    double   delta_p[3], delta_v[3], delta_q[4], dt_sum;
    double   cov[81];          /* row-major 9x9                                                                  */
    int      n_used;           /* samples that integrated (neither the first nor skipped)                        */
    int      valid;
} aria_preint_result;          /* 744 bytes                                                                      */
typedef struct {
    int      struct_size;      /* = sizeof(aria_fuse_config)                                                     */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking: not
                                * ordered against the legacy default stream, see aria_pose_config)               */
    double   gravity[3];       /* what aria_fuse_filter_init writes into a filter: the reference's defaults       */
    double   accel_noise, gyro_noise, accel_bias_walk, gyro_bias_walk, pos_noise, rot_noise;
} aria_fuse_config;            /* 88 bytes                                                                       */

void  aria_fuse_default_config(aria_fuse_config* cfg);
int   aria_fuse_create(const aria_fuse_config* cfg, aria_fuse_t* out);
void  aria_fuse_destroy(aria_fuse_t h);
void* aria_fuse_stream(aria_fuse_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when some track or interval was invalid (above). */
int   aria_fuse_check(aria_fuse_t h);
/* SensorFusion's constructor (IMU.cpp:104-124) and member defaults (IMU.hpp:87-117): zero state, identity orientation,
 * P0 = diag(0.01 x9, 0.001 x3, 0.0001 x3), times -1, not initialised; gravity and noise from cfg (NULL: the defaults).
 * Host only. */
int   aria_fuse_filter_init(aria_fuse_filter* filter, const aria_fuse_config* cfg);
/* Device-resident batch: track k owns the samples d_imu_offset[k] .. d_imu_offset[k+1] of d_imu and the frames
 * d_frame_offset[k] .. d_frame_offset[k+1] of d_imu_end, d_visual and d_states; both offset arrays hold n_tracks + 1 entries
 * and must stay within [0, n_imu_total] and [0, n_frames_total]. d_imu_end is relative to the track's first sample.
 * d_filters_inout[k] is read at the start and written at the end, so a sequence may be fed in chunks. Enqueued on the
 * handle's stream, one launch, no synchronisation. Data errors: aria_fuse_check. */
int   aria_fuse_run_batch_device(aria_fuse_t h, aria_fuse_filter* d_filters_inout, const aria_imu_sample* d_imu,
                                 const int* d_imu_offset, int n_imu_total, const int* d_imu_end, const aria_fuse_visual* d_visual,
                                 const int* d_frame_offset, int n_frames_total, int n_tracks, aria_fuse_state* d_states);
/* One track, host arrays; blocks. Invalid input: ARIA_E_INVALID, the filter untouched, the states zeroed. */
int   aria_fuse_run(aria_fuse_t h, aria_fuse_filter* filter_inout, const aria_imu_sample* imu, int n_imu, const int* imu_end,
                    const aria_fuse_visual* visual, int n_frames, aria_fuse_state* states);
/* Measurements from what aria_pose_estimate_batch_device leaves in HBM, without a host round trip: t = d_timestamps[i],
 * R, p = the result's R, t, accept = valid && n_pose_inliers > min_pose_inliers (src/euroc_eval.cpp:191). This is the
 * RELATIVE pose with unit-length t, which is what euroc_eval.cpp:209 hands the filter. Enqueued on the handle's stream. */
int   aria_fuse_visual_from_pose_device(aria_fuse_t h, const aria_pose_result* d_pose_results, const double* d_timestamps, int n,
                                        int min_pose_inliers, aria_fuse_visual* d_visual);
/* Preintegration of n_intervals intervals [d_begin[i], d_end[i]) of d_imu (n_imu samples). d_bias: 6 doubles (accelerometer,
 * gyro bias; IMUPreintegrator::setBias) shared by the call, or NULL = zero. Enqueued on the handle's stream. */
int   aria_fuse_preintegrate_batch_device(aria_fuse_t h, const aria_imu_sample* d_imu, int n_imu, const int* d_begin,
                                          const int* d_end, int n_intervals, const double* d_bias_or_null,
                                          aria_preint_result* d_out);
/* The same over host arrays; blocks. */
int   aria_fuse_preintegrate(aria_fuse_t h, const aria_imu_sample* imu, int n_imu, const int* begin, const int* end,
                             int n_intervals, const double* bias_or_null, aria_preint_result* out);

/* ---- trajectory evaluation: the reference's ground-truth lookup (EuRoCReader::getGroundTruth, src/legacy/EuRoCReader.cpp:
 * 311-346) and its trajectory error (computeATE / computeRPE, src/euroc_eval.cpp:28-61), plus the Umeyama alignment its
 * documentation defines ATE with (docs/milestones/H07_EUROC_DATASET_AUDIT.md:602-611) and its code leaves out. Batched over
 * query timestamps and over trajectories. Additive to ABI 4. aria_slam_amd/eval_ref.py restates all of it in NumPy and is the
 * definition; parity with an Eigen build of the reference is not pinned by any test (Eigen is not available to this project).
 * fp64 throughout.
 *
 * Ground-truth sampling. Query t takes the lower bound over the n_gt rows (first row with timestamp >= t). Past the last row:
 *   the last row, copied (its own timestamp included). At or before the first row: the first row, copied. Otherwise rows
 *   a = lower bound - 1, b = lower bound, alpha = (t - t_a) / (t_b - t_a) with t_a < t <= t_b (an exact hit of row b gives
 *   alpha = 1 between b - 1 and b); p, v, bg, ba = (1 - alpha) a + alpha b in that operation order; q = slerp as Eigen writes
 *   it, ours by definition: d = a.b; |d| >= 1 - 2^-52: weights 1 - alpha and alpha; else th = acos |d|, weights
 *   sin((1 - alpha) th) / sin th and sin(alpha th) / sin th; the second weight negated when d < 0; not renormalised. The
 *   output's t is the query. Invalid: n_gt < 1, a non-finite field of any row, a timestamp smaller than its predecessor's --
 *   found by a scan of its own before any row is sampled; then EVERY output of the call is zeroed with valid = 0. A non-finite
 *   query invalidates its own output only. Either defers ARIA_E_INVALID to aria_eval_check.
 * Trajectory metrics. Trajectory k owns the poses offset[k] .. offset[k+1] of the estimate (the convention of d_vertex_offset
 *   of aria_graph_optimize_batch_device, which can be passed as it is). Positions are read in place: ARIA_EVAL_EST_POSE12 =
 *   entries 3, 7, 11 of 12-double [R t] rows, ARIA_EVAL_EST_FUSE_STATE = p of aria_fuse_state records,
 *   ARIA_EVAL_EST_XYZ = packed triples. Truth positions are p of aria_eval_truth records, indexed like the estimate, or
 *   (truth_shared != 0) one trajectory of n_truth records that every trajectory is scored against, pose i against record
 *   i - offset[k]. A pose is USED when its mask byte (optional array, one byte per pose) is nonzero and, for fuse states, its
 *   record has initialized != 0 and valid != 0. n = number of used poses, sums over used poses in index order:
 *     ate_raw  = sqrt(sum |e_i - g_i|^2 / n), -1 when n = 0                                  (computeATE: no alignment)
 *     rpe_raw  = sqrt(sum |(e_i - e_{i-delta}) - (g_i - g_{i-delta})|^2 / pairs) over the i >= delta whose two ends are both
 *                used, -1 when there is no such pair (so whenever the length <= delta)           (computeRPE)
 *     Umeyama (estimate onto truth), two passes: centroids mu_e, mu_g; C = sum (g_i - mu_g)(e_i - mu_e)^T / n, var =
 *       sum |e_i - mu_e|^2 / n. C = U diag(sigma) V^T by one-sided Jacobi ON C ITSELF (never C^T C: that squares the
 *       condition number), sigma sorted descending, u3 := u1 x u2. R = [u1 u2 u3] diag(1, 1, det V) V^T, which is Umeyama's
 *       U diag(1, 1, det U det V) V^T whatever sign the third left vector had; scale = (sigma1 + sigma2 + d sigma3) / var with
 *       d = det U det V (similarity) or 1 exactly (rigid); t = mu_g - scale R mu_e. Mode none: scale 1, R = I, t = 0.
 *     ate_rmse / ate_mean / ate_max of |scale R e_i + t - g_i|, rpe_aligned of |scale R (e_i - e_{i-delta}) - (g_i - g_{i-delta})|.
 *   Degenerate alignment (rigid and similarity only): n < 3, or sigma2 <= 1e-10 sigma1 (collinear or coincident points; the
 *   threshold is a definition): align_valid = 0, scale, R, t and the aligned fields are -1, the raw fields, sigma and the
 *   counts stay filled. In mode none only n = 0 is degenerate.
 * Invalid input. offset[k] > offset[k+1], a range leaving [0, n_poses_total] (or [0, n_truth] for truth that is not shared), a
 *   shared truth whose length differs from the trajectory's, rpe_delta < 1, an align mode or estimate kind that does not
 *   exist, a non-finite position of a used pose or of its truth: that trajectory's result is zeroed (valid = 0), its per-pose
 *   errors are written as 0 when its range is in bounds and not at all otherwise, the other trajectories are unaffected,
 *   and aria_eval_check reports ARIA_E_INVALID once.
 * Determinism. No float atomics; fixed-tree reductions. A trajectory's bits depend on its own poses, truth and mask only:
 *   reproducible run to run, independent of its place in the batch, of its neighbours and of how the batch is split
 *   (a call of more than 32768 trajectories is split into launches of that many by the library itself). */
typedef struct aria_eval_s* aria_eval_t;
enum { ARIA_EVAL_ALIGN_NONE = 0, ARIA_EVAL_ALIGN_SE3 = 1, ARIA_EVAL_ALIGN_SIM3 = 2 };
enum { ARIA_EVAL_EST_POSE12 = 0, ARIA_EVAL_EST_FUSE_STATE = 1, ARIA_EVAL_EST_XYZ = 2 };
typedef struct {
    double   t;                /* seconds                                                                        */
    double   p[3];
    double   q[4];             /* w, x, y, z                                                                     */
    double   v[3], bg[3], ba[3];
} aria_eval_truth;             /* 136 bytes: the columns of state_groundtruth_estimate0/data.csv, in their order  */
typedef struct {
    double   ate_raw, rpe_raw;
    double   scale, R[9], t[3];                    /* row-major; aligned = scale R e + t                          */
    double   sigma[3];                             /* singular values of C, descending                            */
    double   ate_rmse, ate_mean, ate_max, rpe_aligned;
    int      n_poses;          /* length of the trajectory                                                       */
    int      n_used;           /* poses that took part                                                           */
    int      n_rpe_pairs;
    int      align_valid;
    int      valid;
    int      reserved;
} aria_eval_result;            /* 200 bytes                                                                      */
typedef struct {
    int      struct_size;      /* = sizeof(aria_eval_config)                                                     */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking: not
                                * ordered against the legacy default stream, see aria_pose_config)               */
    int      align_mode;       /* what a caller passes on when it has no preference: ARIA_EVAL_ALIGN_SIM3         */
    int      rpe_delta;        /* likewise: 10 (computeRPE's default)                                            */
} aria_eval_config;            /* 24 bytes                                                                       */

void  aria_eval_default_config(aria_eval_config* cfg);
int   aria_eval_create(const aria_eval_config* cfg, aria_eval_t* out);
void  aria_eval_destroy(aria_eval_t h);
void* aria_eval_stream(aria_eval_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when some call or trajectory was invalid (above). */
int   aria_eval_check(aria_eval_t h);
/* n queries against n_gt ground-truth rows, all in HBM. d_valid (optional): n ints, 1 = sampled. Enqueued on the handle's
 * stream (a scan of the rows, then one lane per query), no synchronisation. */
int   aria_eval_sample_truth_device(aria_eval_t h, const aria_eval_truth* d_gt, int n_gt, const double* d_timestamps, int n,
                                    aria_eval_truth* d_out, int* d_valid_or_null);
/* The same over host arrays; blocks. Invalid input: ARIA_E_INVALID (the outputs zeroed as above). */
int   aria_eval_sample_truth(aria_eval_t h, const aria_eval_truth* gt, int n_gt, const double* timestamps, int n,
                             aria_eval_truth* out, int* valid_or_null);
/* n_traj trajectories over device arrays. d_est: n_poses_total records of est_kind. d_offset: n_traj + 1 ints. d_truth:
 * n_truth records. d_mask (optional): n_poses_total bytes. d_pose_err (optional): n_poses_total doubles, the aligned error
 * of every used pose, -1 for a pose that is not used or when the alignment is degenerate. Trajectories may share poses (they
 * are only read); a shared pose's entry of d_pose_err is then that of one of its trajectories. One workgroup per trajectory.
 * Enqueued on the handle's stream, no synchronisation. Data errors: aria_eval_check. */
int   aria_eval_batch_device(aria_eval_t h, const void* d_est, int est_kind, const int* d_offset, int n_poses_total, int n_traj,
                             const aria_eval_truth* d_truth, int n_truth, int truth_shared, const uint8_t* d_mask_or_null,
                             int align_mode, int rpe_delta, double* d_pose_err_or_null, aria_eval_result* d_results);
/* The same over host arrays; blocks. ARIA_E_INVALID when some trajectory was invalid (the others are still scored). */
int   aria_eval_batch(aria_eval_t h, const void* est, int est_kind, const int* offset, int n_poses_total, int n_traj,
                      const aria_eval_truth* truth, int n_truth, int truth_shared, const uint8_t* mask_or_null, int align_mode,
                      int rpe_delta, double* pose_err_or_null, aria_eval_result* results);

/* ---- object detector: everything the reference does AROUND its network, on the device and batched over frames. The
 * reference's detector (include/interfaces/IObjectDetector.hpp:10-46; src/legacy/TRTInference.cpp) resizes and repacks the
 * image on the host (TRTInference::preprocess, :68-93), runs the engine, copies the [300, 6] head back and decodes it on the
 * host (TRTInference::postprocess, :95-142, with cv::dnn::NMSBoxes): two blocking copies per frame. Here the network is the
 * caller's (anything that reads d_input and writes d_raw on a stream) and the two stages around it are kernels, so the boxes
 * reach aria_flag_keypoints_device without leaving HBM. aria_slam_amd/detect_ref.py restates both stages in NumPy and is the
 * definition; the device is bitwise equal to it. Additive to ABI 4.
 *
 * Preprocess. cv::resize(image, Size(input_w, input_h)) as the 8-bit INTER_LINEAR fixed-point path computes it (a stretch,
 *   no letterbox): per axis, in fp32, f = (d + 0.5f) * (src / (float)dst) - 0.5f, s = floor(f), f -= s; s < 0 -> s = 0, f = 0;
 *   s >= src - 1 -> s = src - 1, f = 0 (both taps the last pixel); weights a = cvRound(f * 2048) and 2048 - a. Horizontal pass
 *   S = p[s] * (2048 - a) + p[s + 1] * a in int32, vertical pass (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
 *   The value is then (float)v * (float)(1.0 / 255.0) (convertTo, :76), stored planar (HWC -> CHW, :79-87) as fp32, or rounded
 *   once to fp16 (nearest even) when the handle was created with out_half. channels = 3: interleaved pixels; swap_rb = 1
 *   exchanges planes 0 and 2 (cvtColor BGR2RGB, :75). channels = 1: the gray plane written three times (what GRAY2BGR in front
 *   of detect() gives, src/euroc_eval.cpp:149).
 * Postprocess. Frame f's candidates are n_candidates rows [x1, y1, x2, y2, confidence, class_id] of floats in network-input
 *   coordinates. scale_x = (float)src_width / input_w, scale_y likewise (:164-165). A candidate takes part when
 *   confidence >= conf (:116; NaN fails) and confidence > conf (NMSBoxes' own, strict, test); bx = (int)(x * scale) is the fp32
 *   product truncated toward zero (:118-121); class_id = (int)raw[5]. NMSBoxes: stable sort by descending score (ties keep
 *   candidate order), then greedy in that order: a box is kept when 1.f - (float)jaccardDistance(box, k) <= nms for EVERY box k
 *   kept before it -- a suppressed box suppresses nothing. jaccardDistance on Rect(x1, y1, x2 - x1, y2 - y1) in fp64: 0 when
 *   Aa + Ab <= DBL_EPSILON, else 1 - Aab / (Aa + Ab - Aab), the intersection empty when its width or height is <= 0.
 *   Kept boxes are written in that order as aria_detection (corners (float)bx1, by1, bx2, by2); those whose class is in the
 *   dynamic set are also written as aria_box -- the corners mode 0 of aria_flag_keypoints_device expects.
 * Divergences from the reference, both where it is undefined: a candidate with a non-finite coordinate or a scaled
 *   coordinate outside +-2^20 is dropped before NMS (the cast to int is undefined there); areas are exact (cv::Rect::area()
 *   overflows int). class_id saturates at the int range and is 0 for a NaN.
 * Determinism. No float atomics; a frame's rows depend on its own candidates only: reproducible run to run and independent
 *   of the frame's place in the batch and of its neighbours. */
typedef struct aria_det_s* aria_det_t;
/* == aria::core::Detection (include/core/Types.hpp:103-112), 24 bytes */
typedef struct { float x1, y1, x2, y2, confidence; int class_id; } aria_detection;
#define ARIA_DET_MAX_CANDIDATES 1024
#define ARIA_DET_MAX_CLASS_IDS 32
typedef struct {
    int   struct_size;     /* = sizeof(aria_det_config)                                                       */
    int   device;
    void* stream;          /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking: not ordered
                            * against the legacy default stream, see aria_pose_config). The network runs on a stream of the
                            * caller's choice: give the handle THAT stream, or order the three steps with events          */
    int   input_w;         /* network input size (default 640 x 640, TRTInference.cpp:38-40)                  */
    int   input_h;
    int   max_batch;       /* frames per call (default 1)                                                     */
    int   max_candidates;  /* rows of the network's head per frame, <= 1024 (default 300, TRTInference.cpp:105) */
    int   out_half;        /* 0: d_input is fp32 (default), 1: fp16                                           */
    int   reserved;
} aria_det_config;         /* 40 bytes */

void  aria_det_default_config(aria_det_config* cfg);
int   aria_det_create(const aria_det_config* cfg, aria_det_t* out);
void  aria_det_destroy(aria_det_t h);
void* aria_det_stream(aria_det_t h);
/* Synchronises the handle's stream and returns the deferred error of the postprocess calls since the last check, once:
 * ARIA_E_OUTPUT_TOO_SMALL when some frame kept more rows than det_cap or box_cap (its lists were truncated and its counts
 * are the truncated ones); *det_rows_needed / *box_rows_needed (either may be NULL) then tell the largest counts any frame
 * needed since the last check (0 when nothing was truncated on that side). */
int   aria_det_check(aria_det_t h, int* det_rows_needed, int* box_rows_needed);
/* Buffers that belong to the handle, allocated on the first call, for callers without a device allocator of their own (the
 * C++ adapter): max_batch network inputs (3 * input_h * input_w elements each), max_batch * max_candidates * 6 floats of raw
 * head, and max_batch * max_candidates rows of each result list with their counts. Any output pointer may be NULL. */
int   aria_det_device_buffers(aria_det_t h, void** d_input, float** d_raw, aria_detection** d_dets, int** d_ndets,
                              aria_box** d_boxes, int** d_nboxes);
/* TRTInference::preprocess (src/legacy/TRTInference.cpp:68-93) for n_frames images in HBM: frame f at d_images +
 * f * frame_stride, rows row_stride bytes apart (what aria_orb_extract_batch_device reads, as it lies), channels 1 or 3.
 * Writes d_input[f][3][input_h][input_w] (fp32 or fp16; 16-byte aligned for full-width stores). Enqueued on the handle's
 * stream, no synchronisation. Argument errors (channels, n_frames > max_batch, non-positive sizes, sizes above 16384,
 * strides smaller than the rows they hold) are returned before any launch. */
int   aria_det_preprocess_batch_device(aria_det_t h, const uint8_t* d_images, int n_frames, int width, int height,
                                       int row_stride, int64_t frame_stride, int channels, int swap_rb, void* d_input);
/* TRTInference::postprocess (src/legacy/TRTInference.cpp:95-142) for n_frames heads in HBM: frame f's candidates at d_raw +
 * f * n_candidates * 6. class_ids: HOST list of up to 32 dynamic class ids; NULL = the ten of src/main.cpp:29-40;
 * n_class_ids < 0 = every class. Writes frame f's detections at d_dets + f * det_cap and d_ndets[f]; when d_boxes is not NULL
 * the dynamic subset at d_boxes + f * box_cap and d_nboxes[f] -- the layout aria_flag_keypoints_device reads. One workgroup
 * per frame. Enqueued on the handle's stream, no synchronisation; truncation is deferred to aria_det_check. */
int   aria_det_postprocess_batch_device(aria_det_t h, const float* d_raw, int n_frames, int n_candidates, int src_width,
                                        int src_height, float conf, float nms, const int* class_ids, int n_class_ids,
                                        aria_detection* d_dets, int* d_ndets, int det_cap, aria_box* d_boxes, int* d_nboxes,
                                        int box_cap);
/* Blocking host forms on caller-owned host buffers (staged through the handle). image: packed rows of row_stride bytes;
 * input: 3 * input_h * input_w elements. raw: n_candidates * 6 floats; up to det_cap / box_cap rows are written and
 * *n_dets / *n_boxes are the counts NEEDED: ARIA_E_OUTPUT_TOO_SMALL when one exceeds its capacity. boxes / n_boxes may be NULL. */
int   aria_det_preprocess(aria_det_t h, const uint8_t* image, int width, int height, int row_stride, int channels, int swap_rb,
                          void* input);
int   aria_det_postprocess(aria_det_t h, const float* raw, int n_candidates, int src_width, int src_height, float conf, float nms,
                           const int* class_ids, int n_class_ids, aria_detection* dets, int det_cap, int* n_dets,
                           aria_box* boxes, int box_cap, int* n_boxes);
/* The per-axis table of the resize (host-only, no handle, for tests): entry d = first tap | weight of the second tap << 16.
 * Returns the entries written or a negative status. */
int   aria_det_resize_table(int src, int dst, uint32_t* out, int cap);
/* Algorithmic bytes of one preprocessed frame: width * height * channels read + 3 * input_w * input_h * element written. */
int64_t aria_det_algorithmic_bytes(int width, int height, int channels, int input_w, int input_h, int out_half);

/* ---- sparse stereo: a depth per left keypoint of a RECTIFIED stereo pair, and the metric scale of a relative pose. The
 * reference has no stereo code (its roadmap item H19; its EuRoC reader names cam1 and never reads it), so the NumPy
 * restatement aria_slam_amd/stereo_ref.py is the definition and the device equals it bit for bit. Additive to ABI 4.
 *
 * Precondition. Both images are rectified: a scene point lies on the same row of both. Rectification and undistortion are
 *   not part of the stage: see aria_rect_* ("rectification" below), whose output this stage reads. Float parameters of the config are used as fp32; scale[o] is the fp32 level scale of
 *   aria_orb_level_info, with the octave clamped to 0..7.
 * 1. Candidates. For a left keypoint (xL, yL, oL), a right keypoint j = (xR, yR, oR) is a candidate when, in fp32 as
 *   written, |oR - oL| <= max_octave_diff, |yR - yL| <= band_factor * scale[oR] and
 *   xL - max_disparity <= xR <= xL - min_disparity. The best candidate has the least 256-bit Hamming distance, ties to the
 *   lowest j. No candidate, or a best distance >= th_hamming: unmatched.
 * 2. SAD slide on the level-0 images. uL0 = rint(xL), vL0 = rint(yL), uR0 = rint(xR_best), round-half-even. With w =
 *   sad_half_window and L = sad_slide, both (2w+1)^2 windows are centred on row vL0; unmatched when the left window or a
 *   right window at uR0 + inc, inc in [-L, L], leaves the image. SAD(inc) = sum |IL - IR| over the window, exact integers,
 *   no centre normalisation. The best inc has the least SAD, ties to the lowest inc; a best inc at -L or +L is unmatched.
 * 3. Sub-pixel. d1, d2, d3 = SAD(best - 1), SAD(best), SAD(best + 1); den = 2 (d1 + d3 - 2 d2), an integer; den == 0 is
 *   unmatched. delta = (float)(d1 - d3) / (float)den; disparity = (float)(uL0 - uR0 - best) - delta; unmatched unless
 *   min_disparity <= disparity < max_disparity; then disparity = max(disparity, 0.01f), u_right = xL - disparity,
 *   depth = (fx * baseline) / disparity with the product formed once in fp32, X = (xL - cx) * depth / fx,
 *   Y = (yL - cy) * depth / fy -- fp32, in this order, no contraction.
 * 4. Median filter per pair. Over the surviving observations med is the SAD at index n / 2 of the ascending list; those with
 *   (float)sad > median_factor * (float)med become unmatched (strict: a perfectly shifted pair has med = 0 and keeps its
 *   zeros).
 * Outputs per pair. kp_stride records aria_stereo_obs, one per left keypoint (records at and beyond the pair's left count
 *   are written unmatched); an unmatched record holds right_idx = -1, depth = -1 and zero elsewhere; no NaN or Inf is ever
 *   written. And the matched keypoints as aria_match (query_idx = left index, train_idx = right_idx, distance = hamming)
 *   in ascending left index with their count -- the match input of aria_map_triangulate_batch_device with extrinsics
 *   [I|0], [I|(-baseline, 0, 0)].
 * Scale of a relative pose (x2 ~ R x1 + t, |t| = 1, aria_pose_result). Over every match whose mask byte is nonzero and
 *   whose two observations have right_idx >= 0: X1, X2 = the views' (X, Y, depth) as fp64, s_m = t . (X2 - R X1) with R's
 *   rows applied in order and every sum left to right. scale = the value at index n / 2 of the ascending s_m. valid = 0 and
 *   scale = 1.0 when the pose record is invalid (n_used = 0), n_used < min_scale_matches, or scale <= 0.
 * Determinism. No float atomics; bitwise reproducible and independent of the batch split. */
typedef struct aria_stereo_s* aria_stereo_t;
typedef struct {
    int      struct_size;       /* = sizeof(aria_stereo_config)                                                  */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking, as in
                                 * aria_pose_config)                                                              */
    double   fx, fy, cx, cy;    /* intrinsics of the rectified left camera (default EuRoC cam0)                   */
    double   baseline;          /* metres (default 0.110, EuRoC's nominal)                                        */
    double   min_disparity;     /* default 0                                                                      */
    double   max_disparity;     /* default fx: depth >= baseline                                                  */
    double   band_factor;       /* default 2.0, >= 0                                                              */
    double   median_factor;     /* default 2.1, >= 0                                                              */
    int      th_hamming;        /* default 75                                                                     */
    int      sad_half_window;   /* w: default 5, 1..7                                                             */
    int      sad_slide;         /* L: default 5, 1..16                                                            */
    int      max_octave_diff;   /* default 1, >= 0                                                                */
    int      min_scale_matches; /* default 5, >= 1                                                                */
    int      reserved;
} aria_stereo_config;
typedef struct {
    float u_right, disparity, depth, X, Y;
    int   right_idx, hamming, sad;
} aria_stereo_obs;              /* 32 bytes                                                                       */
typedef struct {
    double scale;
    int    n_used, valid;
} aria_stereo_scale;            /* 16 bytes                                                                       */

void  aria_stereo_default_config(aria_stereo_config* cfg);
int   aria_stereo_create(const aria_stereo_config* cfg, aria_stereo_t* out);
void  aria_stereo_destroy(aria_stereo_t h);
void* aria_stereo_stream(aria_stereo_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check, once:
 * ARIA_E_INVALID when some pair's keypoint counts were outside [0, kp_stride] (match: the pair is skipped -- every record
 * unmatched, no matches; the others are unaffected) or, in the scale call, its counts or match indices were out of range
 * (valid = 0, n_used = 0). */
int   aria_stereo_check(aria_stereo_t h);
/* Device-resident batch form over what aria_orb_extract_batch_device leaves in HBM for the left and the right frames.
 * Pair p reads the level-0 images at d_img_left / d_img_right + p*img_stride (W x H bytes, `pitch` bytes per row,
 * W, H <= 4096), keypoints at d_kp_* + p*kp_stride (d_n_*[p] of them) and descriptors at d_desc_* + p*kp_stride*32;
 * writes kp_stride records at d_obs + p*kp_stride, the match list at d_matches + p*match_cap (match_cap >= kp_stride)
 * and d_nmatches[p]. kp_stride <= 8192. Enqueued on the handle's stream, no synchronisation. */
int   aria_stereo_match_batch_device(aria_stereo_t h, const uint8_t* d_img_left, const uint8_t* d_img_right, int64_t img_stride,
                                     int width, int height, int pitch, const aria_keypoint* d_kp_left,
                                     const uint8_t* d_desc_left, const int* d_n_left, const aria_keypoint* d_kp_right,
                                     const uint8_t* d_desc_right, const int* d_n_right, int64_t kp_stride, int n_pairs,
                                     aria_stereo_obs* d_obs, aria_match* d_matches, int* d_nmatches, int match_cap);
/* One pair from host buffers; blocks. obs: n_left records; matches: up to n_left rows, *n_matches = their count. */
int   aria_stereo_match(aria_stereo_t h, const uint8_t* img_left, const uint8_t* img_right, int width, int height, int pitch,
                        const aria_keypoint* kp_left, const uint8_t* desc_left, int n_left, const aria_keypoint* kp_right,
                        const uint8_t* desc_right, int n_right, aria_stereo_obs* obs, aria_match* matches, int* n_matches);
/* Metric scale of n_pairs relative poses, with the pointer and stride conventions of aria_pose_estimate_batch_device: pair p
 * reads d_pose[p], matches at d_matches + p*match_cap (d_nmatches[p]; match_cap <= 8192), the optional mask at
 * d_mask + p*match_cap (NULL = every match) and the stereo observations of the query / train frames at
 * d_obs_query / d_obs_train + p*kp_stride (d_nq[p] / d_nt[p] keypoints); view 1 is the query side when query_is_first = 1.
 * Writes d_out[p]. Enqueued on the handle's stream, no synchronisation. */
int   aria_stereo_scale_batch_device(aria_stereo_t h, const aria_pose_result* d_pose, const uint8_t* d_mask,
                                     const aria_match* d_matches, const int* d_nmatches, int match_cap, int query_is_first,
                                     const aria_stereo_obs* d_obs_query, const int* d_nq, const aria_stereo_obs* d_obs_train,
                                     const int* d_nt, int64_t kp_stride, int n_pairs, aria_stereo_scale* d_out);
/* One pose from host buffers; blocks. Out-of-range match indices: ARIA_E_INVALID. */
int   aria_stereo_scale_pose(aria_stereo_t h, const aria_pose_result* pose, const uint8_t* mask, const aria_match* matches,
                             int n_matches, int query_is_first, const aria_stereo_obs* obs_query, int nq,
                             const aria_stereo_obs* obs_train, int nt, aria_stereo_scale* out);

/* ---- rectification: undistortion and stereo rectification of image batches in HBM, and of keypoints. The reference parses
 * the radtan coefficients of cam0/sensor.yaml and never uses them, and has no stereo rectification, so the NumPy restatement
 * aria_slam_amd/rectify_ref.py is the definition and the device equals it bit for bit. Parity with OpenCV's stereoRectify,
 * initUndistortRectifyMap, remap and fisheye:: functions is not pinned and not claimed. Two distortion models, one per handle
 * (aria_rect_config::model): radtan, dist = k1, k2, p1, p2, k3 (k3 optional, 0), steps 2 and 4; and the fisheye model KB4
 * (Kannala-Brandt with four coefficients: OpenCV's "fisheye", Kalibr's "equidistant"), dist = k1, k2, k3, k4, 0, steps 2k and
 * 4k. KB4 needs atan and tan; rect_atan and rect_tan below build them from + - * / and sqrt, so the bitwise rule holds for both
 * models. Out of scope: Aria's FISHEYE624 (6 radial, 2 tangential and 4 thin-prism coefficients do not fit the 144-byte camera
 * record), KB3, rays at or beyond 90 degrees from the axis (a pinhole destination cannot hold them), cylindrical and
 * equirectangular destinations. Additive to ABI 4.
 *
 * Steps 1, 2 and 4 are fp64 without contraction, use only + - * / and sqrt, and sum left to right. Step 3 is integer.
 * 1. Stereo geometry (host only, aria_rect_stereo_geometry). Inputs: K_l, K_r = (fx, fy, cx, cy) and the row-major 4x4 T_BS
 *   (sensor to body, as in sensor.yaml) of both cameras. T = inverse_rigid(T_BS_r) T_BS_l, so x_r = R x_l + t; R is T's
 *   rotation block after one Gram-Schmidt pass over its rows (row 0 normalised, row 1 less its part along row 0 and
 *   normalised, row 2 their cross product), because sensor.yaml's 12 digits are orthonormal to 1e-12 only. The right
 *   camera centre in the left frame is c = -R^T t; baseline = |c|. With z = (0, 0, 1): e_x = c / |c|,
 *   e_y = (z + R^T z) x e_x normalised, e_z = e_x x e_y (Fusiello's construction: no trigonometry). R1 has the rows e_x, e_y,
 *   e_z; R2 = R1 R^T. The right camera lands at +x: disparities are positive. New intrinsics left zero by the caller become
 *   fx' = fy' = (fy_l + fy_r) / 2 and cx', cy' = the means of the two principal points.
 * 2. Map. For camera c = (fx, fy, cx, cy, dist, R_c) and the destination pixel (u, v): x = (u - cx') / fx',
 *   y = (v - cy') / fy'; (X, Y, Z) = R_c^T (x, y, 1); xn = X / Z, yn = Y / Z, r2 = xn xn + yn yn;
 *   rad = ((k3 r2 + k2) r2 + k1) r2 + 1; xd = xn rad + (2 p1 xn yn + p2 (r2 + 2 xn xn));
 *   yd = yn rad + (p1 (r2 + 2 yn yn) + 2 p2 xn yn); su = fx xd + cx, sv = fy yd + cy; qx = floor(su 32 + 0.5),
 *   qy = floor(sv 32 + 0.5); ix = qx >> 5, iy = qy >> 5. The pixel is invalid when Z <= 0, su or sv is not finite, ix < 0,
 *   iy < 0, ix + 1 > Wsrc - 1 or iy + 1 > Hsrc - 1. A valid entry is the uint32 qx | qy << 16, an invalid one 0xFFFFFFFF.
 *   Sizes: source 2..2047, destination 1..2047 per dimension. Plain undistortion is R_c = I.
 * 3. Pixel. fx5 = qx & 31, fy5 = qy & 31; a, b, c, d = the source bytes at (ix, iy), (ix + 1, iy), (ix, iy + 1),
 *   (ix + 1, iy + 1); out = (a (32 - fx5)(32 - fy5) + b fx5 (32 - fy5) + c (32 - fx5) fy5 + d fx5 fy5 + 512) >> 10. An invalid
 *   pixel takes `fill`.
 * 4. Points. A keypoint's fp32 (x, y) widened to fp64: xd = (x - cx) / fx, yd = (y - cy) / fy; from (xd, yd) exactly 20
 *   iterations of x <- (xd - dx) / rad, y <- (yd - dy) / rad with rad, dx, dy the expressions of step 2 at the current
 *   (x, y); (X, Y, Z) = R_c (x, y, 1); u' = fx' X / Z + cx', v' = fy' Y / Z + cy', both stored as fp32; every other field of
 *   the record is copied. Z <= 0 or a stored value that is not finite: (-1, -1). No NaN or Inf is ever written.
 * KB4. fp64 without contraction, every expression in the order written, fixed loop counts.
 *   rect_atan(r), r >= 0: t = r; three times t = t / (1 + sqrt(1 + t t)); s = t t; p = 1/25; for k = 11 .. 0:
 *   p = 1/(2k+1) - s p (the constants are the fp64 quotients 1.0 / (2k+1)); the result is 8 (t p). A non-finite r gives a
 *   non-finite result. |rect_atan - atan| <= 1e-13 on [0, 1000].
 *   rect_tan(a), 0 <= a < pi/2: h = a 0.125, s = h h; ps = pc = 1; for k = 8 .. 1: ps = 1 - (s / ((2k)(2k+1))) ps and
 *   pc = 1 - (s / ((2k-1)(2k))) pc; t = (h ps) / pc; three times t = (2 t) / (1 - t t). Relative error <= 1e-12 on [0, 1.5].
 *   With q = a a: P(a) = (((k4 q + k3) q + k2) q + k1) q + 1 and D(a) = (((9 k4 q + 7 k3) q + 5 k2) q + 3 k1) q + 1, the
 *   derivative of a P(a).
 * 2k. Map. Step 2 up to xn = X / Z, yn = Y / Z; r = sqrt(xn xn + yn yn), a = rect_atan(r); sc = 1 when r == 0, else
 *   (a P(a)) / r; xd = xn sc, yd = yn sc; su, sv, qx, qy, the bounds and the word as in step 2. The pixel is also invalid when
 *   D(a) <= 0: beyond that angle the polynomial folds back and pixels outside the lens's field would read from inside the image.
 * 4k. Points. xd = (x - cx) / fx, yd = (y - cy) / fy, td = sqrt(xd xd + yd yd); from a = td exactly 10 Newton steps
 *   a = a - (a P(a) - td) / D(a). The point is valid when a is finite, 0 <= a, a < 1.5707963267948966, D(a) > 0 and
 *   |a P(a) - td| <= 1e-9. Then sc = 1 when td == 0, else rect_tan(a) / td; x = xd sc, y = yd sc; rotation, projection, the
 *   fp32 store and the (-1, -1) rule as in step 4. An invalid point is (-1, -1).
 * Determinism. No float atomics; bitwise reproducible and independent of the batch split. */
typedef struct aria_rect_s* aria_rect_t;
enum { ARIA_RECT_MODEL_RADTAN = 0, ARIA_RECT_MODEL_KB4 = 1 };
typedef struct {
    double fx, fy, cx, cy;      /* intrinsics of the raw camera                                                    */
    double dist[5];             /* radtan k1, k2, p1, p2, k3; KB4 k1, k2, k3, k4, 0                                */
    double R[9];                /* rectifying rotation, row-major: x_rect = R x_cam; identity = plain undistortion */
} aria_rect_camera;             /* 144 bytes                                                                       */
typedef struct {
    int      struct_size;       /* = sizeof(aria_rect_config)                                                      */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      src_width, src_height;   /* raw images, 2..2047                                                       */
    int      dst_width, dst_height;   /* undistorted / rectified images, 1..2047                                   */
    int      n_cameras;         /* 1 or 2                                                                          */
    aria_rect_camera cam[2];
    double   new_fx, new_fy, new_cx, new_cy;   /* intrinsics of the destination images, shared by the cameras      */
    int      fill;              /* byte of an invalid pixel, 0..255 (default 0)                                    */
    int      model;             /* ARIA_RECT_MODEL_*, of every camera of the handle (default radtan)               */
} aria_rect_config;             /* 368 bytes                                                                       */

/* EuRoC cam0 at 752x480, plain undistortion (R = I), new K = K, one camera. */
void  aria_rect_default_config(aria_rect_config* cfg);
/* Builds the maps of the cameras on the device. ARIA_E_INVALID for sizes out of range, non-positive or non-finite focal
 * lengths, n_cameras outside 1..2, fill outside 0..255, a model that is neither ARIA_RECT_MODEL_*, KB4 with dist[4] != 0. */
int   aria_rect_create(const aria_rect_config* cfg, aria_rect_t* out);
void  aria_rect_destroy(aria_rect_t h);
void* aria_rect_stream(aria_rect_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check, once:
 * ARIA_E_INVALID when some frame's keypoint count was outside [0, kp_stride] (that frame is skipped, the others are
 * unaffected). */
int   aria_rect_check(aria_rect_t h);
/* Step 1; host only, no handle. K_*: 4 doubles, T_BS_*: 16 doubles row-major. Fills cfg->cam[0].R, cfg->cam[1].R and each
 * of cfg->new_fx, new_fy, new_cx, new_cy that is zero; *baseline (may be NULL) = |c| in the unit of T_BS. */
int   aria_rect_stereo_geometry(const double* K_l, const double* K_r, const double* T_BS_l, const double* T_BS_r,
                                aria_rect_config* cfg, double* baseline);
/* Steps 2-3 over a batch in HBM: frame f of camera `cam` is read at d_src + f*src_stride (`src_pitch` <= 524288 bytes per row) and
 * written at d_dst + f*dst_stride (`dst_pitch` bytes per row, any alignment); bytes outside the dst_width x dst_height
 * pixels are never written. The output is the input layout of aria_orb_extract_batch_device and
 * aria_stereo_match_batch_device. Enqueued on the handle's stream, no synchronisation. */
int   aria_rect_remap_batch_device(aria_rect_t h, int cam, const uint8_t* d_src, int64_t src_stride, int src_pitch, int n_frames,
                                   uint8_t* d_dst, int64_t dst_stride, int dst_pitch);
/* One image from host buffers; blocks. */
int   aria_rect_remap(aria_rect_t h, int cam, const uint8_t* src, int src_pitch, uint8_t* dst, int dst_pitch);
/* Step 4 over what aria_orb_extract_batch_device left for raw images: frame f moves its d_n[f] keypoints at
 * d_kp_in + f*kp_stride to d_kp_out + f*kp_stride (in place allowed; records at and beyond the count are not touched).
 * Enqueued on the handle's stream, no synchronisation. */
int   aria_rect_points_batch_device(aria_rect_t h, int cam, const aria_keypoint* d_kp_in, const int* d_n, int64_t kp_stride,
                                    int n_frames, aria_keypoint* d_kp_out);
/* One frame's keypoints from host buffers; blocks. */
int   aria_rect_points(aria_rect_t h, int cam, const aria_keypoint* kp_in, int n, aria_keypoint* kp_out);
/* Host read-back of a camera's map, dst_width * dst_height entries row by row. Returns the entries written or a negative
 * status (ARIA_E_OUTPUT_TOO_SMALL when cap is less). */
int   aria_rect_get_map(aria_rect_t h, int cam, uint32_t* out, int cap);
/* Algorithmic bytes of one remapped image: one byte read and one written per destination pixel, 2 * W * H. */
int64_t aria_rect_algorithmic_bytes(int dst_w, int dst_h);

/* ---- dense stereo: a disparity for every pixel of a RECTIFIED pair (census + four-path semi-global matching over 64
 * disparities), a depth map, and the stereo observation at each keypoint. The reference has no code for it (the rest of its
 * roadmap item H19), so the NumPy restatement aria_slam_amd/dense_ref.py is the definition and the device equals it bit for
 * bit. Additive to ABI 4.
 *
 * Inputs are two rectified 8-bit images of W x H (aria_rect_*); row y of the left corresponds to row y of the right. D = 64,
 * d in 0..63. Steps 1-7 are integer arithmetic.
 * 1. Census. Window 9 wide, 7 high, the 62 neighbours without the centre, coordinates clamped to the image; a bit is
 *   neighbour < centre. The bit order inside the 64-bit word is not observable.
 * 2. Cost. C(y, x, d) = popcount(cenL(y, x) ^ cenR(y, x - d)) when x - d >= 0, else the constant 64.
 * 3. Aggregation over the four paths left-to-right, right-to-left, top-to-bottom, bottom-to-top with fixed P1, P2. At the
 *   first pixel of a path L_r = C; after it L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d-1) + P1, L_r(q, d+1) + P1, m + P2) - m
 *   with q the previous pixel and m = min_k L_r(q, k); d-1 / d+1 outside 0..63 do not take part. S = the sum over the paths.
 *   1 <= P1 <= P2 <= 127, so L_r <= 64 + P2 fits a byte and S fits 16 bits.
 * 4. Winner. best = argmin_d S(y, x, d), ties to the lowest d.
 * 5. Uniqueness. Invalid when some d with |d - best| > 1 has S(d) * (100 - uniqueness) < S(best) * 100.
 * 6. Left-right check (skipped as a whole when lr_max_diff < 0). dR(y, xr) = argmin over d with xr + d <= W - 1 of
 *   S(y, xr + d, d), ties to the lowest d. Invalid when x - best < 0 or |dR(y, x - best) - best| > lr_max_diff.
 * 7. Sub-pixel in 1/16 px. For 0 < best < 63: den2 = max(S(best-1) + S(best+1) - 2 S(best), 1),
 *   d16 = 16 best + ((S(best-1) - S(best+1)) * 16 + den2) / (2 den2), the division truncating towards zero; d16 = 16 best at
 *   best = 0 and best = 63; an invalid pixel holds -16. One int16 per pixel.
 * 8. Depth, fp32, one rounding per operation: depth = fb / ((float)d16 * 0.0625f) with fb = (float)fx * (float)baseline formed
 *   once; 0 where d16 <= 0. No NaN or Inf is ever written.
 * 9. Keypoint sampling into aria_stereo_obs. u = rint(x), v = rint(y), round-half-even. Unmatched (the sparse stage's
 *   unmatched record, byte for byte) when (u, v) is outside the image or d16(v, u) <= 0; otherwise
 *   disparity = (float)d16 * 0.0625f and u_right, depth, X, Y by the fp32 chain of step 3 of the sparse stage,
 *   right_idx = ARIA_DENSE_NO_KEYPOINT, hamming = 0, sad = 0. Records at and beyond the frame's count are written unmatched.
 * Scratch. Per pair in flight and pixel: two census words (16 B), 64 partial sums of S as uint16 (128 B) and the packed
 *   minimum of step 6 (4 B): 148 * max_width * max_height bytes. pairs in flight = scratch_bytes / that (at most 4096); a batch
 *   of any size runs in groups of that many on the handle's stream.
 * Determinism. The minimum of step 6 is an integer atomic-min on (S << 8 | d): order-independent. No float atomics; bitwise
 *   reproducible and independent of the batch split. */
#define ARIA_DENSE_NO_KEYPOINT 0x7FFFFFFF
typedef struct aria_dense_s* aria_dense_t;
typedef struct {
    int      struct_size;       /* = sizeof(aria_dense_config)                                                    */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    double   fx, fy, cx, cy;    /* intrinsics of the rectified left camera (default EuRoC cam0)                   */
    double   baseline;          /* metres (default 0.110)                                                         */
    int      num_disparities;   /* 64; anything else is ARIA_E_INVALID                                            */
    int      P1, P2;            /* default 8, 32; 1 <= P1 <= P2 <= 127                                            */
    int      uniqueness;        /* default 10, 0..99                                                              */
    int      lr_max_diff;       /* default 1, <= 63; negative = no left-right check                               */
    int      max_width, max_height;   /* default 752 x 480, 1..4096: the largest pair a call may bring            */
    int      reserved;
    int64_t  scratch_bytes;     /* HBM budget for census and S, default 1 GiB                                     */
} aria_dense_config;            /* 96 bytes                                                                       */

void  aria_dense_default_config(aria_dense_config* cfg);
/* ARIA_E_INVALID for a bad field, and for a scratch_bytes that does not hold one pair of max_width x max_height. */
int   aria_dense_create(const aria_dense_config* cfg, aria_dense_t* out);
void  aria_dense_destroy(aria_dense_t h);
void* aria_dense_stream(aria_dense_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check, once:
 * ARIA_E_INVALID when some frame's keypoint count of a sampling call was outside [0, kp_stride] (that frame is skipped:
 * every record unmatched; the others are unaffected). */
int   aria_dense_check(aria_dense_t h);
/* Steps 1-8 over a batch in HBM. Pair p reads its images at d_left / d_right + p*img_stride (`pitch` bytes per row) and
 * writes W x H int16 at d_disp + p*disp_stride and, unless d_depth is NULL, W x H floats at d_depth + p*depth_stride;
 * strides and pitches of the outputs are in elements, and elements outside the W x H pixels are never written.
 * W <= max_width, H <= max_height; W < 64 is legal. Enqueued on the handle's stream, no synchronisation. */
int   aria_dense_compute_batch_device(aria_dense_t h, const uint8_t* d_left, const uint8_t* d_right, int64_t img_stride, int width,
                                      int height, int pitch, int n_pairs, int16_t* d_disp, int64_t disp_stride, int disp_pitch,
                                      float* d_depth, int64_t depth_stride, int depth_pitch);
/* One pair from host buffers; blocks. disp: width * height int16, depth (may be NULL): width * height floats, both dense. */
int   aria_dense_compute(aria_dense_t h, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                         int16_t* disp, float* depth);
/* Step 9 over a batch in HBM: frame f samples the map at d_disp + f*disp_stride at its d_n[f] keypoints at
 * d_kp + f*kp_stride and writes kp_stride records at d_obs + f*kp_stride. kp_stride <= 2^20, n_frames <= 65535. Enqueued on
 * the handle's stream, no synchronisation. */
int   aria_dense_sample_batch_device(aria_dense_t h, const int16_t* d_disp, int64_t disp_stride, int disp_pitch, int width,
                                     int height, const aria_keypoint* d_kp, const int* d_n, int64_t kp_stride, int n_frames,
                                     aria_stereo_obs* d_obs);
/* One frame from host buffers; blocks. disp_pitch in elements; obs: n records. */
int   aria_dense_sample(aria_dense_t h, const int16_t* disp, int width, int height, int disp_pitch, const aria_keypoint* kp, int n,
                        aria_stereo_obs* obs);
/* Pairs the handle keeps in flight (see "Scratch"), or a negative status. */
int   aria_dense_pairs_in_flight(aria_dense_t h);
/* Scratch bytes one pair in flight needs at this size: 148 * width * height. Host only, no handle. */
int64_t aria_dense_scratch_bytes_per_pair(int width, int height);
/* Algorithmic bytes of one pair: both images read, the int16 disparity and the fp32 depth written, 8 * W * H. */
int64_t aria_dense_algorithmic_bytes(int width, int height);

/* ---- dense depth fusion: the fp32 depth maps of aria_dense_* integrated along the trajectory into one truncated signed
 * distance volume in HBM, and the surface points read back out of it. The reference has no code for it (its roadmap items
 * H17, H20 and H22 sit on such a map), so the NumPy restatement aria_slam_amd/tsdf_ref.py is the definition and the device
 * equals it bit for bit. Out of scope: bilinear depth lookup, volume shifting or hashing,
 * and any alert logic (path planning is the stage below; normals and ray casting are the stage "ray casting of the
 * volume"; triangle meshes are the stage "mesh of the volume"). Additive to ABI 4.
 *
 * Unless stated otherwise the arithmetic is fp32, one rounding per operation, no contraction, in exactly the order written.
 * 1. Volume. nx, ny, nz voxels, each a multiple of 8 in 8..1024; `voxel` the edge in metres (> 0); origin[3] the world
 *   corner of voxel (0,0,0); trunc > 0 and inv_trunc = 1.0f / trunc formed once; min_depth <= max_depth; max_weight and
 *   min_weight in 1..65535; fx, fy, cx, cy converted once with (float). One aria_tsdf_voxel of 8 bytes per voxel at the
 *   linear index (k*ny + j)*nx + i, x fastest; cleared = all bytes zero. The centre of voxel (i,j,k) is
 *   c = origin + ((float)i + 0.5f) * voxel per axis.
 * 2. Frame inputs. An fp32 depth map of W x H with a pitch in elements (what aria_dense_compute_batch_device writes);
 *   world-to-camera extrinsics [R|t], 12 doubles row-major (one half of the mapper's d_extrinsics record, x_cam = R X + t),
 *   each converted with (float) once; an optional gray image (`pitch` bytes per row); an optional byte mask per frame, 0 =
 *   skip the frame. An unmasked frame with a non-finite extrinsic is skipped as a whole and defers ARIA_E_INVALID; the
 *   other frames are unaffected.
 * 3. Integration. For each voxel the frames are applied in ascending frame order:
 *   a. xc = ((r00*cX + r01*cY) + r02*cZ) + t0; yc and zc the same from rows 1 and 2.
 *   b. Reject unless zc >= min_depth (a NaN fails every test here and below).
 *   c. iz = 1.0f / zc; u = (fx * xc) * iz + cx; v = (fy * yc) * iz + cy.
 *   d. ur = rintf(u), vr = rintf(v), half-even. Reject unless 0 <= ur <= W-1 and 0 <= vr <= H-1, compared in float; then
 *     ui = (int)ur, vi = (int)vr.
 *   e. D = depth[vi, ui]. Reject unless D >= min_depth and D <= max_depth (drops 0, negatives, NaN and Inf).
 *   f. sdf = D - zc. Reject if sdf < -trunc. s = fminf(1.0f, sdf * inv_trunc).
 *   g. w = (float)weight; tsdf = (tsdf * w + s) / (w + 1.0f); weight = min(weight + 1, max_weight).
 *   h. With an image, in 32-bit integers: g = image[vi, ui], gray = (gray*W0 + g + ((W0 + 1) >> 1)) / (W0 + 1) with W0 the
 *     weight before step g. Without an image gray is untouched.
 *   A rejected voxel-frame changes no byte.
 * 4. Surface points. For voxel a in ascending linear index and axis in 0, 1, 2 (+x, +y, +z), b is the next voxel along
 *   that axis if it is inside the volume. A point is emitted when both weights are >= min_weight and
 *   (tsdf_a < 0) != (tsdf_b < 0), zero counting as non-negative: alpha = tsdf_a / (tsdf_a - tsdf_b); X = c_a with
 *   alpha * voxel added on that axis; gray = alpha < 0.5f ? gray_a : gray_b; weight = min(weight_a, weight_b). The output
 *   order is exactly this order. With a capacity `cap` the first min(total, cap) points are written, the count word
 *   receives total, and total > cap defers ARIA_E_OUTPUT_TOO_SMALL.
 * Determinism. No float atomics; a voxel is owned by one lane, which walks the frames of a call in order. The result is
 *   bitwise independent of how the frames are split into calls and reproducible from run to run. */
typedef struct aria_tsdf_s* aria_tsdf_t;
typedef struct {
    float    tsdf;              /* in units of trunc, [-1, 1]                                                      */
    uint16_t weight;
    uint8_t  gray;
    uint8_t  reserved;          /* always 0                                                                        */
} aria_tsdf_voxel;              /* 8 bytes                                                                         */
typedef struct {
    float    X[3];
    uint8_t  gray;
    uint8_t  axis;              /* 0, 1, 2: the crossing lies between voxel a and its +x, +y, +z neighbour         */
    uint16_t weight;
} aria_tsdf_point;              /* 16 bytes                                                                        */
typedef struct {
    int      struct_size;       /* = sizeof(aria_tsdf_config)                                                     */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      nx, ny, nz;        /* default 256 x 256 x 128; each a multiple of 8 in 8..1024                        */
    int      max_weight;        /* default 64, 1..65535                                                            */
    int      min_weight;        /* default 2, 1..65535: what the extraction asks of both voxels                    */
    int      reserved;
    float    voxel;             /* default 0.05 m                                                                  */
    float    trunc;             /* default 0.20 m                                                                  */
    float    origin[3];         /* default (-6.4, -6.4, 0): the default camera at the world origin looks into it   */
    float    min_depth, max_depth;   /* default 0.3, 10                                                            */
    float    reserved2;
    double   fx, fy, cx, cy;    /* intrinsics of the depth maps (default EuRoC cam0)                               */
} aria_tsdf_config;             /* 104 bytes                                                                       */

void  aria_tsdf_default_config(aria_tsdf_config* cfg);
/* Allocates the volume (aria_tsdf_volume_bytes) once and zeroes it. ARIA_E_INVALID for a bad field, before any device is
 * touched; a volume that does not fit returns the HIP error, before any kernel runs. */
int   aria_tsdf_create(const aria_tsdf_config* cfg, aria_tsdf_t* out);
void  aria_tsdf_destroy(aria_tsdf_t h);
void* aria_tsdf_stream(aria_tsdf_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when some unmasked frame had a non-finite extrinsic (that frame was skipped), else
 * ARIA_E_OUTPUT_TOO_SMALL when an extraction found more points than its capacity. */
int   aria_tsdf_check(aria_tsdf_t h);
/* Every byte of the volume back to zero. Enqueued on the handle's stream, no synchronisation. */
int   aria_tsdf_clear(aria_tsdf_t h);
/* Step 3 over a batch in HBM. Frame f reads its depth map at d_depth + f*depth_stride (`depth_pitch` elements per row, both
 * in elements), its 12 doubles at d_extrinsics + 12*f, its byte at d_frame_mask + f (NULL = every frame) and its image at
 * d_img + f*img_stride (`img_pitch` bytes per row; NULL = gray untouched). width, height in 1..16384, n_frames <= 65535.
 * Every voxel record is read once and written at most once per call, whatever n_frames is. Enqueued on the handle's stream,
 * no synchronisation. */
int   aria_tsdf_integrate_batch_device(aria_tsdf_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int width,
                                       int height, const double* d_extrinsics, const uint8_t* d_frame_mask, const uint8_t* d_img,
                                       int64_t img_stride, int img_pitch, int n_frames);
/* One frame from host buffers; blocks. depth_pitch in elements; img may be NULL. A non-finite extrinsic: ARIA_E_INVALID and
 * the volume untouched. */
int   aria_tsdf_integrate(aria_tsdf_t h, const float* depth, int width, int height, int depth_pitch, const double* extrinsics,
                          const uint8_t* img, int img_pitch);
/* Step 4 into HBM: the first min(total, cap) points at d_points (may be NULL when cap = 0), total at *d_count (device).
 * Records beyond the written ones are not touched. Enqueued on the handle's stream, no synchronisation. */
int   aria_tsdf_extract_points_device(aria_tsdf_t h, aria_tsdf_point* d_points, int64_t cap, int64_t* d_count);
/* The same into host memory; blocks. *total = the points the volume holds; ARIA_E_OUTPUT_TOO_SMALL when cap is less (the
 * first cap points are still written). points may be NULL when cap = 0. */
int   aria_tsdf_extract_points(aria_tsdf_t h, aria_tsdf_point* points, int64_t cap, int64_t* total);
/* The volume in HBM, nx*ny*nz records in the layout of rule 1; valid for the life of the handle. */
aria_tsdf_voxel* aria_tsdf_device_voxels(aria_tsdf_t h);
/* Host read-back of the box [i0, i0+ni) x [j0, j0+nj) x [k0, k0+nk): ni*nj*nk records, x fastest; blocks. */
int   aria_tsdf_read_box(aria_tsdf_t h, int i0, int j0, int k0, int ni, int nj, int nk, aria_tsdf_voxel* out);
/* 8 * nx * ny * nz, or ARIA_E_INVALID for sizes rule 1 refuses. Host only, no handle. */
int64_t aria_tsdf_volume_bytes(int nx, int ny, int nz);
/* Algorithmic bytes of one integration call: every record read and written once (16 B per voxel) and every depth pixel
 * read once per frame (4 B). */
int64_t aria_tsdf_algorithmic_bytes(int nx, int ny, int nz, int width, int height, int n_frames);

/* ---- path planning: a 2-D traversability grid collapsed out of a height band of the volume of aria_tsdf_*, an exact
 * clearance field and an integer cost map, exact cost-to-go fields for a batch of goals, and paths traced for a batch of
 * queries. The reference has no code for it (its roadmap items H20 and H22 sit on such a map), so the NumPy restatement
 * aria_slam_amd/nav_ref.py is the definition and the device equals it bit for bit. Out of scope: 3-D planning, RRT*,
 * any-angle paths or path smoothing, moving obstacles, the alert logic of H22, audio, grids that shift with the camera, and
 * fields split over more than one workgroup. Additive to ABI 4. ("plan" already names the ORB level plan, hence "nav".)
 *
 * All arithmetic is in integers; the one exception is the fp32 compare of rule 2.
 * 1. Grid. The volume geometry nx, ny, nz as in rule 1 of the dense depth fusion: each a multiple of 8 in 8..1024. up_axis
 *   is 0, 1 or 2; the plane axes (U, V) are the other two in ascending order and nu, nv their sizes. Cell (u, v) has the
 *   linear index c = v*nu + u. The band is [band0, band1) on up_axis, 0 <= band0 < band1 <= n_up. A cell's state is a
 *   uint8: 0 FREE, 1 OCCUPIED, 2 UNKNOWN. A new handle holds UNKNOWN cells.
 * 2. Cells from a volume (aria_tsdf_voxel records in that stage's layout). Over the voxels of a cell's column inside the
 *   band, n_seen counts weight >= min_weight and n_solid counts weight >= min_weight && tsdf < occ_tsdf (an fp32 compare).
 *   The cell is OCCUPIED if n_solid >= occ_count, else FREE if n_seen >= free_count, else UNKNOWN. Cells may also be set
 *   from a uint8 array; a value above 2 is ARIA_E_INVALID: the host form refuses the call, the device form defers the error
 *   and leaves the old cells in place.
 * 3. Clearance. R = clear_radius in 0..64, CAP = (R+1)*(R+1). d2(c) is the minimum of du*du + dv*dv over the OCCUPIED cells
 *   with |du| <= R and |dv| <= R inside the grid, CAP when there is none; the grid border is no obstacle. uint16.
 * 4. Cost. blocked(c) when the cell is OCCUPIED, or d2(c) < block_d2, or the cell is UNKNOWN and allow_unknown == 0. Else
 *   pen(c) = (d2 < soft_d2 ? penalty*(soft_d2 - d2)/soft_d2 : 0) + (UNKNOWN ? unknown_penalty : 0) in 32-bit integers with
 *   truncating division. 0 <= block_d2 <= soft_d2 <= CAP, soft_d2 >= 1, penalty and unknown_penalty in 0..1000. The cost
 *   is a uint16, 0xFFFF = blocked. Every path cost stays below 2^31: at most 2^20 cells times a step of at most 14 + 2000.
 * 5. Moves m = 0..7 in this order: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1); base = 10 for m < 4, else
 *   14. A move c -> b is allowed when b is inside the grid and not blocked; a diagonal move also needs (u+du, v) and
 *   (u, v+dv) not blocked (paths do not cut corners). step(c -> b) = base + pen(b).
 * 6. Goal field. For a goal cell g, D is the least solution of D(g) = 0 and D(c) = min over the allowed moves of
 *   step(c -> b) + D(b) for c not blocked; D = 0x7FFFFFFF for blocked and unreachable cells. A goal that is blocked or
 *   outside the grid gives an all-0x7FFFFFFF field; that is no error.
 * 7. Paths. A query is (su, sv, goal_index). Status 2 OUT_OF_GRID: the start is outside the grid, the goal index is outside
 *   [0, G), or that goal was outside the grid. 1 UNREACHABLE: D(start) = 0x7FFFFFFF. 0 OK. 3 TRUNCATED: more cells than
 *   path_cap. For 0 and 3 the path starts at the start cell; from c the next cell is b of the FIRST m in move order that is
 *   allowed and has step(c -> b) + D(b) == D(c); the path ends at g. The record: cost = D(start), n_cells (start and goal
 *   included, the full length even when truncated), min_d2 over the full path, status; for status 1 and 2 cost =
 *   0x7FFFFFFF, n_cells = 0, min_d2 = 0. The cells go to paths[q*path_cap + i] as linear indices: the first
 *   min(n_cells, path_cap) are written and nothing beyond them is touched. Any TRUNCATED query defers
 *   ARIA_E_OUTPUT_TOO_SMALL.
 * Determinism. The least solution of rule 6 is unique, so the device result is bitwise independent of the relaxation
 *   schedule, of the order in which concurrent relaxations see each other's integer updates, and of the run. No float
 *   atomics, no grid-wide barrier; the convergence loop of a field is bounded by nu*nv + 1 rounds, and reaching the bound
 *   defers ARIA_E_OVERFLOW. */
typedef struct aria_nav_s* aria_nav_t;
typedef struct {
    int32_t  cost;              /* D(start), 0x7FFFFFFF for status 1 and 2                                         */
    int32_t  n_cells;           /* the full length of the path, start and goal included                            */
    int32_t  min_d2;            /* the least clearance d2 over the full path                                       */
    int32_t  status;            /* 0 OK, 1 UNREACHABLE, 2 OUT_OF_GRID, 3 TRUNCATED                                 */
} aria_nav_record;              /* 16 bytes                                                                        */
#define ARIA_NAV_OK 0
#define ARIA_NAV_UNREACHABLE 1
#define ARIA_NAV_OUT_OF_GRID 2
#define ARIA_NAV_TRUNCATED 3
#define ARIA_NAV_INF 0x7FFFFFFF
typedef struct {
    int      struct_size;       /* = sizeof(aria_nav_config)                                                      */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      nx, ny, nz;        /* the volume's geometry; default 256 x 256 x 128                                  */
    int      up_axis;           /* default 1: the first camera's y is the world's vertical in this chain           */
    int      band0, band1;      /* default [ny/2 - 8, ny/2 + 16) = [120, 144)                                      */
    int      min_weight;        /* default 2, 1..65535                                                             */
    float    occ_tsdf;          /* default 0: a seen voxel behind the surface is solid                             */
    int      occ_count;         /* default 1, 1..1024                                                              */
    int      free_count;        /* default 1, 1..1024                                                              */
    int      clear_radius;      /* default 8, 0..64 cells                                                          */
    int      block_d2;          /* default 16                                                                      */
    int      soft_d2;           /* default 64                                                                      */
    int      penalty;           /* default 20, 0..1000                                                             */
    int      unknown_penalty;   /* default 10, 0..1000                                                             */
    int      allow_unknown;     /* default 1; 0 = UNKNOWN cells are blocked                                        */
    int      max_goals;         /* default 256, 1..65535: the goals of one solve                                   */
    float    voxel;             /* default 0.05 m: for the world helpers of the bindings only                      */
    float    origin[3];         /* default (-6.4, -6.4, 0)                                                         */
    int      reserved;
} aria_nav_config;              /* 104 bytes                                                                       */

void  aria_nav_default_config(aria_nav_config* cfg);
/* Allocates the grid and the field buffer (aria_nav_field_bytes) once. ARIA_E_INVALID for a bad field, before any device
 * is touched. */
int   aria_nav_create(const aria_nav_config* cfg, aria_nav_t* out);
void  aria_nav_destroy(aria_nav_t h);
void* aria_nav_stream(aria_nav_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when a set_cells_device call held a value above 2, else ARIA_E_OVERFLOW when a field did not settle within
 * its bound (results are not valid), else ARIA_E_OUTPUT_TOO_SMALL when some query was TRUNCATED. */
int   aria_nav_check(aria_nav_t h);
/* Rules 2-4 from a volume in HBM (aria_tsdf_device_voxels of a volume of this geometry). Enqueued on the handle's stream,
 * no synchronisation. */
int   aria_nav_update_from_volume_device(aria_nav_t h, const aria_tsdf_voxel* d_voxels);
/* Rules 3-4 on nu*nv given cells in HBM. Enqueued. */
int   aria_nav_set_cells_device(aria_nav_t h, const uint8_t* d_cells);
/* The same from host memory; blocks. */
int   aria_nav_set_cells(aria_nav_t h, const uint8_t* cells);
/* Host read-back of nu*nv cells, clearances and costs; each blocks. */
int   aria_nav_read_cells(aria_nav_t h, uint8_t* out);
int   aria_nav_read_clearance(aria_nav_t h, uint16_t* out);
int   aria_nav_read_costs(aria_nav_t h, uint16_t* out);
/* Rule 6 for n_goals goals (d_goals: 2*n_goals int32, u then v) into the handle's field buffer, one workgroup per goal.
 * n_goals > max_goals is ARIA_E_INVALID; 0 is accepted. Enqueued. */
int   aria_nav_solve_device(aria_nav_t h, const int32_t* d_goals, int n_goals);
/* Rule 7 for n_queries queries (d_queries: 3*n_queries int32) against the fields of the last solve. d_paths may be NULL when
 * path_cap is 0. A trace after the map changed and before a new solve is ARIA_E_INVALID, refused before anything is
 * enqueued. Enqueued. */
int   aria_nav_trace_device(aria_nav_t h, const int32_t* d_queries, int n_queries, aria_nav_record* d_records, int32_t* d_paths,
                            int path_cap);
/* Solve and trace from host arrays; blocks. Path entries that rule 7 does not write keep the caller's bytes.
 * ARIA_E_OUTPUT_TOO_SMALL when some query was TRUNCATED (records and paths are still written). */
int   aria_nav_plan(aria_nav_t h, const int32_t* goals, int n_goals, const int32_t* queries, int n_queries, aria_nav_record* records,
                    int32_t* paths, int path_cap);
/* The field buffer in HBM: goal g at + g*nu*nv, int32; valid for the life of the handle. */
int32_t* aria_nav_device_fields(aria_nav_t h);
/* Host read-back of the field of goal g of the last solve, nu*nv int32; blocks. */
int   aria_nav_read_field(aria_nav_t h, int g, int32_t* out);
/* The relaxation rounds each of the first n_goals goals of the last solve took (0 for a goal without a field); blocks. */
int   aria_nav_read_rounds(aria_nav_t h, int32_t* out, int n_goals);
/* 4 * nu * nv * max_goals, or ARIA_E_INVALID for sizes the stage refuses. Host only, no handle. */
int64_t aria_nav_field_bytes(int nu, int nv, int max_goals);

/* ---- obstacle alerts: a frame's fp32 depth map (aria_dense_*) and its NMS-ed boxes (aria_det_*) turned into a short,
 * prioritised, non-repeating list of warnings for a person who walks: an exact order statistic of the valid depths inside
 * three image zones and every detection box, a priority from class and distance, and per-key cooldowns that persist along
 * a track. This is the reference's roadmap item H22 ("Depth-based alerts with spatial audio feedback; alert prioritisation
 * by risk + zone + distance with anti-spam cooldowns"). The reference has the port IAudioFeedback
 * (include/interfaces/IAudioFeedback.hpp:7-78, no adapter) and a sketch of the caller, NavigationAudioEngine
 * (docs/milestones/H16_AUDIO_FEEDBACK.md:393-493), with no depth source and no canAnnounce; so the NumPy restatement
 * aria_slam_amd/alert_ref.py is the definition, it restates the sketch's rules wherever the sketch has them, and the
 * device equals it bit for bit. Out of scope: sound synthesis and TTS, traffic-light and sign classification (H22.1-2: a
 * network), tracking of objects across frames, BEHIND, alerts from the volume or the plan, and tuning of the defaults
 * (band, percentiles and zone_alert_m are assumptions nobody has tuned on a recording). Additive to ABI 4.
 *
 * Priorities and directions take the reference's enum values: LOW 0, MEDIUM 1, HIGH 2, CRITICAL 3; CENTER 0, LEFT 1,
 * RIGHT 2 (BEHIND is never produced). The rule arithmetic is integer arithmetic and fp32 compares; the two fp32 divisions of
 * rule 3 and the fp32 product (the division by the width) of rule 1 are formed in fp32 exactly as written.
 * 1. Sources of a frame: up to 64. The config fixes width, height and the row band [zone_top, zone_bottom). Sources 0, 1, 2
 *   are the zones CENTER, LEFT, RIGHT over that band: column x is LEFT when ((float)x + 0.5f) / (float)width < 0.35f, RIGHT
 *   when it is > 0.65f, else CENTER (H16:463-468), in fp32; the host finds the two boundaries once, by that very test
 *   (aria_alert_zone_bounds). Source 3 + i is detection i of the frame, i < min(d_ndets[f], max_dets), max_dets <= 61; the
 *   records are aria_detection as aria_det_postprocess_batch_device writes them (d_dets + f*det_cap). A detection's
 *   rectangle is columns [max(0, (int)x1), min(width, (int)x2)) and rows likewise (Rect(x1, y1, x2-x1, y2-y1)); it is empty
 *   when a corner is non-finite or outside +-2^20. A count outside [0, det_cap] skips the frame's detections and defers
 *   ARIA_E_INVALID. aria_alert_check notes the largest count seen above max_dets (aria_alert_dets_seen).
 * 2. Measurement. The valid depths of a rectangle are those with min_depth <= D <= max_depth (fp32 compares; 0, negatives,
 *   NaN and Inf drop out; 0 < min_depth <= max_depth, finite) in the fp32 depth map, which has a pitch in elements, as
 *   aria_dense_compute_batch_device writes it. With n valid and n >= min_valid, distance is the value at index
 *   k = (n * pct_num) / pct_den of the ascending list (64-bit integers, 0 <= pct_num < pct_den): zones use zone_pct
 *   (default 5/100: the near edge, robust to speckle), detections det_pct (default 1/2: the median). Otherwise there is no
 *   measurement. One 16-byte aria_alert_meas per source slot at d_meas + f*64; a slot that is no source, or has no
 *   measurement, holds distance -1 and k 0. No NaN or Inf is ever written.
 * 3. Candidates. A zone is a candidate when it has a measurement and distance < zone_alert_m; its class_id is -1 and its
 *   direction its zone. A detection is always a candidate: without a measurement its distance is default_depth (5.0f,
 *   H16:437) and the flag NO_DEPTH is set; its direction comes from cx = (x1 + x2) / 2.0f; nrm = cx / (float)width; LEFT
 *   when nrm < 0.35f, else RIGHT when nrm > 0.65f, else CENTER (a NaN gives CENTER). Priority (H16:470-478):
 *   distance < crit_m: CRITICAL; else distance < high_m and dangerous: HIGH; else distance < medium_m: MEDIUM; else LOW.
 *   Dangerous: the class is in the config's list (up to 32 ids, default {0, 1, 2, 3, 5, 7}); class -1 is dangerous when
 *   obstacle_dangerous is set. Flags: BEEP when distance < beep_m (1.5f, H16:453); CRITICAL_ALERT and INTERRUPT when
 *   CRITICAL (H16:404-407).
 * 4. Order inside a frame: descending priority, then ascending distance (fp32 compare), then ascending direction value,
 *   then ascending source index: a strict total order.
 * 5. Cooldowns. A candidate's key is class_key*3 + direction, class_key = 0 for class -1, else 1 + min(max(class_id, 0), 83):
 *   255 keys in a table of 256. A track's state, aria_alert_state, is 2320 bytes; cleared = all zero bytes. Frames of a track
 *   carry int64 timestamps in nanoseconds (EuRoC's own); a timestamp lower than that of the last accepted frame before it in
 *   the call skips the frame and defers ARIA_E_INVALID. Candidates are walked in rule 4's order; one is announced when its key
 *   was never announced, or its priority is above the key's last announced priority, or
 *   t - last_ns[key] >= cooldown_ns[priority] (defaults 2000, 800, 500, 0 ms for LOW..CRITICAL, H16:395-400). At most
 *   max_events_per_frame (default 2) are announced per frame. Announcing stores t and the priority in the key's state.
 * 6. Events. Announced candidates are appended to the track's list (d_events + track*event_cap) as 32-byte
 *   aria_alert_event, in frame order and then rule 4's order; `frame` is the index into the call's frames. d_nevents[track]
 *   receives the total of the call, the first event_cap are written and nothing beyond them is touched; more defers
 *   ARIA_E_OUTPUT_TOO_SMALL, and the state still advances as if all had been written. A track whose offsets are decreasing
 *   or outside [0, n_frames] is skipped (0 events, the state untouched) and defers ARIA_E_INVALID.
 * Determinism. The order statistic is an exact selection on the bit patterns (positive floats order as their bits) by
 *   radix passes over LDS histograms filled by integer atomics: counts are order-independent. No float atomics anywhere.
 *   Results are bitwise reproducible, independent of a frame's place in a batch and, for timestamps that do not decrease, of
 *   how a track is cut into calls (the state does not hold the last timestamp: rule 5's test of it starts afresh with every
 *   call). Tracks may share frames; frames are only read. */
typedef struct aria_alert_s* aria_alert_t;
#define ARIA_ALERT_SOURCES 64
#define ARIA_ALERT_MAX_DETS 61
#define ARIA_ALERT_LOW 0
#define ARIA_ALERT_MEDIUM 1
#define ARIA_ALERT_HIGH 2
#define ARIA_ALERT_CRITICAL 3
#define ARIA_ALERT_CENTER 0
#define ARIA_ALERT_LEFT 1
#define ARIA_ALERT_RIGHT 2
#define ARIA_ALERT_BEEP 1
#define ARIA_ALERT_CRITICAL_ALERT 2
#define ARIA_ALERT_INTERRUPT 4
#define ARIA_ALERT_NO_DEPTH 8
#define ARIA_ALERT_MEAS_SOURCE 1   /* the slot is a source of the frame                                            */
#define ARIA_ALERT_MEAS_OK 2       /* ... and has a measurement                                                    */
typedef struct {
    float    distance;          /* the order statistic, -1 = none                                                  */
    int32_t  n_valid;           /* valid depths inside the rectangle                                               */
    int32_t  k;                 /* the index taken, 0 without a measurement                                        */
    int32_t  flags;             /* ARIA_ALERT_MEAS_*                                                               */
} aria_alert_meas;              /* 16 bytes                                                                        */
typedef struct {
    int32_t  frame, source, class_id, direction, priority;
    float    distance;
    int32_t  flags, reserved;
} aria_alert_event;             /* 32 bytes                                                                        */
typedef struct {
    int64_t  last_ns[256];      /* by key: the timestamp of the last announcement                                  */
    uint8_t  last_prio1[256];   /* by key: its priority + 1, 0 = never                                             */
    int64_t  events_total;      /* announcements over the life of the state                                        */
    int64_t  reserved;
} aria_alert_state;             /* 2320 bytes                                                                      */
typedef struct {
    int      struct_size;       /* = sizeof(aria_alert_config)                                                    */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      width, height;     /* default 752 x 480, 1..8192                                                      */
    int      zone_top, zone_bottom;   /* default [120, 480): 0 <= zone_top < zone_bottom <= height                 */
    int      max_dets;          /* default 32, 0..61                                                               */
    int      min_valid;         /* default 16, >= 1                                                                */
    float    min_depth, max_depth;    /* default 0.1, 20 m                                                         */
    int      zone_pct_num, zone_pct_den;   /* default 5 / 100                                                      */
    int      det_pct_num, det_pct_den;     /* default 1 / 2                                                        */
    float    zone_alert_m;      /* default 3.0                                                                     */
    float    default_depth;     /* default 5.0, finite                                                             */
    float    crit_m, high_m, medium_m, beep_m;   /* default 1.0, 2.0, 3.0, 1.5                                    */
    int      obstacle_dangerous;   /* default 1                                                                    */
    int      n_dangerous;       /* default 6, 0..32                                                                */
    int      dangerous[32];     /* default {0, 1, 2, 3, 5, 7}                                                      */
    int      max_events_per_frame;   /* default 2, 0..64                                                           */
    int      reserved;
    int64_t  cooldown_ns[4];    /* by priority, default 2000, 800, 500, 0 ms; >= 0                                 */
} aria_alert_config;            /* 264 bytes                                                                       */

void  aria_alert_default_config(aria_alert_config* cfg);
/* ARIA_E_INVALID for a bad field (pct_num >= pct_den, max_dets > 61, an empty band, ...), before any device is touched. */
int   aria_alert_create(const aria_alert_config* cfg, aria_alert_t* out);
void  aria_alert_destroy(aria_alert_t h);
void* aria_alert_stream(aria_alert_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when some frame's detection count was outside [0, det_cap], some timestamp decreased or some track's
 * offsets were bad, else ARIA_E_OUTPUT_TOO_SMALL when some track announced more than event_cap events. */
int   aria_alert_check(aria_alert_t h);
/* The largest detection count above max_dets that the calls before the last aria_alert_check met (such a frame used its
 * first max_dets detections), 0 when there was none. */
int   aria_alert_dets_seen(aria_alert_t h);
/* Rules 1-2 over n_frames depth maps in HBM: frame f at d_depth + f*depth_stride, `depth_pitch` elements per row (>= width).
 * d_dets / d_ndets may both be NULL: zones only. Writes 64 records per frame at d_meas. Enqueued on the handle's stream. */
int   aria_alert_measure_batch_device(aria_alert_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int n_frames,
                                      const aria_detection* d_dets, const int* d_ndets, int det_cap, aria_alert_meas* d_meas);
/* Rules 3-6 over n_tracks tracks: track t owns the frames [d_track_offset[t], d_track_offset[t+1]) of the n_frames frames
 * that d_timestamps, d_meas, d_dets and d_ndets describe (d_dets / d_ndets may both be NULL). d_states[t] is read and
 * written in place. Enqueued. */
int   aria_alert_arbitrate_batch_device(aria_alert_t h, const int* d_track_offset, int n_tracks, const int64_t* d_timestamps,
                                        int n_frames, const aria_alert_meas* d_meas, const aria_detection* d_dets, const int* d_ndets,
                                        int det_cap, aria_alert_state* d_states, aria_alert_event* d_events, int event_cap,
                                        int* d_nevents);
/* Both, through a measurement buffer of the handle. Enqueued. */
int   aria_alert_run_batch_device(aria_alert_t h, const float* d_depth, int64_t depth_stride, int depth_pitch, int n_frames,
                                  const aria_detection* d_dets, const int* d_ndets, int det_cap, const int* d_track_offset,
                                  int n_tracks, const int64_t* d_timestamps, aria_alert_state* d_states, aria_alert_event* d_events,
                                  int event_cap, int* d_nevents);
/* The same three over caller-owned host arrays; each blocks and returns what aria_alert_check would. Event slots that
 * rule 6 does not write keep the caller's bytes. */
int   aria_alert_measure(aria_alert_t h, const float* depth, int64_t depth_stride, int depth_pitch, int n_frames,
                         const aria_detection* dets, const int* ndets, int det_cap, aria_alert_meas* meas);
int   aria_alert_arbitrate(aria_alert_t h, const int* track_offset, int n_tracks, const int64_t* timestamps, int n_frames,
                           const aria_alert_meas* meas, const aria_detection* dets, const int* ndets, int det_cap,
                           aria_alert_state* states, aria_alert_event* events, int event_cap, int* nevents);
int   aria_alert_run(aria_alert_t h, const float* depth, int64_t depth_stride, int depth_pitch, int n_frames,
                     const aria_detection* dets, const int* ndets, int det_cap, const int* track_offset, int n_tracks,
                     const int64_t* timestamps, aria_alert_state* states, aria_alert_event* events, int event_cap, int* nevents);
/* out[0] = the first CENTER column, out[1] = the first RIGHT column of rule 1. Host only, no handle. */
int   aria_alert_zone_bounds(int width, int out[2]);
/* Algorithmic bytes of one measurement call: the band's pixels read once (4 B) plus 16 B per source slot, per frame. */
int64_t aria_alert_algorithmic_bytes(int width, int zone_top, int zone_bottom, int n_frames);

/* ---- absolute pose from the point map: a camera pose from 3D-2D correspondences (PnP RANSAC), the step that places a
 * frame in the frame and scale of the map that aria_map_* keeps in HBM -- the two-view stage above fixes |t| = 1 per pair,
 * so chained deltas agree with the map only for the first pair. The reference has no PnP code (its notes name the method:
 * docs/milestones/H04_POSE_ESTIMATION_AUDIT.md section 8); aria_slam_amd/pnp_ref.py is the definition, and parity with
 * OpenCV's solvePnPRansac is not claimed. Batched over pairs; additive to ABI 4.
 *
 * Pose. x_cam = R X + t, world to camera, the map stage's convention; R row-major.
 * Points. x = (u - cx) / fx, y = (v - cy) / fy in fp64. For scoring a pair's points are taken relative to its first
 *   correspondence's X0: d = X - X0 in fp64, rounded to fp32, and (x, y) rounded to fp32 -- a map far from the origin
 *   loses nothing in fp32. A pose is scored as (R, t0 = R X0 + t) rounded to fp32. A correspondence with a scoring value
 *   that is not finite or beyond 1e15 in magnitude never scores; a pose with |t0| beyond 1e15 is invalid (so that every
 *   square of the test below stays finite).
 * Hypotheses. `hypotheses` per pair; the hash of the two-view stage with 6 distinct indices per hypothesis (slots
 *   j = 0..5, at most 256 draws per slot), 4 (slots j = 0..3) with the P3P solver. Results depend on (seed, pair id,
 *   correspondences, solver) only.
 * Solvers. Two minimal solvers, chosen per handle by aria_pnp_set_solver; the default is the 6-point DLT. Each yields one
 *   model and one validity bit per hypothesis; everything from "Inliers" on is the same for both.
 * Minimal solver, DLT. 6-point DLT, one model per sample, fp64. Conditioning in sample order: c = mean of the six X, s = mean
 *   of |X - c| (invalid when s is 0 or not finite), Xh = ((X - c) / s, 1). Rows [Xh, 0, -x Xh] and [0, Xh, -y Xh]; 11 of
 *   the 12 are taken: both rows of sample points 0..4 and the x-row of point 5. Gaussian elimination with partial pivoting
 *   (first row of largest |a|); a pivot with |pivot| <= 1e-9 * max|A_ij| marks the sample invalid. Back substitution with
 *   p11 = 1: after the conditioning p11 is proportional to the depth of the sample's centroid, positive for points in
 *   front of the camera. P = [M | m]; invalid when det M <= 0. M = U S V^T (V from the 3x3 Jacobi of the two-view stage
 *   on M^T M, u_i = M v_i / sigma_i, third columns as cross products); invalid when sigma3 <= 1e-9 sigma1. R = U V^T,
 *   lambda = (s1 + s2 + s3) / 3, t' = m / lambda, t = s t' - R c.
 * Minimal solver, P3P. Sample points 1..3 are solved, point 4 picks among the roots; fp64, and only + - * / and sqrt (no
 *   cbrt, acos or cos: their results cannot be held between host and device); the elimination of Persson and Nordberg's
 *   "Lambda Twist" with fixed iteration counts and a fixed order of candidates.
 *   Setup: unit bearings y_i = (x_i, y_i, 1) / |.|, a_ij = |X_i - X_j|^2 from the differences, b_ij = y_i . y_j; the
 *   unknowns are the distances l_i > 0 with l_i^2 + l_j^2 - 2 b_ij l_i l_j = a_ij. Invalid when
 *   |(X1 - X2) x (X1 - X3)|^2 <= 1e-12 * max(a_ij)^2: collinear or coincident sample points.
 *   Cubic: with M12, M13, M23 the symmetric forms of the three equations, D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23;
 *   det(D1 + g D2) = 0, coefficients from 3x3 determinants (columns of D1 and D2 mixed), invalid when c3 = 0. One real root
 *   of the monic cubic by 30 Newton steps from the inflection point x_i, or, when the derivative's discriminant
 *   D = a^2 - 3 b is positive, from x_i - (2/3) sqrt(D) if f(x_i) > 0 and x_i + (2/3) sqrt(D) otherwise; a step whose
 *   derivative is 0 is not taken.
 *   Rank-2 form: D0 = D1 + g D2; its non-zero eigenvalues from l^2 - tr l + m (m = the sum of the principal 2x2 minors),
 *   the root of larger magnitude as (tr + sign(tr) sqrt(tr^2 - 4 m)) / 2, the other as m / l; each eigenvector the largest
 *   of the three row cross products of D0 - l I (ties to the earliest), normalised. Invalid unless the eigenvalues have
 *   opposite signs; s = sqrt(-l_neg / l_pos), e1 and e2 the eigenvectors of l_pos and l_neg.
 *   Candidates, four slots in this order: (+s, -s) x (first, second root of tau). The plane (e1 - s e2) . l = 0 gives
 *   l1 = w0 l2 + w1 l3; with l3 = tau l2 the first two equations give A tau^2 + B tau + C = 0, solved as
 *   q = -(B + sign(B) sqrt(B^2 - 4 A C)) / 2, tau = q / A, then C / q. A slot is kept when the discriminant is >= 0,
 *   tau > 0, 1 + tau^2 - 2 b23 tau > 0 and l1 > 0, with l2 = sqrt(a23 / (1 + tau^2 - 2 b23 tau)).
 *   Polish: five Newton steps on the three distance equations per slot, the 3x3 system by its adjugate; a step with a zero
 *   determinant is not taken.
 *   Pose: Y_i = l_i y_i; R = [Y1-Y2, Y1-Y3, (Y1-Y2) x (Y1-Y3)] [X1-X2, X1-X3, (X1-X2) x (X1-X3)]^-1 (the inverse from cross
 *   products over |(X1-X2) x (X1-X3)|^2), t = Y1 - R X1.
 *   Choice: Xc = R X4 + t per slot; a slot that is not finite or has Xc.z <= 0 is dropped; the model is the slot with the
 *   least (Xc.x / Xc.z - x4)^2 + (Xc.y / Xc.z - y4)^2, ties to the earliest; no slot left: invalid. One model per
 *   hypothesis is a decision: scoring every root would quadruple the scoring loop. The price: an outlier in slot 4 can
 *   pick the wrong root of an otherwise clean sample.
 * Inliers. In fp32 and division-free: Xc = R d + t0, each component ((r0 dx + r1 dy) + r2 dz) + t0; a point is an inlier
 *   when Xc.z > 0 and (Xc.x - x Xc.z)^2 + (Xc.y - y Xc.z)^2 <= thr2 * Xc.z^2, thr2 = (threshold_px / ((fx + fy) / 2))^2.
 * Winner. Most inliers; ties to the lowest h; an invalid hypothesis scores -1. Integer counts, fixed reduction order.
 * Refinement. When the winner has >= 6 inliers and refine_iters > 0: up to refine_iters Gauss-Newton steps in fp64 on the
 *   normalised reprojection residuals (Xc.x / Xc.z - x, Xc.y / Xc.z - y), Xc = R (X - X0) + t0, over the winner's inlier
 *   set, which is not re-evaluated between steps. It starts from the winner as scored, R replaced by the nearest rotation
 *   (the same U V^T). The update is left-multiplicative: R <- Exp(w) R, t0 <- Exp(w) t0 + v. The 21 + 6 entries of the
 *   normal equations are summed in a fixed order (per thread over its strided share of the correspondences, then a fixed
 *   tree); the 6x6 system is solved by Cholesky in one lane; a pivot that is not positive, or a step that is not finite,
 *   ends the refinement with the last good pose. It stops early when |(w, v)| <= 1e-12. `iterations` is the number of steps
 *   taken. The refined pose is rescored in fp32 and kept (refined = 1) when its count is >= the winner's; otherwise the
 *   result is the winner as scored.
 * Outputs. The mask and n_inliers are those of the kept pose; t = t0 - R X0; rms_px is the RMS of the residuals above
 *   over them, in fp64 in a fixed order, times (fx + fy) / 2.
 * Validity. valid = 0 with fewer than 6 correspondences (4 with P3P), with no valid hypothesis, or when a result field would not be
 *   finite: R = I, t = 0, counts 0, best_hypothesis = -1, zero mask. No field is ever NaN or Inf.
 * Determinism. No float atomics; bitwise reproducible run to run and independent of how pairs are split into calls.
 * Planar scenes. A 6-point DLT is degenerate on a planar sample: every pivot test fails on a planar scene, which yields
 *   valid = 0 with the default solver. A plane is no degeneracy of P3P: select it (aria_pnp_set_solver) where the view
 *   may be a wall, a floor or a table top. It also needs fewer hypotheses: a clean 4-sample at 50 % outliers is a 1 in 16
 *   draw, a clean 6-sample 1 in 64. The refinement still needs 6 inliers, so a pair of 4 or 5 correspondences yields the
 *   winner as scored. */
#define ARIA_PNP_SOLVER_DLT6 0
#define ARIA_PNP_SOLVER_P3P  1
typedef struct aria_pnp_s* aria_pnp_t;
typedef struct {
    double X[3];               /* world point                                                                    */
    float  u, v;               /* pixel                                                                          */
} aria_pnp_corr;               /* 32 bytes                                                                       */
typedef struct {
    double R[9], t[3];         /* x_cam = R X + t                                                                */
    double rms_px;             /* RMS reprojection error of the final inliers                                    */
    int    n_corr, n_inliers, best_hypothesis, iterations, refined, valid;
} aria_pnp_result;             /* 128 bytes                                                                      */
typedef struct {
    int      struct_size;      /* = sizeof(aria_pnp_config)                                                     */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle owns one (non-blocking: NOT ordered against
                                * the legacy default stream, see aria_pose_config)                               */
    int      hypotheses;       /* per pair: multiple of 64, 64..16384 (default 1024)                            */
    int      refine_iters;     /* 0..16 (default 5)                                                              */
    double   fx, fy, cx, cy;   /* intrinsics (default EuRoC cam0)                                                */
    double   threshold_px;     /* default 2.0: the map stage's max_reproj_px, the error a map point was admitted with */
    uint64_t seed;             /* sample hash seed (default 0)                                                   */
} aria_pnp_config;

void  aria_pnp_default_config(aria_pnp_config* cfg);
int   aria_pnp_create(const aria_pnp_config* cfg, aria_pnp_t* out);
void  aria_pnp_destroy(aria_pnp_t h);
void* aria_pnp_stream(aria_pnp_t h);
/* The minimal solver of the calls issued after this one (aria_pnp_estimate, _estimate_batch_device, _debug_hypotheses; the
 * association does not depend on it). A launch parameter: nothing is synchronised, work already enqueued keeps the solver
 * it was issued with. An unknown value: ARIA_E_INVALID, the handle unchanged. A new handle has ARIA_PNP_SOLVER_DLT6. */
int   aria_pnp_set_solver(aria_pnp_t h, int solver);
int   aria_pnp_get_solver(aria_pnp_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check:
 * ARIA_E_INVALID when some pair's count was outside [0, corr_cap] (estimate) or its counts or match indices were out of
 * range (associate). Such a pair is detected before any of its data is read and skipped (n_corr = 0, valid = 0, zero
 * mask; no correspondences); the other pairs are unaffected. */
int   aria_pnp_check(aria_pnp_t h);
/* One pair, host buffers; blocks. pair_base is the pair id the sample hash uses. mask (optional): n bytes. */
int   aria_pnp_estimate(aria_pnp_t h, const aria_pnp_corr* corr, int n, int pair_base, aria_pnp_result* out, uint8_t* mask);
/* Device-resident batch form: pair p reads d_ncorr[p] correspondences at d_corr + p*corr_cap, writes d_out[p] and, if
 * d_mask is not NULL, corr_cap bytes at d_mask + p*corr_cap (zero beyond the pair's correspondences). The sample hash
 * sees pair id pair_base + p. Enqueued on the handle's stream; nothing is synchronised, except when the workspace grows. */
int   aria_pnp_estimate_batch_device(aria_pnp_t h, const aria_pnp_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap,
                                     int pair_base, aria_pnp_result* d_out, uint8_t* d_mask);
/* Test hook: for one pair (host buffers), every hypothesis's 6 sample indices (sample_idx[h*6 + j]; -1 when n < 6; with
 * P3P slots 0..3 hold the sample and slots 4 and 5 are -1), R
 * (R[h*9 + k]) and t0 (t0[h*3 + k]) in fp32 as scored (zero when invalid) and inlier count (counts[h], -1 when invalid). */
int   aria_pnp_debug_hypotheses(aria_pnp_t h, const aria_pnp_corr* corr, int n, int pair_base, int* sample_idx, float* R,
                                float* t0, int* counts);
/* The join that keeps the chain device-resident: correspondences of n_pairs tracked pairs against the map's arena, read
 * with its device-resident size, no host round trip. For pair p the map points used are those with pair == anchor_base + p;
 * anchor_view (1 or 2) says whether their idx1 or idx2 indexes the anchor frame, the train side of pair p's matches
 * (d_matches + p*match_cap, d_nmatches[p] of them; the query keypoints at d_kp_query + p*kp_stride, d_nq[p] of them).
 * Match m yields a correspondence -- X of the map point, the pixel of kp_query[m.query_idx] -- when such a point has that
 * index equal to m.train_idx; of several such points the one at the lowest arena position is taken. Correspondences are
 * written in match order, stably compacted, at d_corr + p*match_cap, their number at d_ncorr[p]; d_corr_match (optional)
 * receives each correspondence's match index at d_corr_match + p*match_cap, so a mask can be carried back. The result
 * is the input of aria_pnp_estimate_batch_device with corr_cap = match_cap. A count outside [0, match_cap] or
 * [0, kp_stride], a query_idx outside [0, d_nq[p]) or a train_idx outside [0, kp_stride) is a deferred error of the pair
 * (d_ncorr[p] = 0). Enqueued on the handle's stream, which must be ordered after the work that filled the map: the call takes
 * the arena's address as it is when called, so a reserve, a growth or a filter of the map between this call and its
 * completion is the caller's error (create both handles on one stream, or check the map first). A map on another device
 * than the handle's: ARIA_E_INVALID. Cost: the call clears and fills a table of n_pairs * kp_stride ints, so kp_stride
 * should be the keypoint capacity, not a generous bound (at most 2^24). */
int   aria_pnp_associate_batch_device(aria_pnp_t h, aria_map_t map, int anchor_base, int anchor_view,
                                      const aria_keypoint* d_kp_query, const int* d_nq, int64_t kp_stride,
                                      const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                      aria_pnp_corr* d_corr, int* d_ncorr, int* d_corr_match);

/* ---- local bundle adjustment: the poses and points of one sliding window refined together against every pixel that saw
 * them -- the step that ties the chain's stages to each other (two-view pose fixes |t| = 1 per pair, the mapper triangulates
 * each pair alone, PnP holds the points fixed, the pose graph never looks at a pixel). The reference has no code for it (its
 * notes name the step: README.md:1162, docs/milestones/H10_POSE_GRAPH_AUDIT.md:501-540); aria_slam_amd/ba_ref.py is the
 * definition, and parity with g2o or Ceres is not claimed. Batched over windows; additive to ABI 4.
 *
 * Window. n_poses <= 16 (ARIA_BA_MAX_POSES) world-to-camera poses [R t], 12 doubles row-major, a fixed byte each; n_points
 *   points X[3] in fp64, a fixed byte each; n_obs records aria_ba_obs sorted strictly ascending by (point, pose): a point's
 *   observations are contiguous, at most 16, without duplicates. Intrinsics fx, fy, cx, cy from the config, fp64.
 * Validity. A window is invalid when a count is negative or beyond its capacity, n_poses > 16, an index is out of range,
 *   the order is not strictly ascending, or a pose, point or pixel is not finite: valid = 0, stop_reason = 2, the other
 *   fields 0, the used mask 0, nothing beyond the records is read, poses and points are left bitwise untouched, and
 *   aria_ba_check reports ARIA_E_INVALID once. The other windows of the batch are unaffected.
 * Residual. Xc = R X + t, r = (fx Xc.x / Xc.z + cx - u, fy Xc.y / Xc.z + cy - v) in pixels, e = |r|. An observation with
 *   Xc.z <= min_depth at the initial state is dropped for the whole call (its byte of the used mask is 0). A trial state at
 *   which a used observation has Xc.z <= min_depth, or whose chi2 is not finite, is rejected.
 * Robust weight. Huber with huber_px = delta (0 = off): w = 1 and the cost e^2 when e <= delta, else w = delta / e and the
 *   cost 2 delta e - delta^2. chi2 = the sum of the costs over the used observations.
 * Updates. Pose: R <- Exp(w) R, t <- Exp(w) t + v, Exp as in the absolute-pose refinement, parameters ordered (w, v).
 *   Point: X <- X + dX. A fixed pose or point gets no update and keeps its bits. A point with fewer than two used
 *   observations is treated as fixed for the call; its observations still constrain their poses.
 * Step. U_i = sum w Jc^T Jc, V_j = sum w Jp^T Jp, W_o = w Jc^T Jp, bc_i = -sum w Jc^T r, bp_j = -sum w Jp^T r; damping
 *   H + lambda I; Vd_j = V_j + lambda I inverted through its 3x3 Cholesky factor; over the free poses
 *   S_ik = [i == k](U_i + lambda I) - sum_j W_ij Vd_j^-1 W_kj^T, g_i = bc_i - sum_j W_ij Vd_j^-1 bp_j, solved by dense
 *   Cholesky of at most 96 x 96; dX_j = Vd_j^-1 (bp_j - sum_i W_ij^T dc_i). A pivot that is not positive rejects the trial.
 * LM control. That of the pose-graph stage above, constants unchanged: lambda0 = 1e-5 * the largest diagonal entry of U over
 *   the free poses and V over the free points, the gain ratio with the denominator dx.(lambda dx + b) + 1e-3, accepted
 *   when rho > 0, the 1/3 clamp, lambda *= ni, ni *= 2 on a rejection, ten rejected trials end the call (stop_reason 1).
 *   rho uses the robust chi2. The LM state restarts per call.
 * Determinism. No float atomics; every sum has a fixed order that depends on the window alone: results are bitwise
 *   reproducible run to run and independent of the window's place in a batch, of the batch's split into calls and of the
 *   number of scratch slots. The summation order is not ba_ref's: the device is held to it by measured tolerances.
 * Out of scope: windows of more than 16 poses or a reduced system outside the LDS; intrinsics or distortion as parameters;
 *   stereo or depth observations; merging duplicate points; writing refined points back into the map arena;
 *   marginalisation and priors; global BA; IMU factors; parity with g2o or Ceres. */
#define ARIA_BA_MAX_POSES 16
typedef struct aria_ba_s* aria_ba_t;
typedef struct {
    int   point, pose;         /* indices into the window's points and poses                                      */
    float u, v;                /* pixel                                                                          */
} aria_ba_obs;                 /* 16 bytes                                                                       */
typedef struct {
    double chi2_initial, chi2_final, lambda;
    double rms_px;             /* over the used observations at the final state, unweighted                      */
    int    n_obs_used, iterations_done, trials;
    int    stop_reason;        /* 0 = iterations done, 1 = ten rejected trials, 2 = invalid window               */
    int    valid, reserved;
} aria_ba_result;              /* 56 bytes; no field is ever NaN or Inf for a valid window                       */
typedef struct {
    int      struct_size;      /* = sizeof(aria_ba_config)                                                      */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle owns one (non-blocking, see aria_pose_config) */
    double   fx, fy, cx, cy;   /* intrinsics (default EuRoC cam0)                                                */
    double   huber_px;         /* default sqrt(5.991); 0 = no robust weight                                      */
    double   min_depth;        /* default 1e-6                                                                   */
    int      max_iterations;   /* 1..100 (default 10): what a call with iterations = 0 runs                      */
    int      max_windows;      /* scratch slots = windows per launch, 1..65535 (default 256); more windows run as
                                * consecutive launches, and the slot count changes no bit of a result            */
} aria_ba_config;

void  aria_ba_default_config(aria_ba_config* cfg);
int   aria_ba_create(const aria_ba_config* cfg, aria_ba_t* out);
void  aria_ba_destroy(aria_ba_t h);
void* aria_ba_stream(aria_ba_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check: ARIA_E_INVALID
 * when some window was invalid (above) or the track builder refused one, else ARIA_E_OUTPUT_TOO_SMALL when the track
 * builder found more points or observations than its capacities. */
int   aria_ba_check(aria_ba_t h);
/* One window, host buffers; blocks. poses_inout: n_poses * 12 doubles, points_inout: n_points * 3, both updated in place.
 * iterations: 1..100, or 0 for the config's. used (optional): n_obs bytes. An invalid window returns ARIA_E_INVALID with
 * *result filled as above. */
int   aria_ba_optimize(aria_ba_t h, double* poses_inout, const uint8_t* pose_fixed, int n_poses, double* points_inout,
                       const uint8_t* point_fixed, int n_points, const aria_ba_obs* obs, int n_obs, int iterations,
                       aria_ba_result* result, uint8_t* used);
/* Device-resident batch form: window b reads d_n_poses[b] poses at d_poses + b*pose_cap*12 with their fixed bytes at
 * d_pose_fixed + b*pose_cap, d_n_points[b] points at d_points + b*point_cap*3 with d_point_fixed + b*point_cap, and
 * d_n_obs[b] observations at d_obs + b*obs_cap; updates poses and points in place; writes d_out[b] and, if d_used is not
 * NULL, obs_cap bytes at d_used + b*obs_cap (zero beyond the window's observations). Enqueued on the handle's stream;
 * nothing is synchronised, except when the workspace grows (it is sized by max_windows, point_cap and obs_cap). */
int   aria_ba_optimize_batch_device(aria_ba_t h, double* d_poses, const uint8_t* d_pose_fixed, double* d_points,
                                    const uint8_t* d_point_fixed, const aria_ba_obs* d_obs, const int* d_n_poses,
                                    const int* d_n_points, const int* d_n_obs, int n_windows, int pose_cap, int point_cap,
                                    int obs_cap, int iterations, aria_ba_result* d_out, uint8_t* d_used);
/* Test hook: one window (host buffers) linearised at its state and damped with `lambda`. chi2, n_obs_used; with F free
 * poses in pose order, S (6F x 6F, row-major, both triangles) and g (6F); V (n_points * 9) and bp (n_points * 3) of every
 * point over its used observations. */
int   aria_ba_debug_linearize(aria_ba_t h, const double* poses, const uint8_t* pose_fixed, int n_poses, const double* points,
                              const uint8_t* point_fixed, int n_points, const aria_ba_obs* obs, int n_obs, double lambda,
                              double* chi2, int* n_obs_used, double* S, double* g, double* V, double* bp);

/* The track builder: windows of points and observations from what the batch chain leaves in HBM, equal to
 * ba_ref.window_from_chain bit for bit (integers and copies only). The chain is n_chain_pairs pairs with ids pair_base + q,
 * their keypoints at d_kp1 + q*kp_stride (view 1, d_n1[q] of them) and d_kp2 + q*kp_stride (view 2), their matches at
 * d_matches + q*match_cap (d_nmatches[q]; query_is_first says which side of a match indexes view 1), as
 * aria_map_triangulate_batch_device took them. Precondition: view 2 of pair q is the same extraction as view 1 of pair
 * q + 1. Window b covers the pairs d_pair_first[b] .. + d_n_pairs[b] - 1 (1..15 pairs, inside the chain): frame f is view 1
 * of pair d_pair_first[b] + f, the last frame view 2 of the last pair. Its points are the arena's points whose pair lies in
 * the window, in arena order; a point of pair p yields the observations (f, pixel of view-1 keypoint idx1), (f + 1, pixel of
 * view-2 keypoint idx2) and then, for each later pair of the window, the match whose view-1 index equals the index carried
 * so far -- the lowest match index of several -- which adds that pair's view-2 pixel and carries its view-2 index on; the
 * first pair without such a match ends the track. Observations come out sorted. Written: X at d_points + b*point_cap*3,
 * observations at d_obs + b*obs_cap, each point's arena position at d_point_src + b*point_cap, d_n_points[b], d_n_obs[b].
 * A window outside the chain, a count out of range or an index out of range is a deferred ARIA_E_INVALID of the window, more
 * points or observations than the capacities a deferred ARIA_E_OUTPUT_TOO_SMALL; either way its counts are 0. Enqueued on
 * the handle's stream, which must be ordered after the work that filled the map (the rule of
 * aria_pnp_associate_batch_device); a map on another device than the handle's: ARIA_E_INVALID. The same physical point
 * triangulated in two pairs stays two points. */
int   aria_ba_window_from_chain_device(aria_ba_t h, aria_map_t map, const int* d_pair_first, const int* d_n_pairs, int n_windows,
                                       int pair_base, int n_chain_pairs, const aria_keypoint* d_kp1, const int* d_n1,
                                       const aria_keypoint* d_kp2, const int* d_n2, int64_t kp_stride,
                                       const aria_match* d_matches, const int* d_nmatches, int match_cap, int query_is_first,
                                       int point_cap, int obs_cap, double* d_points, aria_ba_obs* d_obs, int* d_point_src,
                                       int* d_n_points, int* d_n_obs);

/* ---- ray casting of the volume: a ray per pixel marched through the aria_tsdf_voxel records of the dense depth fusion, the
 * zero crossing refined on the trilinear interpolant and that interpolant differentiated: a predicted fp32 depth map at a
 * pose (what aria_alert_measure_batch_device and aria_tsdf_integrate_batch_device read), world-frame normals, the fused gray
 * and a head-light shade, batched over views. The reference has no code for it (its roadmap item H21 is a 3-D viewer), so the
 * NumPy restatement aria_slam_amd/ray_ref.py is the definition and the device equals it bit for bit. The stage owns no
 * volume: it is handed the records in HBM with their geometry. Out of scope: meshes (the stage "mesh of the volume"), adaptive step lengths, colour, shadows
 * or any second light, frame-to-model ICP (this stage makes it possible; it is the follow-up), and a volume that changes
 * between aria_ray_update_from_volume_device and a cast. Additive to ABI 4.
 *
 * All arithmetic is fp32, one rounding per operation, no contraction, in exactly the order written. A NaN fails every
 * comparison. lerp(a, b, w) means a + w * (b - a).
 * 1. Geometry and configuration. nx, ny, nz, voxel, origin[3], min_weight as in rule 1 of the dense depth fusion, with the
 *   same validity ranges. The records' tsdf values must not be infinite (the fusion writes values in [-1, 1]): with an
 *   infinite tsdf the depth of a hit can be a NaN, whose bits are not defined, and `nearest` of its view is then not defined
 *   either. inv_voxel = 1.0f / voxel. fx, fy, cx, cy are doubles converted once with (float); inv_fx = 1.0f / fx,
 *   inv_fy = 1.0f / fy. near > 0, far >= near, step > 0, all finite. n_steps = (int)floorf((far - near) / step) + 1 must lie
 *   in 1..8192.
 * 2. View. World-to-camera [R|t], 12 doubles row-major, each converted with (float) once (the record
 *   aria_tsdf_integrate_batch_device reads). The camera centre per world axis a, with r0a, r1a, r2a column a of R:
 *   o_a = -((r0a*t0 + r1a*t1) + r2a*t2); in grid units og_a = (o_a - origin_a) * inv_voxel - 0.5f. Views may carry a byte
 *   mask: a view whose byte is 0 is skipped, and nothing of it is written, its record included. An unmasked view with a
 *   non-finite extrinsic writes zeros to every requested output and valid = 0 to its record, and defers ARIA_E_INVALID; the
 *   other views are unaffected.
 * 3. Pixel (u, v), integers in [0, W) x [0, H): a = ((float)u - cx) * inv_fx; b = ((float)v - cy) * inv_fy;
 *   d_a = (r0a*a + r1a*b) + r2a; dg_a = d_a * inv_voxel. The ray is parameterised by the camera depth z, what the depth maps
 *   of aria_dense_* hold and what the integration compares against.
 * 4. Sample k. z_k = near + (float)k * step, formed from k, never accumulated. g_a = og_a + z_k * dg_a; r_a = rintf(g_a),
 *   half-even. The sample is inside when 0 <= r_a <= n_a - 1 on all three axes, compared in float; its voxel is then
 *   ((int)r_x, (int)r_y, (int)r_z). It is seen when inside and weight >= min_weight.
 * 5. Walk. k runs from 0 to n_steps - 1, ascending. The first k whose sample is seen with tsdf < 0 ends the walk. It is a
 *   hit when k >= 1 and sample k-1 is seen with tsdf >= 0; otherwise a miss (a back face, or a start inside a surface). No
 *   such k is also a miss. A miss writes depth 0.0f, normal (0, 0, 0), gray 0, shade 0.
 * 6. Trilinear value T(z). g as in rule 4; b_a = floorf(g_a); f_a = g_a - b_a. T is defined when 0 <= b_a and
 *   b_a + 1.0f <= n_a - 1 on all three axes and all eight voxels b + {0,1}^3 have weight >= min_weight; t_xyz are their tsdf
 *   values. c00 = lerp(t000, t100, f_x), c10 = lerp(t010, t110, f_x), c01 = lerp(t001, t101, f_x), c11 = lerp(t011, t111, f_x);
 *   c0 = lerp(c00, c10, f_y), c1 = lerp(c01, c11, f_y); T = lerp(c0, c1, f_z).
 * 7. Refinement of a hit at k. F0 = T(z_{k-1}), F1 = T(z_k). If both are defined and F0 >= 0 && F1 <= 0 && F0 > F1 then
 *   A = F0, B = F1; otherwise A = tsdf_{k-1}, B = tsdf_k, the nearest-voxel values of rule 5, for which A - B > 0 always
 *   holds. alpha = A / (A - B); depth = z_{k-1} + alpha * step.
 * 8. Gray. alpha < 0.5f ? gray_{k-1} : gray_k, of the nearest voxels of rule 5 (the extraction's rule).
 * 9. Normal, in the world frame, pointing to the free side. Take the cell of rule 6 at z = depth with its f and c**; if that
 *   cell is not defined the normal is 0. Gx = lerp(lerp(t100 - t000, t110 - t010, f_y), lerp(t101 - t001, t111 - t011, f_y),
 *   f_z); Gy = lerp(c10 - c00, c11 - c01, f_z); Gz = c1 - c0; len = sqrtf((Gx*Gx + Gy*Gy) + Gz*Gz). If len > 0,
 *   n = (Gx/len, Gy/len, Gz/len), else n = 0. The gradient is that of ONE cell's interpolant and therefore discontinuous
 *   across cells: neighbouring pixels on either side of a cell face can differ by the jump of the one-sided differences.
 * 10. Shade, a head-light Lambert term. With a non-zero normal dl = sqrtf((d_x*d_x + d_y*d_y) + d_z*d_z),
 *   c = fabsf((n_x*d_x + n_y*d_y) + n_z*d_z) / dl, shade = (uint8_t)rintf(fminf(255.0f, 255.0f * c)); otherwise 0.
 * 11. View record aria_ray_view: n_hit; n_ended, the walks that ended at a seen negative sample, hit or not; nearest, the
 *   least hit depth, 0.0f without a hit; valid. The counts and the minimum are taken with integer operations (the minimum on
 *   the bit pattern of the positive float); no float atomics.
 * Outputs per view, each pointer NULL = that plane is not written, each with its own stride per view and pitch per row, in
 *   elements: fp32 depth; fp32 normals, three floats per pixel interleaved (stride in floats, pitch in pixels); uint8 gray;
 *   uint8 shade. Elements outside W x H are never written.
 * Determinism. One writer per pixel. The result is bitwise independent of batch position, of the split into calls, of
 *   `skip` and of the run.
 * Known limit. Where the trilinear pair of rule 7 does not bracket the crossing that the nearest-voxel walk found -- in a
 *   grid-aligned view whose samples fall on the crossing itself this is the common case -- rule 7 falls back to the
 *   nearest-voxel values, which costs up to about half a step of depth error (DESIGN.md section 26 has the measured
 *   figures). */
typedef struct aria_ray_s* aria_ray_t;
typedef struct {
    int32_t  n_hit;
    int32_t  n_ended;           /* walks that ended at a seen negative sample, hit or not                          */
    float    nearest;           /* the least hit depth, 0.0f without a hit                                         */
    int32_t  valid;             /* 0: a non-finite extrinsic                                                       */
} aria_ray_view;                /* 16 bytes                                                                        */
#define ARIA_RAY_DEPTH 1
#define ARIA_RAY_NORMAL 2
#define ARIA_RAY_GRAY 4
#define ARIA_RAY_SHADE 8
typedef struct {
    int      struct_size;       /* = sizeof(aria_ray_config)                                                      */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      nx, ny, nz;        /* the volume's geometry; default 256 x 256 x 128                                  */
    int      min_weight;        /* default 2, 1..65535                                                             */
    int      skip;              /* default 1: no record load in a brick of 8 x 8 x 8 voxels that cannot end a walk; */
                                /* 0 = every sample loads its record. The same bytes either way.                   */
    float    voxel;             /* default 0.05 m                                                                  */
    float    origin[3];         /* default (-6.4, -6.4, 0)                                                         */
    float    near, far, step;   /* default 0.3, 10, 0.05 (= voxel): 195 samples                                    */
    double   fx, fy, cx, cy;    /* intrinsics of the views (default EuRoC cam0)                                    */
} aria_ray_config;              /* 96 bytes                                                                        */

void  aria_ray_default_config(aria_ray_config* cfg);
/* ARIA_E_INVALID for a bad field (n_steps outside 1..8192 included), before any device is touched. */
int   aria_ray_create(const aria_ray_config* cfg, aria_ray_t* out);
void  aria_ray_destroy(aria_ray_t h);
void* aria_ray_stream(aria_ray_t h);
/* Synchronises the handle's stream and returns, once, the deferred ARIA_E_INVALID of an unmasked view with a non-finite
 * extrinsic since the last check. */
int   aria_ray_check(aria_ray_t h);
/* Remembers d_voxels (nx*ny*nz records in the layout of rule 1 of the dense depth fusion, aria_tsdf_device_voxels of a volume
 * of this geometry) and builds the skip words from them: one bit per brick of 8 x 8 x 8 voxels, set when the brick holds a
 * voxel with weight >= min_weight && tsdf < 0. The records must stay where they are, and unchanged, until the casts that
 * follow have run; after the volume changed, update again. Enqueued on the handle's stream, no synchronisation. */
int   aria_ray_update_from_volume_device(aria_ray_t h, const aria_tsdf_voxel* d_voxels);
/* Rules 2-11 for n_views views of width x height. View f reads its 12 doubles at d_extrinsics + 12*f and its byte at
 * d_view_mask + f (NULL = every view), and writes depth at d_depth + f*depth_stride + v*depth_pitch + u, its normal at
 * d_normal + f*normal_stride + 3*(v*normal_pitch + u), gray and shade like depth, and its record at d_views + f; every
 * output pointer, d_views included, may be NULL. width, height in 1..16384, n_views in 0..65535, a pitch at least the width
 * and, for n_views > 1, a stride that holds a view. A cast before the first update is ARIA_E_INVALID, refused before
 * anything is enqueued. Enqueued on the handle's stream, no synchronisation. */
int   aria_ray_cast_batch_device(aria_ray_t h, const double* d_extrinsics, const uint8_t* d_view_mask, int n_views, int width,
                                 int height, float* d_depth, int64_t depth_stride, int depth_pitch, float* d_normal,
                                 int64_t normal_stride, int normal_pitch, uint8_t* d_gray, int64_t gray_stride, int gray_pitch,
                                 uint8_t* d_shade, int64_t shade_stride, int shade_pitch, aria_ray_view* d_views);
/* One view into dense host buffers (width*height elements each, 3*width*height for the normals; any may be NULL); blocks.
 * A non-finite extrinsic returns ARIA_E_INVALID, with zeros in the outputs. */
int   aria_ray_cast(aria_ray_t h, const double* extrinsics, int width, int height, float* depth, float* normal, uint8_t* gray,
                    uint8_t* shade, aria_ray_view* view);
/* The bytes one cast writes: (4, 12, 1, 1 per pixel for the planes of the ARIA_RAY_* bit set `planes`) * width * height
 * + 16, times n_views; ARIA_E_INVALID for sizes the cast refuses. Host only, no handle. */
int64_t aria_ray_algorithmic_bytes(int width, int height, int n_views, int planes);

/* ---- frame-to-model tracking: batched point-to-plane ICP of a live fp32 depth map (what aria_dense_compute_batch_device
 * writes) against the depth map and world-frame normals aria_ray_cast_batch_device predicted from the volume, which corrects
 * the pose the frame is then integrated at. The reference has no code for it (KinectFusion's tracking step, under its roadmap
 * items H17 and H21), so the NumPy restatement aria_slam_amd/icp_ref.py is the definition and the device equals it bit for
 * bit. Out of scope: a live-normal or angle compatibility test, Huber or any other weights, colour / photometric terms, depth
 * pyramids (levels are strides on the full-resolution maps) and a motion model. Additive to ABI 4.
 *
 * Unless stated otherwise all arithmetic is fp32, one rounding per operation, no contraction, in exactly the order written. A
 * NaN fails every comparison.
 * Inputs per frame f: the live depth map D of W x H; the model view as the ray casting stage wrote it: depth M (0 = miss),
 *   interleaved normals N in the world frame (zero = none) and the 12 doubles Tm (world to model camera) it was cast at; a
 *   guess T0, 12 doubles, world to live camera (usually Tm itself); an optional byte mask. fx, fy, cx, cy are doubles converted
 *   once with (float); inv_fx = 1.0f / fx, inv_fy = 1.0f / fy.
 * 1. State. Trel = Tm o T0^-1, live camera to model camera, formed once in fp64: Rrel_ij = (Rm_i0*R0_j0 + Rm_i1*R0_j1) +
 *   Rm_i2*R0_j2; trel_i = tm_i - ((Rrel_i0*t0_0 + Rrel_i1*t0_1) + Rrel_i2*t0_2). Its 12 doubles are converted with (float)
 *   for the per-pixel work of each iteration, and Rm with (float) once. No world coordinate appears per pixel: a map 1 km from
 *   the origin loses nothing.
 * 2. Levels. Level l uses the live pixels with u % s == 0 && v % s == 0, s = stride[l], a power of two <= 16; it runs
 *   iterations[l] in 0..64 iterations; at most 4 levels, at least one iteration in all (default strides 4, 2, 1 with 4, 5,
 *   10 iterations). The model maps are always read at full resolution.
 * 3. Correspondence of the live pixel (u, v) with depth D, valid when min_depth <= D <= max_depth.
 *   p = ((((float)u - cx) * inv_fx) * D, (((float)v - cy) * inv_fy) * D, D); q_i = ((r_i0*p_x + r_i1*p_y) + r_i2*p_z) + t_i
 *   with the fp32 Trel. Reject unless q_z > 0. iz = 1.0f / q_z; um = rintf((fx*q_x)*iz + cx), vm = rintf((fy*q_y)*iz + cy),
 *   half-even; reject unless 0 <= um <= W - 1 and 0 <= vm <= H - 1, compared in float. Mz = M[vm, um], Nw = N[vm, um]: reject
 *   unless Mz > 0 and some component of Nw != 0. n_i = (Rm_i0*Nw_0 + Rm_i1*Nw_1) + Rm_i2*Nw_2; reject unless
 *   (n_0*n_0 + n_1*n_1) + n_2*n_2 <= 1.5f (the normals of the ray casting stage have length 1; the bound is what makes the
 *   proof of rule 4 hold for any input). pm = (((um - cx) * inv_fx) * Mz, ((vm - cy) * inv_fy) * Mz, Mz); e = q - pm; reject
 *   unless (e_0*e_0 + e_1*e_1) + e_2*e_2 <= dist_max*dist_max and (q_0*q_0 + q_1*q_1) + q_2*q_2 <= reach*reach. Residual
 *   r = (n_0*e_0 + n_1*e_1) + n_2*e_2. J = (q x n, n): c_0 = q_1*n_2 - q_2*n_1, c_1 = q_2*n_0 - q_0*n_2,
 *   c_2 = q_0*n_1 - q_1*n_0, each two products and one difference.
 * 4. The system, in integers. Per frame and iteration 29 int64 sums over the correspondences: [0..20] J_i*J_j for i <= j, row
 *   by row; [21..26] J_i*r; [27] r*r; [28] the count. Each product is formed in fp64, where the product of two fp32 values is
 *   exact, multiplied by 2^24, 2^30 and 2^36 for the three groups (exact), rounded half-even to int64 and added. Integer
 *   addition is associative: the sums do not depend on schedule, grid, wave order or atomics.
 *   No overflow: a component of q x n is at most |q| |n| <= reach * sqrt(1.5) * (1 + 2^-20) <= 156.8 for reach <= 128, and
 *   those of n are smaller, so |J_i*J_j| * 2^24 < 2^38.6; |r| <= |n| |e| <= 1.225 (1 + 2^-20) for dist_max <= 1, so
 *   |J_i*r| * 2^30 < 2^37.6 and r*r * 2^36 < 2^36.6. With W*H <= 2^24 terms every sum stays below 2^62.6 < 2^63. Hence the
 *   validity ranges dist_max <= 1, reach <= 128, W*H <= 2^24. (A term is also an integer below 2^53 in fp64, so a kernel may
 *   add up to 2^14 of them exactly in fp64 before it converts: aria_slam_amd/csrc/icp_track.hip does.)
 * 5. Solve, fp64, scalar operations in this order. A_ij = (double)S / 2^24, b_i = (double)S / 2^30 (the conversion rounds to
 *   nearest even above 2^53); count = S[28]; rms = sqrt(((double)S[27] / 2^36) / (double)count), 0 for count 0. The frame is
 *   LOST when count < min_corr, or at the first Cholesky pivot that is not > min_pivot * (double)count. Cholesky by columns
 *   j = 0..5: s = A_jj, then s = s - L_jm*L_jm for m = 0..j-1; the pivot is s; L_jj = sqrt(s); for i = j+1..5: s = A_ji, then
 *   s = s - L_im*L_jm for m = 0..j-1; L_ij = s / L_jj. Forward: s = -b_i, s = s - L_im*y_m for m = 0..i-1, y_i = s / L_ii.
 *   Back, i = 5..0: s = y_i, s = s - L_mi*x_m for m = i+1..5, x_i = s / L_ii. delta = x;
 *   |delta| = sqrt(((((x0*x0 + x1*x1) + x2*x2) + x3*x3) + x4*x4) + x5*x5). The rotation increment is the Cayley map of
 *   w = delta[0:3], rational, so that the solve uses only + - * / sqrt: a = 0.5 * w, s = (a0*a0 + a1*a1) + a2*a2,
 *   Rinc_ii = ((1 - s) + 2*(a_i*a_i)) / (1 + s), Rinc_ij = (2*(a_i*a_j) + 2*K_ij) / (1 + s) with K = [a]x. Then
 *   Trel <- [Rinc | delta[3:6]] o Trel: R_ij = (Rinc_i0*R_0j + Rinc_i1*R_1j) + Rinc_i2*R_2j, t_i = ((Rinc_i0*t_0 + Rinc_i1*t_1)
 *   + Rinc_i2*t_2) + delta_{3+i}. A frame whose |delta| < eps after its update skips the rest of its level. A lost frame keeps
 *   T0 and stops.
 * 6. Output per frame: T = Trel^-1 o Tm, 12 doubles: R_ij = (Rrel_0i*Rm_0j + Rrel_1i*Rm_1j) + Rrel_2i*Rm_2j,
 *   t_i = (Rrel_0i*d_0 + Rrel_1i*d_1) + Rrel_2i*d_2 with d = tm - trel; a lost frame's T is T0. The record aria_icp_result:
 *   valid; iterations_run, the accumulations solved, a losing one included; n_corr, rms and delta = |delta| (0 when lost) of
 *   the last of them, and the level it belonged to. A frame whose mask byte is 0 writes nothing. An unmasked frame with a
 *   non-finite Tm or T0 writes a zero record (valid = 0), no pose, and defers ARIA_E_INVALID; the other frames are unaffected.
 * Determinism. The result is bitwise independent of batch position, of the split into calls, of the schedule and of the run. */
typedef struct aria_icp_s* aria_icp_t;
typedef struct {
    int32_t  valid;             /* 0: lost (rule 5) or a non-finite pose                                           */
    int32_t  iterations_run;
    int32_t  n_corr;            /* correspondences of the last accumulation                                        */
    int32_t  level;             /* the level the last accumulation belonged to                                     */
    double   rms;               /* sqrt(sum r^2 / n_corr) of the last accumulation, in metres                      */
    double   delta;             /* |delta| of the last solve, 0 when it lost the frame                             */
} aria_icp_result;              /* 32 bytes                                                                        */
#define ARIA_ICP_MAX_LEVELS 4
#define ARIA_ICP_TERMS 29
typedef struct {
    int      struct_size;       /* = sizeof(aria_icp_config)                                                      */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    double   fx, fy, cx, cy;    /* intrinsics of the live and the model maps (default EuRoC cam0)                  */
    float    min_depth, max_depth;   /* default 0.3, 10; 0 < min_depth <= max_depth                                */
    float    dist_max;          /* default 0.1 m, in (0, 1]                                                        */
    float    reach;             /* default 64 m, in (0, 128]                                                       */
    int      min_corr;          /* default 64, 1..2^24                                                             */
    int      n_levels;          /* default 3, 1..4                                                                 */
    double   min_pivot;         /* default 5e-6, >= 0: measured, DESIGN.md section 27                              */
    double   eps;               /* default 1e-6, >= 0                                                              */
    int      stride[ARIA_ICP_MAX_LEVELS];       /* default 4, 2, 1                                                 */
    int      iterations[ARIA_ICP_MAX_LEVELS];   /* default 4, 5, 10                                                */
} aria_icp_config;              /* 120 bytes                                                                       */

void  aria_icp_default_config(aria_icp_config* cfg);
/* ARIA_E_INVALID for a bad field, before any device is touched. */
int   aria_icp_create(const aria_icp_config* cfg, aria_icp_t* out);
void  aria_icp_destroy(aria_icp_t h);
void* aria_icp_stream(aria_icp_t h);
/* Synchronises the handle's stream and returns, once, the deferred ARIA_E_INVALID of an unmasked frame with a non-finite
 * pose since the last check. */
int   aria_icp_check(aria_icp_t h);
/* Rules 1-6 for n_frames frames of width x height. Frame f reads its live depth at d_depth + f*depth_stride + v*depth_pitch + u,
 * the model depth likewise, the model normal at d_model_normal + f*normal_stride + 3*(v*normal_pitch + u) (strides and pitches
 * in elements; the normals: stride in floats, pitch in pixels), its 12 doubles at d_model_extrinsics + 12*f and d_guess + 12*f
 * and its byte at d_mask + f (NULL = every frame); it writes 12 doubles at d_extrinsics_out + 12*f and its record at
 * d_results + f, either of which may be NULL. width, height in 1..16384 with width*height <= 2^24, n_frames in 0..4096, a
 * pitch at least the width and, for n_frames > 1, a stride that holds a frame: anything else is ARIA_E_INVALID, refused before
 * anything is enqueued. The call enqueues sum(iterations) x (accumulate, solve) on the handle's stream: no graph, no host
 * synchronisation, no grid-wide barrier. */
int   aria_icp_track_batch_device(aria_icp_t h, const float* d_depth, int64_t depth_stride, int depth_pitch,
                                  const float* d_model_depth, int64_t model_depth_stride, int model_depth_pitch,
                                  const float* d_model_normal, int64_t normal_stride, int normal_pitch,
                                  const double* d_model_extrinsics, const double* d_guess, const uint8_t* d_mask, int n_frames,
                                  int width, int height, double* d_extrinsics_out, aria_icp_result* d_results);
/* One frame from dense host buffers (width*height floats each, 3*width*height for the normals); blocks. extrinsics_out and
 * result may be NULL. A non-finite pose returns ARIA_E_INVALID. */
int   aria_icp_track(aria_icp_t h, const float* depth, const float* model_depth, const float* model_normal,
                     const double* model_extrinsics, const double* guess, int width, int height, double* extrinsics_out,
                     aria_icp_result* result);
/* The 29 integers of rule 4 of one accumulation per frame, at the Trel given as 12 doubles at d_trel + 12*f (live camera to
 * model camera) on the level pixels of `stride` (1, 2, 4, 8 or 16), with no solve: d_system + 29*f. The maps as above. */
int   aria_icp_debug_system_device(aria_icp_t h, const float* d_depth, int64_t depth_stride, int depth_pitch,
                                   const float* d_model_depth, int64_t model_depth_stride, int model_depth_pitch,
                                   const float* d_model_normal, int64_t normal_stride, int normal_pitch,
                                   const double* d_model_extrinsics, const double* d_trel, int n_frames, int width, int height,
                                   int stride, int64_t* d_system);
/* The bytes a call must move: per iteration and level pixel 4 of live depth and 4 + 12 of the model, and 320 per frame (two
 * poses read, one written, the record); ARIA_E_INVALID for a configuration or sizes the call refuses. Host only, no handle. */
int64_t aria_icp_algorithmic_bytes(const aria_icp_config* cfg, int width, int height, int n_frames);

/* ---- mesh of the volume: the aria_tsdf_voxel records of the dense depth fusion contoured into a triangle mesh, the one
 * output of the dense chain a consumer can use as a surface (a map viewer, a mesh tool, a later collision or visibility
 * query). The reference has no code for it (its roadmap item H21 is a 3-D map viewer), so the NumPy restatement
 * aria_slam_amd/mesh_ref.py is the definition and the device equals it byte for byte. The stage owns no volume: it is handed
 * the records in HBM with their geometry. Every cell is cut into the six tetrahedra of the Kuhn (Freudenthal) split around
 * its body diagonal and each tetrahedron is contoured on its own: the split is translation invariant, so neighbouring cells
 * agree on every shared face, and the 16-case table is derived from one orientation rule. Out of scope: the 256-case
 * marching-cubes table, vertex normals, welding or decimation, colour beyond gray, meshing a sub-box, re-meshing only the
 * bricks that changed, and a volume that changes between aria_mesh_update_from_volume_device and an extract. Additive to
 * ABI 4.
 *
 * All arithmetic is fp32, one rounding per operation, no contraction, in exactly the order written. A NaN fails every
 * comparison. The records' tsdf values must be finite, as in the ray casting stage.
 * 1. Geometry. nx, ny, nz, voxel, origin[3], min_weight as in rule 1 of the dense depth fusion, with the same validity
 *   ranges. Records lie at the linear index (k*ny + j)*nx + i. The centre of voxel (i, j, k) is
 *   c = origin + ((float)i + 0.5f) * voxel per axis. A voxel is seen when weight >= min_weight. It is inside when tsdf < 0;
 *   zero and -0.0f are outside, as in rule 4 of the fusion.
 * 2. Edges and vertices. Voxel a owns seven edges (a, d), d = 1..7: the bits of d name the axes stepped by +1 (1 = x, 2 = y,
 *   4 = z), so 3, 5 and 6 are face diagonals and 7 is the body diagonal of the cell at a. The far end b must lie inside the
 *   volume. The edge carries a vertex when a and b are both seen and exactly one of them is inside; the rule is edge local
 *   and does not ask whether a live cell uses the vertex. alpha = tsdf_a / (tsdf_a - tsdf_b); X = c_a with alpha * voxel
 *   added on every axis of d, the same product on each; gray = alpha < 0.5f ? gray_a : gray_b;
 *   weight = min(weight_a, weight_b); dir = d. Vertices are numbered in ascending (linear index of a, d). For d in {1, 2, 4}
 *   this is rule 4 of the fusion word for word: those vertices, in order, are the records of aria_tsdf_extract_points with
 *   axis = log2(d).
 * 3. Cells and tetrahedra. Cell (i, j, k) exists for i < nx-1, j < ny-1, k < nz-1; its corners are q = bx + 2 by + 4 bz, the
 *   voxels (i+bx, j+by, k+bz). It is live when all eight corners are seen. Tetrahedron p = 0..5 belongs to the axis
 *   permutations pi in the order xyz, xzy, yxz, yzx, zxy, zyx; its corners are (0, 2^pi0, 2^pi0 + 2^pi1, 7). Every edge of
 *   a tetrahedron joins a corner to a corner whose bit set contains it, so it is the edge (lower corner's voxel, difference
 *   of the bit sets) of rule 2, owned by one of the cell's corners 0..6.
 * 4. Table. By the tetrahedron's 4-bit inside mask (bit t = its corner t inside): 0 or 4 inside, nothing. 1 inside (corner a)
 *   the triangle through the edges from a to the outside corners in ascending order; 3 inside (corner c outside), through
 *   the edges from the inside corners, ascending, to c. 2 inside (a < b inside, c < d outside): the quad (a,c), (a,d), (b,d),
 *   (b,c), split as (0,1,2), (0,2,3). Orientation: with every vertex at its edge midpoint, (v1 - v0) x (v2 - v0) has a
 *   positive dot product with (mean of the outside corners - mean of the inside corners); otherwise the last two vertices
 *   of each triangle are swapped. This depends only on p and the mask: a table of 6 x 16 entries, with
 *   0,1,1,2,1,2,2,1,1,2,2,1,2,1,1,0 triangles by mask.
 * 5. Triangles. The live cells in ascending linear index of corner 0, then tetrahedra 0..5, then table order. A triangle is
 *   three uint32 vertex numbers of rule 2. At most 12 per cell.
 * 6. Capacities. The first min(total, cap) vertices and the first min(total, cap) triangles are written; triangles carry the
 *   full numbering whatever the vertex capacity. The two int64 count words receive the totals (vertices, triangles). A total
 *   above its capacity defers ARIA_E_OUTPUT_TOO_SMALL. A vertex total above 2^32 - 1 defers ARIA_E_OVERFLOW, and the
 *   triangles are then not valid. Records beyond the written ones are never touched.
 * 7. Properties that follow. No directed edge (v0 -> v1, v1 -> v2, v2 -> v0 of a triangle) occurs twice. Inside any block of
 *   live cells every directed edge is met by its reverse exactly once: the mesh is a closed oriented manifold wherever the
 *   data is complete, and its boundary runs along faces between a live cell and a cell that is not. An exact zero gives
 *   alpha = 0, hence coincident vertices and zero-area triangles; they are kept, so the topology stays intact.
 * Determinism. No float atomics, one writer per record: the result is bitwise independent of run, handle and stream. */
typedef struct aria_mesh_s* aria_mesh_t;
typedef struct {
    float    X[3];              /* world coordinates in metres                                                     */
    uint8_t  gray;
    uint8_t  dir;               /* d of rule 2: 1, 2, 4 axis edges, 3, 5, 6 face diagonals, 7 the body diagonal     */
    uint16_t weight;            /* min of the two voxels' weights                                                  */
} aria_mesh_vertex;             /* 16 bytes                                                                        */
typedef struct {
    uint32_t v[3];              /* vertex numbers of rule 2                                                        */
} aria_mesh_triangle;           /* 12 bytes                                                                        */
typedef struct {
    int      struct_size;       /* = sizeof(aria_mesh_config)                                                     */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking)  */
    int      nx, ny, nz;        /* the volume's geometry; default 256 x 256 x 128                                  */
    int      min_weight;        /* default 2, 1..65535                                                             */
    float    voxel;             /* default 0.05 m                                                                  */
    float    origin[3];         /* default (-6.4, -6.4, 0)                                                         */
} aria_mesh_config;             /* 48 bytes                                                                        */

void  aria_mesh_default_config(aria_mesh_config* cfg);
/* ARIA_E_INVALID for a bad field, before any device is touched. The handle keeps aria_mesh_scratch_bytes on the device. */
int   aria_mesh_create(const aria_mesh_config* cfg, aria_mesh_t* out);
void  aria_mesh_destroy(aria_mesh_t h);
void* aria_mesh_stream(aria_mesh_t h);
/* Synchronises the handle's stream and returns, once, what the extracts since the last check deferred: ARIA_E_OVERFLOW
 * before ARIA_E_OUTPUT_TOO_SMALL. */
int   aria_mesh_check(aria_mesh_t h);
/* Remembers d_voxels (nx*ny*nz records in the layout of rule 1, aria_tsdf_device_voxels of a volume of this geometry) and
 * runs rules 2 and 3 over them: a word per voxel (its edges that carry a vertex, its cell's corner signs and triangle count)
 * and two counts per 256 voxels. The records must stay where they are, and unchanged, until the extracts that follow have
 * run; after the volume changed, update again. Enqueued on the handle's stream, no synchronisation. */
int   aria_mesh_update_from_volume_device(aria_mesh_t h, const aria_tsdf_voxel* d_voxels);
/* Rules 2-6 into device memory: vertices at d_vertices (vcap records), triangles at d_triangles (tcap records), the totals at
 * d_counts[0] (vertices) and d_counts[1] (triangles). A pointer may be NULL with its capacity 0; d_counts may not. An
 * extract before the first update is ARIA_E_INVALID, refused before anything is enqueued. Enqueued on the handle's stream,
 * no synchronisation. */
int   aria_mesh_extract_device(aria_mesh_t h, aria_mesh_vertex* d_vertices, int64_t vcap, aria_mesh_triangle* d_triangles,
                               int64_t tcap, int64_t* d_counts);
/* The same into host arrays; blocks, and returns what aria_mesh_check would. counts: two int64. */
int   aria_mesh_extract(aria_mesh_t h, aria_mesh_vertex* vertices, int64_t vcap, aria_mesh_triangle* triangles, int64_t tcap,
                        int64_t* counts);
/* What a handle of this geometry keeps on the device: 4 bytes per voxel and 24 per 256 voxels; ARIA_E_INVALID for dims the
 * create refuses. Host only, no handle. */
int64_t aria_mesh_scratch_bytes(int nx, int ny, int nz);
/* The bytes one update + extract must move: every record read once (8), its word written once and read once (8), 16 per
 * vertex and 12 per triangle written. Host only, no handle. */
int64_t aria_mesh_algorithmic_bytes(int nx, int ny, int nz, int64_t n_vertices, int64_t n_triangles);

/* ---- guided matching: landmarks projected into a frame by a predicted pose, the keypoints searched in a small window
 * around each projection, the best descriptor match kept (the step ORB-SLAM calls SearchByProjection) -- correspondences for
 * aria_pnp_estimate_batch_device against landmarks of ANY earlier pair, where aria_pnp_associate_batch_device reaches only
 * the points of the previous one. The reference has no code for it, so the NumPy restatement aria_slam_amd/proj_ref.py is
 * the definition and the device equals it bit for bit. Additive to ABI 4.
 *
 * Inputs per frame f of a batch: a predicted world-to-camera pose at d_pose + 12 f (12 doubles [R|t], row-major: rows of
 *   (r0 r1 r2 t)); the extractor's batch outputs, keypoints at d_kp + f*kp_stride (d_n[f] of them), descriptors at
 *   d_desc + f*kp_stride*32, kp_stride <= 8192; the image size width x height (<= 4096 each); and a range
 *   (first, count) = d_range[2f], d_range[2f+1] into ONE array of n_landmarks aria_proj_landmark records, count <= land_cap
 *   <= 2^20. A map appends in pair order, so "the landmarks of the last K pairs" is one range and the frames of a batch share
 *   one array; ranges may overlap.
 * Rules per landmark i of the frame's range (array index first + i), in this order. radius_px and ratio are used as fp32;
 *   scale[o] is the fp32 level scale of aria_orb_level_info.
 * 1. Projection in fp64, no contraction. Xc = R X + t, each component ((r0 X0 + r1 X1) + r2 X2) + t. The landmark is visible
 *   when octave >= 0, Xc.z > min_depth, and u = (float)(fx * Xc.x / Xc.z + cx), v = (float)(fy * Xc.y / Xc.z + cy) satisfy
 *   0 <= u < width and 0 <= v < height in fp32 (a NaN fails every test). A landmark that is not visible has u = v = 0,
 *   kp_idx = hamming = second = -1, flags = 0. octave < 0 marks a dead landmark, which is never visible.
 * 2. Candidates. Keypoint k < d_n[f] is a candidate when, in fp32 as written, |octave_k - octave_i| <= max_octave_diff with
 *   both octaves clamped to 0..7, fabsf(x_k - u) <= r and fabsf(y_k - v) <= r, r = radius_px * scale[octave_i]: a square
 *   window with inclusive edges.
 * 3. Best and second. hamming = the least 256-bit Hamming distance over the candidates, ties to the lowest k; second = the
 *   least distance over the OTHER candidates (it may equal hamming), -1 with a single candidate. No candidate:
 *   hamming = second = -1.
 * 4. Acceptance. Rejected when hamming >= th_hamming; rejected when second >= 0 and not
 *   (float)hamming < ratio * (float)second. A single candidate passes the ratio test.
 * 5. Uniqueness. An accepted landmark claims its best keypoint; a keypoint goes to the claim of least hamming, ties to the
 *   lowest i. The losers are unmatched: they do not fall back to their second candidate.
 * 6. Record. flags: bit 0 visible, bit 1 had candidates, bit 2 accepted, bit 3 won its keypoint. kp_idx = the keypoint when
 *   bit 3 is set, else -1. hamming and second keep their values whenever bit 1 is set; u and v whenever bit 0 is.
 * Outputs per frame. land_cap records aria_proj_obs at d_obs + f*land_cap (records at and beyond count are written as not
 *   visible). And the matched landmarks in ascending i, stably compacted: aria_pnp_corr at d_corr + f*land_cap (the
 *   landmark's X and the matched keypoint's stored fp32 pixel), aria_proj_pair at d_pairs + f*land_cap (the array index
 *   first + i and kp_idx), their number at d_ncorr[f] -- the input of aria_pnp_estimate_batch_device with
 *   corr_cap = land_cap; d_pairs carries an inlier mask back to landmarks and keypoints. No NaN or Inf is ever written.
 * Invalid frames. d_n[f] outside [0, kp_stride], first < 0, count outside [0, land_cap], first + count > n_landmarks, or a
 *   non-finite pose entry: detected before any keypoint, descriptor or landmark of the frame is read; every record of the
 *   frame is not visible, d_ncorr[f] = 0, and aria_proj_check reports ARIA_E_INVALID once. The other frames are unaffected.
 * Determinism. Integer atomics only; bitwise reproducible; independent of the batch split, of the frame's place in the
 *   batch, of how landmarks are chunked over workgroups and of the cell size of the keypoint binning.
 * Defaults. min_depth 0.1 (the map stage's), radius_px 15, ratio 0.9, th_hamming 100, max_octave_diff 1: ORB-SLAM's
 *   published tracking constants. Nobody has tuned them on a recording here.
 * Out of scope: a predicted scale level from the landmark's distance; the viewing-angle test; ORB-SLAM's rotation-histogram
 *   check; fusing duplicate map points; updating a landmark's descriptor; relocalisation. */
typedef struct aria_proj_s* aria_proj_t;
typedef struct {
    int      struct_size;       /* = sizeof(aria_proj_config)                                                     */
    int      device;
    void*    stream;            /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking, as in
                                 * aria_pose_config)                                                              */
    double   fx, fy, cx, cy;    /* intrinsics (default EuRoC cam0)                                                */
    double   min_depth;         /* default 0.1, finite                                                            */
    double   radius_px;         /* default 15, used as fp32, 0..1024                                              */
    float    ratio;             /* default 0.9, 0..1                                                              */
    int      th_hamming;        /* default 100, 0..257                                                            */
    int      max_octave_diff;   /* default 1, 0..8                                                                */
    int      reserved;
} aria_proj_config;             /* 80 bytes                                                                       */
typedef struct {
    double  X[3];               /* world point                                                                    */
    uint8_t desc[32];           /* the descriptor the landmark is recognised by                                   */
    int     octave;             /* of the keypoint it was made from; < 0: dead, never visible                     */
    int     source;             /* carried, never interpreted (the join below: the arena position)                */
} aria_proj_landmark;           /* 64 bytes                                                                       */
typedef struct {
    float u, v;
    int   kp_idx, hamming, second, flags;
} aria_proj_obs;                /* 24 bytes                                                                       */
typedef struct {
    int landmark, keypoint;
} aria_proj_pair;               /* 8 bytes                                                                        */

void  aria_proj_default_config(aria_proj_config* cfg);
int   aria_proj_create(const aria_proj_config* cfg, aria_proj_t* out);
void  aria_proj_destroy(aria_proj_t h);
void* aria_proj_stream(aria_proj_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when a frame of a search was invalid (above) or a map point of the join was out of range (below). */
int   aria_proj_check(aria_proj_t h);
/* Device-resident batch form (layout above). Enqueued on the handle's stream; nothing is synchronised, except when the
 * handle's workspace grows: 20 bytes per keypoint slot and 4 per 32 x 32 pixel cell of every frame of the batch. */
int   aria_proj_search_batch_device(aria_proj_t h, const double* d_pose, const aria_keypoint* d_kp, const uint8_t* d_desc,
                                    const int* d_n, int64_t kp_stride, int width, int height,
                                    const aria_proj_landmark* d_land, int n_landmarks, const int* d_range, int land_cap,
                                    int n_frames, aria_proj_obs* d_obs, aria_pnp_corr* d_corr, aria_proj_pair* d_pairs,
                                    int* d_ncorr);
/* One frame from host arrays, every landmark searched (first = 0, count = land_cap = n_landmarks); blocks, and returns what
 * aria_proj_check would. obs, corr, pairs: n_landmarks records each (corr and pairs filled up to *n_corr). */
int   aria_proj_search(aria_proj_t h, const double* pose, const aria_keypoint* kp, const uint8_t* desc, int n, int width,
                       int height, const aria_proj_landmark* land, int n_landmarks, aria_proj_obs* obs, aria_pnp_corr* corr,
                       aria_proj_pair* pairs, int* n_corr);
/* The join with the map: arena positions [first, min(first + max_count, size)) become landmarks at d_land[0..), their number
 * at d_nland[0]; the arena is read with its device-resident size, as aria_pnp_associate_batch_device reads it, and the
 * stream-ordering caveats written there hold here. For a point of pair p, slot s = p - pair_base must lie in [0, n_slots)
 * and idx = idx1 (view 1) or idx2 (view 2) in [0, d_n[s]) with d_n[s] <= kp_stride: the landmark is the point's X, the
 * descriptor row and the octave of keypoint idx of slot s (d_kp + s*kp_stride, d_desc + s*kp_stride*32), and source = the
 * arena position. A point out of range becomes a dead landmark (octave -1, zero X and descriptor, source = its position)
 * and a deferred ARIA_E_INVALID. Records at and beyond the number written are dead with source -1, so all max_count
 * records are defined. Integer copies only. first >= 0, 0 <= max_count, first + max_count < 2^31; a map on another device
 * than the handle's: ARIA_E_INVALID. */
int   aria_proj_landmarks_from_map_device(aria_proj_t h, aria_map_t map, int64_t first, int64_t max_count, int pair_base,
                                          int view, const aria_keypoint* d_kp, const uint8_t* d_desc, const int* d_n,
                                          int64_t kp_stride, int n_slots, aria_proj_landmark* d_land, int* d_nland);

/* ---- place recognition: a binary bag-of-words keyframe index that does not forget -------------------------------------
 * The brute-force keyframe scan (aria_kfdb_scan, LoopClosure.cpp:72-114) scores a query against every stored keyframe and
 * keeps 500 of them; this stage scores a query against the bags of up to `capacity` keyframes and names the best K, which
 * alone go through the exact check. The reference names the cure (docs/milestones/H09_LOOP_CLOSURE_AUDIT.md 2.1, 6.3) and
 * has no code for it: aria_slam_amd/bow_ref.py is the definition and the device equals it bit for bit. Everything is integer
 * arithmetic except one correctly rounded fp64 division per score. The vocabulary is flat: the nearest word of a descriptor
 * is found by the matcher's kNN-2 kernel against all V words. Additive to ABI 4.
 *
 * 1. Vocabulary. V words, 1 <= V <= 4096, 32 bytes each, and a weight idf_q[w] (uint16, < 4096) per word. Bit b of a
 *    descriptor is bit b & 7 of byte b >> 3, the matcher's order.
 * 2. Quantise. A descriptor's word is the word at the least Hamming distance, ties to the lowest word index.
 * 3. Train. k-majority clustering from F frames holding n descriptors in all, in frame order. n < V, F > 65535 or a count
 *    outside [0, desc_stride]: ARIA_E_INVALID. Initial word j is training descriptor floor(j * n / V). An iteration quantises
 *    every descriptor, then sets each bit of a word to 1 iff 2 * ones > members (a tie gives 0; a word without members keeps
 *    its bits). Training stops after train_iters iterations or after the first that changes no word.
 * 4. Weights. The training set is quantised once more; n_w = training frames holding word w. idf_q[w] = 0 when n_w is 0 or
 *    F, else log2(F / n_w) in Q8 by a shift-and-square logarithm on 64-bit integers (bow_ref.ilog2_q8 is its definition,
 *    truncations included; no libm call anywhere).
 * 5. Bag of a frame. tf[w] = the frame's descriptors on word w (uint16; at most `rows` <= 4096 descriptors), v[w] =
 *    tf[w] * idf_q[w], the norm N = sum v[w] < 2^24. N = 0: the bag is empty, scores 0 against everything, is never returned.
 * 6. Score. S = sum_w min(v[w] * Nd, u[w] * Nq) for a query (v, Nq) and an entry (u, Nd): an exact integer <= Nq * Nd < 2^48;
 *    score = (double)S / (double)(Nq * Nd), one IEEE division: DBoW2's L1 score 1 - |a - b|_1 / 2 of the L1-normalised bags.
 *    Identical bags score exactly 1.0, disjoint bags 0.0.
 * 7. Database. A deque of at most `capacity` entries (id, tf, N); adding beyond capacity drops the oldest; index i = the
 *    position, oldest first: aria_kfdb's semantics, so the two stay index-aligned when fed together. A ring in HBM:
 *    capacity * 2 * roundup(V, 8) bytes, allocated when a vocabulary is set; nothing is copied on a drop. A new vocabulary
 *    (train, set, load) empties the database.
 * 8. Query. Candidates: non-empty entries with query_id - id >= min_frames_between and score > 0. Result: the best
 *    K = top_k <= 32 by score descending, ties to the lower index, as K records aria_bow_hit per query (index -1, id -1, S 0,
 *    score 0 where there is none) and their number. Every query of a batch sees the database as it was at the call.
 * Determinism: integer sums and integer atomics only; training, bags and hits are bitwise reproducible and independent of how
 * frames and queries are batched. */
typedef struct aria_bow_s* aria_bow_t;
typedef struct {
    int      struct_size;          /* = sizeof(aria_bow_config)                                                   */
    int      device;
    void*    stream;               /* borrowed hipStream_t, or NULL = the handle creates and owns one (non-blocking) */
    int      words;                /* V that training makes, 1..4096 (default 4096)                               */
    int      rows;                 /* most descriptors of a frame, 1..4096 (default 4096)                         */
    int      capacity;             /* entries (default 65536)                                                     */
    int      top_k;                /* 1..32 (default 10)                                                          */
    int      min_frames_between;   /* default 30 (HipLoopDetector's)                                              */
    int      train_iters;          /* default 10                                                                  */
} aria_bow_config;                 /* 40 bytes                                                                    */
typedef struct {
    int32_t index;                 /* position in the database, oldest first; -1 = none                           */
    int32_t reserved;              /* 0                                                                           */
    int64_t id;
    int64_t S;                     /* the numerator of the score                                                  */
    double  score;
} aria_bow_hit;                    /* 32 bytes                                                                    */

void  aria_bow_default_config(aria_bow_config* cfg);
int   aria_bow_create(const aria_bow_config* cfg, aria_bow_t* out);
void  aria_bow_destroy(aria_bow_t h);
void* aria_bow_stream(aria_bow_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when a frame's count was outside [0, min(desc_stride, rows)] (that frame alone got an empty bag) or the norm
 * of an added or queried bag was not the sum of its weighted counts, or not below 2^24 (that entry alone is stored empty, that
 * query alone is asked as an empty one). */
int   aria_bow_check(aria_bow_t h);
/* V of the vocabulary in use, 0 before there is one. Every call below that needs a vocabulary returns ARIA_E_INVALID then. */
int   aria_bow_words(aria_bow_t h);
/* Training (rules 3 and 4) of cfg.words words. Frame f's descriptors lie at d_desc + f * desc_stride * 32, d_counts[f] of
 * them. Blocks: the host reads the counts first and one changed flag per iteration. *iters_run = iterations run. */
int   aria_bow_train_device(aria_bow_t h, const uint8_t* d_desc, const int* d_counts, int n_frames, int64_t desc_stride,
                            int* iters_run);
int   aria_bow_train(aria_bow_t h, const uint8_t* desc, const int* counts, int n_frames, int64_t desc_stride, int* iters_run);
/* Host arrays: V * 32 bytes and V weights (each < 4096). get: words and idf_q may be NULL; *V is always written. */
int   aria_bow_set_vocabulary(aria_bow_t h, const uint8_t* words, const uint16_t* idf_q, int V);
int   aria_bow_get_vocabulary(aria_bow_t h, uint8_t* words, uint16_t* idf_q, int* V);
/* The vocabulary file, little-endian: "ARIABOW\0", version (u32 = 1), V (u32), V * 32 bytes of words, V * u16 weights. A file
 * that cannot be read, is truncated, is longer, or holds a bad magic, version, V or weight: ARIA_E_INVALID. */
int   aria_bow_save(aria_bow_t h, const char* path);
int   aria_bow_load(aria_bow_t h, const char* path);
/* Bags of a batch of frames (layout as in training): n_frames rows of V uint16 at d_tf and n_frames norms at d_norm. A count
 * above min(desc_stride, rows) or below 0 defers ARIA_E_INVALID for that frame alone and writes an empty bag. Enqueued. */
int   aria_bow_transform_batch_device(aria_bow_t h, const uint8_t* d_desc, const int* d_counts, int n_frames, int64_t desc_stride,
                                      uint16_t* d_tf, int32_t* d_norm);
/* n bags (as the transform writes them) appended in order with the ids of a HOST array, read before the call returns. Enqueued. */
int   aria_bow_add_batch_device(aria_bow_t h, const uint16_t* d_tf, const int32_t* d_norm, const long long* ids, int n);
/* Transform and add of one frame, 0 <= n <= rows. The host form blocks for its upload only. */
int   aria_bow_add(aria_bow_t h, long long id, const uint8_t* desc_host, int n);
int   aria_bow_add_device(aria_bow_t h, long long id, const uint8_t* d_desc, int n);
int   aria_bow_size(aria_bow_t h);
int   aria_bow_info(aria_bow_t h, int index, long long* id, int* norm);
/* n_queries bags against the database: top_k records per query at d_hits, the number of real ones at d_counts. query_ids: a
 * HOST array, read before the call returns. Enqueued, except when the workspace grows (16 bytes per entry and query of a
 * chunk of at most 256 queries and 2^25 pairs). */
int   aria_bow_query_batch_device(aria_bow_t h, const uint16_t* d_tf, const int32_t* d_norm, const long long* query_ids,
                                  int n_queries, aria_bow_hit* d_hits, int* d_counts);
/* Transform and query of one frame; hits: top_k records on the HOST. Blocks, and returns what aria_bow_check would. */
int   aria_bow_query(aria_bow_t h, long long query_id, const uint8_t* desc_host, int n, aria_bow_hit* hits, int* n_out);
int   aria_bow_query_device(aria_bow_t h, long long query_id, const uint8_t* d_desc, int n, aria_bow_hit* hits, int* n_out);

/* ---- loop alignment: the similarity X2 = s R X1 + t between the landmarks two keyframes of a loop own (batched Sim(3)
 * RANSAC). Place recognition (aria_bow_*) and the two-view verification (aria_fund_*, aria_pose_*) yield a loop edge whose
 * translation has length 1 by construction, while every odometry edge of a map-tracked run is in the map's units; both
 * keyframes own triangulated landmarks in the map's arena, so a match between them is a pair of 3-D points, and the
 * similarity that aligns them gives the edge's translation in map units, the scale drift s around the loop, and a
 * verification stronger than the epipolar one. This is the role of ORB-SLAM's ComputeSim3. The reference has no code for it
 * (its H09 and H10 audits name the loop edge's unknown scale as the open problem); aria_slam_amd/sim3_ref.py is the
 * definition, and parity with ORB-SLAM's Sim3Solver is not claimed. Batched over pairs; additive to ABI 4.
 *
 * Correspondences. aria_sim3_corr holds the landmark of keyframe 1 in CAMERA 1's coordinates, the landmark of keyframe 2 in
 *   CAMERA 2's coordinates and the pixels of the two matched keypoints. Camera coordinates on purpose: they are near the
 *   origin, so the fp32 scoring needs no centring, and a map 1 km from the origin loses nothing, because the join
 *   (aria_sim3_associate_batch_device) does the move to camera coordinates in fp64.
 * Model. X2 = s R X1 + t; R row-major. With fix_scale = 1, s = 1 everywhere (a metric stereo map).
 * Points. x_j = ((u_j - cx) / fx, (v_j - cy) / fy) in fp64. For scoring X1, X2, x1, x2 are rounded to fp32. A correspondence
 *   with a scoring value beyond 1e15 in magnitude never scores; a model with |t| beyond 1e15 is invalid (every square of the
 *   test below stays finite).
 * Hypotheses. `hypotheses` per pair; the hash of the two-view stage with 3 distinct indices per hypothesis (slots j = 0..2,
 *   at most 256 draws per slot), keyed by (seed, pair id, h). A sample is invalid when a slot stays -1; when in either frame
 *   |(Xb - Xa) x (Xc - Xa)|^2 <= 1e-12 * max(|Xb - Xa|^2, |Xc - Xa|^2, |Xc - Xb|^2)^2 (the P3P solver's collinearity test);
 *   or when the model is not finite.
 * Closed form. fp64, + - * / and sqrt only. Centroids c1, c2 (((Xa + Xb) + Xc) / 3); M = sum (X2_i - c2)(X1_i - c1)^T, rank 2
 *   because three points are coplanar. V and the eigenvalues of M^T M from the 3x3 Jacobi of the two-view stage, sorted
 *   descending with its select network; sigma_k = sqrt(max(lambda_k, 0)); u_k = M v_k / sigma_k for the two largest,
 *   u3 = u1 x u2, v3 = v1 x v2, R = sum u_k v_k^T (a rotation, never a reflection). s = (sigma_1 + sigma_2) / sum |X1_i - c1|^2,
 *   Umeyama's least-squares scale, invalid outside [min_scale, max_scale]; s = 1 with fix_scale. t = c2 - s R c1.
 * Inliers. fp32, division-free and two-sided, because a triangulated monocular point is uncertain along its ray and certain
 *   in the image: Y2 = s R X1 + t, each component s ((r0 X + r1 Y) + r2 Z) + t_k, against x2; Y1 = R^T (X2 - t), each
 *   component (r_0k d0 + r_1k d1) + r_2k d2 with d = X2 - t, against x1 -- no 1 / s: the test is invariant to a positive scale
 *   of Y1. Inlier when for both: Y.z > 0 and (Y.x - x Y.z)^2 + (Y.y - y Y.z)^2 <= thr2 * Y.z^2,
 *   thr2 = (threshold_px / ((fx + fy) / 2))^2.
 * Winner. Most inliers; ties to the lowest h; an invalid hypothesis scores -1. Integer counts, fixed reduction order.
 * Refinement. When the winner has >= 4 inliers and refine_iters > 0: up to refine_iters Gauss-Newton steps in fp64 on the four
 *   normalised reprojection residuals per inlier (Y2 against x2, Y1 against x1), over the winner's inlier set, which is not
 *   re-evaluated between steps. It starts from the winner's closed form in fp64 (what was scored is its fp32 rounding). Seven
 *   parameters (w, v, sigma), six with fix_scale, and a left-multiplicative update: R <- Exp(w) R, t <- E(sigma) (Exp(w) t) + v,
 *   s <- E(sigma) s. E is NOT libm's exp: it is the fixed polynomial 1 + x (1 + x/2 (1 + x/3 ( ... (1 + x/12)))), + * / only, so
 *   host and device compute the same bits; E(0) = E'(0) = 1 is all a Gauss-Newton step needs, and at the fixed point sigma = 0.
 *   The 28 + 7 entries of the normal equations are summed in a fixed order (per thread over its strided share, then a fixed
 *   tree); Cholesky in one lane; a pivot that is not positive, a step that is not finite, or an s outside
 *   [min_scale, max_scale] ends the refinement with the last good model. It stops early at |dx| <= 1e-12. The refined model is
 *   rescored in fp32 and kept (refined = 1) when its count is >= the winner's; otherwise the result is the winner's closed form.
 *   Two cameras at one centre (t = 0) cannot see s in the image: the sigma column vanishes, the pivot test ends the
 *   refinement, and s is the closed form's.
 * Outputs. The mask and n_inliers are those of the kept model; rms_px is the RMS over both directions of the kept inliers
 *   (sqrt(sum of the four squared residuals / (2 n_inliers))), in fp64 in a fixed order, times (fx + fy) / 2. n_corr is the
 *   number of correspondences read (0 for a pair refused by the checks below).
 * Validity. valid = 0 with fewer than 3 correspondences, with no valid hypothesis, or when a result field would not be finite:
 *   R = I, t = 0, s = 1, n_inliers = 0, best_hypothesis = -1, zero mask. No field is ever NaN or Inf. valid = 1 says a model
 *   was found; whether it is a loop is the caller's gate on n_inliers (ORB-SLAM's constant is 20, untuned here). A count
 *   outside [0, corr_cap], or an X or a pixel that is not finite, is found before any arithmetic: the pair is invalid with
 *   n_corr = 0, aria_sim3_check reports ARIA_E_INVALID once, the other pairs of the launch are unaffected.
 * Determinism. No float atomics; bitwise reproducible run to run, independent of how pairs are split into calls and of a
 *   pair's place in a launch.
 * threshold_px = 3.0 is sqrt(9.21) rounded, ORB-SLAM's chi-square bound at octave 0; min_inliers = 20 likewise. Both are
 *   assumptions nobody has tuned on a recording.
 * Not built: fusing duplicate landmarks, guided re-matching after the first alignment (ORB-SLAM's SearchBySim3), per-octave
 *   thresholds, relocalisation. (The Sim(3) pose graph that distributes s around the loop and the correction of the map's
 *   points are aria_sgraph_*, below.) */
typedef struct aria_sim3_s* aria_sim3_t;
typedef struct {
    double X1[3];              /* landmark of keyframe 1, camera 1's coordinates                                 */
    double X2[3];              /* landmark of keyframe 2, camera 2's coordinates                                 */
    float  u1, v1, u2, v2;     /* pixels of the two matched keypoints                                            */
} aria_sim3_corr;              /* 64 bytes                                                                       */
typedef struct {
    double R[9], t[3], s;      /* X2 = s R X1 + t                                                                */
    double rms_px;             /* RMS reprojection error of the final inliers, both directions                   */
    int    n_corr, n_inliers, best_hypothesis, iterations, refined, valid;
} aria_sim3_result;            /* 136 bytes                                                                      */
typedef struct {
    int      struct_size;      /* = sizeof(aria_sim3_config)                                                    */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle owns one (non-blocking: NOT ordered against
                                * the legacy default stream, see aria_pose_config)                               */
    int      hypotheses;       /* per pair: multiple of 64, 64..16384 (default 1024)                            */
    int      refine_iters;     /* 0..16 (default 5)                                                              */
    int      fix_scale;        /* 0 or 1 (default 0); 1: s = 1 everywhere                                        */
    int      reserved;         /* 0                                                                              */
    double   fx, fy, cx, cy;   /* intrinsics (default EuRoC cam0)                                                */
    double   threshold_px;     /* default 3.0 = sqrt(9.21) rounded; untuned                                      */
    double   min_scale, max_scale; /* defaults 0.05 and 20: a model outside them is invalid                      */
    uint64_t seed;             /* sample hash seed (default 0)                                                   */
} aria_sim3_config;

void  aria_sim3_default_config(aria_sim3_config* cfg);
int   aria_sim3_create(const aria_sim3_config* cfg, aria_sim3_t* out);
void  aria_sim3_destroy(aria_sim3_t h);
void* aria_sim3_stream(aria_sim3_t h);
/* Synchronises the handle's stream and returns the deferred error of the batch calls since the last check: ARIA_E_INVALID
 * when some pair's count was outside [0, corr_cap] or one of its values was not finite (estimate), or its counts or match
 * indices were out of range (associate). Such a pair is skipped; the other pairs are unaffected. */
int   aria_sim3_check(aria_sim3_t h);
/* One pair, host buffers; blocks. pair_base is the pair id the sample hash uses. mask (optional): n bytes. */
int   aria_sim3_estimate(aria_sim3_t h, const aria_sim3_corr* corr, int n, int pair_base, aria_sim3_result* out, uint8_t* mask);
/* Device-resident batch form, with the meaning of aria_pnp_estimate_batch_device: pair p reads d_ncorr[p] correspondences at
 * d_corr + p*corr_cap, writes d_out[p] and, if d_mask is not NULL, corr_cap bytes at d_mask + p*corr_cap (zero beyond the
 * pair's correspondences). The sample hash sees pair id pair_base + p. Enqueued; nothing is synchronised, except when the
 * workspace grows. */
int   aria_sim3_estimate_batch_device(aria_sim3_t h, const aria_sim3_corr* d_corr, const int* d_ncorr, int n_pairs, int corr_cap,
                                      int pair_base, aria_sim3_result* d_out, uint8_t* d_mask);
/* Test hook: for one pair (host buffers), every hypothesis's 3 sample indices (sample_idx[h*3 + j]; -1 when n < 3), R
 * (R[h*9 + k]), t (t[h*3 + k]) and s (s[h]) in fp32 as scored (zero when invalid) and inlier count (counts[h], -1 when
 * invalid). */
int   aria_sim3_debug_hypotheses(aria_sim3_t h, const aria_sim3_corr* corr, int n, int pair_base, int* sample_idx, float* R,
                                 float* t, float* s, int* counts);
/* The join that keeps the chain device-resident; aria_pnp_associate_batch_device twice over. Pair p's keyframe 1 is the
 * query side of its matches (d_matches + p*match_cap, d_nmatches[p] of them; keypoints at d_kp1 + p*kp_stride, d_n1[p] of
 * them) and keyframe 2 the train side (d_kp2, d_n2). Keyframe j owns the arena points with pair == d_anchorJ[p] (a device
 * array of n_pairs ints), indexed by their idx{viewJ} (viewJ = 1 or 2). A match yields a correspondence when both sides have
 * such a point; of several points the one at the lowest arena position is taken, per side. Xj = Rj X + tj with the 12-double
 * world-to-camera rows [R t] at d_poseJ + 12 p, in fp64, each component ((r0 X + r1 Y) + r2 Z) + t; the pixels are the
 * keypoints'. Correspondences are written in match order, stably compacted, at d_corr + p*match_cap, their number at
 * d_ncorr[p], each one's match index (optional) at d_corr_match + p*match_cap: the input of
 * aria_sim3_estimate_batch_device with corr_cap = match_cap. Integers and copies only, plus the one rigid move. A count
 * outside [0, match_cap] or [0, kp_stride], a query_idx outside [0, d_n1[p]) or a train_idx outside [0, d_n2[p]) is a
 * deferred error of the pair (d_ncorr[p] = 0). The stream order, the arena-address caveat and the other-device refusal are
 * those of aria_pnp_associate_batch_device. Cost: the call clears and fills two tables of n_pairs * kp_stride ints (kp_stride
 * at most 2^24), and, unlike the PnP join, whose pairs are anchor_base + p, the fill compares every arena point with every
 * pair's anchor: n_pairs * arena integer compares per table. That is nothing for the handful of candidates a loop detector
 * hands over and 47 times the PnP join at 4096 pairs against 2.4 M points; a sorted anchor list or a hash is not built. */
int   aria_sim3_associate_batch_device(aria_sim3_t h, aria_map_t map, const int* d_anchor1, const int* d_anchor2, int view1,
                                       int view2, const double* d_pose1, const double* d_pose2, const aria_keypoint* d_kp1,
                                       const int* d_n1, const aria_keypoint* d_kp2, const int* d_n2, int64_t kp_stride,
                                       const aria_match* d_matches, const int* d_nmatches, int n_pairs, int match_cap,
                                       aria_sim3_corr* d_corr, int* d_ncorr, int* d_corr_match);

/* ---- Sim(3) pose-graph optimisation and map correction after a loop: the roles of ORB-SLAM's OptimizeEssentialGraph and
 * CorrectLoop, batched over graphs. The reference has no code for either (its SE(3) graph, aria_graph_*, takes [R t] and
 * cannot repair the scale a monocular run drifts in). Additive to ABI 4. aria_slam_amd/sgraph_ref.py restates the stage in
 * NumPy and is its definition: aria_graph_*'s with a seventh coordinate. fp64, + - * / and sqrt only.
 *
 * Vertex. S = (R, t, s), camera-to-world: x_w = s R x_c + t. A B = (sA sB, RA RB, sA RA tB + tA); S^-1 = (1/s, R^T,
 *   -(R^T t) / s). The record holds R row-major, then t, then s; pose rows [R t] interleave t, and the two copy calls below
 *   convert (64-bit integer copies).
 * Edge. Z = (R, t, s) measures S_from^-1 S_to; an odometry edge from SE(3) poses has s = 1; a loop edge from an
 *   aria_sim3_result with keyframe 1 = `to` and keyframe 2 = `from` is its (R, t, s) as they stand. Information
 *   info_scale * I7 (ORB-SLAM's identity, not tuned).
 * Error. E = Z^-1 S_i^-1 S_j; e = (t_E, qv_E, (s_E - 1/s_E) / 2) with qv_E the vector part of R_E's unit quaternion, w >= 0.
 *   The scale term is sinh(log s_E): odd under inversion, slope 1 at 1, no log. chi2 = sum info_scale * e.e.
 * Update. S <- S * D(d), d of 7: D = (R(dq), dt, f(d7)) with aria_graph_*'s fromMQT on d[0..5] and f(x) = x + sqrt(x^2 + 1)
 *   for x >= 0, 1 / (-x + sqrt(x^2 + 1)) for x < 0: the exact inverse of the scale error, always positive. The rotation is
 *   then replaced by that of its unit quaternion. Analytic 7x7 Jacobians (sgraph_ref.py); with every scale 1 their upper-left
 *   6x6 are aria_graph_*'s.
 * LM, solver, determinism. Those of aria_graph_* on 7x7 blocks, lambda0 = 1e-5 max diag(H) over the free vertices. One
 *   workgroup per graph; one form of the solve (the vectors in the handle's scratch, any size).
 * fix_scale (per handle, for a metric map). The scale row of the error and the seventh row and column of both Jacobians are
 *   zero, d7 = 0 exactly, and every vertex's s comes back bit for bit. With every s = 1 the poses are aria_graph_*'s up to
 *   rounding.
 * Invalid input. aria_graph_*'s rules, and a vertex s or an edge s that is not finite or <= 0: that graph gets valid = 0,
 *   stop_reason 2, and none of its vertices is written; the other graphs of the batch are unaffected.
 * Map correction. A point of pair p with pair_base <= p < pair_base + n_table and v = d_pair_vertex[p - pair_base] >= 0 (the
 *   pair's anchor keyframe) moves by X' = S_new[v] S_old[v]^-1 X in one fixed operation order, the same bits as the
 *   restatement: d = X - t_old; c_k = ((Ro[0][k] d0 + Ro[1][k] d1) + Ro[2][k] d2) / s_old;
 *   X'_k = s_new * ((Rn[k][0] c0 + Rn[k][1] c1) + Rn[k][2] c2) + t_new_k. Every other byte of the record is untouched. A pair
 *   outside the table, or v = -1, leaves the point alone. A v >= n_vertices, a used vertex whose s (old or new) is not finite
 *   or <= 0, or an X that is not finite leaves the point alone, counts it as refused and defers ARIA_E_INVALID.
 * Poses after correction. [R_new t_new] with s dropped: a point at camera coordinates x_c is now at s_new x_c -- the local
 *   structure is rescaled, the camera is not.
 * Not built: a multi-workgroup solve of one very large graph; the register and LDS forms of aria_graph_*'s solve; covisibility
 *   and spanning-tree edge selection (the "essential" of the essential graph); landmark fusion and SearchBySim3; bundle
 *   adjustment after the correction; correcting the TSDF volume; per-edge 7x7 information; robust kernels; tuning of the
 *   adapters' x10 loop weight. */
typedef struct aria_sgraph_s* aria_sgraph_t;
typedef struct {
    int      struct_size;      /* = sizeof(aria_sgraph_config)                                                  */
    int      device;
    void*    stream;           /* borrowed hipStream_t, or NULL = the handle owns one (non-blocking, see aria_graph_config) */
    int      max_graphs;       /* as aria_graph_config                                                           */
    int      max_vertices;
    int      max_edges;
    int      pcg_max_iters;
    double   pcg_rel_tol;
    int      fix_scale;        /* 0 or 1 (default 0)                                                             */
    int      reserved;         /* 0                                                                              */
} aria_sgraph_config;          /* 48 bytes                                                                       */
typedef struct {
    double   R[9], t[3], s;    /* x_w = s R x_c + t                                                              */
} aria_sgraph_vertex;          /* 104 bytes                                                                      */
typedef struct {
    int32_t  from, to;         /* vertex indices of the graph                                                    */
    double   info_scale;       /* information = info_scale * I7                                                  */
    double   Z[12];            /* rows of [R t] of the measured S_from^-1 S_to                                   */
    double   s;                /* its scale                                                                      */
} aria_sgraph_edge;            /* 120 bytes                                                                      */
typedef struct {
    double   chi2_initial, chi2_final, lambda;
    int      iterations_done, trials, pcg_iterations, valid, stop_reason, reserved;   /* as aria_graph_result */
} aria_sgraph_result;          /* 48 bytes                                                                       */
typedef struct {
    int      moved, left_alone, refused, reserved;
} aria_sgraph_correct_stats;   /* 16 bytes                                                                       */

void  aria_sgraph_default_config(aria_sgraph_config* cfg);
int   aria_sgraph_create(const aria_sgraph_config* cfg, aria_sgraph_t* out);
void  aria_sgraph_destroy(aria_sgraph_t h);
void* aria_sgraph_stream(aria_sgraph_t h);
/* Synchronises the handle's stream and returns the deferred error of the device calls since the last check, once:
 * ARIA_E_INVALID when some graph was invalid or some point was refused, else ARIA_E_TOO_LARGE when some graph had more
 * vertices or edges than the handle was created for (that graph: valid = 0, nothing read, nothing written). */
int   aria_sgraph_check(aria_sgraph_t h);
/* One graph, host arrays; blocks. Invalid input: ARIA_E_INVALID, larger than the handle: ARIA_E_TOO_LARGE, in both cases
 * nothing is written. */
int   aria_sgraph_optimize(aria_sgraph_t h, aria_sgraph_vertex* vertices_inout, int n_vertices, int fixed_index,
                           const aria_sgraph_edge* edges, int n_edges, int iterations, aria_sgraph_result* result);
/* Device-resident batch with the offsets and the meaning of aria_graph_optimize_batch_device: graph g owns the vertices
 * d_vertex_offset[g] .. d_vertex_offset[g+1] and the edges d_edge_offset[g] .. d_edge_offset[g+1] (indices relative to the
 * graph), fixed vertex d_fixed[g]. Writes d_vertices in place and d_results[g]. Enqueued; data errors: aria_sgraph_check. */
int   aria_sgraph_optimize_batch_device(aria_sgraph_t h, aria_sgraph_vertex* d_vertices, const int* d_vertex_offset,
                                        const aria_sgraph_edge* d_edges, const int* d_edge_offset, const int* d_fixed,
                                        int n_graphs, int iterations, aria_sgraph_result* d_results);
/* Test hook: one graph (host arrays) linearised at its vertices. chi2; b (n_vertices * 7); H_diag (n_vertices * 49, row-major
 * 7x7 diagonal blocks); H_off (n_edges * 49, the block at (from, to) of every edge; its transpose sits at (to, from)).
 * Nothing of the fixed vertex is removed. Blocks. */
int   aria_sgraph_debug_linearize(aria_sgraph_t h, const aria_sgraph_vertex* vertices, int n_vertices, int fixed_index,
                                  const aria_sgraph_edge* edges, int n_edges, double* chi2, double* b, double* H_diag,
                                  double* H_off);
/* n vertices from n pose rows (12 doubles each, camera-to-world), s = 1; and n pose rows from n vertices, s dropped. Enqueued. */
int   aria_sgraph_vertices_from_pose_device(aria_sgraph_t h, const double* d_poses, aria_sgraph_vertex* d_vertices, int n);
int   aria_sgraph_poses_from_vertices_device(aria_sgraph_t h, const aria_sgraph_vertex* d_vertices, double* d_poses, int n);
/* The map correction (above) on the map handle's arena, read with its device-resident size. d_stats (optional) is cleared and
 * then counts the points moved, left alone and refused. Enqueued on this handle's stream; the stream order, the arena-address
 * caveat and the other-device refusal are those of aria_pnp_associate_batch_device. This call writes the arena of another
 * handle: nothing else may use the map until it has run. */
int   aria_sgraph_correct_map_device(aria_sgraph_t h, aria_map_t map, const int* d_pair_vertex, int n_table, int pair_base,
                                     const aria_sgraph_vertex* d_old, const aria_sgraph_vertex* d_new, int n_vertices,
                                     aria_sgraph_correct_stats* d_stats);
/* The same correction on n_points records of the caller's own device array (a map kept elsewhere, a test). */
int   aria_sgraph_correct_points_device(aria_sgraph_t h, aria_map_point* d_points, int64_t n_points, const int* d_pair_vertex,
                                        int n_table, int pair_base, const aria_sgraph_vertex* d_old,
                                        const aria_sgraph_vertex* d_new, int n_vertices, aria_sgraph_correct_stats* d_stats);

/* ---- synthetic workload: integer-only generator, identical bytes everywhere ------------ */
int aria_synth_frame_pair(uint64_t seed, int width, int height, uint8_t* frame_a, uint8_t* frame_b);
int aria_synth_sequence(uint64_t seed0, int n_pairs, int width, int height, uint8_t* out, int n_threads);

#ifdef __cplusplus
}
#endif
#endif
