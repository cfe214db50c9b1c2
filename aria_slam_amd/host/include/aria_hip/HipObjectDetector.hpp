// aria::adapters::hip::HipObjectDetector -- the reference's IObjectDetector port (include/interfaces/IObjectDetector.hpp:10-46)
// over the aria_det_* family of the C-ABI: TRTInference::preprocess and ::postprocess (src/legacy/TRTInference.cpp:68-142) run as
// kernels, the network between them is an injected hook. The reference's implementation of this port (YoloTrtDetector, named in
// IObjectDetector.hpp:9) owns a TensorRT engine; this one owns no network: whoever constructs it supplies
//     void hook(const void* d_input, void* d_output, int batch, void* stream)
// which must enqueue, on `stream`, work that reads batch x 3 x input_h x input_w values at d_input (fp32, or fp16 with half) and
// writes batch x max_candidates x 6 floats [x1, y1, x2, y2, confidence, class_id] (network-input coordinates) at d_output.
// Everything -- upload, preprocess, hook, postprocess, download -- is ordered on the handle's one stream.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct ObjectDetectorConfig {
    int input_w = 640, input_h = 640;      // TRTInference.cpp:38-40
    int max_candidates = 300;              // rows of the head the hook writes per frame (:105)
    int max_batch = 1;
    bool half = false;                     // the hook wants fp16 input
    // The port documents RGB input (IObjectDetector.hpp:15) and the network wants RGB, so nothing is swapped by default;
    // true reproduces TRTInference::preprocess on a BGR image (:75).
    bool swap_rb = false;
    std::vector<int> dynamic_classes;      // ids whose boxes deviceBoxes() lists; empty = the ten of src/main.cpp:29-40
    bool all_classes = false;              // every class is dynamic
    int device = 0;
    void* stream = nullptr;                // borrowed hipStream_t, or nullptr: the handle owns one
};

// The members are inline (below the class): FrontEnd and the factory use them, and they need nothing but the C-ABI.
class HipObjectDetector : public interfaces::IObjectDetector {
public:
    using InferenceHook = std::function<void(const void* d_input, void* d_output, int batch, void* stream)>;

    explicit HipObjectDetector(InferenceHook hook, const ObjectDetectorConfig& cfg = {});
    ~HipObjectDetector() override;

    // IObjectDetector: RGB, row-major, 3 channels (IObjectDetector.hpp:15)
    void detect(const std::uint8_t* image_data, int width, int height, std::vector<core::Detection>& detections,
                float conf_threshold = 0.5f, float nms_threshold = 0.45f) override;
    void detectAsync(const std::uint8_t* image_data, int width, int height) override;
    void getDetections(std::vector<core::Detection>& detections, float conf_threshold = 0.5f, float nms_threshold = 0.45f) override;
    void sync() override;

    // The front end's images are gray (IFeatureExtractor.hpp:14): the plane is written three times, what cvtColor GRAY2BGR in
    // front of detect() gives in the reference (src/euroc_eval.cpp:149), without building the 3-channel image.
    void detectGray(const std::uint8_t* image_data, int width, int height, std::vector<core::Detection>& detections,
                    float conf_threshold = 0.5f, float nms_threshold = 0.45f);
    void detectGrayAsync(const std::uint8_t* image_data, int width, int height);

    // Batch path: n_frames images already in HBM (the batch extractor's frame buffer, as it lies), results left in HBM.
    void detectBatchDevice(const std::uint8_t* d_images, int n_frames, int width, int height, int row_stride, std::int64_t frame_stride,
                           int channels, float conf_threshold = 0.5f, float nms_threshold = 0.45f);
    // The lists the last getDetections / detectBatchDevice left in HBM, in the layout aria_flag_keypoints_device reads
    // (frame f's boxes at boxes + f * cap). They belong to the handle.
    struct DeviceBoxes {
        const aria_box* boxes = nullptr;
        const int* n_boxes = nullptr;
        const aria_detection* detections = nullptr;
        const int* n_detections = nullptr;
        int cap = 0;
    };
    DeviceBoxes deviceBoxes() const { return lists_; }
    // aria_det_check: ARIA_OK or ARIA_E_OUTPUT_TOO_SMALL (cannot happen with the handle's own lists, which hold every candidate)
    int check();
    void* stream() const;
    int device() const { return cfg_.device; }
    const ObjectDetectorConfig& config() const { return cfg_; }

private:
    [[noreturn]] static void fail(const char* where, int status) { detail::fail("HipObjectDetector", where, status); }
    static void expect(const char* where, int rc) { detail::expect("HipObjectDetector", where, rc); }
    void enqueue(const std::uint8_t* image_data, int width, int height, int channels);
    void postprocess(int n_frames, int width, int height, float conf, float nms);
    ObjectDetectorConfig cfg_;
    InferenceHook hook_;
    detail::DeviceScratch img_;         // the uploaded host image; before h_ (see Stage.hpp, DECLARATION ORDER)
    detail::StageOwner<aria_det_t, aria_det_destroy> h_;
    void* d_input_ = nullptr;
    float* d_raw_ = nullptr;
    DeviceBoxes lists_;
    aria_detection* d_dets_ = nullptr;
    int* d_ndets_ = nullptr;
    aria_box* d_boxes_ = nullptr;
    int* d_nboxes_ = nullptr;
    bool pending_ = false;
    int pending_w_ = 0, pending_h_ = 0;
};

// Out-of-line constructor call for callers that prefer not to instantiate the class themselves (HipObjectDetector.cpp).
interfaces::ObjectDetectorPtr makeObjectDetector(HipObjectDetector::InferenceHook hook, const ObjectDetectorConfig& cfg = {});

// ---- implementation

static_assert(sizeof(core::Detection) == sizeof(aria_detection), "core::Detection must be the 24-byte aria_detection");

inline HipObjectDetector::HipObjectDetector(InferenceHook hook, const ObjectDetectorConfig& cfg)
    : cfg_(cfg), hook_(std::move(hook)), img_("HipObjectDetector", cfg.device) {
    if (!hook_) throw std::invalid_argument("HipObjectDetector: an inference hook is required (there is no built-in network)");
    if (cfg_.dynamic_classes.size() > ARIA_DET_MAX_CLASS_IDS) throw std::invalid_argument("HipObjectDetector: more than 32 dynamic classes");
    aria_det_config c;
    aria_det_default_config(&c);
    c.device = cfg_.device;
    c.stream = cfg_.stream;
    c.input_w = cfg_.input_w;
    c.input_h = cfg_.input_h;
    c.max_batch = cfg_.max_batch;
    c.max_candidates = cfg_.max_candidates;
    c.out_half = cfg_.half ? 1 : 0;
    expect("aria_det_create", aria_det_create(&c, h_.out()));
    void* in = nullptr;
    expect("aria_det_device_buffers", aria_det_device_buffers(h_.get(), &in, &d_raw_, &d_dets_, &d_ndets_, &d_boxes_, &d_nboxes_));
    d_input_ = in;
}

inline HipObjectDetector::~HipObjectDetector() = default;

inline void* HipObjectDetector::stream() const { return aria_det_stream(h_.get()); }

inline int HipObjectDetector::check() {
    const int rc = aria_det_check(h_.get(), nullptr, nullptr);
    if (rc != ARIA_OK && rc != ARIA_E_OUTPUT_TOO_SMALL) fail("aria_det_check", rc);
    return rc;
}

inline void HipObjectDetector::sync() {
    expect("aria_stream_synchronize", aria_stream_synchronize(cfg_.device, stream()));
}

// upload, preprocess and the hook of one host image, all on the handle's stream; nothing is waited for (TRTInference.cpp:171-192)
inline void HipObjectDetector::enqueue(const std::uint8_t* image_data, int width, int height, int channels) {
    if (!image_data || width < 1 || height < 1) throw std::invalid_argument("HipObjectDetector: bad image");
    const std::size_t bytes = (std::size_t)width * height * channels;
    img_.reserve(stream(), bytes);
    expect("aria_copy_h2d_async", aria_copy_h2d_async(cfg_.device, stream(), img_.data(), image_data, bytes));
    expect("aria_det_preprocess_batch_device",
           aria_det_preprocess_batch_device(h_.get(), (const std::uint8_t*)img_.data(), 1, width, height, width * channels, (std::int64_t)bytes,
                                            channels, cfg_.swap_rb ? 1 : 0, d_input_));
    hook_(d_input_, d_raw_, 1, stream());
    pending_ = true;
    pending_w_ = width;
    pending_h_ = height;
}

inline void HipObjectDetector::postprocess(int n_frames, int width, int height, float conf, float nms) {
    const int* ids = cfg_.dynamic_classes.empty() ? nullptr : cfg_.dynamic_classes.data();
    const int n_ids = cfg_.all_classes ? -1 : (int)cfg_.dynamic_classes.size();
    const int cap = cfg_.max_candidates;
    expect("aria_det_postprocess_batch_device",
           aria_det_postprocess_batch_device(h_.get(), d_raw_, n_frames, cap, width, height, conf, nms, ids, n_ids, d_dets_, d_ndets_, cap,
                                             d_boxes_, d_nboxes_, cap));
    lists_.boxes = d_boxes_;
    lists_.n_boxes = d_nboxes_;
    lists_.detections = d_dets_;
    lists_.n_detections = d_ndets_;
    lists_.cap = cap;
}

inline void HipObjectDetector::detectAsync(const std::uint8_t* image_data, int width, int height) { enqueue(image_data, width, height, 3); }
inline void HipObjectDetector::detectGrayAsync(const std::uint8_t* image_data, int width, int height) { enqueue(image_data, width, height, 1); }

// TRTInference::getDetections (TRTInference.cpp:195-199): the thresholds arrive here, after the network has run
inline void HipObjectDetector::getDetections(std::vector<core::Detection>& detections, float conf_threshold, float nms_threshold) {
    detections.clear();
    if (!pending_) return;
    pending_ = false;
    postprocess(1, pending_w_, pending_h_, conf_threshold, nms_threshold);
    int n = 0;
    expect("aria_copy_d2h_async", aria_copy_d2h_async(cfg_.device, stream(), &n, d_ndets_, sizeof(int)));
    sync();
    if (n <= 0) return;
    detections.resize((std::size_t)n);
    expect("aria_copy_d2h_async",
           aria_copy_d2h_async(cfg_.device, stream(), detections.data(), d_dets_, (std::size_t)n * sizeof(aria_detection)));
    sync();
}

inline void HipObjectDetector::detect(const std::uint8_t* image_data, int width, int height, std::vector<core::Detection>& detections,
                               float conf_threshold, float nms_threshold) {
    detectAsync(image_data, width, height);
    getDetections(detections, conf_threshold, nms_threshold);
}

inline void HipObjectDetector::detectGray(const std::uint8_t* image_data, int width, int height, std::vector<core::Detection>& detections,
                                   float conf_threshold, float nms_threshold) {
    detectGrayAsync(image_data, width, height);
    getDetections(detections, conf_threshold, nms_threshold);
}

inline void HipObjectDetector::detectBatchDevice(const std::uint8_t* d_images, int n_frames, int width, int height, int row_stride,
                                          std::int64_t frame_stride, int channels, float conf_threshold, float nms_threshold) {
    expect("aria_det_preprocess_batch_device",
           aria_det_preprocess_batch_device(h_.get(), d_images, n_frames, width, height, row_stride, frame_stride, channels,
                                            cfg_.swap_rb ? 1 : 0, d_input_));
    hook_(d_input_, d_raw_, n_frames, stream());
    postprocess(n_frames, width, height, conf_threshold, nms_threshold);
}

}  // namespace aria::adapters::hip
