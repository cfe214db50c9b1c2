// aria::factory -- the HIP execution mode of the reference's PipelineFactory (include/factory/PipelineFactory.hpp:9-47):
// FactoryConfig{mode, cuda_device, max_features} selects which adapters are injected into SlamPipeline's constructor
// (include/pipeline/SlamPipeline.hpp:32-40). createHipComponents() builds the three front-end components the HIP mode
// injects -- extractor, matcher, loop detector -- and createHip() wires them into the FrontEnd (the part of SlamPipeline
// this repository implements). INTEGRATION.md shows the ExecutionMode::HIP branch a maintainer adds to
// PipelineFactory::create with exactly these calls.
#pragma once
#include <memory>

#include "aria_hip/FrontEnd.hpp"
#include "aria_hip/HipObjectDetector.hpp"
#include "aria_hip/HipObstacleAlerter.hpp"
#include "aria_hip/compat.hpp"

namespace aria::factory {

struct HipFactoryConfig {
    int hip_device = 0;            // FactoryConfig::cuda_device (PipelineFactory.hpp:24)
    int max_features = 1000;       // FactoryConfig::max_features (:27)
    void* stream = nullptr;        // borrowed hipStream_t shared by the three components, or nullptr: createHip() then makes
                                   // one stream for extractor + matcher (and keeps it alive as long as the FrontEnd)
    pipeline::FrontEndConfig frontend;
    bool enable_loop_closure = true;        // PipelineConfig::enable_loop_closure (SlamPipeline.hpp:17)
    int loop_min_frames_between = 200;      // src/euroc_eval.cpp:103
    double loop_min_score = 0.4;
    int loop_min_matches = 50;
};

struct HipComponents {
    interfaces::FeatureExtractorPtr extractor;
    interfaces::MatcherPtr matcher;
    interfaces::LoopDetectorPtr loop_detector;      // null when loop closure is disabled
    std::shared_ptr<void> shared_stream;            // owner of the stream made for the components (empty: caller's stream or
                                                    // none); must be released after them
};

HipComponents createHipComponents(const HipFactoryConfig& cfg);
std::unique_ptr<pipeline::FrontEnd> createHip(const HipFactoryConfig& cfg = {});
// The fourth component SlamPipeline's constructor takes (include/pipeline/SlamPipeline.hpp:32-40): the detector around the
// caller's network, on cfg.hip_device. It gets a stream of its own unless det.stream names one (the reference's detector has
// its own too, TRTInference.cpp:53), so it runs beside the extraction. createHip(cfg, hook) also injects it into the FrontEnd.
interfaces::ObjectDetectorPtr createHipDetector(const HipFactoryConfig& cfg, adapters::hip::HipObjectDetector::InferenceHook hook,
                                                adapters::hip::ObjectDetectorConfig det = {});
std::unique_ptr<pipeline::FrontEnd> createHip(const HipFactoryConfig& cfg, adapters::hip::HipObjectDetector::InferenceHook hook,
                                              adapters::hip::ObjectDetectorConfig det = {});
// The consumer of a frame's depth map and boxes (the sketch's NavigationAudioEngine, H16:421-493) on cfg.hip_device: it speaks
// through `audio` (not owned; nullptr = events only) and names detections by class_names.
std::unique_ptr<adapters::hip::HipObstacleAlerter> createHipAlerter(const HipFactoryConfig& cfg, interfaces::IAudioFeedback* audio,
                                                                    std::vector<std::string> class_names = {},
                                                                    adapters::hip::ObstacleAlerterConfig alert = {});

}  // namespace aria::factory
