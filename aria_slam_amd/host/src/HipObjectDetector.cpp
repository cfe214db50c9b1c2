// See aria_hip/HipObjectDetector.hpp: the adapter's members are inline there (FrontEnd and the factory use them from translation
// units that are also built without this file). This unit only makes the library carry one out-of-line copy of them.
#include "aria_hip/HipObjectDetector.hpp"

namespace aria::adapters::hip {

interfaces::ObjectDetectorPtr makeObjectDetector(HipObjectDetector::InferenceHook hook, const ObjectDetectorConfig& cfg) {
    return std::make_unique<HipObjectDetector>(std::move(hook), cfg);
}

}  // namespace aria::adapters::hip
