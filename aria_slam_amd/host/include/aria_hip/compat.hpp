// Stand-in for the two reference headers the adapters need, for builds where the reference tree (and Eigen,
// which its core/Types.hpp includes) is not on the include path -- e.g. this repository's own tests.
//
// In an aria-slam checkout, compile the adapters with -DARIA_HIP_USE_REFERENCE_HEADERS -I<aria-slam>/include and
// this file forwards to the real ports (include/interfaces/IFeatureExtractor.hpp, include/interfaces/IMatcher.hpp,
// include/core/Types.hpp). Otherwise it declares layout-compatible minimal versions of exactly the members the
// hot path touches: KeyPoint (24 B), Match (12 B), the Frame fields the extractor fills, and the two ports.
#pragma once

#ifdef ARIA_HIP_USE_REFERENCE_HEADERS
#include "interfaces/IAudioFeedback.hpp"
#include "interfaces/IFeatureExtractor.hpp"
#include "interfaces/ILoopDetector.hpp"
#include "interfaces/IMapper.hpp"
#include "interfaces/IMatcher.hpp"
#include "interfaces/IObjectDetector.hpp"
#include "interfaces/ISensorFusion.hpp"
#else

#include <cstddef>
#include <cstdint>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace aria::core {

struct KeyPoint {
    float x, y, size, angle, response;
    int octave;
};

struct Frame {
    std::uint64_t id = 0;
    double timestamp = 0.0;
    int width = 0, height = 0;
    std::vector<KeyPoint> keypoints;
    std::vector<std::uint8_t> descriptors;                    // N x 32, row-major
    alignas(16) double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // Eigen::Matrix4d in the reference
    std::size_t descriptorSize() const { return 32; }
    std::size_t numKeypoints() const { return keypoints.size(); }
};

struct Match {
    int query_idx, train_idx;
    float distance;
};

// include/core/Types.hpp:103-112 (the box test of SlamPipeline::filterDynamicKeypoints, SlamPipeline.hpp:96-99)
struct Detection {
    float x1, y1, x2, y2;
    float confidence;
    int class_id;
    bool contains(float x, float y) const { return x >= x1 && x <= x2 && y >= y1 && y <= y2; }
};

// include/core/Types.hpp:33-45: the members the loop-closure path touches (pose members are Eigen types there)
struct KeyFrame {
    std::uint64_t id = 0;
    double timestamp = 0.0;
    Frame frame;
    alignas(16) double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

// include/core/Types.hpp:114-121
struct LoopCandidate {
    std::uint64_t query_id = 0;
    std::uint64_t match_id = 0;
    double score = 0.0;
    std::vector<Match> matches;
    alignas(16) double relative_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

// Minimal stand-ins for the three Eigen types the mapper port uses (Vector3d, Matrix3d, Matrix4d): element access only
template <int R, int C>
struct Matrix {
    double d[R * C] = {};
    double& operator()(int r, int c) { return d[r * C + c]; }
    double operator()(int r, int c) const { return d[r * C + c]; }
    double& operator()(int i) { return d[i]; }
    double operator()(int i) const { return d[i]; }
    static Matrix Identity() {
        Matrix m;
        for (int i = 0; i < (R < C ? R : C); i++) m(i, i) = 1.0;
        return m;
    }
};
using Vector3 = Matrix<3, 1>;
using Matrix3 = Matrix<3, 3>;
using Matrix4 = Matrix<4, 4>;

struct Quaternion {
    double w = 1, x = 0, y = 0, z = 0;
};

// include/core/Types.hpp:48-66 (descriptor, observations, num_observations: what the mapper fills)
struct MapPoint {
    std::uint64_t id = 0;
    Vector3 position;
    Vector3 normal;
    std::vector<std::uint8_t> descriptor;
    std::vector<std::pair<std::uint64_t, int>> observations;   // keyframe id -> keypoint index
    int num_observations = 0;
    float min_distance = 0.0f, max_distance = 0.0f;
    bool is_bad = false;
};

// include/core/Types.hpp:69-88: position + orientation; toMatrix() = [R(q) t; 0 1]
struct Pose {
    Vector3 position;
    Quaternion orientation;
    double timestamp = 0.0;
    Matrix<6, 6> covariance = Matrix<6, 6>::Identity();
    Matrix4 toMatrix() const {
        const double w = orientation.w, x = orientation.x, y = orientation.y, z = orientation.z;
        Matrix4 T = Matrix4::Identity();
        T(0, 0) = 1 - 2 * (y * y + z * z); T(0, 1) = 2 * (x * y - z * w); T(0, 2) = 2 * (x * z + y * w);
        T(1, 0) = 2 * (x * y + z * w); T(1, 1) = 1 - 2 * (x * x + z * z); T(1, 2) = 2 * (y * z - x * w);
        T(2, 0) = 2 * (x * z - y * w); T(2, 1) = 2 * (y * z + x * w); T(2, 2) = 1 - 2 * (x * x + y * y);
        for (int r = 0; r < 3; r++) T(r, 3) = position(r);
        return T;
    }
};

// include/core/Types.hpp:90-94
struct ImuMeasurement {
    double timestamp = 0.0;
    Vector3 accel;          // m/s^2
    Vector3 gyro;           // rad/s
};

}  // namespace aria::core

namespace aria::interfaces {

class IFeatureExtractor {
public:
    virtual ~IFeatureExtractor() = default;
    virtual void extract(const std::uint8_t* image_data, int width, int height, core::Frame& frame) = 0;
    virtual void extractAsync(const std::uint8_t* image_data, int width, int height, core::Frame& frame) {
        extract(image_data, width, height, frame);
    }
    virtual void sync() {}
    virtual void setMaxFeatures(int n) = 0;
    virtual int getMaxFeatures() const = 0;
};
using FeatureExtractorPtr = std::unique_ptr<IFeatureExtractor>;

class IMatcher {
public:
    virtual ~IMatcher() = default;
    virtual void match(const core::Frame& query, const core::Frame& train, std::vector<core::Match>& matches,
                       float ratio_threshold = 0.75f) = 0;
    virtual void matchMultiple(const core::Frame& query, const std::vector<core::Frame>& candidates,
                               std::vector<std::vector<core::Match>>& all_matches, float ratio_threshold = 0.75f) {
        all_matches.resize(candidates.size());
        for (std::size_t i = 0; i < candidates.size(); i++) match(query, candidates[i], all_matches[i], ratio_threshold);
    }
};
using MatcherPtr = std::unique_ptr<IMatcher>;

// include/interfaces/IObjectDetector.hpp:10-48 (image_data: RGB, row-major, 3 channels)
class IObjectDetector {
public:
    virtual ~IObjectDetector() = default;
    virtual void detect(const std::uint8_t* image_data, int width, int height, std::vector<core::Detection>& detections,
                        float conf_threshold = 0.5f, float nms_threshold = 0.45f) = 0;
    virtual void detectAsync(const std::uint8_t* image_data, int width, int height) = 0;
    virtual void getDetections(std::vector<core::Detection>& detections, float conf_threshold = 0.5f,
                               float nms_threshold = 0.45f) = 0;
    virtual void sync() = 0;
};
using ObjectDetectorPtr = std::unique_ptr<IObjectDetector>;

// include/interfaces/ILoopDetector.hpp:11-31
class ILoopDetector {
public:
    virtual ~ILoopDetector() = default;
    virtual void addKeyFrame(const core::KeyFrame& kf) = 0;
    virtual std::optional<core::LoopCandidate> detect(const core::KeyFrame& query) = 0;
    virtual int getLoopCount() const = 0;
    virtual void setMinFramesBetween(int n) = 0;
    virtual void setMinScore(double s) = 0;
    virtual void setMinMatches(int n) = 0;
};
using LoopDetectorPtr = std::unique_ptr<ILoopDetector>;

// include/interfaces/IMapper.hpp:11-45
class IMapper {
public:
    virtual ~IMapper() = default;
    virtual void triangulate(const core::Frame& frame1, const core::Frame& frame2, const core::Pose& pose1, const core::Pose& pose2,
                             const std::vector<core::Match>& matches, const core::Matrix3& K,
                             std::vector<core::MapPoint>& new_points) = 0;
    virtual const std::vector<core::MapPoint>& getMapPoints() const = 0;
    virtual void exportPLY(const std::string& filename) const = 0;
    virtual void exportPCD(const std::string& filename) const = 0;
    virtual void clear() = 0;
    virtual std::size_t size() const = 0;
};
using MapperPtr = std::unique_ptr<IMapper>;

// include/interfaces/ISensorFusion.hpp:9-30 (getVelocity returns Eigen::Vector3d there)
class ISensorFusion {
public:
    virtual ~ISensorFusion() = default;
    virtual void predictIMU(const core::ImuMeasurement& imu) = 0;
    virtual void updateVO(const core::Pose& vo_pose) = 0;
    virtual core::Pose getFusedPose() const = 0;
    virtual core::Vector3 getVelocity() const = 0;
    virtual void reset() = 0;
    virtual void reset(const core::Pose& initial_pose) = 0;
};
using SensorFusionPtr = std::unique_ptr<ISensorFusion>;

// include/interfaces/IAudioFeedback.hpp:7-78 (the port has no adapter in the reference; the obstacle alerter speaks through it)
enum class AudioPriority { LOW, MEDIUM, HIGH, CRITICAL };
enum class AudioDirection { CENTER, LEFT, RIGHT, BEHIND };
class IAudioFeedback {
public:
    virtual ~IAudioFeedback() = default;
    virtual bool initialize() = 0;
    virtual void shutdown() = 0;
    virtual bool isReady() const = 0;
    virtual void speak(const std::string& text, AudioPriority priority = AudioPriority::MEDIUM, bool interrupt = false) = 0;
    virtual void playBeep(AudioDirection direction, int frequency_hz = 800, int duration_ms = 200, float volume = 0.7f) = 0;
    virtual void playCriticalAlert(AudioDirection direction) = 0;
    virtual void setVolume(float volume) = 0;
    virtual float getVolume() const = 0;
    virtual void setMuted(bool muted) = 0;
    virtual bool isMuted() const = 0;
    virtual void spinOnce() = 0;
};
using AudioFeedbackPtr = std::unique_ptr<IAudioFeedback>;

}  // namespace aria::interfaces

#endif  // ARIA_HIP_USE_REFERENCE_HEADERS
