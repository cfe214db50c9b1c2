// aria::adapters::hip::HipSensorFusion -- the ISensorFusion port (include/interfaces/ISensorFusion.hpp, the slot
// SlamPipeline.hpp:37, 57-58, 78 leaves for it) over the C-ABI (include/aria_orb_hip.h, "visual-inertial fusion"): the
// reference's SensorFusion EKF (include/legacy/IMU.hpp:53-118, src/legacy/IMU.cpp:102-305) on the device.
// aria_slam_amd/fusion_ref.py is the definition of the stage; parity with an Eigen build of the reference is not pinned.
//
// predictIMU and updateVO queue their events on the host; a getter flushes the queue through one aria_fuse_run, the filter
// record (aria_fuse_filter) travelling with it, so the result does not depend on when the getters are called. updateVO hands
// the filter vo_pose.timestamp, R(vo_pose.orientation) and vo_pose.position, what addVisualPose takes (IMU.cpp:224); the
// first one initialises the filter. getFusedPose returns position, orientation, the filter's time (last_imu_time) and the
// 6x6 covariance of [position, orientation error], the blocks of P at the rows / columns {0, 1, 2, 6, 7, 8}. reset() is the
// constructor's state; reset(pose) starts the filter at that pose with zero velocity, initialised, as the first visual pose
// would.
//
// The array form run() and the legacy class's names (addIMU, addVisualPose) are there for drivers that hold whole sequences.
#pragma once
#include <vector>

#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

#ifdef ARIA_HIP_USE_REFERENCE_HEADERS
using FusionVec3 = Eigen::Vector3d;
#else
using FusionVec3 = core::Vector3;
#endif

class HipSensorFusion : public interfaces::ISensorFusion {
public:
    explicit HipSensorFusion(const aria_fuse_config* cfg = nullptr);     // nullptr: aria_fuse_default_config
    ~HipSensorFusion() override;

    // the port
    void predictIMU(const core::ImuMeasurement& imu) override;
    void updateVO(const core::Pose& vo_pose) override;
    core::Pose getFusedPose() const override;
    FusionVec3 getVelocity() const override;
    void reset() override;
    void reset(const core::Pose& initial_pose) override;

    // the legacy class's surface over plain arrays (IMU.hpp:67-77); R row-major
    void addIMU(double t, const double accel[3], const double gyro[3]);
    void addVisualPose(double t, const double R[9], const double p[3]);
    bool isInitialized() const;
    // the whole filter record after the queued events, and the per-frame states of the last flush
    const aria_fuse_filter& filter() const;
    const std::vector<aria_fuse_state>& lastStates() const { return states_; }
    // one track, host arrays, through aria_fuse_run on this object's filter; throws std::runtime_error on an error status
    void run(const aria_imu_sample* imu, int n_imu, const int* imu_end, const aria_fuse_visual* visual, int n_frames,
             aria_fuse_state* states);

private:
    static void expect(const char* where, int rc) { detail::expect("HipSensorFusion", where, rc); }
    void flush() const;
    detail::StageOwner<aria_fuse_t, aria_fuse_destroy> h_;
    aria_fuse_config cfg_{};
    mutable aria_fuse_filter filter_{};
    mutable std::vector<aria_imu_sample> imu_;
    mutable std::vector<int> imu_end_;
    mutable std::vector<aria_fuse_visual> visual_;
    mutable std::vector<aria_fuse_state> states_;
};

}  // namespace aria::adapters::hip
