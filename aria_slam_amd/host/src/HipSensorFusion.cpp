// See aria_hip/HipSensorFusion.hpp.
#include "aria_hip/HipSensorFusion.hpp"

#include <stdexcept>
#include <string>

namespace aria::adapters::hip {

namespace {

// the two header sets spell a quaternion differently: accessors with the reference's Eigen type, fields in the stand-in
#ifdef ARIA_HIP_USE_REFERENCE_HEADERS
void quatOf(const core::Pose& p, double q[4]) {
    q[0] = p.orientation.w(); q[1] = p.orientation.x(); q[2] = p.orientation.y(); q[3] = p.orientation.z();
}
void setQuat(core::Pose& p, const double q[4]) { p.orientation = Eigen::Quaterniond(q[0], q[1], q[2], q[3]); }
#else
void quatOf(const core::Pose& p, double q[4]) {
    q[0] = p.orientation.w; q[1] = p.orientation.x; q[2] = p.orientation.y; q[3] = p.orientation.z;
}
void setQuat(core::Pose& p, const double q[4]) { p.orientation = core::Quaternion{q[0], q[1], q[2], q[3]}; }
#endif

// Eigen's toRotationMatrix, row-major
void rotOf(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
                 tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

}  // namespace

HipSensorFusion::HipSensorFusion(const aria_fuse_config* cfg) {
    aria_fuse_default_config(&cfg_);
    if (cfg) cfg_ = *cfg;
    expect("aria_fuse_filter_init", aria_fuse_filter_init(&filter_, &cfg_));
    expect("aria_fuse_create", aria_fuse_create(&cfg_, h_.out()));
}

HipSensorFusion::~HipSensorFusion() = default;

void HipSensorFusion::addIMU(double t, const double accel[3], const double gyro[3]) {
    aria_imu_sample s{};
    s.t = t;
    for (int k = 0; k < 3; k++) { s.accel[k] = accel[k]; s.gyro[k] = gyro[k]; }
    imu_.push_back(s);
}

void HipSensorFusion::addVisualPose(double t, const double R[9], const double p[3]) {
    aria_fuse_visual v{};
    v.t = t;
    for (int k = 0; k < 9; k++) v.R[k] = R[k];
    for (int k = 0; k < 3; k++) v.p[k] = p[k];
    v.accept = 1;
    imu_end_.push_back((int)imu_.size());
    visual_.push_back(v);
}

void HipSensorFusion::predictIMU(const core::ImuMeasurement& imu) {
    const double a[3] = {imu.accel(0), imu.accel(1), imu.accel(2)}, g[3] = {imu.gyro(0), imu.gyro(1), imu.gyro(2)};
    addIMU(imu.timestamp, a, g);
}

void HipSensorFusion::updateVO(const core::Pose& vo_pose) {
    double q[4], R[9];
    quatOf(vo_pose, q);
    rotOf(q, R);
    const double p[3] = {vo_pose.position(0), vo_pose.position(1), vo_pose.position(2)};
    addVisualPose(vo_pose.timestamp, R, p);
}

void HipSensorFusion::flush() const {
    if (!imu_.empty() && (imu_end_.empty() || imu_end_.back() < (int)imu_.size())) {
        // samples after the last visual pose: a frame without a measurement consumes them
        aria_fuse_visual v{};
        v.t = imu_.back().t;
        v.R[0] = v.R[4] = v.R[8] = 1.0;
        v.accept = 0;
        imu_end_.push_back((int)imu_.size());
        visual_.push_back(v);
    }
    if (visual_.empty()) return;
    states_.assign(visual_.size(), aria_fuse_state{});
    const int rc = aria_fuse_run(h_.get(), &filter_, imu_.data(), (int)imu_.size(), imu_end_.data(), visual_.data(), (int)visual_.size(),
                                 states_.data());
    imu_.clear();
    imu_end_.clear();
    visual_.clear();
    expect("aria_fuse_run", rc);
}

void HipSensorFusion::run(const aria_imu_sample* imu, int n_imu, const int* imu_end, const aria_fuse_visual* visual, int n_frames,
                          aria_fuse_state* states) {
    flush();
    expect("aria_fuse_run", aria_fuse_run(h_.get(), &filter_, imu, n_imu, imu_end, visual, n_frames, states));
}

const aria_fuse_filter& HipSensorFusion::filter() const {
    flush();
    return filter_;
}

bool HipSensorFusion::isInitialized() const { return filter().initialized != 0; }

core::Pose HipSensorFusion::getFusedPose() const {
    const aria_fuse_filter& f = filter();
    core::Pose out;
    for (int k = 0; k < 3; k++) out.position(k) = f.p[k];
    setQuat(out, f.q);
    out.timestamp = f.last_imu_time;
    static const int h[6] = {0, 1, 2, 6, 7, 8};
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) out.covariance(a, b) = f.P[h[a] * 15 + h[b]];
    return out;
}

FusionVec3 HipSensorFusion::getVelocity() const {
    const aria_fuse_filter& f = filter();
    FusionVec3 v;
    for (int k = 0; k < 3; k++) v(k) = f.v[k];
    return v;
}

void HipSensorFusion::reset() {
    imu_.clear();
    imu_end_.clear();
    visual_.clear();
    states_.clear();
    expect("aria_fuse_filter_init", aria_fuse_filter_init(&filter_, &cfg_));
}

void HipSensorFusion::reset(const core::Pose& initial_pose) {
    reset();
    for (int k = 0; k < 3; k++) filter_.p[k] = initial_pose.position(k);
    quatOf(initial_pose, filter_.q);
    filter_.last_imu_time = filter_.last_visual_time = initial_pose.timestamp;
    filter_.initialized = 1;
}

}  // namespace aria::adapters::hip
