// Reader for the on-disk format either side of the hot path: the ASL / EuRoC MAV layout
//     <root>/mav0/cam0/data.csv      "#timestamp [ns],filename" then "1403636579763555584,1403636579763555584.png"
//     <root>/mav0/cam0/data/*.png    8-bit grayscale 752x480
// as the reference reads it (src/legacy/EuRoCReader.cpp:23-27, 70-108: skip header/comment lines, split at the
// first comma, trim, sort by timestamp; :277-309: imread(IMREAD_GRAYSCALE)). OpenCV's imgcodecs is replaced by a
// dependency-free PNG decoder (zlib inflate only): 8-bit, non-interlaced, colour types 0 (gray), 2 (RGB), 4 (gray+a),
// 6 (RGBA); colour is converted with OpenCV's BGR2GRAY fixed-point weights.
//     <root>/mav0/imu0/data.csv      "#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z": gyro in columns 1-3, accelerometer in 4-6
// is read when it is there (EuRoCReader.cpp:110-154: rows of fewer than 7 fields dropped, sorted by timestamp), together with
// the samples every image consumes (getNext, :295-305: prev_image_time < t <= image_time, 0 before the first image); a
// sequence without imu0 still loads.
//     <root>/mav0/state_groundtruth_estimate0/data.csv   "#timestamp, p xyz, q wxyz, v xyz, b_w xyz, b_a xyz" (17 fields)
// is read when it is there (EuRoCReader.cpp:37-41, 157-216: rows of fewer than 17 fields dropped, sorted by timestamp -- a
// stable sort here, ours by definition), else <root>/mav0/leica0/data.csv is tried as the reference does. A Leica file has 4
// fields per row, so under the 17-field rule the fallback yields no rows, exactly as in the reference; a sequence without
// ground truth still loads.
//     <root>/mav0/cam1/data.csv + data/*.png   the right camera of a stereo rig, in cam0's format
// is read when it is there (the reference's reader names cam1 and never reads it): a cam1 image is paired with the cam0 image
// of EQUAL timestamp (the parsed seconds are compared). hasRight(i) tells whether image i has a partner; a sequence without
// cam1 loads exactly as before.
// The stereo stage (aria_hip/HipStereoMatcher.hpp) needs RECTIFIED pairs; this reader does not rectify: see aria_rect_*
// (aria_hip/HipRectifier.hpp), which takes the calibration read here.
//     <root>/mav0/cam0/sensor.yaml, <root>/mav0/cam1/sensor.yaml
// are read when they are there, key by key and line by line as the reference reads cam0's (EuRoCReader.cpp:220-275:
// "intrinsics:" and "distortion_coefficients:" as bracketed lists on the key's line), plus "resolution:" and the 16 values of
// T_BS's "data:" list, which may run over several lines. hasCalibration(cam) tells whether camera cam (0 or 1) has one; a
// sequence without them loads exactly as before.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace aria::io {

struct AslImage {
    double timestamp = 0.0;          // seconds (EuRoCReader::parseTimestamp: ns * 1e-9)
    std::string path;
};

struct AslImu {
    double timestamp = 0.0;          // seconds
    double accel[3] = {0, 0, 0};     // m/s^2
    double gyro[3] = {0, 0, 0};      // rad/s
};

struct AslGroundTruth {              // the 17 doubles of aria_eval_truth, in its order
    double timestamp = 0.0;          // seconds
    double p[3] = {0, 0, 0};
    double q[4] = {1, 0, 0, 0};      // w, x, y, z
    double v[3] = {0, 0, 0};
    double bg[3] = {0, 0, 0};
    double ba[3] = {0, 0, 0};
};

struct AslCalibration {             // one camera's sensor.yaml
    double intrinsics[4] = {0, 0, 0, 0};     // fx, fy, cx, cy
    double distortion[5] = {0, 0, 0, 0, 0};  // radtan k1, k2, p1, p2, k3 (k3 = 0 when the file has four); KB4 k1, k2, k3, k4, 0
    double T_BS[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // sensor to body, row-major
    int width = 0, height = 0;               // resolution, 0 when the file has none
    std::string distortion_model;            // "radial-tangential" in EuRoC; empty when the file has none
    // The model as aria_rect_config::model takes it: 0 (ARIA_RECT_MODEL_RADTAN) for "radial-tangential", "radtan", "plumb_bob"
    // and a file without the key, 1 (ARIA_RECT_MODEL_KB4) for "equidistant", "fisheye" and "kb4", -1 for any other name.
    int rectModel() const {
        const std::string& m = distortion_model;
        if (m.empty() || m == "radial-tangential" || m == "radtan" || m == "plumb_bob") return 0;
        if (m == "equidistant" || m == "fisheye" || m == "kb4") return 1;
        return -1;
    }
};

class AslSequence {
public:
    // dataset_path may be the sequence root (containing mav0/) or the mav0 directory itself
    bool load(const std::string& dataset_path);
    std::size_t size() const { return images_.size(); }
    const AslImage& at(std::size_t i) const { return images_[i]; }
    // Decodes image i to 8-bit grayscale, row-major, tightly packed. Throws std::runtime_error on a bad file.
    void read(std::size_t i, std::vector<std::uint8_t>& gray, int& width, int& height) const;
    // imu0, sorted by timestamp (empty without imu0), and the samples [imuBegin(i), imuEnd(i)) that image i consumes
    const std::vector<AslImu>& imu() const { return imu_; }
    std::size_t imuBegin(std::size_t i) const { return imu_begin_[i]; }
    std::size_t imuEnd(std::size_t i) const { return imu_end_[i]; }
    // ground truth, sorted by timestamp (empty when the sequence has none)
    const std::vector<AslGroundTruth>& groundTruth() const { return ground_truth_; }
    bool hasGroundTruth() const { return !ground_truth_.empty(); }
    // cam1: whether image i has a right image of equal timestamp, and its decoded pixels (throws like read())
    bool hasRight(std::size_t i) const { return i < right_.size() && !right_[i].empty(); }
    bool hasStereo() const;          // cam1 is there and every cam0 image has its partner
    void readRight(std::size_t i, std::vector<std::uint8_t>& gray, int& width, int& height) const;
    // sensor.yaml of cam0 (cam = 0) / cam1 (cam = 1): whether it was there with four intrinsics, and its content (throws
    // std::runtime_error without one)
    bool hasCalibration(int cam) const { return cam >= 0 && cam < 2 && has_calibration_[cam]; }
    const AslCalibration& calibration(int cam) const;

private:
    std::vector<AslImage> images_;
    std::vector<std::string> right_;             // per image: path of the cam1 partner, empty without one
    std::vector<AslImu> imu_;
    std::vector<std::size_t> imu_begin_, imu_end_;
    std::vector<AslGroundTruth> ground_truth_;
    AslCalibration calibration_[2];
    bool has_calibration_[2] = {false, false};
};

// One sensor.yaml (see header comment). False when the file is missing or holds no four intrinsics.
bool load_sensor_yaml(const std::string& path, AslCalibration& out);

// PNG -> 8-bit grayscale (see header comment). Throws std::runtime_error.
void decode_png_gray(const std::vector<std::uint8_t>& file, std::vector<std::uint8_t>& gray, int& width, int& height);

}  // namespace aria::io
