// See aria_hip/AslSequence.hpp.
#include "aria_hip/AslSequence.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace aria::io {

namespace {

inline std::uint32_t be32(const std::uint8_t* p) { return ((std::uint32_t)p[0] << 24) | (p[1] << 16) | (p[2] << 8) | p[3]; }

inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

bool file_exists(const std::string& p) {
    std::ifstream f(p);
    return f.good();
}

// EuRoCReader::loadGroundTruth (:157-216). Returns whether any row was read.
bool load_ground_truth(const std::string& csv, std::vector<AslGroundTruth>& out) {
    std::ifstream file(csv);
    if (!file.is_open()) return false;
    std::string line;
    std::getline(file, line);                                                 // header (:166)
    while (std::getline(file, line)) {
        if (line.empty() || line[0] == '#') continue;                         // :169
        std::stringstream ss(line);
        std::string token;
        std::vector<std::string> tokens;
        while (std::getline(ss, token, ',')) tokens.push_back(token);
        if (tokens.size() < 17) continue;                                     // :179
        AslGroundTruth g;
        double* d = &g.timestamp;                                             // 17 packed doubles (static_assert below)
        d[0] = std::strtod(tokens[0].c_str(), nullptr) * 1e-9;
        for (std::size_t k = 1; k < 17; k++) d[k] = std::strtod(tokens[k].c_str(), nullptr);
        out.push_back(g);
    }
    std::stable_sort(out.begin(), out.end(), [](const AslGroundTruth& a, const AslGroundTruth& b) { return a.timestamp < b.timestamp; });
    return !out.empty();
}
static_assert(sizeof(AslGroundTruth) == 17 * sizeof(double), "AslGroundTruth is 17 packed doubles");

// "timestamp,filename" rows of a camera's data.csv (EuRoCReader.cpp:70-108), sorted by timestamp. False when the file is absent.
bool load_camera(const std::string& cam, std::vector<AslImage>& out) {
    std::ifstream file(cam + "/data.csv");
    if (!file.is_open()) return false;
    std::string line;
    std::getline(file, line);                                                 // header (EuRoCReader.cpp:78-79)
    while (std::getline(file, line)) {
        if (line.empty() || line[0] == '#') continue;                         // :82
        std::stringstream ss(line);
        std::string ts, name;
        std::getline(ss, ts, ',');
        std::getline(ss, name, ',');
        const auto b = name.find_first_not_of(" \t");
        if (b == std::string::npos) continue;
        name.erase(0, b);
        name.erase(name.find_last_not_of(" \t\r\n") + 1);                     // :90-91
        AslImage img;
        img.timestamp = std::strtod(ts.c_str(), nullptr) * 1e-9;              // nanoseconds -> seconds
        img.path = cam + "/data/" + name;
        out.push_back(img);
    }
    std::stable_sort(out.begin(), out.end(), [](const AslImage& a, const AslImage& b) { return a.timestamp < b.timestamp; });
    return true;
}

void read_gray(const std::string& path, std::vector<std::uint8_t>& gray, int& width, int& height) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<std::uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    decode_png_gray(bytes, gray, width, height);
}

}  // namespace

void decode_png_gray(const std::vector<std::uint8_t>& file, std::vector<std::uint8_t>& gray, int& width, int& height) {
    static const std::uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (file.size() < 8 + 25 || std::memcmp(file.data(), sig, 8) != 0) throw std::runtime_error("png: bad signature");
    std::size_t pos = 8;
    int w = 0, h = 0, depth = 0, ctype = -1, interlace = 0;
    std::vector<std::uint8_t> idat;
    bool done = false;
    while (!done && pos + 12 <= file.size()) {
        const std::uint32_t len = be32(&file[pos]);
        const char* type = reinterpret_cast<const char*>(&file[pos + 4]);
        if (pos + 12 + len > file.size()) throw std::runtime_error("png: truncated chunk");
        const std::uint8_t* data = &file[pos + 8];
        if (!std::memcmp(type, "IHDR", 4)) {
            if (len < 13) throw std::runtime_error("png: bad IHDR");
            w = (int)be32(data); h = (int)be32(data + 4); depth = data[8]; ctype = data[9]; interlace = data[12];
        } else if (!std::memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), data, data + len);
        } else if (!std::memcmp(type, "IEND", 4)) {
            done = true;
        }
        pos += 12 + len;
    }
    if (w <= 0 || h <= 0 || w > 16384 || h > 16384) throw std::runtime_error("png: bad size");
    if (depth != 8 || interlace != 0) throw std::runtime_error("png: only 8-bit non-interlaced images are supported");
    int ch;
    switch (ctype) {
        case 0: ch = 1; break;
        case 2: ch = 3; break;
        case 4: ch = 2; break;
        case 6: ch = 4; break;
        default: throw std::runtime_error("png: unsupported colour type");
    }
    const std::size_t stride = (std::size_t)w * ch;
    std::vector<std::uint8_t> raw((stride + 1) * (std::size_t)h);
    uLongf out_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &out_len, idat.data(), (uLong)idat.size()) != Z_OK || out_len != raw.size())
        throw std::runtime_error("png: inflate failed");
    // undo the per-scanline filters in place (PNG spec section 9)
    std::vector<std::uint8_t> prev(stride, 0), cur(stride);
    gray.resize((std::size_t)w * h);
    for (int y = 0; y < h; y++) {
        const std::uint8_t* src = &raw[(stride + 1) * y];
        const int ft = src[0];
        for (std::size_t i = 0; i < stride; i++) {
            const int a = i >= (std::size_t)ch ? cur[i - ch] : 0, b = prev[i], c = i >= (std::size_t)ch ? prev[i - ch] : 0;
            int v = src[1 + i];
            switch (ft) {
                case 0: break;
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                default: throw std::runtime_error("png: bad filter type");
            }
            cur[i] = (std::uint8_t)v;
        }
        std::uint8_t* g = &gray[(std::size_t)y * w];
        if (ch <= 2) {
            for (int x = 0; x < w; x++) g[x] = cur[(std::size_t)x * ch];
        } else {
            // cv::cvtColor RGB -> gray, 8-bit path: (R*4899 + G*9617 + B*1868 + 8192) >> 14
            for (int x = 0; x < w; x++) {
                const std::uint8_t* p = &cur[(std::size_t)x * ch];
                g[x] = (std::uint8_t)((p[0] * 4899 + p[1] * 9617 + p[2] * 1868 + 8192) >> 14);
            }
        }
        prev.swap(cur);
    }
    width = w;
    height = h;
}

// the numbers of a bracketed list that starts on `text`'s first '[' (up to the closing ']' or the end of the text)
static std::vector<double> bracket_numbers(const std::string& text) {
    std::vector<double> v;
    const std::size_t lo = text.find('[');
    if (lo == std::string::npos) return v;
    std::size_t hi = text.find(']', lo);
    if (hi == std::string::npos) hi = text.size();
    std::string body = text.substr(lo + 1, hi - lo - 1);
    for (char& c : body)
        if (c == ',') c = ' ';
    std::stringstream ss(body);
    std::string token;
    while (ss >> token) {
        char* end = nullptr;
        const double d = std::strtod(token.c_str(), &end);
        if (end != token.c_str()) v.push_back(d);
    }
    return v;
}

bool load_sensor_yaml(const std::string& path, AslCalibration& out) {
    std::ifstream file(path);
    if (!file.is_open()) return false;
    out = AslCalibration{};
    std::vector<std::string> lines;
    std::string line;
    while (std::getline(file, line)) lines.push_back(line);
    bool in_tbs = false, have_k = false;
    for (std::size_t n = 0; n < lines.size(); n++) {
        const std::string& ln = lines[n];
        const std::size_t first = ln.find_first_not_of(" \t");
        if (first != std::string::npos && ln.compare(first, 4, "T_BS") == 0) in_tbs = true;
        if (ln.find("intrinsics:") != std::string::npos) {                    // EuRoCReader.cpp:233
            const std::vector<double> v = bracket_numbers(ln);
            if (v.size() >= 4) { for (int k = 0; k < 4; k++) out.intrinsics[k] = v[(std::size_t)k]; have_k = true; }
        } else if (ln.find("distortion_coefficients:") != std::string::npos) { // :247
            const std::vector<double> v = bracket_numbers(ln);
            for (std::size_t k = 0; k < v.size() && k < 5; k++) out.distortion[k] = v[k];
        } else if (ln.find("distortion_model:") != std::string::npos) {
            std::string m = ln.substr(ln.find(':') + 1);
            const std::size_t a = m.find_first_not_of(" \t"), b = m.find_last_not_of(" \t\r");
            out.distortion_model = a == std::string::npos ? std::string() : m.substr(a, b - a + 1);
        } else if (ln.find("resolution:") != std::string::npos) {
            const std::vector<double> v = bracket_numbers(ln);
            if (v.size() >= 2) { out.width = (int)v[0]; out.height = (int)v[1]; }
        } else if (in_tbs && ln.find("data:") != std::string::npos) {
            std::string text = ln;
            std::size_t k = n;
            while (text.find(']') == std::string::npos && k + 1 < lines.size()) text += " " + lines[++k];
            const std::vector<double> v = bracket_numbers(text);
            if (v.size() == 16)
                for (int j = 0; j < 16; j++) out.T_BS[j] = v[(std::size_t)j];
            in_tbs = false;
        }
    }
    return have_k;
}

const AslCalibration& AslSequence::calibration(int cam) const {
    if (!hasCalibration(cam)) throw std::runtime_error("no mav0/cam" + std::to_string(cam) + "/sensor.yaml with intrinsics");
    return calibration_[cam];
}

bool AslSequence::load(const std::string& dataset_path) {
    images_.clear();
    std::string cam = dataset_path + "/mav0/cam0";
    if (!file_exists(cam + "/data.csv")) cam = dataset_path + "/cam0";        // path already points at mav0
    if (!load_camera(cam, images_)) return false;
    std::string line;
    // cam1 beside cam0, paired by equal timestamp; its absence is not an error
    right_.clear();
    std::vector<AslImage> cam1;
    if (load_camera(cam.substr(0, cam.size() - 4) + "cam1", cam1)) {
        right_.assign(images_.size(), std::string());
        std::size_t k = 0;
        for (std::size_t i = 0; i < images_.size(); i++) {                    // both lists are sorted
            while (k < cam1.size() && cam1[k].timestamp < images_[i].timestamp) k++;
            if (k < cam1.size() && cam1[k].timestamp == images_[i].timestamp) right_[i] = cam1[k].path;
        }
    }
    // sensor.yaml of both cameras; their absence is not an error
    for (int c = 0; c < 2; c++)
        has_calibration_[c] = load_sensor_yaml(cam.substr(0, cam.size() - 4) + "cam" + std::to_string(c) + "/sensor.yaml", calibration_[c]);
    // imu0 beside cam0 (EuRoCReader.cpp:110-154); its absence is not an error
    imu_.clear();
    std::ifstream imu_file(cam.substr(0, cam.size() - 4) + "imu0/data.csv");
    if (imu_file.is_open()) {
        std::getline(imu_file, line);                                         // header (:119)
        while (std::getline(imu_file, line)) {
            if (line.empty() || line[0] == '#') continue;                     // :122
            std::stringstream ss(line);
            std::string token;
            std::vector<std::string> tokens;
            while (std::getline(ss, token, ',')) tokens.push_back(token);
            if (tokens.size() < 7) continue;                                  // :132
            AslImu m;
            m.timestamp = std::strtod(tokens[0].c_str(), nullptr) * 1e-9;
            for (int k = 0; k < 3; k++) {                                     // timestamp, gyro xyz, accel xyz (:137-143)
                m.gyro[k] = std::strtod(tokens[(std::size_t)(1 + k)].c_str(), nullptr);
                m.accel[k] = std::strtod(tokens[(std::size_t)(4 + k)].c_str(), nullptr);
            }
            imu_.push_back(m);
        }
        std::stable_sort(imu_.begin(), imu_.end(), [](const AslImu& a, const AslImu& b) { return a.timestamp < b.timestamp; });
    }
    // getNext (:295-305): image i takes the samples with prev_image_time < t <= image_time, in order
    imu_begin_.assign(images_.size(), 0);
    imu_end_.assign(images_.size(), 0);
    std::size_t k = 0;
    for (std::size_t i = 0; i < images_.size(); i++) {
        const double prev = i > 0 ? images_[i - 1].timestamp : 0.0, now = images_[i].timestamp;
        while (k < imu_.size() && imu_[k].timestamp <= now && !(imu_[k].timestamp > prev)) k++;   // consumed, not handed on
        imu_begin_[i] = k;
        while (k < imu_.size() && imu_[k].timestamp <= now) k++;
        imu_end_[i] = k;
    }
    // ground truth beside cam0 (EuRoCReader.cpp:37-41): state_groundtruth_estimate0, else leica0; neither is an error
    ground_truth_.clear();
    const std::string mav = cam.substr(0, cam.size() - 4);
    if (!load_ground_truth(mav + "state_groundtruth_estimate0/data.csv", ground_truth_))
        load_ground_truth(mav + "leica0/data.csv", ground_truth_);            // 4 fields per row: no row survives (:179)
    return !images_.empty();                                                  // :105
}

void AslSequence::read(std::size_t i, std::vector<std::uint8_t>& gray, int& width, int& height) const {
    read_gray(images_.at(i).path, gray, width, height);
}

bool AslSequence::hasStereo() const {
    if (right_.empty()) return false;
    for (const std::string& p : right_)
        if (p.empty()) return false;
    return true;
}

void AslSequence::readRight(std::size_t i, std::vector<std::uint8_t>& gray, int& width, int& height) const {
    if (!hasRight(i)) throw std::runtime_error("no cam1 image for " + images_.at(i).path);
    read_gray(right_[i], gray, width, height);
}

}  // namespace aria::io

// ---- plain-C hooks so tests (ctypes) can exercise the reader without a C++ harness ----
extern "C" {

int aria_asl_decode_png_gray(const std::uint8_t* bytes, std::size_t n, std::uint8_t* out, std::size_t cap, int* width, int* height) {
    try {
        std::vector<std::uint8_t> file(bytes, bytes + n), gray;
        int w = 0, h = 0;
        aria::io::decode_png_gray(file, gray, w, h);
        if (width) *width = w;
        if (height) *height = h;
        if (gray.size() > cap) return -5;
        std::memcpy(out, gray.data(), gray.size());
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

// Writes up to cap timestamps (seconds) in reader order; returns the number of images or -1.
int aria_asl_list(const char* dataset_path, double* timestamps, int cap, char* first_path, int first_path_cap) {
    aria::io::AslSequence s;
    if (!s.load(dataset_path)) return -1;
    for (std::size_t i = 0; i < s.size() && (int)i < cap; i++) timestamps[i] = s.at(i).timestamp;
    if (first_path && first_path_cap > 0) std::snprintf(first_path, (std::size_t)first_path_cap, "%s", s.at(0).path.c_str());
    return (int)s.size();
}

// Per image 1 when it has a cam1 partner of equal timestamp, else 0; returns the number of images or -1.
int aria_asl_stereo(const char* dataset_path, int* has_right, int cap) {
    aria::io::AslSequence s;
    if (!s.load(dataset_path)) return -1;
    for (std::size_t i = 0; i < s.size() && (int)i < cap; i++) has_right[i] = s.hasRight(i) ? 1 : 0;
    return (int)s.size();
}

// Camera cam's sensor.yaml as 27 doubles: intrinsics[4], distortion[5], T_BS[16], width, height; returns 1 with a calibration,
// 0 without, -1 when the sequence does not load.
int aria_asl_calibration(const char* dataset_path, int cam, double* out27) {
    aria::io::AslSequence s;
    if (!s.load(dataset_path)) return -1;
    if (!s.hasCalibration(cam)) return 0;
    const aria::io::AslCalibration& c = s.calibration(cam);
    std::memcpy(out27, c.intrinsics, 4 * sizeof(double));
    std::memcpy(out27 + 4, c.distortion, 5 * sizeof(double));
    std::memcpy(out27 + 9, c.T_BS, 16 * sizeof(double));
    out27[25] = c.width;
    out27[26] = c.height;
    return 1;
}

// IMU samples as rows [t, accel xyz, gyro xyz] (the layout of aria_imu_sample) and [begin, end) per image; returns the number
// of samples (0 without imu0) or -1. n_images receives the number of images.
int aria_asl_imu(const char* dataset_path, double* samples, int cap, int* ranges, int image_cap, int* n_images) {
    aria::io::AslSequence s;
    if (!s.load(dataset_path)) return -1;
    const auto& imu = s.imu();
    for (std::size_t i = 0; i < imu.size() && (int)i < cap; i++) {
        samples[7 * i] = imu[i].timestamp;
        for (int k = 0; k < 3; k++) { samples[7 * i + 1 + k] = imu[i].accel[k]; samples[7 * i + 4 + k] = imu[i].gyro[k]; }
    }
    for (std::size_t i = 0; i < s.size() && (int)i < image_cap; i++) {
        ranges[2 * i] = (int)s.imuBegin(i);
        ranges[2 * i + 1] = (int)s.imuEnd(i);
    }
    if (n_images) *n_images = (int)s.size();
    return (int)imu.size();
}

// Ground truth as rows of 17 doubles (the layout of aria_eval_truth); returns the number of rows (0 without any) or -1.
int aria_asl_ground_truth(const char* dataset_path, double* rows, int cap) {
    aria::io::AslSequence s;
    if (!s.load(dataset_path)) return -1;
    const auto& gt = s.groundTruth();
    for (std::size_t i = 0; i < gt.size() && (int)i < cap; i++) std::memcpy(rows + 17 * i, &gt[i], 17 * sizeof(double));
    return (int)gt.size();
}

}  // extern "C"
