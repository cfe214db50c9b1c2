// See aria_hip/HipPlaceIndex.hpp.
#include "aria_hip/HipPlaceIndex.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace aria::adapters::hip {

namespace {
int rowsOf(const core::Frame& f) {
    if (f.descriptors.size() < f.numKeypoints() * 32) throw std::invalid_argument("HipPlaceIndex: descriptors shorter than numKeypoints()*32");
    return (int)f.numKeypoints();
}
}  // namespace

HipPlaceIndex::HipPlaceIndex(const PlaceIndexConfig& cfg) : top_k_(cfg.top_k) {
    aria_bow_config c;
    aria_bow_default_config(&c);
    c.device = cfg.device;
    c.stream = cfg.stream;
    c.words = cfg.words;
    c.rows = cfg.rows;
    c.capacity = cfg.capacity;
    c.top_k = cfg.top_k;
    c.min_frames_between = cfg.min_frames_between;
    c.train_iters = cfg.train_iters;
    const int rc = aria_bow_create(&c, &h_);
    if (rc != ARIA_OK) fail("aria_bow_create", rc);
}

HipPlaceIndex::~HipPlaceIndex() { aria_bow_destroy(h_); }

void HipPlaceIndex::fail(const char* where, int status) {
    std::string msg = std::string("HipPlaceIndex: ") + where + ": " + aria_status_string(status);
    const char* hip = aria_last_hip_error();
    if (hip && hip[0]) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
}

int HipPlaceIndex::train(const std::vector<const core::Frame*>& frames) {
    std::vector<int> counts;
    std::size_t stride = 1;
    for (const core::Frame* f : frames) {
        counts.push_back(rowsOf(*f));
        stride = std::max(stride, (std::size_t)counts.back());
    }
    std::vector<std::uint8_t> block(std::max<std::size_t>(frames.size(), 1) * stride * 32, 0);
    for (std::size_t k = 0; k < frames.size(); k++)
        if (counts[k]) std::memcpy(block.data() + k * stride * 32, frames[k]->descriptors.data(), (std::size_t)counts[k] * 32);
    int run = 0;
    const int rc = aria_bow_train(h_, block.data(), counts.data(), (int)frames.size(), (std::int64_t)stride, &run);
    if (rc != ARIA_OK) fail("aria_bow_train", rc);
    return run;
}

void HipPlaceIndex::load(const std::string& path) {
    const int rc = aria_bow_load(h_, path.c_str());
    if (rc != ARIA_OK) fail("aria_bow_load", rc);
}

void HipPlaceIndex::save(const std::string& path) const {
    const int rc = aria_bow_save(h_, path.c_str());
    if (rc != ARIA_OK) fail("aria_bow_save", rc);
}

int HipPlaceIndex::words() const { return aria_bow_words(h_); }

void HipPlaceIndex::add(std::uint64_t id, const core::Frame& frame) {
    const int n = rowsOf(frame);
    const int rc = aria_bow_add(h_, (long long)id, n ? frame.descriptors.data() : nullptr, n);
    if (rc != ARIA_OK) fail("aria_bow_add", rc);
}

std::vector<aria_bow_hit> HipPlaceIndex::query(std::uint64_t query_id, const core::Frame& frame) {
    const int n = rowsOf(frame);
    std::vector<aria_bow_hit> hits((std::size_t)top_k_);
    int count = 0;
    const int rc = aria_bow_query(h_, (long long)query_id, n ? frame.descriptors.data() : nullptr, n, hits.data(), &count);
    if (rc != ARIA_OK) fail("aria_bow_query", rc);
    hits.resize((std::size_t)std::max(0, std::min(count, top_k_)));
    return hits;
}

int HipPlaceIndex::size() const { return aria_bow_size(h_); }

std::uint64_t HipPlaceIndex::id(int index) const {
    long long v = -1;
    const int rc = aria_bow_info(h_, index, &v, nullptr);
    if (rc != ARIA_OK) fail("aria_bow_info", rc);
    return (std::uint64_t)v;
}

}  // namespace aria::adapters::hip
