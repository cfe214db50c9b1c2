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
    expect("aria_bow_create", aria_bow_create(&c, h_.out()));
}

HipPlaceIndex::~HipPlaceIndex() = default;

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
    expect("aria_bow_train", aria_bow_train(h_.get(), block.data(), counts.data(), (int)frames.size(), (std::int64_t)stride, &run));
    return run;
}

void HipPlaceIndex::load(const std::string& path) {
    expect("aria_bow_load", aria_bow_load(h_.get(), path.c_str()));
}

void HipPlaceIndex::save(const std::string& path) const {
    expect("aria_bow_save", aria_bow_save(h_.get(), path.c_str()));
}

int HipPlaceIndex::words() const { return aria_bow_words(h_.get()); }

void HipPlaceIndex::add(std::uint64_t id, const core::Frame& frame) {
    const int n = rowsOf(frame);
    expect("aria_bow_add", aria_bow_add(h_.get(), (long long)id, n ? frame.descriptors.data() : nullptr, n));
}

std::vector<aria_bow_hit> HipPlaceIndex::query(std::uint64_t query_id, const core::Frame& frame) {
    const int n = rowsOf(frame);
    std::vector<aria_bow_hit> hits((std::size_t)top_k_);
    int count = 0;
    expect("aria_bow_query",
           aria_bow_query(h_.get(), (long long)query_id, n ? frame.descriptors.data() : nullptr, n, hits.data(), &count));
    hits.resize((std::size_t)std::max(0, std::min(count, top_k_)));
    return hits;
}

int HipPlaceIndex::size() const { return aria_bow_size(h_.get()); }

std::uint64_t HipPlaceIndex::id(int index) const {
    long long v = -1;
    expect("aria_bow_info", aria_bow_info(h_.get(), index, &v, nullptr));
    return (std::uint64_t)v;
}

}  // namespace aria::adapters::hip
