// aria::adapters::hip::HipPlaceIndex -- place recognition over the C-ABI (include/aria_orb_hip.h, "place recognition"): a flat
// binary bag-of-words vocabulary trained on the device, the bag of every keyframe in a ring database, and the scored top-K of
// a query. The reference names a vocabulary as the cure for its O(N) keyframe scan (docs/milestones/H09_LOOP_CLOSURE_AUDIT.md
// 2.1, 6.3) and has no code for it; aria_slam_amd/bow_ref.py is the definition of every step.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aria_hip/compat.hpp"
#include "aria_hip/detail/Stage.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

struct PlaceIndexConfig {
    int words = 4096;                 // V that train() makes
    int rows = 4096;                  // most descriptors of a frame
    int capacity = 65536;             // entries; the oldest is dropped beyond it, as in the keyframe database
    int top_k = 10;                   // hits per query, <= 32
    int min_frames_between = 30;      // candidates: query id - entry id >= this
    int train_iters = 10;
    void* stream = nullptr;
    int device = 0;
};

class HipPlaceIndex {
public:
    explicit HipPlaceIndex(const PlaceIndexConfig& cfg = {});
    ~HipPlaceIndex();

    // k-majority training from the descriptors (N x 32 each) of a batch of frames; returns the iterations run. A new
    // vocabulary (train, load) empties the database.
    int train(const std::vector<const core::Frame*>& frames);
    void load(const std::string& path);
    void save(const std::string& path) const;
    int words() const;                // 0 before there is a vocabulary

    void add(std::uint64_t id, const core::Frame& frame);
    // the best top_k entries by score, best first; index = position in the database, oldest first
    std::vector<aria_bow_hit> query(std::uint64_t query_id, const core::Frame& frame);
    int size() const;
    std::uint64_t id(int index) const;
    int topK() const { return top_k_; }
    aria_bow_t handle() const { return h_.get(); }

private:
    static void expect(const char* where, int rc) { detail::expect("HipPlaceIndex", where, rc); }
    detail::StageOwner<aria_bow_t, aria_bow_destroy> h_;
    int top_k_ = 10;
};

}  // namespace aria::adapters::hip
