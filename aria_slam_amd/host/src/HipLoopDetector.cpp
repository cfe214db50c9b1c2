// See aria_hip/HipLoopDetector.hpp. Control flow of src/legacy/LoopClosure.cpp:24-114 of the reference.
#include "aria_hip/HipLoopDetector.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "aria_hip/HipPlaceIndex.hpp"
#include "aria_orb_hip.h"

namespace aria::adapters::hip {

namespace {
[[noreturn]] void fail(const char* where, int status) { detail::fail("HipLoopDetector", where, status); }
void expect(const char* where, int rc) { detail::expect("HipLoopDetector", where, rc); }
}  // namespace

HipLoopDetector::HipLoopDetector(int min_frames_between, double min_score, int min_matches, int slot_rows, int capacity,
                                 void* stream, int device)
    : matcher_(stream, device), min_frames_between_(min_frames_between), min_score_(min_score), min_matches_(min_matches),
      slot_rows_(slot_rows) {
    expect("aria_kfdb_create", aria_kfdb_create(device, stream, capacity, slot_rows, db_.out()));
    good_.resize((size_t)capacity);
}

HipLoopDetector::~HipLoopDetector() = default;

int HipLoopDetector::size() const { return aria_kfdb_size(db_.get()); }

std::uint64_t HipLoopDetector::keyframeId(int index) const {
    long long id = -1;
    expect("aria_kfdb_info", aria_kfdb_info(db_.get(), index, &id, nullptr));
    return (std::uint64_t)id;
}

void HipLoopDetector::addKeyFrame(const core::KeyFrame& kf) {
    const int n = (int)kf.frame.numKeypoints();
    if ((size_t)n * 32 > kf.frame.descriptors.size()) fail("addKeyFrame: descriptors shorter than numKeypoints()*32", ARIA_E_INVALID);
    // push_back + pop_front beyond 500
    expect("aria_kfdb_add", aria_kfdb_add(db_.get(), (long long)kf.id, kf.frame.descriptors.data(), n));
    if (place_) {                                                                          // the C-ABI directly: this file links without HipPlaceIndex.cpp
        expect("aria_bow_add", aria_bow_add(place_->handle(), (long long)kf.id, n ? kf.frame.descriptors.data() : nullptr, n));
    }
}

void HipLoopDetector::setPlaceIndex(std::shared_ptr<HipPlaceIndex> index, int top_k) {
    if (index && (aria_bow_words(index->handle()) == 0 || aria_bow_size(index->handle()) != size() || top_k < 1))
        fail("setPlaceIndex: the index needs a vocabulary and as many entries as the database", ARIA_E_INVALID);
    place_ = std::move(index);
    place_top_k_ = top_k;
}

std::vector<std::pair<int, double>> HipLoopDetector::findCandidates(const core::KeyFrame& query) {
    std::vector<std::pair<int, double>> candidates;
    if (query.frame.descriptors.empty()) return candidates;                        // LoopClosure.cpp:75
    const int nq = (int)query.frame.numKeypoints();
    if ((size_t)nq * 32 > query.frame.descriptors.size()) fail("findCandidates: descriptors shorter than numKeypoints()*32", ARIA_E_INVALID);
    matcher_.reserve(nq, slot_rows_);
    if (place_) {
        // the index names at most top_k keyframes; only they are matched exactly. Its deque may be longer than the
        // database's: the same keyframe lies `shift` positions later there
        const int shift = aria_bow_size(place_->handle()) - size();
        std::vector<aria_bow_hit> hits((size_t)place_->topK());
        int n_hits = 0;
        expect("aria_bow_query",
               aria_bow_query(place_->handle(), (long long)query.id, query.frame.descriptors.data(), nq, hits.data(), &n_hits));
        place_queries_++;
        hits.resize((size_t)std::max(0, std::min(n_hits, std::min(place_top_k_, place_->topK()))));
        match_buf_.resize((size_t)std::max(nq, 1));
        for (const aria_bow_hit& h : hits) {
            const int i = h.index - shift;
            long long id = 0;
            int cnt = 0;
            if (i < 0 || aria_kfdb_info(db_.get(), i, &id, &cnt) != ARIA_OK || id != (long long)h.id) continue;
            if ((long long)query.id - id < (long long)min_frames_between_) continue;   // :81
            if (cnt <= 0) continue;                                                     // :83
            int good = 0;
            place_candidates_++;
            expect("aria_kfdb_match",
                   aria_kfdb_match(db_.get(), matcher_.handle(), i, query.frame.descriptors.data(), nq, 0.7f,
                                   reinterpret_cast<aria_match*>(match_buf_.data()), (int)match_buf_.size(), &good));
            const double score = (double)good / std::max(1, nq);                       // :98
            if (score > 0.1) candidates.push_back({i, score});                          // :99
        }
        std::sort(candidates.begin(), candidates.end(), [](const auto& a, const auto& b) {
            return a.second > b.second || (a.second == b.second && a.first < b.first);  // :105-106, ties in database order
        });
        if (candidates.size() > 5) candidates.resize(5);                                // :109-111
        return candidates;
    }
    int n_kf = 0;
    expect("aria_kfdb_scan",
           aria_kfdb_scan(db_.get(), matcher_.handle(), query.frame.descriptors.data(), nq, 0.7, good_.data(), (int)good_.size(), &n_kf));
    for (int i = 0; i < n_kf; i++) {
        long long id = 0;
        int cnt = 0;
        aria_kfdb_info(db_.get(), i, &id, &cnt);
        if ((long long)query.id - id < (long long)min_frames_between_) continue;   // :81
        if (cnt <= 0) continue;                                                     // :83
        const double score = (double)good_[(size_t)i] / std::max(1, nq);           // :98
        if (score > 0.1) candidates.push_back({i, score});                          // :99
    }
    std::stable_sort(candidates.begin(), candidates.end(),
                     [](const auto& a, const auto& b) { return a.second > b.second; });   // :105-106
    if (candidates.size() > 5) candidates.resize(5);                                // :109-111
    return candidates;
}

std::optional<core::LoopCandidate> HipLoopDetector::detect(const core::KeyFrame& query) {
    if (size() < min_frames_between_) return std::nullopt;                          // :34-36
    const auto candidates = findCandidates(query);                                  // :39
    const int nq = (int)query.frame.numKeypoints();
    for (const auto& [idx, score] : candidates) {
        if (score < min_score_) continue;                                           // :42
        long long id = 0;
        int cnt = 0;
        aria_kfdb_info(db_.get(), idx, &id, &cnt);
        if ((long long)query.id - id < (long long)min_frames_between_) continue;    // :47
        // verification: the ratio-0.7 match list (LoopClosure.cpp:120-131), at least min_matches of them. The keyframe is
        // matched where it lies in the database (no download + upload of its descriptors)
        match_buf_.resize((size_t)std::max(nq, 1));
        int n = 0;
        expect("aria_kfdb_match",
               aria_kfdb_match(db_.get(), matcher_.handle(), idx, query.frame.descriptors.data(), nq, 0.7f,
                               reinterpret_cast<aria_match*>(match_buf_.data()), (int)match_buf_.size(), &n));
        core::LoopCandidate cand{};
        cand.matches.assign(match_buf_.begin(), match_buf_.begin() + n);
        if ((int)cand.matches.size() < min_matches_) continue;
        if (verifier_ && !verifier_(query, (std::uint64_t)id, cand)) continue;
        cand.query_id = query.id;                                                   // :57-61
        cand.match_id = (std::uint64_t)id;
        cand.score = score;
        loop_count_++;                                                              // :63
        return cand;
    }
    return std::nullopt;
}

}  // namespace aria::adapters::hip
