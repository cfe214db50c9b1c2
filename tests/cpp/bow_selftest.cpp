// Place recognition through the C++ adapters (tests/test_cpp_bow.py builds and runs this on the GPU): HipPlaceIndex on a
// generated scene, HipLoopDetector with and without an index, and a generated walk of 1200 keyframes that returns to its start.
// Frames are descriptor lists: a place is 300 random descriptors, a view of it 200 of them with 8 flipped bits each.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "aria_hip/HipLoopDetector.hpp"
#include "aria_hip/HipPlaceIndex.hpp"

using namespace aria;
using namespace aria::adapters::hip;

namespace {

constexpr int kPoints = 300, kView = 200, kFlips = 8;
std::mt19937_64 rng(12345);

std::vector<std::uint8_t> makePlace() {
    std::vector<std::uint8_t> p((size_t)kPoints * 32);
    for (auto& b : p) b = (std::uint8_t)(rng() & 0xFF);
    return p;
}

core::KeyFrame viewOf(const std::vector<std::uint8_t>& place, std::uint64_t id) {
    core::KeyFrame kf;
    kf.id = id;
    kf.frame.id = id;
    std::vector<int> order(kPoints);
    for (int i = 0; i < kPoints; i++) order[i] = i;
    for (int i = 0; i < kView; i++) std::swap(order[i], order[i + (int)(rng() % (std::uint64_t)(kPoints - i))]);
    kf.frame.keypoints.resize(kView);
    kf.frame.descriptors.resize((size_t)kView * 32);
    for (int i = 0; i < kView; i++) {
        kf.frame.keypoints[i] = core::KeyPoint{(float)(order[i] % 20) * 30.0f, (float)(order[i] / 20) * 30.0f, 31.0f, 0.0f, 1.0f, 0};
        std::uint8_t* d = kf.frame.descriptors.data() + (size_t)i * 32;
        std::memcpy(d, place.data() + (size_t)order[i] * 32, 32);
        for (int f = 0; f < kFlips; f++) {
            const int b = (int)(rng() % 256);
            d[b >> 3] ^= (std::uint8_t)(1 << (b & 7));
        }
    }
    return kf;
}

}  // namespace

int main(int argc, char** argv) {
    // ---- the adapter on a scene of 40 places: train on one view, fill with a second, query with a third
    {
        std::vector<std::vector<std::uint8_t>> places;
        for (int p = 0; p < 40; p++) places.push_back(makePlace());
        std::vector<core::KeyFrame> train, db, qs;
        for (int p = 0; p < 40; p++) train.push_back(viewOf(places[p], p));
        for (int p = 0; p < 40; p++) db.push_back(viewOf(places[p], p));
        for (int p = 0; p < 40; p++) qs.push_back(viewOf(places[p], 1000 + p));
        PlaceIndexConfig cfg;
        cfg.words = 256; cfg.rows = 256; cfg.capacity = 64; cfg.top_k = 4; cfg.min_frames_between = 10;
        HipPlaceIndex ix(cfg);
        std::vector<const core::Frame*> tf;
        for (auto& k : train) tf.push_back(&k.frame);
        const int before = ix.words();
        const int run = ix.train(tf);
        for (auto& k : db) ix.add(k.id, k.frame);
        int right = 0;
        for (int p = 0; p < 40; p++) {
            const auto hits = ix.query(qs[p].id, qs[p].frame);
            right += !hits.empty() && hits[0].index == p && hits[0].id == p && hits[0].score > 0 && hits[0].score <= 1.0;
        }
        // save and load into a second index: the same first hit
        const char* path = argc > 1 ? argv[1] : "bow_selftest.bow";
        ix.save(path);
        HipPlaceIndex iy(cfg);
        iy.load(path);
        for (auto& k : db) iy.add(k.id, k.frame);
        const auto a = ix.query(qs[7].id, qs[7].frame), b = iy.query(qs[7].id, qs[7].frame);
        const int same = a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(aria_bow_hit)) == 0;
        std::printf("adapter %d %d %d %d %d %d %d\n", before, ix.words(), run, ix.size(), right, same, (int)ix.id(39));
    }

    // ---- the walk: keyframes 0..5 are six places, 6..1193 are places of their own, 1194..1199 see places 0..5 again
    constexpr int N = 1200, BACK = 6;
    std::vector<std::vector<std::uint8_t>> start;
    for (int p = 0; p < BACK; p++) start.push_back(makePlace());
    std::vector<core::KeyFrame> walk;
    for (int k = 0; k < N; k++) {
        if (k < BACK) walk.push_back(viewOf(start[k], k));
        else if (k >= N - BACK) walk.push_back(viewOf(start[k - (N - BACK)], k));
        else walk.push_back(viewOf(makePlace(), k));
    }

    // ---- a detector without an index is what it was: two instances, one of which had setPlaceIndex(nullptr)
    {
        HipLoopDetector a(30, 0.3, 30, 256, 500), b(30, 0.3, 30, 256, 500);
        b.setPlaceIndex(nullptr);
        int equal = 1, loops = 0;
        for (int k = 0; k < 80; k++) {
            const core::KeyFrame& kf = k >= 74 ? walk[k - 74] : walk[k];      // the last six are keyframes 0..5 again (as ids 74..79)
            core::KeyFrame q = kf;
            q.id = k;
            q.frame.id = k;
            const auto ca = a.findCandidates(q), cb = b.findCandidates(q);
            equal &= ca == cb;
            const auto da = a.detect(q), db = b.detect(q);
            equal &= da.has_value() == db.has_value();
            if (da && db) {
                equal &= da->match_id == db->match_id && da->score == db->score && da->matches.size() == db->matches.size();
                loops++;
            }
            a.addKeyFrame(q);
            b.addKeyFrame(q);
        }
        std::printf("plain_equal %d %d %d\n", equal, loops, a.getLoopCount() == b.getLoopCount());
    }

    // ---- with an index, top_k 10 and a capacity of 2000 the loop to keyframes 0..5 is found; a detector of capacity 500
    //      without an index has dropped them: today's break
    {
        PlaceIndexConfig cfg;
        cfg.words = 256; cfg.rows = 256; cfg.capacity = 2000; cfg.top_k = 10; cfg.min_frames_between = 30;
        auto ix = std::make_shared<HipPlaceIndex>(cfg);
        std::vector<const core::Frame*> tf;
        for (int k = 0; k < N; k += N / 64) tf.push_back(&walk[k].frame);           // every 18th frame: 67 of them
        const int run = ix->train(tf);
        HipLoopDetector with(30, 0.3, 30, 256, 2000), without(30, 0.3, 30, 256, 500);
        with.setPlaceIndex(ix, 10);
        int found = 0, right = 0, found_without = 0, false_with = 0;
        for (int k = 0; k < N; k++) {
            const bool asks = k >= N - BACK || (k >= 600 && k < 606);                // the return, and six frames mid-walk
            if (asks) {
                const auto c = with.detect(walk[k]);
                const auto d = without.detect(walk[k]);
                if (k >= N - BACK) {
                    found += c.has_value();
                    right += c.has_value() && c->match_id == (std::uint64_t)(k - (N - BACK)) && (int)c->matches.size() >= 30;
                    found_without += d.has_value();
                } else {
                    false_with += c.has_value();
                }
            }
            with.addKeyFrame(walk[k]);
            without.addKeyFrame(walk[k]);
        }
        std::printf("walk %d %d %d %d %d %d %d %d %lld %lld\n", run, with.size(), ix->size(), without.size(), found, right, found_without,
                    false_with, with.placeQueries(), with.placeCandidates());
    }
    std::printf("DONE\n");
    return 0;
}
