// Host self-test of the pure helpers of aria_slam_amd/csrc/stereo_match.hip: ld_u32, load_row<HW>, sad_slide<HW>, hist_select,
// order_key and key_value. Their text is not copied here: tests/test_stereo_helpers_selftest.py cuts it out of the .hip file
// between its marker comments, with the ST_* constants, into stereo_helpers_pasted.inc, and builds this program with the host
// address sanitizer. Every row under test ends exactly at the end of its heap block (and starts at its start), so "reads
// nothing outside the row" is checked, not trusted; the padding between rows holds 0xA5, which no byte loop reads.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#define __device__
#define __forceinline__ inline
// v_sad_u8: the sum of the four byte differences on top of the accumulator
static inline uint32_t sad_u8_standin(uint32_t a, uint32_t b, uint32_t c) { for (int k = 0; k < 32; k += 8) c += (uint32_t)std::abs((int)(a >> k & 255) - (int)(b >> k & 255)); return c; }
#define __builtin_amdgcn_sad_u8 sad_u8_standin
static inline long long __double_as_longlong(double x) { long long b; std::memcpy(&b, &x, 8); return b; }
static inline double __longlong_as_double(long long b) { double x; std::memcpy(&x, &b, 8); return x; }

#include "stereo_helpers_pasted.inc"

static long checks = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } checks++; } while (0)

static std::mt19937 rng(12345);
static uint8_t rnd_byte() { return (uint8_t)(rng() & 255); }

template <int HW>
static void test_load_row() {
    constexpr int width = 2 * HW + 1;
    for (int rep = 0; rep < 50; rep++) {
        uint8_t* row = (uint8_t*)std::malloc(width);              // the block IS the row
        for (int i = 0; i < width; i++) row[i] = rep == 0 ? 255 : rep == 1 ? 0 : rnd_byte();
        uint32_t r[4] = {0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF};
        load_row<HW>(row, r);
        for (int i = 0; i < 16; i++) EXPECT((r[i >> 2] >> (8 * (i & 3)) & 255) == (i < width ? row[i] : 0u));
        std::free(row);
    }
}

template <int HW>
static void test_sad_slide() {
    constexpr int width = 2 * HW + 1;
    for (int nsh = 3; nsh <= ST_MAX_SHIFTS; nsh++) {
        const int pitch = width + ST_MAX_SHIFTS + 5 + (nsh % 3);
        // left: the last row of the window ends at the end of the block; right: the last row of the window at the last shift does
        const size_t nl = (size_t)(width - 1) * pitch + width, nr = nl + nsh - 1;
        uint8_t* L = (uint8_t*)std::malloc(nl);
        uint8_t* R = (uint8_t*)std::malloc(nr);
        std::memset(L, 0xA5, nl);
        std::memset(R, 0xA5, nr);
        const int mode = nsh % 4;                                 // random; 0 against 255; equal; random
        for (int r = 0; r < width; r++) {
            for (int c = 0; c < width; c++) L[(size_t)r * pitch + c] = mode == 1 ? 0 : rnd_byte();
            for (int c = 0; c < width + nsh - 1; c++) R[(size_t)r * pitch + c] = mode == 1 ? 255 : mode == 2 ? L[(size_t)r * pitch + c % width] : rnd_byte();
        }
        for (int lane = 0; lane < ST_GROUP; lane++) {
            uint32_t acc[ST_PASSES];
            for (int ps = 0; ps < ST_PASSES; ps++) acc[ps] = 0xFFFFFFFFu - ps;
            sad_slide<HW>(L, R, pitch, lane, nsh, acc);
            for (int ps = 0; ps < ST_PASSES; ps++) {
                const int sh = lane + ps * ST_GROUP;
                if (sh >= nsh) { EXPECT(acc[ps] == 0xFFFFFFFFu - ps); continue; }   // a shift beyond the slide is not touched
                uint32_t want = 0;
                for (int r = 0; r < width; r++)
                    for (int c = 0; c < width; c++) want += (uint32_t)std::abs((int)L[(size_t)r * pitch + c] - (int)R[(size_t)r * pitch + c + sh]);
                EXPECT(acc[ps] == want);
                if (mode == 1) EXPECT(want == (uint32_t)width * width * 255);
            }
        }
        std::free(L);
        std::free(R);
    }
}

static void check_hist(const std::vector<int>& hist) {
    std::vector<int> sorted;
    for (int b = 0; b < 256; b++) for (int c = 0; c < hist[b]; c++) sorted.push_back(b);
    const int total = (int)sorted.size();
    std::vector<int> ranks = {0, total - 1, total / 2};
    for (int k = 0; k < total; k += std::max(1, total / 97)) ranks.push_back(k);
    for (int k : ranks) {
        int kk = k;
        const int b = hist_select(hist.data(), kk);
        EXPECT(b == sorted[k]);
        int below = 0;
        for (int i = 0; i < b; i++) below += hist[i];
        EXPECT(kk == k - below && kk >= 0 && kk < hist[b]);
    }
}

static void test_hist_select() {
    std::vector<int> h(256, 0);
    h[255] = 8192; check_hist(h);                                 // everything in the last bin, every bin before it empty
    h.assign(256, 0); h[0] = 1; check_hist(h);
    h.assign(256, 0); h[224] = 1; check_hist(h);
    h.assign(256, 0); h[200] = 3; h[255] = 5; check_hist(h);      // empty leading bins, a full last bin
    h.assign(256, 0); h[0] = 4; h[254] = 1; h[255] = 1; check_hist(h);
    h.assign(256, 32); check_hist(h);
    for (int rep = 0; rep < 200; rep++) {
        h.assign(256, 0);
        const int lead = rng() % 250, n = 1 + rng() % 300;
        for (int i = 0; i < n; i++) h[lead + rng() % (256 - lead)]++;
        check_hist(h);
    }
}

static void test_keys() {
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    std::vector<double> v = {0.0, -0.0, den, -den, 4 * den, -4 * den, std::numeric_limits<double>::min(), -std::numeric_limits<double>::min(),
                             inf, -inf, 1.0, -1.0, std::nextafter(1.0, 2.0), std::nextafter(-1.0, -2.0), std::numeric_limits<double>::max(),
                             -std::numeric_limits<double>::max(), 0.5, -0.5, 2.0, -2.0};
    for (int i = 0; i < 4000; i++) {
        const unsigned long long b = ((unsigned long long)rng() << 32) | rng();
        const double x = __longlong_as_double((long long)b);
        if (!std::isnan(x)) v.push_back(x);
    }
    for (double x : v) {                                          // the pair is a bijection on the bits
        const double y = key_value(order_key(x));
        EXPECT(__double_as_longlong(y) == __double_as_longlong(x));
    }
    EXPECT(order_key(-0.0) + 1 == order_key(0.0));                // -0.0 directly below +0.0, nothing between
    std::vector<double> by_value = v, by_key = v;
    std::sort(by_value.begin(), by_value.end());
    std::sort(by_key.begin(), by_key.end(), [](double a, double b) { return order_key(a) < order_key(b); });
    for (size_t i = 0; i < v.size(); i++) EXPECT(by_value[i] == by_key[i]);
    for (size_t i = 0; i + 1 < by_key.size(); i++)
        if (by_key[i] < by_key[i + 1]) EXPECT(order_key(by_key[i]) < order_key(by_key[i + 1]));
}

int main() {
    static_assert(ST_GROUP == 16 && ST_MAX_SHIFTS == 33 && ST_PASSES == 3 && ST_MAX_W == 7, "the geometry the test walks");
    uint8_t four[4] = {1, 2, 3, 4};
    EXPECT(ld_u32(four) == 0x04030201u);
    test_load_row<1>(); test_load_row<2>(); test_load_row<3>(); test_load_row<4>(); test_load_row<5>(); test_load_row<6>(); test_load_row<7>();
    test_sad_slide<1>(); test_sad_slide<2>(); test_sad_slide<3>(); test_sad_slide<4>(); test_sad_slide<5>(); test_sad_slide<6>(); test_sad_slide<7>();
    test_hist_select();
    test_keys();
    std::printf("OK %ld\n", checks);
    return 0;
}
