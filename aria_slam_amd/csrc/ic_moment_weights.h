// Weights of the intensity-centroid moments (orb.cpp ICAngles) as the B operand of an int8 matrix product.
//
// m10 = sum u * I(u, v) and m01 = sum v * I(u, v) over the radius-15 disc |u| <= umax[|v|] are a contraction of the
// 31-row window with two weight vectors. The window is cut into 64 pieces of 16 bytes: piece p = row p >> 1, half p & 1 of a
// 31 x 32-byte window that starts at (x - 15, y - 15); pieces 62 and 63 (a "row 31") carry zero weights. Byte j of
// piece p is the pixel (u, v) = (16 * half + j - 15, row - 15); column u = 16 (half 1, j = 15) lies outside the disc.
//   role 0: u inside the disc, else 0          role 1: v inside the disc, else 0
// Every weight fits int8 (|u|, |v| <= 15) and each role's weights sum to 0 (the disc is symmetric), so the contraction may
// run on pixels with any constant subtracted: I - 128 (the byte XOR 0x80, read as signed) gives the same moments, and
// |sum| <= 128 * sum |w| < 2^31.
// Plain C++ (no device code): the kernel includes it, and so does the host program that replays the contraction
// (tests/cpp/ic_moment_selftest.cpp).
#pragma once
#include <cstdint>

namespace aria {

// end-of-row table of the radius-15 disc (orb.cpp computeKeyPoints umax; verified against the host
// computation in tests/test_host_logic.py)
#define ARIA_UMAX_LIST {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3}

constexpr int kIcPieces = 64;           // 16 k-steps of the 16x16x64 product x 4 lane groups
constexpr int kIcPieceBytes = 16;

struct IcMomentWeights { int8_t w[2][kIcPieces][kIcPieceBytes]; };

constexpr IcMomentWeights make_ic_moment_weights() {
    constexpr int umax[16] = ARIA_UMAX_LIST;
    IcMomentWeights t{};
    for (int p = 0; p < kIcPieces; p++)
        for (int j = 0; j < kIcPieceBytes; j++) {
            const int row = p >> 1, half = p & 1;
            const int u = 16 * half + j - 15, v = row - 15;
            const int au = u < 0 ? -u : u, av = v < 0 ? -v : v;
            const bool in = row < 31 && au <= 15 && au <= umax[av];
            t.w[0][p][j] = (int8_t)(in ? u : 0);
            t.w[1][p][j] = (int8_t)(in ? v : 0);
        }
    return t;
}

constexpr int ic_moment_weight_sum(int role) {
    const IcMomentWeights t = make_ic_moment_weights();
    int s = 0;
    for (int p = 0; p < kIcPieces; p++)
        for (int j = 0; j < kIcPieceBytes; j++) s += t.w[role][p][j];
    return s;
}
constexpr long long ic_moment_weight_abs_sum(int role) {
    const IcMomentWeights t = make_ic_moment_weights();
    long long s = 0;
    for (int p = 0; p < kIcPieces; p++)
        for (int j = 0; j < kIcPieceBytes; j++) s += t.w[role][p][j] < 0 ? -t.w[role][p][j] : t.w[role][p][j];
    return s;
}
// The kernel cuts a piece out of five dwords that start up to 3 bytes before it. For half 1 the fifth dword can only
// hold the piece's bytes j >= 13; it is loaded in the steps kIcTailStepLo..kIcTailStepHi only (piece 4 * step + kb), so
// outside them those bytes must carry zero weights.
constexpr int kIcTailStepLo = 4, kIcTailStepHi = 10;
constexpr bool ic_moment_tail_is_zero_outside(int lo, int hi) {
    const IcMomentWeights t = make_ic_moment_weights();
    for (int p = 0; p < kIcPieces; p++) {
        const int step = p >> 2;
        if ((p & 1) == 0 || (step >= lo && step <= hi)) continue;
        for (int role = 0; role < 2; role++)
            for (int j = 13; j < kIcPieceBytes; j++)
                if (t.w[role][p][j] != 0) return false;
    }
    return true;
}
static_assert(ic_moment_tail_is_zero_outside(kIcTailStepLo, kIcTailStepHi), "a step outside the range needs its fifth dword");
static_assert(ic_moment_weight_sum(0) == 0 && ic_moment_weight_sum(1) == 0,
              "the moments of I - 128 equal the moments of I only while each role's weights sum to 0");
static_assert(128 * ic_moment_weight_abs_sum(0) < (1ll << 31) && 128 * ic_moment_weight_abs_sum(1) < (1ll << 31),
              "the int32 accumulator holds every moment");

}  // namespace aria
