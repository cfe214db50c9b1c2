// Host replay of the matrix-core moment phase of the batch k_describe (aria_slam_amd/csrc/orb_kernels.hip, describe16<0>)
// against the direct intensity-centroid loops of orb.cpp ICAngles. No GPU: the lane -> operand maps, the piece order, the
// byte XOR and the int8 products are restated in plain C++ on the weight table the kernel uses (ic_moment_weights.h).
//   A: lane (kb = lane >> 4, m = lane & 15), step k: the 16 bytes of piece 4k + kb of keypoint-row m, XOR 0x80, as int8
//   B: lane (kb, n): the same piece of role (n >> 2) & 1
//   D: lane (g, n), register j = row 4g + j, column n; row 4g + r is keypoint 4r + g; lane (g, r) takes register r of its own
//      column for m10 and of the lane four up for m01
// Prints "OK <cases>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>

#include "ic_moment_weights.h"

using namespace aria;

static const IcMomentWeights kW = make_ic_moment_weights();
static int g_umax[16];

// orb.cpp computeKeyPoints: the end-of-row table of the circular patch, halfPatchSize 15
static void make_umax() {
    const int hp = 15;
    const int vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) g_umax[v] = (int)std::lrint(std::sqrt((double)hp * hp - v * v));
    for (int v = hp, v0 = 0; v >= vmin; --v) {
        while (g_umax[v0] == g_umax[v0 + 1]) ++v0;
        g_umax[v] = v0;
        ++v0;
    }
}

// orb.cpp ICAngles, the moments only
static void direct_moments(const uint8_t* img, int pitch, int x, int y, int& m10, int& m01) {
    const uint8_t* c = img + (size_t)y * pitch + x;
    m10 = 0; m01 = 0;
    for (int u = -15; u <= 15; ++u) m10 += u * c[u];
    for (int v = 1; v <= 15; ++v) {
        int v_sum = 0;
        const int d = g_umax[v];
        for (int u = -d; u <= d; ++u) {
            const int val_plus = c[u + v * pitch], val_minus = c[u - v * pitch];
            v_sum += val_plus - val_minus;
            m10 += u * (val_plus + val_minus);
        }
        m01 += v * v_sum;
    }
}

struct Kp { int x, y; };

// the wave's phase for 16 keypoints (kp[4r + g] is parked on lane (g, r)); false if an accumulator left int32
static bool mfma_moments(const uint8_t* img, int w, int h, int pitch, const Kp* kp, int* m10, int* m01) {
    long long D[16][16] = {};
    for (int k = 0; k < 16; k++) {
        int8_t A[64][16], B[64][16];
        for (int lane = 0; lane < 64; lane++) {
            const int kb = lane >> 4, m = lane & 15, n = lane & 15;
            const Kp& q = kp[4 * (m & 3) + (m >> 2)];             // row m = 4g + r holds keypoint 4r + g
            const int prow = kb >> 1, phalf = kb & 1;
            const int row = k < 15 ? 2 * k + prow : 30;
            // five dwords from the dword-aligned start, the piece cut out at the start's byte in its dword (v_alignbyte); an
            // image that is not dword-aligned takes the byte-exact load (sh = 0, the fifth dword unused)
            const bool exact = ((uintptr_t)img & 3) != 0 || (pitch & 3) != 0;
            const int sh = exact ? 0 : (q.x - 15) & 3;
            const int px = q.x - 15 + 16 * phalf - sh, py = q.y - 15 + row;
            if (px < 0 || px + 20 > w || py < 0 || py >= h) { printf("piece outside its image row: x %d y %d\n", q.x, q.y); return false; }
            const uint8_t* src = img + (size_t)py * pitch + px;
            if (!exact && ((uintptr_t)src & 3)) { printf("aligned load at an unaligned address: x %d y %d\n", q.x, q.y); return false; }
            // the fifth dword: half 0 takes the first dword of the row's half 1 (the lane 16 up has loaded it); half 1 loads it
            // in the steps kIcTailStepLo..Hi only and meets zero weights with whatever it holds in the others
            uint8_t bytes[20];
            memcpy(bytes, src, 16);
            if (phalf == 0 || (k >= kIcTailStepLo && k <= kIcTailStepHi)) memcpy(bytes + 16, src + 16, 4);
            else memset(bytes + 16, 0xA5 ^ lane, 4);
            for (int j = 0; j < 16; j++) A[lane][j] = (int8_t)(bytes[sh + j] ^ 0x80);
            memcpy(B[lane], kW.w[(n >> 2) & 1][4 * k + kb], 16);
        }
        for (int m = 0; m < 16; m++)
            for (int n = 0; n < 16; n++) {
                long long s = 0;
                for (int kb = 0; kb < 4; kb++)
                    for (int j = 0; j < 16; j++) s += (int)A[kb * 16 + m][j] * (int)B[kb * 16 + n][j];
                D[m][n] += s;
                if (D[m][n] >= (1ll << 31) || D[m][n] < -(1ll << 31)) { printf("accumulator overflow\n"); return false; }
            }
    }
    for (int g = 0; g < 4; g++)
        for (int r = 0; r < 4; r++) {                              // lane (g, r): register r = row 4g + r
            m10[4 * r + g] = (int)D[4 * g + r][r];                 // its own column
            m01[4 * r + g] = (int)D[4 * g + r][r + 4];             // the column of the lane four up
        }
    return true;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

enum Fill { RANDOM, ZERO, FULL, LEFT, RIGHT, TOP, BOTTOM, BINARY, N_FILL };

int main() {
    make_umax();
    const int want[16] = ARIA_UMAX_LIST;
    for (int i = 0; i < 16; i++)
        if (g_umax[i] != want[i]) { printf("umax[%d] = %d, the table has %d\n", i, g_umax[i], want[i]); return 1; }
    int sum[2] = {0, 0};
    for (int role = 0; role < 2; role++)
        for (int p = 0; p < kIcPieces; p++)
            for (int j = 0; j < kIcPieceBytes; j++) sum[role] += kW.w[role][p][j];
    if (sum[0] != 0 || sum[1] != 0) { printf("weight sums %d %d\n", sum[0], sum[1]); return 1; }

    long cases = 0;
    const int w = 81, h = 66;
    for (int pitch : {81, 84, 96})
        for (int lead = 0; lead < (pitch == 81 ? 4 : 1); lead++)   // the odd pitch also starts at every alignment of a dword
            for (int fill = 0; fill < N_FILL; fill++)
                for (int rep = 0; rep < (fill == RANDOM || fill == BINARY ? 2 : 1); rep++) {
                    // exactly the image's bytes: a read outside them is a heap overflow for the sanitizer
                    std::vector<uint8_t> buf((size_t)lead + (size_t)(h - 1) * pitch + w);
                    uint8_t* img = buf.data() + lead;
                    for (int y = 0; y < h; y++)
                        for (int x = 0; x < (y == h - 1 ? w : pitch); x++) {
                            uint8_t v = 0;
                            switch (fill) {
                                case RANDOM: v = (uint8_t)rnd(); break;
                                case ZERO: v = 0; break;
                                case FULL: v = 255; break;
                                case LEFT: v = x < 40 ? 255 : 0; break;
                                case RIGHT: v = x < 40 ? 0 : 255; break;
                                case TOP: v = y < 33 ? 255 : 0; break;
                                case BOTTOM: v = y < 33 ? 0 : 255; break;
                                default: v = (rnd() & 1) ? 255 : 0; break;
                            }
                            img[(size_t)y * pitch + x] = v;
                        }
                    // x = 31 .. 49 = w - 32 covers every x mod 16 and both edges; y its three values; the half-plane fills put
                    // their edge through the keypoint (x = 40, y = 33: the extreme moments) and beside it
                    for (int x0 = 31; x0 <= w - 32; x0++)
                        for (int y0 = 31; y0 <= h - 32; y0++) {
                            Kp kp[16];
                            for (int i = 0; i < 16; i++) {
                                kp[i].x = i == 0 ? x0 : 31 + (int)(rnd() % (unsigned)(w - 62));
                                kp[i].y = i == 0 ? y0 : 31 + (int)(rnd() % (unsigned)(h - 62));
                            }
                            // keypoint 0 moves through the 16 slots: every (row, lane) of the maps is exercised
                            const int slot = (x0 + 3 * y0 + rep) & 15;
                            const Kp t = kp[slot]; kp[slot] = kp[0]; kp[0] = t;
                            int m10[16], m01[16];
                            if (!mfma_moments(img, w, h, pitch, kp, m10, m01)) return 1;
                            for (int i = 0; i < 16; i++) {
                                int d10, d01;
                                direct_moments(img, pitch, kp[i].x, kp[i].y, d10, d01);
                                if (d10 != m10[i] || d01 != m01[i]) {
                                    printf("mismatch: fill %d pitch %d lead %d slot %d x %d y %d: m10 %d (direct %d), m01 %d (direct %d)\n",
                                           fill, pitch, lead, i, kp[i].x, kp[i].y, m10[i], d10, m01[i], d01);
                                    return 1;
                                }
                                cases++;
                            }
                        }
                }
    printf("OK %ld\n", cases);
    return 0;
}
