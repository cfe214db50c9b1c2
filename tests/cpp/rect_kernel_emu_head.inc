// Host shim for tests/test_rectify_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/rectify.hip (the text
// between "namespace {" and the C-ABI, pasted between this file and rect_kernel_emu_tail.inc by the test) compile as plain
// C++17. The three kernels have no barrier and no shared memory, so the lanes of a workgroup run one after the other on the
// calling thread; the only atomic is the deferred-error OR. Test infrastructure only.
// Every load of a source image goes through __builtin_memcpy in the kernel text (rect_ld_u16, rect_ld_u64). Here that name is
// a checked copy: a load that leaves the rows of the image emu_remap was given -- a byte of the pitch padding, a row below the
// last, another frame's gap -- is counted (emu_bad_loads) and reads zeros instead of touching memory it may not own. Such a load
// can leave every pixel right (the kernel may not use the byte) and still be a fault on the device.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct dim3e { int x = 0, y = 0, z = 0; };
static dim3e threadIdx, blockIdx;
using std::min; using std::max;
static inline int atomicOr(int* p, int v) { const int o = *p; *p = o | v; return o; }
struct alignas(16) uint4 { uint32_t x, y, z, w; };
static const uint8_t* g_src = nullptr;                            // the source batch of the running emu_remap
static int64_t g_src_stride = 0;
static int g_src_pitch = 1, g_src_w = 0, g_src_h = 0, g_src_frames = 0;
static long g_bad_loads = 0;
static inline void emu_checked_load(void* to, const void* from, size_t n) {
    if (g_src) {
        const int64_t o = (const uint8_t*)from - g_src;
        const int64_t f = (o >= 0 && g_src_stride > 0) ? o / g_src_stride : 0;
        const int64_t r = o - f * g_src_stride;
        if (o < 0 || f >= g_src_frames || r / g_src_pitch >= g_src_h || r % g_src_pitch + (int64_t)n > g_src_w) {
            g_bad_loads++;
            std::memset(to, 0, n);
            return;
        }
    }
    std::memcpy(to, from, n);
}
#define __builtin_memcpy emu_checked_load
