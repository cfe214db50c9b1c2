// Host shim for tests/test_nav_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/nav_grid.hip (the text between
// "namespace {" and the goal-field section, pasted between this file and nav_kernel_emu_tail.inc by the test) compile as plain
// C++17. The kernels of that text have no barrier and no shared memory, so the lanes of a workgroup run one after the other on
// the calling thread; the only atomics are the deferred-error ORs. Test infrastructure only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "aria_orb_hip.h"
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct dim3e { unsigned x = 0, y = 0, z = 0; };
static dim3e threadIdx, blockIdx;
using std::min; using std::max;
static inline int atomicOr(int* p, int v) { const int o = *p; *p = o | v; return o; }
static inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
