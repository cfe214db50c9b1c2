// Host shim for tests/test_ray_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/tsdf_raycast.hip (the text
// between "namespace {" and the C-ABI section, pasted between this file and ray_kernel_emu_tail.inc by the test) compile as
// plain C++17. The kernels have no barrier and no shared memory, so the lanes of a workgroup run one after the other on the
// calling thread; the only atomic is the deferred-error OR. ray_tally, the one cross-lane step of the
// file, is served here lane by lane: the same counts and the same minimum on the bit patterns. Test infrastructure only.
#include <algorithm>
#include <cfloat>
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
static inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline void ray_tally(aria_ray_view* rec, bool ended, bool hit, float depth) {
    rec->n_ended += ended ? 1 : 0;
    if (!hit) return;
    rec->n_hit += 1;
    if (__float_as_uint(depth) < __float_as_uint(rec->nearest)) rec->nearest = depth;
}
