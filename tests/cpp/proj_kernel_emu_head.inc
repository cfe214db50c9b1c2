// Host shim for tests/test_proj_kernel_emulation.py: lets KERNEL SOURCE of aria_slam_amd/csrc/proj_search.hip -- the plain
// per-landmark arithmetic between its two marker comments, k_proj_resolve and k_proj_from_map, pasted between this file and
// proj_kernel_emu_tail.inc by the test -- compile as plain C++17. That text has no barrier, no shared memory and no cross-lane
// operation, so the lanes of a workgroup run one after the other on the calling thread; the only atomic is the deferred-error
// OR. Test infrastructure only.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "aria_orb_hip.h"
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define PROJ_HD static inline
struct dim3e { unsigned x = 0, y = 0, z = 0; };
static dim3e threadIdx, blockIdx, blockDim;
using std::min; using std::max;
static inline int atomicOr(int* p, int v) { const int o = *p; *p = o | v; return o; }
constexpr int PJ_BLOCK = 256;
constexpr int ERRBIT_PROJ_INPUT = 1;
