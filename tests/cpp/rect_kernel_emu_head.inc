// Host shim for tests/test_rectify_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/rectify.hip (the text
// between "namespace {" and the C-ABI, pasted between this file and rect_kernel_emu_tail.inc by the test) compile as plain
// C++17. The three kernels have no barrier and no shared memory, so the lanes of a workgroup run one after the other on the
// calling thread; the only atomic is the deferred-error OR. Test infrastructure only.
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
