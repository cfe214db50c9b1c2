// Host shim for tests/test_icp_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/icp_track.hip (the text
// between "namespace {" and the C-ABI section, pasted between this file and icp_kernel_emu_tail.inc by the test) compile as
// plain C++17. The kernels have no barrier and no shared memory, so the lanes of a workgroup run one after the other on the
// calling thread. icp_commit, the one cross-lane step of the file, is served here lane by lane: each lane's fp64 partial sums
// are converted and added to the row in turn, the integer atomics served in the order the lanes come. tri6 is the packed
// index of solver_device.h, which is device code. Test infrastructure only.
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
constexpr int tri6(int a, int c) { return a <= c ? 6 * a - a * (a - 1) / 2 + (c - a) : 6 * c - c * (c - 1) / 2 + (a - c); }
static inline void icp_commit(long long* row, double (&s)[28], int count) {
    for (int k = 0; k < 28; k++) row[k] += (long long)s[k];
    row[28] += count;
}
