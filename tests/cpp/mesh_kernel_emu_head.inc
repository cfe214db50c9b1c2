// Host shim for tests/test_mesh_kernel_emulation.py and tests/test_mesh_host.py: lets the per-voxel and per-cell functions of
// aria_slam_amd/csrc/tsdf_mesh.hip (the text between "namespace {" and the kernels section, pasted between this file and
// mesh_kernel_emu_tail.inc by the test) compile as plain C++17. Those functions have no barrier, no shared memory and no
// atomics; the tail walks the chunks and lanes one after the other. Test infrastructure only.
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
using std::min; using std::max;
static inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline int __popc(uint32_t v) { return __builtin_popcount(v); }
