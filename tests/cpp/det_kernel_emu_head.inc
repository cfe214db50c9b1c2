// Host shim for tests/test_detect_kernel_emulation.py: lets the KERNEL SOURCE of aria_slam_amd/csrc/detect_stage.hip (the text
// between "namespace {" and the C-ABI, pasted between this file and det_kernel_emu_tail.inc by the test) compile as plain
// C++20. One std::thread per lane of a workgroup, __syncthreads() is a std::barrier, __shared__ is a function-local static
// (workgroups run one after the other), the integer atomics are std::atomic_ref. Test infrastructure only.
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define ARIA_DET_MAX_CANDIDATES 1024
#define ARIA_DET_MAX_CLASS_IDS 32
typedef struct { float x1, y1, x2, y2, confidence; int class_id; } aria_detection;
typedef struct { float x1, y1, x2, y2; } aria_box;
struct dim3e { int x = 0, y = 0, z = 0; };
static thread_local dim3e threadIdx, blockIdx;
static std::barrier<>* g_bar = nullptr;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
using std::min; using std::max;
static inline float __int_as_float(int v) { float f; std::memcpy(&f, &v, 4); return f; }
static inline int atomicAdd(int* p, int v) { return std::atomic_ref<int>(*p).fetch_add(v); }
static inline int atomicOr(int* p, int v) { return std::atomic_ref<int>(*p).fetch_or(v); }
static inline int atomicMax(int* p, int v) { int o = *p; while (o < v && !std::atomic_ref<int>(*p).compare_exchange_weak(o, v)) {} return o; }
typedef _Float16 __half;
static inline __half __float2half_rn(float v) { return (__half)v; }
static inline unsigned short __half_as_ushort(__half h) { unsigned short u; std::memcpy(&u, &h, 2); return u; }
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
struct uint2 { uint32_t x, y; };
