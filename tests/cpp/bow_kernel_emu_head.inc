// Host shim for tests/test_bow_kernel_emulation.py: lets KERNEL SOURCE of aria_slam_amd/csrc/bow_index.hip -- the plain
// arithmetic between its two marker comments, pasted between this file and bow_kernel_emu_tail.inc by the test -- compile as
// plain C++17. That text has no barrier, no shared memory, no atomic and no cross-lane operation. Test infrastructure only.
#include <climits>
#include <cstdint>
#include <cstring>
#define BOW_HD static inline
namespace {
