// Host shim for the plain rule functions of aria_slam_amd/csrc/alert_stage.hip (tests/test_alert_kernel_emulation.py): the text
// between "// ---- rules" and "// ---- kernels" of that file follows this head unchanged.
#include <cstdint>
#include <cstring>

#include "aria_orb_hip.h"

#define __host__
#define __device__
