// Soft head shift of iS-DQN: what net_kernels.hip hands to the launcher of soft_shift_kernels.hip, a translation unit of its own (its
// kernels are in no code object tests/golden/kernel_order.txt pins).  THE definition: include/isdqn_hip.h, isdqn_net_soft_shift.  No
// kernel in this header.
#pragma once

#include "common.h"

namespace isdqn {

struct SoftShiftArgs {
    float* p;          // the parameter buffer (16-byte aligned)
    float* mirror;     // workspace + wsplit_off (same offsets as the master, 32-byte aligned), or nullptr: the master alone
    int64_t w_off, b_off;  // kernel [out_p][in_p] and bias [out_p] of the last Dense in the buffer (floats; multiples of 8)
    int in_p, R, K;    // columns of a row (a multiple of 8), rows of a head block, heads written: rows [0, (1 + K) * R) are touched
    float omt, tau;
};

// One launch on stream `st`.  ISDQN_ERR_SHAPE / ISDQN_ERR_ARG, nothing launched: an offset or width that is no multiple of 8, an empty
// shape, a misaligned pointer.  The caller checks that the head blocks lie inside the last Dense (it holds the plan).
int launch_soft_shift(const SoftShiftArgs& a, hipStream_t st);

}  // namespace isdqn
