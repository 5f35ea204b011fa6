// Normalize-and-Project (Lyle et al. 2024): what net_kernels.hip hands to the launchers of project_kernels.hip, a translation unit of its
// own (its kernels are in no code object tests/golden/kernel_order.txt pins).  THE definition: include/isdqn_hip.h,
// isdqn_net_project_layout / isdqn_net_project_norms / isdqn_net_project_apply.  The tensors, their real-element predicate and their chunks
// are those of pruning (prune.h: PruneTensor, prune_table_finish); `k` and `scratch_off` of a PruneTensor mean nothing here.  No kernel in
// this header.
#pragma once

#include "prune.h"

namespace isdqn {

struct ProjectArgs {
    float* p;              // the parameter buffer (16-byte aligned)
    float* mirror;         // workspace + wsplit_off (same offsets as the master, 32-byte aligned), or nullptr: the master alone
    const double* target;  // rho_i, one per tensor (the apply alone)
    double* norms;         // n_i = sqrt(S_i), one per tensor, measured in front of the projection
    float* scales;         // s_i, one per tensor (the apply alone)
    double* scratch;       // one partial sum of squares per chunk, tab.total_chunks of them, chunk c of tensor i at first_chunk + c
    PruneTable tab;
};

// bytes of scratch a table needs: one double per chunk
inline int64_t project_scratch_bytes(const PruneTable& tab) { return (int64_t)tab.total_chunks * 8; }
// Two launches on stream `st`: the chunk sums, then one workgroup per tensor that adds them up and stores norms[i].  Writes no parameter.
int launch_project_norms(const ProjectArgs& a, hipStream_t st);
// Two launches on stream `st`: the chunk sums, then every chunk's workgroup adds up its tensor's sums, derives s_i and scales its floats.
int launch_project_apply(const ProjectArgs& a, hipStream_t st);

}  // namespace isdqn
