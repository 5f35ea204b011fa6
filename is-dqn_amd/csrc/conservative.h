// The conservative (CQL) term beside the head losses: what net_launch.h hands to the launcher of conservative_kernels.hip, a translation
// unit of its own (its kernels are in no code object tests/golden/kernel_order.txt pins).  THE definition: include/isdqn_hip.h,
// isdqn_batch_conservative.  No kernel in this header.
#pragma once

#include "common.h"

namespace isdqn {

constexpr int CQL_MAX_PAIRS = 64;  // regressed pairs of a call, as the distributional loss kernels (LossStage)

// The rows a loss kernel has just finished, with the row partition it used: workgroup `blk` of n_blk owns the dout rows
// [blk * rows_per_blk, ...), loss_part[blk][K] and dbh_part[blk][pitch] -- one owner per address, read-modify-write.
struct ConservativeArgs {
    const float* out;            // head-output rows [B][pitch] of the states (Q values, logits or quantiles)
    float* dout;                 // dL/d(head output) [B][pitch] as the loss kernel left it (null: a loss-only call)
    float *loss_part, *dbh_part; // [n_blk][K], [n_blk][pitch]
    const int* action;           // isdqn_batch
    const float* loss_weights;   // (null: 1)
    int B, rows_per_blk, n_blk, K, on0, A;
    int nb, pitch;               // outputs per (head, action): n_bins or n_quantiles (0: scalar heads); row pitch of out / dout
    int quantile;                // nb > 0: quantile heads (else histogram heads)
    float vmin, eta;             // histogram support: v_min, bin width
    float alpha;                 // cql_alpha > 0
    int64_t dout_floats, part_floats;  // extents the plan reports: the "dout" region, the "loss_partials" region
};

// Adds the term on stream `st`, behind the loss kernel and in front of loss_finalize.  ISDQN_ERR_SHAPE: a row or column of the grid
// outside the extents; ISDQN_ERR_UNSUPPORTED: a size the kernels do not run.
int launch_conservative(const ConservativeArgs& a, hipStream_t st);

}  // namespace isdqn
