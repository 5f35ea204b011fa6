// Random ensemble mixture: what net_kernels.hip hands to the launchers of mixture_kernels.hip, a translation unit of its own (its
// kernels are in no code object tests/golden/kernel_order.txt pins).  THE definition: include/isdqn_hip.h, isdqn_mixture_draw /
// isdqn_batch_mixture / ISDQN_ACT_MEAN_HEADS.  No kernel in this header.
#pragma once

#include "common.h"
#include "head_loss.h"  // HeadLossArgs: what every head-loss kernel is handed

namespace isdqn {

constexpr int MIX_MAX_HEADS = 1024;  // isdqn_mixture_draw's limit: one workgroup draws them all

// alpha [H] from (seed, *draw_count), then *draw_count += 1 in a launch of its own: two launches on stream `st`.
int launch_mixture_draw(int H, uint64_t seed, int64_t* draw_count, float* alpha, hipStream_t st);
// mix_td_kernel where td_kernel would stand: `a` as loss_and_finalize fills it for scalar heads (K = 1, on0 = tg0 = 0), `n_blk` =
// ceil(B / 64) workgroups, alpha [H] device floats.  ISDQN_ERR_SHAPE: a partition or pitch the kernel does not walk.
int launch_mix_td(const HeadLossArgs& a, int n_blk, const float* alpha, int H, hipStream_t st);
// out[i] = first argmax_a of sum_h q[i][h * A + a], i < n_rows, on stream `st`.
int launch_argmax_mean(const float* q, int n_rows, int nha_p, int A, int H, int* out, hipStream_t st);

}  // namespace isdqn
