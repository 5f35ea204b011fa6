// What the four head-loss kernels share: td_kernel (net_kernels.hip, scalar heads), hl_loss_kernel (hl_gauss.h), qr_loss_kernel
// (quantile.h) and c51_loss_kernel (categorical.h).  loss_and_finalize (net_kernels.hip) fills one HeadLossArgs and launches the one
// the plan selects; each regresses online head on0 + k at the taken action on head tg0 + k of the next-state rows, k < K.
//
// A transition's discount is isdqn_batch_discount::discount[b] where the batch carries the tensor, else gamma_n (cfg->gamma_n).
// THE contract of a loss kernel -- what it writes from the head-output rows of a finished forward:
//   q_values / targets [B][K]  the scalar Q of the online head at the taken action and the unclamped scalar target (null: not written);
//   priorities [B]             sqrt(mean_k (q - target)^2 + 1e-10) on those scalars, never weighted by loss_weights (null: not written)
//                              -- the TD error of the expectations, not the distributional loss (a cross-entropy never falls below the
//                              target histogram's entropy);
//   loss_part [n_blk][K]       per-workgroup partial sums of the per-pair losses, weighted by loss_weights;
//   dout [B][pitch]            with `dout`: dL/d(head output), zero-filled, non-zero on the taken action's outputs of the K regressed
//                              heads only, weighted by loss_weights and divided by B;
//   dbh_part [n_blk][pitch]    with `dout`: the column sums of the workgroup's dout rows (the head-bias gradient).
// loss_finalize_kernel reduces loss_part and dbh_part in a fixed order.  Every sum here is in a fixed order too (ascending row of the
// workgroup, ascending k; a __shfl_xor butterfly across lanes): bit-identical from run to run, no atomics.
//
// The three distributional kernels are one frame around their own arithmetic: a workgroup takes R <= MAX_ROWS transitions and its waves
// share the R * K (transition, pair)s; loss_prologue stages the transitions, the kernel leaves dL/d(output) of every pair in its dynamic
// LDS (s_dl [R][K][nb]) and the pair's loss and squared TD error in the LossStage, loss_epilogue writes the outputs above.  td_kernel has
// another shape (64 transitions per workgroup, lanes over transitions) and shares the arguments only.
#pragma once

#include "munchausen.h"

namespace isdqn {

constexpr int MAX_ROWS = 4;              // transitions per workgroup of a distributional loss kernel
constexpr int MAX_GROUP = 256;           // bins / quantiles per (head, action) at most
constexpr int PER_LANE = MAX_GROUP / 64;  // of which a lane owns those at lane + 64 t

// Struct members cannot be __restrict__: a kernel copies the pointers it dereferences in its hot loop into __restrict__ locals.
struct HeadLossArgs {
    const float* out;                        // head-output rows [B][pitch] of the states (Q values, logits or quantiles)
    const float* val;                        // ... of the B next states that supply the bootstrap value
    const float* sel;                        // isdqn_net_config::double_q: rows whose head sel_head + k picks the action (null: off)
    int sel_pitch, sel_head;
    const float* mun;                        // munchausen.h: STATE rows whose head mun_head + k is the value head (null: off)
    int mun_pitch, mun_head;
    Munchausen mu;
    int B, R, K, on0, tg0, A;                // R: transitions per workgroup (distributional kernels)
    int nb, pitch;                           // outputs per (head, action): n_bins or n_quantiles (scalar heads: unused); row pitch of out / val / dout
    float vmin, eta, sigma;                  // histogram support: v_min, bin width, HL-Gauss sigma
    float huber_delta;                       // td_kernel: Huber delta; qr_loss_kernel: kappa (0: squared error / plain pinball loss)
    const int* action;                       // isdqn_batch
    const float* reward;
    const uint8_t* terminal;
    const float* loss_weights;               // (null: 1)
    const float* discount;                   // isdqn_batch_discount::discount: the row's discount in gamma_n's place (null: gamma_n)
    float gamma_n;
    float *dout, *q_values, *targets;
    double* priorities;
    float *loss_part, *dbh_part;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// Static LDS of a distributional loss kernel: the workgroup's transitions (padded rows: action -1, reward 0, not-terminal 0) and what
// its waves leave per (row, pair), [R][K] with K <= 64 (checked by the host).
struct LossStage {
    int action[MAX_ROWS];
    float r[MAX_ROWS], nt[MAX_ROWS], w[MAX_ROWS];  // nt: 1 - terminal; w: importance-sampling weights (none: 1)
    float g[MAX_ROWS];                              // the row's discount (isdqn_batch_discount::discount; none: gamma_n)
    float loss[MAX_ROWS * 64], td2[MAX_ROWS * 64];  // weighted loss; (q - target)^2, unweighted (0 on padded rows, stored by the kernel)
};

// Transitions per workgroup: MAX_ROWS while the dL/d(output) staging stays within 32 KB of LDS.
static inline int rows_per_wg(int K, int nb) {
    int R = (8192 / (K * nb));
    return R < 1 ? 1 : R > MAX_ROWS ? MAX_ROWS : R;
}

// Zero-fill of the workgroup's dout rows and the staging of its R transitions, by THREADS threads.  The caller's __syncthreads() follows.
template <int THREADS>
__device__ __forceinline__ void loss_prologue(const HeadLossArgs& a, LossStage& s) {
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * a.R;
    const int rows = min(a.R, a.B - b0);
    float* __restrict__ dout = a.dout;
    if (dout != nullptr)
        for (int i = tid; i < rows * a.pitch; i += THREADS) dout[(int64_t)b0 * a.pitch + i] = 0.f;
    if (tid < a.R) {
        const bool on = tid < rows;
        s.action[tid] = on ? a.action[b0 + tid] : -1;
        s.r[tid] = on ? a.reward[b0 + tid] : 0.f;
        s.nt[tid] = on ? 1.f - (float)a.terminal[b0 + tid] : 0.f;
        s.w[tid] = (on && a.loss_weights != nullptr) ? a.loss_weights[b0 + tid] : 1.f;
        if (on && a.discount != nullptr) ISDQN_BOUNDS_CHECK(a.discount + b0 + tid, 4, 50);
        s.g[tid] = (on && a.discount != nullptr) ? a.discount[b0 + tid] : a.gamma_n;
    }
}

// loss_part, the scatter of s_dl [R][K][nb] into dout, dbh_part and priorities, by THREADS threads after the __syncthreads() that
// completes s_dl, s.loss, s.td2 and the zero-fill.
template <int THREADS>
__device__ __forceinline__ void loss_epilogue(const HeadLossArgs& a, const LossStage& s, const float* s_dl) {
    const int tid = threadIdx.x;
    const int R = a.R, K = a.K, nb = a.nb, on0 = a.on0, pitch = a.pitch;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, a.B - b0);
    const int ldk = a.A * nb;  // outputs of one head
    float *__restrict__ dout = a.dout, *__restrict__ loss_part = a.loss_part, *__restrict__ dbh_part = a.dbh_part;
    double* __restrict__ priorities = a.priorities;
    for (int k = tid; k < K; k += THREADS) {
        float sum = 0.f;
        for (int bl = 0; bl < R; ++bl) sum += s.loss[bl * K + k];  // (padded rows: stored zeros)
        loss_part[(int64_t)blockIdx.x * K + k] = sum;
    }
    if (dout != nullptr) {
        for (int i = tid; i < rows * K * nb; i += THREADS) {
            const int pr = i / nb, j = i - pr * nb;
            const int bl = pr / K, k = pr - bl * K;
            dout[(int64_t)(b0 + bl) * pitch + (int64_t)(on0 + k) * ldk + (int64_t)s.action[bl] * nb + j] = s_dl[i];
        }
        // column c = (h * A + a) * nb + j collects the rows whose action is a, for the regressed heads h in [on0, on0 + K)
        for (int c = tid; c < pitch; c += THREADS) {
            const int h = c / ldk, rem = c - h * ldk, act = rem / nb, j = rem - act * nb;
            float sum = 0.f;
            if (h >= on0 && h < on0 + K)
                for (int bl = 0; bl < rows; ++bl) sum += (s.action[bl] == act) ? s_dl[((int64_t)bl * K + h - on0) * nb + j] : 0.f;
            dbh_part[(int64_t)blockIdx.x * pitch + c] = sum;
        }
    }
    if (priorities != nullptr && tid < rows) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s.td2[tid * K + k];
        priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }
}

}  // namespace isdqn
