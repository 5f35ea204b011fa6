/*
 * isdqn_hip.h -- C ABI of the MI355X (gfx950) iS-DQN hot path.
 *
 * The reference (theovincent/iS-DQN, python package `slimdqn`) has no FFI layer:
 * its hot path is numpy + an XLA executable.  This header is the boundary a
 * maintainer would bind instead (ctypes stub: INTEGRATION.md).  Every entry
 * point names the reference code it replaces (paths relative to the reference
 * root).  Conventions:
 *   - plain pointers and sizes only; all data pointers are DEVICE pointers
 *     unless the parameter name ends in `_host`;
 *   - `stream` is a hipStream_t (0 = default stream); calls enqueue work and
 *     return without synchronising;
 *   - return value: ISDQN_OK or a negative ISDQN_ERR_* (host-detectable
 *     argument errors).  Data-dependent violations that the reference reports
 *     as exceptions (negative priority, query target outside [0, root)) are
 *     reported through a device status word (`dev_status`, OR-ed bits
 *     ISDQN_STATUS_*), so that the fused training step never synchronises;
 *   - nothing here allocates device memory: the caller owns every buffer
 *     (torch tensors in the python host layer).
 */
#ifndef ISDQN_HIP_H
#define ISDQN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
#define ISDQN_OK 0
#define ISDQN_ERR_CAPACITY (-1)    /* sum_tree.py:12  "Capacity to sum tree must be positive."   -> AssertionError */
#define ISDQN_ERR_NEGATIVE (-2)    /* sum_tree.py:31  "Values must be positive."                 -> AssertionError */
#define ISDQN_ERR_SHAPE (-3)       /* sum_tree.py:30  indices/values shape mismatch              -> AssertionError */
#define ISDQN_ERR_EMPTY (-4)       /* replay_buffer.py:200 / samplers.py:41 empty buffer         -> AssertionError */
#define ISDQN_ERR_RANGE (-5)       /* sum_tree.py:73-74 target outside [0, root)                 -> ValueError     */
#define ISDQN_ERR_UNSUPPORTED (-6) /* configuration that is not built (BatchNorm, conv widths above 64 channels, ...) */
#define ISDQN_ERR_HIP (-7)         /* a HIP runtime call failed; see isdqn_last_error()           */
#define ISDQN_ERR_ARG (-8)         /* null pointer / bad size                                     */

/* bits of the device status word */
#define ISDQN_STATUS_NEGATIVE_VALUE 1u /* tree_set saw a value < 0: nothing was modified          */
#define ISDQN_STATUS_TARGET_RANGE 2u   /* tree_query saw a target outside [0, root)               */
#define ISDQN_STATUS_EMPTY_TREE 4u     /* tree_query with root == 0                               */

const char* isdqn_version(void);
const char* isdqn_last_error(void); /* thread-local text of the last ISDQN_ERR_HIP / _ARG */

/* ========================================================================== */
/* Sum tree  (slimdqn/sample_collection/sum_tree.py)                          */
/* ========================================================================== */

/* SumTree.__init__ sizing, sum_tree.py:11-18.  Host-only arithmetic. */
int isdqn_tree_layout(int64_t capacity, int32_t* depth, int64_t* first_leaf_offset, int64_t* n_nodes);

/* SumTree.set, sum_tree.py:20-47.  `nodes` is the float64 node array (n_nodes).
 * Batch of n <= ISDQN_TREE_MAX_BATCH (leaf index, value) pairs.  Bit-exact with the
 * reference: duplicates keep the FIRST occurrence (np.unique), deltas are added to every
 * ancestor sequentially in ascending leaf order (np.add.at).  `max_recorded_priority`
 * (device double, may be NULL) is raised to max(values) as sum_tree.py:32 does. */
#define ISDQN_TREE_MAX_BATCH 4096
int isdqn_tree_set(double* nodes, int32_t depth, const int32_t* indices, const double* values, int32_t n,
                   double* max_recorded_priority, uint32_t* dev_status, void* stream);

/* The two-leaf set of PrioritizedSamplingDistribution.remove, samplers.py:89-103:
 * set([index, last_index], [get(last_index), 0.0]) (or set(index, 0.0) when equal), with the
 * leaf read done on the device so that eviction never synchronises. */
int isdqn_tree_swap_remove(double* nodes, int32_t depth, int32_t index, int32_t last_index, uint32_t* dev_status,
                           void* stream);

/* SumTree.query, sum_tree.py:58-102.  If `targets_are_unit` != 0 the inputs are unit
 * draws u in [0,1) and the target is 0.0 + root*u, which is bit-identical to numpy's
 * Generator.uniform(0.0, root, n) of samplers.py:110 on the same PCG64 stream.
 * Writes n leaf indices (int32). */
int isdqn_tree_query(const double* nodes, int32_t depth, const double* targets, int32_t n, int32_t targets_are_unit,
                     int32_t* out_indices, uint32_t* dev_status, void* stream);

/* isdqn_tree_query plus the importance-sampling weights of prioritized replay (Schaul et al. 2016, section 3.4; the
 * reference has none), in the same launch.  THE definition: for the n sampled leaves with tree values p_i (already raised to
 * the priority exponent alpha by the sampler) and root R, P(i) = p_i / R and, with N the number of stored keys,
 *     w_i = (N P(i))^(-beta) / max_j (N P(j))^(-beta)  =  (p_min / p_i)^beta,     p_min = min_j p_j over the batch
 * (N and R cancel under the batch-max normalisation -- Dopamine's and the paper's "normalise by 1 / max w" -- which is also why
 * no min-tree is needed).  pow(p_min / p_i, (double)beta) is evaluated in float64 and rounded once to float32, so the largest
 * weight is exactly 1.0f and beta = 0 gives exactly 1.0f everywhere.  A sampled leaf with p_i <= 0 (possible only by rounding
 * at the right edge of the tree) is left out of the minimum and gets weight 1.0f; if no sampled leaf is positive all weights
 * are 1.0f (the status word already reports the empty tree).
 * `beta` is a DEVICE float, read by the kernel: a captured graph anneals it without a second capture.  n <=
 * ISDQN_TREE_MAX_BATCH (one workgroup: the batch minimum is reduced through LDS); out_indices and the status bits are
 * bit-identical to isdqn_tree_query on the same inputs; out_leaf (may be NULL) receives the n leaf values p_i. */
int isdqn_tree_query_weighted(const double* nodes, int32_t depth, const double* targets, int32_t n, int32_t targets_are_unit,
                              const float* beta, int32_t* out_indices, double* out_leaf, float* out_weights,
                              uint32_t* dev_status, void* stream);

/* ========================================================================== */
/* Device-resident replay  (slimdqn/sample_collection/replay_buffer.py)        */
/* ========================================================================== */
/* Layout in HBM: single frames `frames[slot][h*w]` (uint8) + an element table indexed by
 * element slot (= key % capacity): frame slots of the state stack and of the next-state
 * stack (-1 = all-zero frame: the zero padding of replay_buffer.py:131-134), action,
 * n-step reward, terminal flag.  ReplayBuffer.sample (:198-213) becomes two kernels:
 * the row gather below and, only for callers that want the reference's batch layout,
 * the stack materialisation. */

/* ReplayBuffer.add, device side (replay_buffer.py:185-196: `self._memory[key] = ...`, the FIFO eviction and the sampler's
 * index bookkeeping).  The host accumulator stages what changed since the last flush in one buffer -- byte offsets into
 * `staged` below, every section 16-byte aligned -- and one launch scatters it:
 *   frames[frame_slots[i]] <- frame_data[i]                          (n_frames new observations of frame_bytes bytes)
 *   element row rows[r]    <- row_frames[r][stack2], row_action[r], row_reward[r], row_terminal[r]     (n_rows)
 *   index_to_slot[index_rows[i]] <- index_vals[i]                                                      (n_index)   */
typedef struct isdqn_staged_updates {
    int32_t n_frames, frame_bytes;
    int64_t off_frame_slots; /* int32 [n_frames]              */
    int64_t off_frame_data;  /* uint8 [n_frames][frame_bytes] */
    int32_t n_rows, stack2;
    int64_t off_rows;         /* int32 [n_rows]               */
    int64_t off_row_frames;   /* int32 [n_rows][stack2]       */
    int64_t off_row_action;   /* int32 [n_rows]               */
    int64_t off_row_reward;   /* float [n_rows]               */
    int64_t off_row_terminal; /* uint8 [n_rows]               */
    int32_t n_index, reserved;
    int64_t off_index_rows;   /* int32 [n_index]              */
    int64_t off_index_vals;   /* int32 [n_index]              */
} isdqn_staged_updates;
int isdqn_replay_apply_staged(const uint8_t* staged, const isdqn_staged_updates* updates, uint8_t* frames, int64_t frame_stride,
                              int32_t* elem_frames, int32_t* elem_action, float* elem_reward, uint8_t* elem_terminal,
                              int32_t* index_to_slot, void* stream);

/* Gather the element rows of `B` sampled elements: frame ids [B][2*stack], action, reward,
 * terminal (itemgetter + np.stack of the scalar fields, replay_buffer.py:206-212).  `slots`
 * are element slots, or -- when `index_to_slot` is not NULL -- the sampler's dense indices
 * (samplers.py:43, :111), mapped through that table (the device copy of `_index_to_key`,
 * samplers.py:45-49, reduced modulo the capacity). */
int isdqn_replay_gather_rows(const int32_t* elem_frames, const int32_t* elem_action, const float* elem_reward,
                             const uint8_t* elem_terminal, int32_t stack, const int32_t* index_to_slot,
                             const int32_t* slots, int32_t B, int32_t* out_frame_ids, int32_t* out_action,
                             float* out_reward, uint8_t* out_terminal, void* stream);

/* Materialise ReplayElement.state / .next_state, each (B, h, w, stack) uint8 in the
 * reference's channel-last layout (replay_buffer.py:131-147 + np.stack :212). */
int isdqn_replay_materialize(const uint8_t* frames, int64_t frame_stride, int32_t h, int32_t w, int32_t stack,
                             const int32_t* frame_ids, int32_t B, uint8_t* out_state, uint8_t* out_next_state,
                             void* stream);

/* Inverse: split channel-last stacks (B, h, w, stack) into 2*B*stack single frames
 * (planar) + the id table, for callers that hold reference-layout batches. */
int isdqn_replay_deinterleave(const uint8_t* state, const uint8_t* next_state, int32_t h, int32_t w, int32_t stack,
                              int32_t B, uint8_t* out_frames, int32_t* out_frame_ids, void* stream);

/* DrQ random-shift augmentation of the frame stacks of `n_rows` sampled transitions (Kostrikov, Yarats and Fergus 2020, K = M = 1;
 * DrQ(eps) of Agarwal et al. 2021; also what DER, SPR and BBF apply), on the device.  The learn step reads frames + frame_stride +
 * frame_ids and never the replay itself, so the option is built beside it: this call writes the shifted copies of the batch's frames
 * into the scratch pool `out_frames` and a table `out_frame_ids` that points into the pool; hand those two to isdqn_batch in place of
 * the store and the gathered table.  No kernel of the learn step knows of it, and every torso that reads frames takes it.
 * THE definition.  frame_ids is [n_rows][2*stack] as isdqn_replay_gather_rows wrote it: ids [0, stack) the state stack of the row,
 * [stack, 2*stack) its next-state stack.
 *   Which draw.  Row r belongs to step t = *aug_count + r / rows_per_step and is row b = r % rows_per_step of that step; half = 0 for
 *     the state stack, 1 for the next-state stack.
 *   The draw.  (x0, x1) = the first two output words of Philox4x32-10 (the function of the noisy layers) at counter
 *     (b, 0x80000000 | half, lo32(t), hi32(t)) under key (lo32(seed), hi32(seed)); bit 31 of counter word 1 keeps these draws disjoint
 *     from the noisy layers' (their word 1 is (stream_id << 16) | vector id) under the same seed.
 *     dx = (int)(((uint64_t)x0 * (2*pad+1)) >> 32) - pad, dy the same from x1: each uniform on [-pad, pad] up to 2^-32 * (2*pad+1).
 *     ONE draw serves all `stack` frames of a half; the two halves draw independently.
 *   The pixels.  out[y][x] = in[clamp(y + dy, 0, h-1)][clamp(x + dx, 0, w-1)]: replicate-pad the frame by `pad` on every side and
 *     crop h x w at offset (pad + dy, pad + dx).
 *   The id table.  An input id >= 0 at row r, position k: out_frame_ids[r][k] = r * 2*stack + k, and that frame of the pool (h*w bytes
 *     at out_frames + (r * 2*stack + k) * frame_stride) is written; the bytes between h*w and frame_stride are not.  An input id -1
 *     (the all-zero frame of the leading padding) stays -1 and its frame of the pool is NOT written.
 *   The counter.  A one-thread launch behind the shift stores *aug_count + n_rows / rows_per_step with an ordinary store (no atomics
 *     anywhere).  So one call over the S*B rows of S steps with rows_per_step = B is bit for bit S calls over B rows each, and a
 *     captured graph that holds the call draws anew at every replay.
 * pad = 0 is the identity copy (the counter still advances); pad >= h or pad >= w is legal, the clamp handles it.
 * ISDQN_ERR_ARG, and nothing is launched: pad < 0 or pad > 127; h, w, stack or n_rows < 1; rows_per_step < 1 or no divisor of n_rows;
 * frame_stride < h*w; a NULL pointer; out_frames overlapping frames -- the store's extent is no argument, so what is refused is the
 * store's base inside the pool and the pool's base inside the store's first frame; out_frame_ids overlapping frame_ids; an id table
 * that is not 4-byte or a counter that is not 8-byte aligned; more than 2^31 - 1 output frames.
 * When h*w, frame_stride and both frame bases are multiples of 16 (84 x 84 = 441 * 16) the copy moves 16-byte pieces through LDS;
 * any other geometry takes a byte path with the same result. */
int isdqn_replay_augment_shift(const uint8_t* frames, int64_t frame_stride, int32_t h, int32_t w, int32_t stack,
                               const int32_t* frame_ids /* [n_rows][2*stack] */, int32_t n_rows, int32_t rows_per_step,
                               int32_t pad, uint64_t seed, int64_t* aug_count,
                               uint8_t* out_frames /* [n_rows*2*stack][frame_stride] */, int32_t* out_frame_ids, void* stream);

/* Horizon windows: an annealed update horizon and discount (SR-SPR, BBF: n 10 -> 3, gamma 0.97 -> 0.997 after every reset).
 * The tables above fix an element's n-step return and next-state stack on the host when the element is added.  A replay built
 * with horizon windows keeps three more tables per element slot, for the largest horizon n_max (1..128) it will serve.  For an
 * element whose state ends at position s of a trajectory of L steps:
 *   elem_window [C][stack + n_max] int32  the frame ids at positions s - stack + 1 .. s + n_max, -1 where the reference has a zero
 *                                         frame (in front of the trajectory, or behind its end);
 *   elem_steps  [C][n_max] float          the per-step rewards from s on (after reward clipping, where set), 0 behind the end;
 *   elem_len    [C] int32                 min(s + n_max, L) - s: how many of those steps lie inside the trajectory;
 * and elem_terminal is the element's terminal flag at n_max.  For any horizon m <= n_max that gives the element the reference builds
 * at update_horizon = m: next state = window[m : m + stack], return = the discounted sum of the first min(m, len) rewards, terminal =
 * terminal_nmax && m >= len.  (The states within n_max - m steps in front of a truncation, which a buffer at m emits and one at n_max
 * never does, are not in it.)
 *
 * The scatter of the three tables' staged rows, beside isdqn_replay_apply_staged and from the same staged buffer: byte offsets into
 * `staged` of rows int32 [n_rows] (the element slots), window int32 [n_rows][stack + n_max], steps float [n_rows][n_max] and len
 * int32 [n_rows].  ISDQN_ERR_ARG: a NULL pointer, n_rows < 0, stack < 1, n_max outside 1..128, a negative or misaligned offset.
 * n_rows == 0 launches nothing. */
int isdqn_replay_apply_staged_horizon(const uint8_t* staged, int32_t n_rows, int64_t off_rows, int64_t off_window, int64_t off_steps,
                                      int64_t off_len, int32_t stack, int32_t n_max, int32_t* elem_window, float* elem_steps,
                                      int32_t* elem_len, void* stream);

/* The gather of a horizon-window replay: B sampled rows, cut at a horizon and discounted at a rate that the kernel READS FROM DEVICE
 * MEMORY (`horizon`: one int32, `gamma`: one float), so a captured graph follows a schedule without a second capture, as it does the
 * importance-sampling exponent.  `slots` and `index_to_slot` as in isdqn_replay_gather_rows.
 * THE definition, for row b with element slot e:
 *   m = clamp(*horizon, 1, n_max), me = min(m, elem_len[e]);
 *   out_frame_ids[b][0 .. stack)       = elem_window[e][0 .. stack);
 *   out_frame_ids[b][stack .. 2 stack) = elem_window[e][m .. m + stack);
 *   in float64 with G = (double)*gamma: g_0 = 1, g_{t+1} = g_t * G, acc_0 = 0, acc_{t+1} = acc_t + (double)elem_steps[e][t] * g_t, t
 *     ascending, every operation rounded on its own (no fused multiply-add);
 *   out_reward[b]   = (float)acc_me;
 *   out_discount[b] = (float)g_m -- m, not me: the two differ only on terminal rows, whose bootstrap is masked.  It is what
 *     isdqn_batch_discount::discount takes;
 *   out_terminal[b] = elem_terminal[e] && m >= elem_len[e];
 *   out_action[b]   = elem_action[e].
 * One launch, plain loads and stores, no atomics; a row's sum runs sequentially in one lane, the id copy goes over lanes.
 * ISDQN_ERR_ARG, and nothing is launched: a NULL pointer (index_to_slot may be NULL), B < 1, stack < 1, n_max outside 1..128. */
int isdqn_replay_gather_horizon(const int32_t* elem_window, const float* elem_steps, const int32_t* elem_len, const int32_t* elem_action,
                                const uint8_t* elem_terminal, int32_t stack, int32_t n_max, const int32_t* index_to_slot,
                                const int32_t* slots, int32_t B, const int32_t* horizon, const float* gamma, int32_t* out_frame_ids,
                                int32_t* out_action, float* out_reward, uint8_t* out_terminal, float* out_discount, void* stream);

/* ========================================================================== */
/* Q-network + iS-DQN update  (slimdqn/networks/architectures/dqn.py, isdqn.py) */
/* ========================================================================== */
#define ISDQN_ARCH_CNN 0 /* dqn.py:48-74  three SAME convs (8s4, 4s2, 3s1) + dense stack */
#define ISDQN_ARCH_FC 1  /* dqn.py:89-103 dense stack only                               */
#define ISDQN_ARCH_IMPALA 2 /* dqn.py:7-36, 75-88  three Stacks (conv3x3, max-pool 3x3/2, two residual blocks) + dense stack */
#define ISDQN_MAX_FEATURES 8

#define ISDQN_PRECISION_BF16X3 0 /* split-bf16 MFMA (hi*hi + lo*hi + hi*lo), fp32 accumulate: ~2^-17 */
#define ISDQN_PRECISION_BF16 1   /* single-pass bf16 MFMA, fp32 accumulate: ~2^-9                    */

typedef struct isdqn_net_config {
    int32_t arch;                         /* ISDQN_ARCH_*                                              */
    int32_t obs_h, obs_w, obs_c;          /* cnn: frame h, w and stack size; fc: obs_c = obs dim, h=w=1 */
    int32_t n_features;                   /* len(features) (isdqn.py:19)                               */
    int32_t features[ISDQN_MAX_FEATURES]; /* cnn: 3 conv widths then dense widths; fc: dense widths     */
    int32_t n_actions;                    /* A                                                         */
    int32_t n_heads;                      /* 1 + n_bellman_iterations (isdqn.py:34-41); 1 = DQN / TF-DQN */
    int32_t dueling;                      /* (behind n_heads, with the other head-shape fields: huber_delta .. hl_min stay contiguous and the
                                           * struct still ends in hl_sigma, double_q.)  Dueling value / advantage heads (Wang et al., "Dueling Network Architectures for
                                           * Deep Reinforcement Learning", ICML 2016).  0: off -- every result, workspace size, region
                                           * offset and launch keeps what it had before the field existed.  1: on.  Anything else:
                                           * ISDQN_ERR_ARG.  THE definition, with w = max(n_bins, n_quantiles, 1), A = n_actions,
                                           * H = n_heads, F = features[n_features - 1] (the width of the last hidden Dense), F2 = F / 2:
                                           * Raw head: the last Dense has R = H * (A + 1) * w outputs; output ((h * (A + 1)) + c) * w + j
                                           * belongs to head h, stream row c, component j; c < A is advantage a = c, c = A is the value.
                                           * Its Flax name stays the head's Dense_n, shape (F, R).
                                           * Streams: the value rows read the hidden units [0, F2), the advantage rows read [F2, F); every
                                           * other weight of the head kernel is a structural zero (-f 32 64 64 1024 gives Wang's two
                                           * 512-wide streams).  With layer_norm the LayerNorm behind the last hidden layer spans both
                                           * halves: the two streams share its statistics.
                                           * Combine: for every row, head and j, in fp32 and in this order,
                                           *     s    = sum_a raw[a][j]                                  in ascending a
                                           *     mean = s / (float)A
                                           *     out[(h * A + a) * w + j] = raw[A][j] + (raw[a][j] - mean)
                                           * The combined rows have exactly the layout and pitch of the heads without the option ("q" at
                                           * w = 1, "logits" at w > 1), and everything downstream reads them as it does without it: the
                                           * four loss kernels, the expectations / means, the argmax kernels and isdqn_net_forward's q_out.
                                           * For histogram heads this is Rainbow's per-atom dueling of the logits, for quantile heads it is
                                           * per quantile.
                                           * Backward: with d the loss kernels' dout [B][pitch],
                                           *     draw[A][j] = sum_a d[a][j]                              in ascending a
                                           *     draw[a][j] = d[a][j] - draw[A][j] / (float)A
                                           * and the gradient of the raw head's bias is the same map applied to the reduced head-bias
                                           * gradient.  Fixed order, no atomics, bit-identical from run to run.
                                           * The structural zeros stay +0.0f for the life of the parameters in `params`, adam_m, adam_v,
                                           * the bf16 hi / lo weight mirror and grad_out of grad_on_batch: they are re-zeroed behind the
                                           * head's Adam launch on that launch's stream (Adam is per element, so this equals a masked
                                           * gradient exactly).  The caller's initialisation writes the zeros.
                                           * Unchanged, on the combined values: q_values, targets, priorities, loss_weights, losses_accum,
                                           * priorities_ready, the tie rule, double_q, Munchausen, the *_target forms, grad_on_batch with
                                           * n_pairs.  shift_params moves whole head blocks of (A + 1) * w rows, the value rows with them.
                                           * isdqn_net_redo zeroes the outgoing column of a recycled last-hidden neuron in every raw row.
                                           * Workspace regions, only with the option, behind every other region: "head_raw" [2B][R padded
                                           * to 8] (the head Dense's output), "head_raw_target" (rows of "q_target" x R padded, whenever
                                           * "q_target" exists), "dout_raw" [B][R padded] and "dbh_raw" [R padded].
                                           * ISDQN_ERR_ARG: F odd, no hidden Dense in front of the head.  ISDQN_ERR_UNSUPPORTED: batch_norm,
                                           * arch impala, w > 1 with R > 5456, more than 64 regressed heads.                          */
    int32_t layer_norm;                   /* 0/1 (dqn.py:56, 63, 70, 97)                               */
    int32_t batch_size;                   /* B: learn_on_batch runs the network on 2B rows (isdqn.py:95) */
    int32_t precision;                    /* ISDQN_PRECISION_*                                         */
    float gamma_n;                        /* gamma ** update_horizon (isdqn.py:107)                    */
    float learning_rate, adam_b1, adam_b2, adam_eps; /* optax.adam(lr, eps=adam_eps) (isdqn.py:46)    */
    float max_grad_norm;                  /* (behind adam_eps, with the other fields of the optimizer: huber_delta .. hl_min stay contiguous
                                           * and the struct still ends in hl_sigma, double_q.)  Clipping of the gradient by its global norm
                                           * in front of Adam (optax.clip_by_global_norm chained with optax.adam).  0: off -- every result,
                                           * workspace size, region offset and launch keeps what it had before the field existed.  > 0
                                           * (+inf allowed: measure, never clip): on.  Negative or NaN: ISDQN_ERR_ARG.  THE definition,
                                           * with c = max_grad_norm and g the reduced gradient the step would have fed to Adam (the sum of
                                           * its split-K / per-image slabs in adam_kernel's own order):
                                           *     n     = sqrt( sum over every trainable parameter element of g^2 )
                                           *     scale = 1 if n < c or n == 0, else c / n
                                           *     Adam consumes fl32(g * scale)
                                           * The norm runs over all leaves together: conv and dense kernels, biases, LayerNorm scale and
                                           * bias, all heads.  Padding elements carry a zero gradient.  With dueling = 1 the structural
                                           * zeros of the head kernel are NOT part of the norm (their raw weight gradient is not zero):
                                           * they are zeroed in the reduced gradient before the squares are taken.  The squares of the fp32
                                           * gradient are accumulated in float64 in a fixed order, without atomics: per workgroup of the
                                           * reduction over the float4 positions it owns (16 in ascending order where slabs are summed,
                                           * 256 through a fixed tree where one slab is the gradient), then over the workgroups' partial
                                           * sums by one workgroup (strided per thread, then a fixed tree).  n and scale are formed in
                                           * float64 and stored as fp32; g * scale is one fp32 multiply per element in front of Adam's
                                           * element update.  Every learn step computes them: learn_on_batch, its *_target and debug forms,
                                           * and grad_on_batch, which updates nothing.  `grad_out`, where a caller passes it, stays the raw,
                                           * unclipped reduced gradient (masked under dueling as without the option): the vector whose
                                           * norm was taken.
                                           * Workspace regions, only with the option, behind every other region: "grad_clip_partials" (one
                                           * float64 per workgroup of the reduction) and "grad_clip", four floats:
                                           *     [0] n of the last step            [1] scale of the last step
                                           *     [2] running sum of n over update steps (fp32: [2] += [0])
                                           *     [3] running count of update steps whose stored fp32 scale is < 1
                                           * The caller zeroes [2] and [3], as it does losses_accum; a gradient-only pass writes [0] and [1]
                                           * alone.  With the option no Dense weight gradient is fused into Adam and no optimizer launch
                                           * runs beside a gradient that is still being written: both streams of the step join in front of
                                           * the norm, and one Adam launch follows it.  ISDQN_ERR_UNSUPPORTED: batch_norm, arch impala (their learn paths run optimizer
                                           * launches of their own).                                                                  */
    float huber_delta;                    /* 0: squared TD error, the reference's loss (isdqn.py:102); > 0: Huber loss with
                                           * this delta (0.5 d^2 for |d| <= delta, delta (|d| - delta/2) beyond; the north
                                           * star's wording), gradient clip(d, -delta, delta)                */
    float munchausen_tau, munchausen_alpha, munchausen_clip;
                                          /* (behind huber_delta, with the other options of the target and the loss: the
                                           * struct still ends in double_q.)  Munchausen targets (Vieillard, Pietquin, Geist,
                                           * "Munchausen Reinforcement Learning", NeurIPS 2020).  munchausen_tau == 0: off -- the other two fields are ignored and every result keeps
                                           * the bits it had before the fields existed.  munchausen_tau > 0: on.  tau < 0 or non-finite,
                                           * alpha outside [0, 1], clip > 0 or non-finite: ISDQN_ERR_ARG; double_q = 1 together with
                                           * tau > 0: ISDQN_ERR_ARG (the soft value has no argmax to decouple).  THE definition, with
                                           * tau = munchausen_tau, alpha = munchausen_alpha, l0 = munchausen_clip: for every regressed
                                           * pair k < K with value head v = target_head + k (iS-DQN: v = k; grad_on_batch with
                                           * n_pairs > 0: the heads the caller names),
                                           *     V(x)      = m + tau * log( sum_a exp((Q^val_v(x, a) - m) / tau) ),  m = max_a Q^val_v(x, a)
                                           *     bonus_bk  = alpha * clip( Q^val_v(s_b, a_b) - V(s_b), l0, 0 )
                                           *                                             ( = alpha * clip(tau ln pi(a_b|s_b), l0, 0) )
                                           *     target_bk = r_b + bonus_bk + (1 - terminal_b) * gamma^n * V(s'_b)
                                           *                                             ( V(s') = sum_a' pi(a'|s') (Q - tau ln pi)(s', a') )
                                           * with pi = softmax(Q^val_v / tau).  Q^val is the network that supplies the next-state value
                                           * with the option off: the same parameters, or `target_params` in the *_target forms and in
                                           * grad_on_batch -- on the STATE rows (the bonus) as well as on the next-state rows.  With the
                                           * same parameters both are rows of the one forward over concat(state, next_state); with
                                           * target_params the target parameters run over all 2B rows into the workspace region
                                           * "q_target" ([2B][n_heads * A padded to 8]; histogram heads: "logits_target", "q_target" its
                                           * expectations), then the online parameters over the B states.  `terminal` does not mask the
                                           * bonus.  With update_horizon > 1 r_b is the n-step return the replay delivers and the bonus
                                           * is that of the FIRST action only: the batch carries no other action.  No gradient flows
                                           * through any Q^val term, the state-row term included, even where that head is itself being
                                           * learned in another pair: dL/dq keeps exactly one non-zero per (transition, pair), at
                                           * (online_head + k, a_b).  Everything behind the target is unchanged: q_values, the squared /
                                           * Huber / HL-Gauss loss, loss_weights, the priorities (the raw TD error on these targets),
                                           * losses_accum, priorities_ready.  alpha = 0 gives soft-DQN targets.  Acting (best_action[s])
                                           * is unchanged: greedy on Q, as the paper's M-DQN.  With n_bins > 0 Q means the expectations
                                           * sum_j softmax(l)_j c_j; `targets` stays the unclamped scalar.  A single head without
                                           * target_params (TF-DQN) is regularised by its own stop-gradient policy: supported.
                                           * batch_norm: supported without target_params (both halves are rows of the training-mode
                                           * forward); with target_params ISDQN_ERR_UNSUPPORTED.  The regions "q_target" /
                                           * "logits_target" hold [2B] rows with tau > 0 ([B] with double_q = 1) and exist only with one
                                           * of the two options, behind every other region: an off configuration's workspace keeps its
                                           * size and offsets.                                                                          */
    int32_t batch_norm;                   /* 0/1 (dqn.py:52-53, 59-60, 66-67, 73-74, 100-101): flax.linen.BatchNorm behind the
                                           * input scaling and behind every hidden layer's ReLU -- `axis=(1, 2)` on image
                                           * tensors (statistics per pixel position over batch AND channels), per feature on
                                           * flattened / dense activations; momentum 0.99, epsilon 1e-5.  learn / loss run it on
                                           * the batch statistics of concat(state, next_state) (isdqn.py:95), which couples the two
                                           * halves: the backward then runs over all 2B rows (csrc/batchnorm.h, generic engine,
                                           * one stream).  forward / best_action(s) use the running averages (isdqn.py:130).
                                           * impala: also behind the ReLU of every residual block (dqn.py:29-30, module
                                           * names "Stack_s/BatchNorm_b").  grad_on_batch runs with it (the analysis agents,
                                           * analysisdqn.py:162-219; with `target_params` the two halves are two forwards on
                                           * their own statistics and the backward covers the B state rows).  The *_target
                                           * learn / loss entry points (DQN) return ISDQN_ERR_UNSUPPORTED with it: the reference's
                                           * DQN cannot run with it either (dqn.py:86 applies the network without a mutable
                                           * batch_stats collection).                                                           */
    int32_t categorical;                  /* (between batch_norm and n_bins, whose loss it switches: huber_delta .. batch_norm and n_bins,
                                           * n_quantiles, hl_min stay contiguous and the struct still ends in hl_sigma, double_q.)  The C51
                                           * categorical projection loss (Bellemare, Dabney and Munos, "A Distributional Perspective on
                                           * Reinforcement Learning", ICML 2017) on the histogram heads.  0: off -- every result, workspace
                                           * size and region offset keeps the bits it had before the field existed.  1: on.  Anything else:
                                           * ISDQN_ERR_ARG; 1 with n_bins = 0 or with n_quantiles > 0: ISDQN_ERR_ARG; with munchausen_tau >
                                           * 0: ISDQN_ERR_UNSUPPORTED (the atom-wise Munchausen form is a follow-up); huber_delta > 0,
                                           * batch_norm, more than 64 regressed heads and n_heads * n_actions * n_bins > 5456 are refused
                                           * exactly as the histogram heads refuse them.  hl_sigma is ignored (it may be 0).  THE
                                           * definition, with categorical = 1: the heads are the histogram heads of n_bins = nb with the
                                           * same layout -- logit ((h * A) + a) * nb + j is atom j of action a of head h, eta = (hl_max -
                                           * hl_min) / nb, the atoms are the bin centres z_j = c_j = hl_min + (j + 1/2) eta (Bellemare's 51
                                           * atoms on [-10, 10] are nb = 51 on [-10.2, 10.2]), Q_h(s, a) = sum_j softmax(l_{h,a})_j z_j;
                                           * forward, best_action(s) and shift_params do not change at all.  For every regressed pair
                                           * k < K with online head o = online_head + k and value head v = target_head + k:
                                           *     a*    = the FIRST index attaining max_a Q^val_v(s', a); with double_q = 1 the first argmax
                                           *             of Q^sel_{online_head+k}(s', .) (same parameters or target_params exactly as for
                                           *             HL-Gauss heads)
                                           *     p_j   = softmax(l^val_v(s', a*))_j
                                           *     g     = (1 - terminal) * gamma^n
                                           *     Tz_j  = min(max(r + g * z_j, z_0), z_{nb-1})
                                           *     b_j   = (Tz_j - z_0) / eta                              in [0, nb - 1]
                                           *     m_i   = sum_j p_j * max(0, 1 - |b_j - i|)               summed in ascending j
                                           *     l_bk  = logsumexp(l^on_o(s, a_b)) - sum_i m_i * l^on_o(s, a_b)_i
                                           *     losses[k] = (1 / B) sum_b w_b l_bk
                                           *     dL/dl_i   = w_b (softmax(l^on)_i - m_i) / B on the taken action's nb logits of head o, zero on
                                           *             every other output
                                           * m is the usual C51 projection written as a gather: in exact arithmetic it equals the
                                           * floor / floor + 1 scatter form, has no l == u case (an atom landing exactly on a support point
                                           * keeps its mass) and needs no atomics.  No gradient flows through p, a* or any target term.
                                           * q_values = the online expectation; targets = the unclamped scalar r + g * Q^val_v(s', a*);
                                           * priorities = sqrt(mean_k (q - target)^2 + 1e-10) on those scalars, not the cross-entropy;
                                           * loss_weights, losses_accum and priorities_ready behave as without the option.           */
    int32_t n_bins;                       /* 0: scalar Q heads (the reference's network).  2..256: HL-Gauss histogram loss ("Stop
                                           * Regressing", Farebrother et al. 2024; the flags of the reference's
                                           * add_histogram_loss_parameters, parser_argument.py:199-228): the last Dense has
                                           * n_heads * n_actions * n_bins outputs, logit ((h * A) + a) * n_bins + j is bin j of
                                           * action a of head h over the support [hl_min, hl_max] cut into n_bins bins of width
                                           * eta = (hl_max - hl_min) / n_bins with centres c_j = hl_min + (j + 1/2) eta.
                                           * Q_h(s, a) = sum_j softmax(l_{h,a})_j c_j -- what forward / best_action(s) return and argmax.
                                           * learn / loss / grad: target_k = r + (1 - terminal) gamma^n max_a' Q_{tg0+k}(s', a') on
                                           * expectations; y = clamp(target_k, hl_min, hl_max); u_i = erf((hl_min + i eta - y) /
                                           * (sqrt(2) hl_sigma)), p_j = (u_{j+1} - u_j) / (u_nb - u_0); loss = mean_b of
                                           * logsumexp(l) - sum_j p_j l_j on the taken action's bins, dL/dl = (softmax(l) - p) / B.
                                           * q_values / targets are the expectation and the unclamped scalar target; priorities stay
                                           * sqrt(mean_k (q - target)^2 + 1e-10) on those expectations, NOT on the cross-entropy (which
                                           * never falls below the target histogram's entropy, ~1.1 nats at sigma / eta = 0.75, and
                                           * would flatten prioritized replay).  Not with huber_delta > 0 (ISDQN_ERR_ARG) nor with
                                           * batch_norm (ISDQN_ERR_UNSUPPORTED).                                                    */
    int32_t n_quantiles;                  /* (behind n_bins, the other width of a per-action block: the struct still ends in
                                           * hl_sigma, double_q.)  QR-DQN quantile-regression heads (Dabney et al., "Distributional
                                           * Reinforcement Learning with Quantile Regression", AAAI 2018).  n_quantiles = N.  0: off --
                                           * every result, workspace size and region offset keeps the bits it had before the field
                                           * existed.  2..256: on.  Anything else: ISDQN_ERR_ARG; together with n_bins > 0:
                                           * ISDQN_ERR_ARG; with munchausen_tau > 0: ISDQN_ERR_UNSUPPORTED (M-IQN's atom-wise form is a
                                           * follow-up); with batch_norm: ISDQN_ERR_UNSUPPORTED; more than 64 regressed heads or
                                           * n_heads * n_actions * N > 5456: ISDQN_ERR_UNSUPPORTED.  THE definition, with N > 0: the last
                                           * Dense has n_heads * n_actions * N outputs, output ((h * A) + a) * N + i is theta_i of action a
                                           * of head h, the estimate of the quantile at tau_i = (i + 1/2) / N.
                                           * Q_h(s, a) = (1 / N) sum_i theta_i -- what forward / best_action(s) return and argmax with the
                                           * existing tie rule.  For every regressed pair k < K with value head v = target_head + k and
                                           * online head o = online_head + k:
                                           *     a*     = the FIRST index attaining max_a Q^val_v(s', a); with double_q = 1 the first
                                           *              argmax of the selector head Q^sel_{online_head+k}(s', .) (same parameters or
                                           *              target_params exactly as for scalar heads)
                                           *     t_j    = r + ((1 - terminal) * gamma^n) * theta^val_j(s', a*)     (the target atoms, fp32,
                                           *              evaluated in that order, uncontracted)
                                           *     u_ij   = t_j - theta^on_i(s, a_b)
                                           *     l_bk   = sum_i (1 / N) sum_j |tau_i - 1{u_ij < 0}| * h_kappa(u_ij),  kappa = huber_delta
                                           *              kappa > 0: h_kappa(u) = L_kappa(u) / kappa with L_kappa(u) = u^2 / 2 for
                                           *              |u| <= kappa and kappa (|u| - kappa / 2) beyond (Dopamine's form);
                                           *              kappa = 0: h_0(u) = |u|, the plain pinball loss
                                           *     losses[k] = (1 / B) sum_b w_b l_bk
                                           *     dL/dtheta^on_i = -(w_b / (B N)) sum_j |tau_i - 1{u_ij < 0}| * h'_kappa(u_ij), with
                                           *              h'_kappa = clip(u, -kappa, kappa) / kappa, or sign(u) at kappa = 0 (sign(0) = 0);
                                           *              zero on every other output
                                           * No gradient flows through any target atom, even where that head is itself learned in another
                                           * pair.  q_values = the online mean; targets = r + (1 - terminal) gamma^n Q^val_v(s', a*), a
                                           * scalar (the mean of the atoms in exact arithmetic); priorities = sqrt(mean_k (q - target)^2 +
                                           * 1e-10) on those scalars, as for histogram heads; loss_weights, losses_accum and
                                           * priorities_ready behave as without the option.  huber_delta > 0 is allowed here: it is
                                           * kappa (QR-DQN's usual value is 1).  Quantile crossing is not prevented, as in the paper.
                                           * The workspace regions keep the names of the histogram heads ("logits", "logits_target",
                                           * "q_target") and hold quantile values.                                                    */
    float hl_min, hl_max, hl_sigma;      /* n_bins > 0: support [hl_min, hl_max] (hl_max > hl_min) and sigma > 0; ignored at 0 */
    int32_t double_q;                     /* 0: the bootstrap value is max_a' Q(s', a') of the value head (the reference; every result
                                           * keeps the bits it had before the field existed).  1: Double Q-learning (van Hasselt et al.
                                           * 2016).  Anything else: ISDQN_ERR_ARG.  THE definition: for every regressed pair k < K with
                                           * value head v = target_head + k and selector head s = online_head + k (iS-DQN: v = k,
                                           * s = 1 + k; grad_on_batch with n_pairs > 0: the heads the caller names),
                                           *     a*_bk     = the FIRST index attaining max_a Q^sel_s(s'_b, a)
                                           *     target_bk = r_b + (1 - terminal_b) * gamma^n * Q^val_v(s'_b, a*_bk)
                                           * Q^val is the network that supplies the next-state value with double_q = 0: the same
                                           * parameters, or `target_params` in the *_target forms and in grad_on_batch.  Q^sel is always
                                           * the ONLINE parameters applied to the next states (iS-DQN: the head being learned selects, the
                                           * head it is regressed on evaluates, both in the rows of the one forward; DQN: the textbook
                                           * Double DQN, which costs one more forward -- the target parameters over the B next states into
                                           * the workspace region "q_target", then the online parameters over concat(state, next_state)).
                                           * No gradient flows through either.  The tie rule is isdqn_net_best_action's: strict >, the
                                           * lowest index wins.  Everything behind the target is unchanged: q_values, the squared / Huber
                                           * / HL-Gauss loss, loss_weights, dL/dq, the priorities (the raw TD error on these targets),
                                           * losses_accum, priorities_ready.  With n_bins > 0 selector and value are the expectations
                                           * sum_j softmax(l)_j c_j; `targets` stays the unclamped scalar.  Where selector and value are
                                           * the same head of the same rows (a single head without target_params: TF-DQN) Q[argmax Q] ==
                                           * max Q and the result has the bits of double_q = 0.  batch_norm: supported without
                                           * target_params (both heads lie in the rows of the training-mode forward); with target_params
                                           * ISDQN_ERR_UNSUPPORTED (the reference defines no statistics for an online forward of the next
                                           * states alone).  The workspace regions "q_target" ([B][n_heads * A padded to 8]; histogram
                                           * heads: also "logits_target") exist only with double_q = 1, behind every other region.  With
                                           * histogram heads the loss takes the value expectation from "logits_target" itself;
                                           * "q_target" then holds the same expectations for the caller to read (informational).     */
} isdqn_net_config;

/* One parameter tensor inside the flat fp32 parameter buffer.  `name` is the Flax
 * module/leaf ("Conv_0/kernel", "LayerNorm_3/scale", "Dense_1/bias", ...); `flax_shape`
 * is the reference shape; `offset`/`size` locate the tensor in the INTERNAL layout:
 *   conv kernel  -> [out][kh*kw taps][in padded to 8]   (Conv_0: [out][in_plane][kh][kw])
 *   dense kernel -> [out][in]          (in = h*w*(c padded to 8) after the conv torso)
 *   vectors      -> as is
 * The python layer converts between the two (import/export of reference checkpoints). */
typedef struct isdqn_tensor_info {
    char name[48];
    int64_t offset; /* in floats */
    int64_t size;   /* in floats, internal (padded) */
    int32_t kind;   /* 0 conv kernel, 1 dense kernel, 2 bias, 3 ln scale, 4 ln bias; BatchNorm_i: 5 scale, 6 bias ("params"
                     * collection), 7 mean, 8 var ("batch_stats" collection: running averages, not touched by Adam).
                     * BatchNorm tensors: dims = [groups, P, C, C padded to 8]; spatial sites (flax_shape (H, W)) hold one
                     * value per pixel position, feature sites (flax_shape (P*C,)) one per internal column p*Cpad + c */
    int32_t layer;  /* index into the layer list */
    int32_t ndim;
    int32_t flax_shape[4];
    int32_t dims[4]; /* internal dims: conv [out, taps, in_pad, 0] ; dense [out, in_internal, 0, 0] */
} isdqn_tensor_info;

/* Parameter buffer size (floats) and tensor table.  `infos` may be NULL to query the count. */
int isdqn_net_param_layout(const isdqn_net_config* cfg, int64_t* n_param_floats, isdqn_tensor_info* infos,
                           int32_t max_infos, int32_t* n_infos);

/* Workspace bytes needed by forward / learn_on_batch for cfg->batch_size. */
int isdqn_net_workspace_bytes(const isdqn_net_config* cfg, int64_t* bytes);

/* Named workspace regions, so tests can read intermediates (activations, gradients). */
int isdqn_net_workspace_region(const isdqn_net_config* cfg, const char* name, int64_t* offset_bytes,
                               int64_t* size_bytes);

/* A batch of B transitions as the update consumes it (ReplayElement fields,
 * replay_buffer.py:26-34).  cnn: stacks are referenced as single frames. */
typedef struct isdqn_batch {
    int32_t B;
    const uint8_t* frames;    /* cnn: base of the frame store                                  */
    int64_t frame_stride;     /* cnn: bytes between consecutive frame slots (>= h*w)           */
    const int32_t* frame_ids; /* cnn: [B][2*stack] state planes then next_state planes, -1 = 0 */
    const float* state;       /* fc:  [B][obs]                                                 */
    const float* next_state;  /* fc:  [B][obs]                                                 */
    const int32_t* action;    /* [B]                                                           */
    const float* reward;      /* [B]  n-step discounted reward                                 */
    const uint8_t* terminal;  /* [B]                                                           */
    int32_t flags;            /* ISDQN_BATCH_* (0 when in doubt)                               */
    void* priorities_ready;   /* hipEvent_t or NULL: recorded on `stream` once q_values / targets / priorities / losses of
                               * this call are final (long before the call's last kernel), so that a caller's second stream
                               * can write the priorities back (R6) and draw the next batch (S4, R5) under the backward pass */
    const float* loss_weights; /* [B] device floats, finite and >= 0, or NULL (= weight 1 everywhere, same bits as before the
                               * field existed): the importance-sampling weights of isdqn_tree_query_weighted.  With l the
                               * configured per-element loss of d = q - target (squared, Huber, HL-Gauss cross-entropy):
                               * losses[k] = (1 / B) sum_b w_b l_bk, dL/dq_bk = w_b l'(d_bk) / B (HL: dL/dlogit = w_b (softmax - p)
                               * / B); losses_accum accumulates the weighted losses; q_values, targets and priorities stay
                               * unweighted (the priorities are the raw TD error that goes back into the tree).  Honoured by
                               * learn / loss / their _target forms / grad_on_batch */
} isdqn_batch;

/* Per-transition discounts (an annealed update horizon: isdqn_replay_gather_horizon's out_discount, gamma ** m at the step's horizon).
 * isdqn_batch keeps its size and its fields: a caller that has discounts hands every entry point that takes a batch the address of
 * the `batch` member of an isdqn_batch_discount and sets ISDQN_BATCH_DISCOUNT in batch.flags, which tells the library that the
 * discount pointer follows the batch.  Without the flag nothing behind the batch is read and every result keeps its bits.
 * discount: [B] device floats, finite and >= 0 (the caller's contract, as for the weights), or NULL (= no flag).  Otherwise discount[b]
 * stands wherever cfg->gamma_n stands for row b -- the scalar TD target, the head chain, the HL-Gauss, quantile and categorical targets,
 * and the Munchausen and double-Q forms of each -- and cfg->gamma_n is ignored.  Honoured by learn / loss / their _target and debug
 * forms / grad_on_batch / isdqn_noisy_learn_on_batch, every torso. */
typedef struct isdqn_batch_discount {
    isdqn_batch batch;     /* flags carries ISDQN_BATCH_DISCOUNT */
    const float* discount; /* [B] */
} isdqn_batch_discount;

/* The workspace keeps a pre-split (bf16 hi + lo) mirror of the weights that the MFMA stages copy from.  Every entry point
 * rebuilds it from `params` first -- `params` is caller-owned memory -- unless the caller passes this flag, promising that
 * the previous call on this workspace was isdqn_net_learn_on_batch with the same `params` and that nothing has written
 * `params` since (learn_on_batch leaves the mirror current: Adam writes both forms).  The captured multi-step graphs of
 * slimdqn/_graph.py use it for every step of a replay (isdqn_net_refresh_mirror in front of a replay when needed). */
#define ISDQN_BATCH_MIRROR_CURRENT 1
/* The batch is the first member of the struct isdqn_batch_discount above. */
#define ISDQN_BATCH_DISCOUNT 2
/* The batch is the first member of the struct isdqn_batch_decay below (through its isdqn_batch_discount). */
#define ISDQN_BATCH_WEIGHT_DECAY 4

/* AdamW: decoupled weight decay in the learn step's optimizer (optax.adamw(..., weight_decay=wd, mask=kernels),
 * torch.optim.AdamW).  THE definition, per parameter element of a tensor that decays: with p0 the element before the step, p1 what the
 * step without decay leaves (Adam on the same gradient and moments), lr = cfg->learning_rate and wd = weight_decay,
 *
 *     p_new = fl32( p1 - fl32( lr * fl32( wd * p0 ) ) )
 *
 * three roundings, never a fused multiply-add.  Moments, step count, bias corrections, the reduced gradient, losses, q_values, targets
 * and priorities are what they are without decay, bit for bit; the S8 weight mirror is written from p_new.  Up to rounding this is
 * optax.adamw's -lr * (adam_direction + wd * p0) and torch's p *= 1 - lr * wd followed by Adam.  An element of a tensor that does not
 * decay, and every element when weight_decay == 0, takes the instructions of a step without decay and gets its bits (the decay is not
 * folded into the arithmetic: -0 - lr * (+0) and -0 - lr * (-0) differ).  Padding elements and a dueling head's structural zeros are +0
 * and stay +0.
 * decay_kinds: bit k set = tensors of isdqn_tensor_info::kind k decay.  ISDQN_DECAY_KINDS_KERNELS (conv and dense kernels) is the usual
 * mask of the optax and torch recipes, ISDQN_DECAY_KINDS_ALL adds biases and the LayerNorm / BatchNorm scales and biases; the running
 * statistics (kinds 7, 8) are never the optimizer's.
 * As with the discounts, isdqn_batch keeps its size: a caller hands the entry points &x.base.batch and sets ISDQN_BATCH_WEIGHT_DECAY in
 * x.base.batch.flags; base.discount is read only when ISDQN_BATCH_DISCOUNT is set as well.
 * Honoured by isdqn_net_learn_on_batch, its _target form and its debug form, every torso, with and without max_grad_norm.  Ignored by
 * the loss-only and gradient-only entry points, which update nothing.  ISDQN_ERR_ARG, nothing launched: weight_decay negative, NaN or
 * infinite; a decay_kinds bit above 6; decay_kinds == 0 with weight_decay > 0.  isdqn_noisy_learn_on_batch answers
 * ISDQN_ERR_UNSUPPORTED to weight_decay > 0 (its optimizer kernel does not know the tensors' kinds). */
#define ISDQN_DECAY_KINDS_KERNELS 0x03
#define ISDQN_DECAY_KINDS_ALL 0x7f
typedef struct isdqn_batch_decay {
    isdqn_batch_discount base; /* base.batch.flags carries ISDQN_BATCH_WEIGHT_DECAY */
    float weight_decay;        /* finite, >= 0; 0 = every bit as without the flag */
    int32_t decay_kinds;       /* bit k: tensors of kind k decay; bits 0..6 only, at least one */
} isdqn_batch_decay;

/* The batch is the first member of the struct isdqn_batch_conservative below (through its isdqn_batch_decay). */
#define ISDQN_BATCH_CONSERVATIVE 8

/* CQL(H), the conservative term of offline Q-learning (Kumar et al. 2020): alpha * (logsumexp_a Q(s, a) - Q(s, a_b)) beside the
 * configured loss.  THE definition.  It applies to every regressed pair k of a call (the selected pairs of isdqn_net_grad_on_batch
 * included), on online head h = on0 + k of the STATE rows.  The action value Q_a comes from the head-output rows the loss reads (the
 * combined rows of a dueling head):
 *     scalar heads:     Q_a = the output;                                dQ_a/d(output) = 1
 *     quantile heads:   Q_a = mean of the N values;                      dQ_a/d(output) = 1 / N on each of the N
 *     histogram heads:  Q_a = sum_j p_j z_j, p = softmax(logits),
 *                       z_j = v_min + (j + 1/2) eta  (HL-Gauss, C51);    dQ_a/d(logit j) = p_j (z_j - Q_a)
 * Per transition b and pair k, with m = max_a Q_a, fp32, full-accuracy expf / logf, the maximum subtracted first:
 *     c_bk      = m + log(sum_a exp(Q_a - m)) - Q_{a_b}
 *     losses[k] = (1 / B) sum_b w_b (l_bk + alpha c_bk)                   (w_b: loss_weights, l_bk: the configured loss)
 * losses_accum follows losses.  With pi = softmax_a Q, dL/d(output of (h, a')) gains
 *     t = fl32(alpha w_b / B (pi_a' - 1{a' = a_b})) * dQ_a'/d(output),
 * added once in fp32 to what the loss left, dout_new = fl32(dout_old + t); the head-bias gradient is the column sum of the new rows.
 * q_values, targets and priorities are those of the call without the term, bit for bit, and nothing flows through the targets.
 * cql_alpha == 0, or no flag: nothing is launched, read or routed differently, every bit is as without the option.  With
 * cql_alpha > 0 a learn step on scalar heads takes the generic loss and head backward (the head chain knows one action per row).
 * As with the decay, isdqn_batch keeps its size: a caller hands the entry points &x.base.base.batch and sets ISDQN_BATCH_CONSERVATIVE
 * in its flags; base.weight_decay / base.decay_kinds are read only when ISDQN_BATCH_WEIGHT_DECAY is set as well, base.base.discount only
 * with ISDQN_BATCH_DISCOUNT.  Honoured by learn / loss / their _target and debug forms / isdqn_net_grad_on_batch /
 * isdqn_noisy_learn_on_batch, every torso.  ISDQN_ERR_ARG, nothing launched: cql_alpha negative, NaN or infinite.
 * ISDQN_ERR_UNSUPPORTED: more than 64 regressed pairs, or histogram / quantile heads with more than 960 actions. */
typedef struct isdqn_batch_conservative {
    isdqn_batch_decay base; /* base.base.batch.flags carries ISDQN_BATCH_CONSERVATIVE */
    float cql_alpha;        /* finite, >= 0; 0 = every bit as without the flag */
    int32_t reserved;       /* 0 */
} isdqn_batch_conservative;

/* The batch is the first member of the struct isdqn_batch_mixture below (through its isdqn_batch_conservative). */
#define ISDQN_BATCH_MIXTURE 16

/* REM, the random ensemble mixture (Agarwal, Schuurmans, Norouzi, "An Optimistic Perspective on Offline Reinforcement Learning", ICML
 * 2020): a DQN with H = cfg->n_heads scalar heads on one torso, trained on a random convex combination of the heads that is drawn anew
 * for every gradient step.  THE definition.  A = n_actions; head-output rows have the layout q[row][h * A + a].
 *
 * The draw, isdqn_mixture_draw(n_heads, seed, draw_count, alpha, stream): 1 <= n_heads <= 1024 and no NULL pointer, else ISDQN_ERR_ARG
 * and nothing is launched.  With c = *draw_count (device int64, read on the device when the kernel runs), for h < H:
 *     x    = Philox4x32-10(counter = {h, 0x52454D00, lo32(c), hi32(c)}, key = {lo32(seed), hi32(seed)}), its first output word
 *     u_h  = (float)((x >> 8) + 1) * 2^-24          exact, in (0, 1]
 *     s    = the fp32 sum of u_h in ascending h
 *     alpha_h = u_h / s                              an IEEE fp32 division
 * alpha [n_heads] device floats.  The call ends by storing c + 1 the way isdqn_noisy_sample does: one thread, an ordinary store, in a
 * launch of its own behind the reader, so a captured graph advances the draw without a second capture.  alpha depends on (seed, c, h,
 * H) alone; H = 1 gives alpha = {1.0f}.
 *
 * The loss.  A call whose batch carries ISDQN_BATCH_MIXTURE regresses ONE "pair" (the loss count K is 1: losses[1], q_values[B][1],
 * targets[B][1]) in which all H heads take part.  With g_b the row's discount (isdqn_batch_discount, else cfg->gamma_n), w_b its loss
 * weight (isdqn_batch::loss_weights, else 1) and Q^val the value network the call uses without the flag (target_params where given,
 * else the next-state rows of the one forward):
 *     Qmix(x, a)  = sum_h alpha_h * Q_h(x, a)         fp32, in a fixed order, product and add rounded separately
 *     q_b         = Qmix^online(s_b, a_b)
 *     a*          = first argmax_a Qmix^val(s'_b, a)  (strict >, the lowest index wins);
 *                   cfg->double_q = 1: first argmax_a of Qmix^online(s'_b, .) under the same alpha, the value read from Qmix^val at a*
 *     target_b    = r_b + (1 - terminal_b) * g_b * Qmix^val(s'_b, a*)
 *     d_b         = q_b - target_b
 *     losses[0]   = (1 / B) sum_b w_b l(d_b)          l: squared error, or Huber with cfg->huber_delta > 0, as without the flag
 *     dL/dQ_h(s_b, a_b) = fl32( alpha_h * fl32( l'(d_b) * (1 / B) * w_b ) )   for h = 0 .. H - 1, zero elsewhere
 * The fixed order of Qmix: with G = 64 / A (integer division; 1 when A > 64), partial g < G is the sum of fl32(alpha_h * Q_h) over
 * h = g, g + G, ... in ascending h, starting from its first product; Qmix is partial 0 + partial 1 + ... in ascending g.  priorities[b] =
 * sqrt(l(d_b) + 1e-10), unweighted, as without the flag at K = 1; losses_accum follows losses; the head-bias gradient is the
 * column sum of dL/dQ in ascending b.  Nothing flows through the target.  A learn step with the flag takes the generic loss and head
 * backward, never the head chain (as with cql_alpha > 0).  With H = 1 and alpha = {1.0f} the *_target learn call leaves the bits of the
 * same call without the flag: losses, q_values, targets, priorities, parameters, moments.
 * As with the conservative term, isdqn_batch keeps its size: a caller hands the entry points &x.base.base.base.batch and sets
 * ISDQN_BATCH_MIXTURE in its flags; the inner slots (discount, decay, cql_alpha) are read only under their own flags.  Without the flag
 * nothing behind the batch is read and every bit is as before the option existed.  Honoured by learn / loss / their _target and debug
 * forms and by isdqn_net_grad_on_batch with n_pairs <= 0; every torso those run, both precisions, dueling heads (the combined rows have
 * the plain layout), max_grad_norm, weight decay, loss weights and discounts as without the flag.
 * Refusals, nothing launched.  ISDQN_ERR_ARG: alpha NULL, n_mix != cfg->n_heads.  ISDQN_ERR_UNSUPPORTED: n_heads > 1024, n_bins > 0,
 * n_quantiles > 0, munchausen_tau > 0, batch_norm, ISDQN_BATCH_CONSERVATIVE with cql_alpha > 0 (a conservative term on the mixture is a
 * follow-up), isdqn_net_grad_on_batch with n_pairs > 0, isdqn_noisy_learn_on_batch. */
typedef struct isdqn_batch_mixture {
    isdqn_batch_conservative base; /* base.base.base.batch.flags carries ISDQN_BATCH_MIXTURE */
    const float* alpha;            /* [n_mix] device floats: the step's mixture weights (isdqn_mixture_draw) */
    int32_t n_mix;                 /* == cfg->n_heads */
    int32_t reserved;              /* 0 */
} isdqn_batch_mixture;
int isdqn_mixture_draw(int32_t n_heads, uint64_t seed, int64_t* draw_count, float* alpha, void* stream);

/* DQNNet.apply on `n_rows` observations (dqn.py:47-103) -> q [n_rows][n_heads*n_actions].
 * cnn: image j reads frame_ids[j*stack .. j*stack+stack-1]; fc: obs [n_rows][obs_c]. */
int isdqn_net_forward(const isdqn_net_config* cfg, const float* params, const uint8_t* frames, int64_t frame_stride,
                      const int32_t* frame_ids, const float* obs, int32_t n_rows, float* q_out, void* workspace,
                      void* stream);

/* iSDQN.learn_on_batch (isdqn.py:82-109): forward on concat(state, next_state), iterated
 * Bellman targets from heads 0..K-1 of the next states, squared TD loss on heads 1..K,
 * backward, Adam (in place on params / adam_m / adam_v; `adam_count` is a device int32
 * step counter incremented by the call).  Outputs (device): losses[K] = td.mean(axis=0)
 * (isdqn.py:103); optionally losses_accum[K] += losses (the `cumulated_losses += losses` of
 * update_online_params, isdqn.py:62, kept on the device so the step never synchronises),
 * q_values[B][K], targets[B][K] and priorities[B] (float64, sqrt(mean_k td + 1e-10): the
 * TD-error writeback the north star asks for; the reference has no trainer wiring for it --
 * see DESIGN.md). */
int isdqn_net_learn_on_batch(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v,
                             int32_t* adam_count, const isdqn_batch* batch, float* losses, float* losses_accum,
                             float* q_values, float* targets, double* priorities, void* workspace, void* stream);

/* Loss only, no update: iSDQN.loss_on_batch (isdqn.py:92-103). */
int isdqn_net_loss_on_batch(const isdqn_net_config* cfg, const float* params, const isdqn_batch* batch, float* losses,
                            float* q_values, float* targets, void* workspace, void* stream);

/* DQN.learn_on_batch / DQN.loss_on_batch (slimdqn/networks/dqn.py:59-83): the baselines on the same kernels.
 * cfg->n_heads == 1 (one head of n_actions outputs; K = 1): head 0 of the states is regressed on
 * r + (1 - terminal) * gamma^n * max_a head 0 of the next states.
 *   - isdqn_net_learn_on_batch / isdqn_net_loss_on_batch with n_heads == 1 is TF-DQN (tfdqn.py:55-80: the next
 *     states go through the SAME parameters, stop-gradient target);
 *   - the *_target forms take the next states through `target_params` (DQN: a copy refreshed every
 *     target_update_frequency steps by the caller, dqn.py:49-50).  losses[1] is the batch mean (dqn.py:69-70). */
int isdqn_net_learn_on_batch_target(const isdqn_net_config* cfg, float* params, const float* target_params, float* adam_m,
                                    float* adam_v, int32_t* adam_count, const isdqn_batch* batch, float* losses,
                                    float* losses_accum, float* q_values, float* targets, double* priorities,
                                    void* workspace, void* stream);
int isdqn_net_loss_on_batch_target(const isdqn_net_config* cfg, const float* params, const float* target_params,
                                   const isdqn_batch* batch, float* losses, float* q_values, float* targets,
                                   void* workspace, void* stream);

/* Rebuild the workspace's weight mirror from `params` now (what every entry point does at its head unless the caller passes
 * ISDQN_BATCH_MIRROR_CURRENT).  For callers that replay a captured graph whose steps all trust the mirror: one eager launch in front
 * of the replay when something wrote the parameters in between (slimdqn/_graph.py), instead of a second capture. */
int isdqn_net_refresh_mirror(const isdqn_net_config* cfg, const float* params, void* workspace, void* stream);

/* BatchNorm networks: params["batch_stats"] <- the batch_stats collection returned by the LAST training-mode forward that ran
 * in `workspace` (learn / loss / grad_on_batch; flax: apply(..., mutable=["batch_stats"])), i.e. running = 0.99 * running +
 * 0.01 * (that forward's batch statistics).  learn_on_batch does this itself for its own forward (isdqn.py:87-88); the analysis
 * agents store the collection of ANOTHER forward -- the evaluation batch's, analysisdqn.py:121-131, analysistfdqn.py:85-95 -- and
 * call this behind that loss pass.  ISDQN_ERR_ARG for a configuration without batch_norm. */
int isdqn_net_bn_commit_running(const isdqn_net_config* cfg, float* params, const void* workspace, void* stream);

/* Gradient of a TD loss, no update: the three gradients AnalysisDQN compares (slimdqn/networks/analysisdqn.py:156-219 --
 * jax.grad of compute_loss_is / compute_loss_tf / compute_loss_tb).  `grad_out` receives the gradient w.r.t. every parameter
 * in the internal layout of isdqn_net_param_layout (n_param_floats floats); parameters and optimizer state are untouched.
 *   n_pairs <= 0 : the configuration's own loss (iS-DQN: online head 1+k on target head k of the same parameters);
 *   n_pairs  > 0 : online heads online_head + k regressed on target heads target_head + k, k < n_pairs
 *                  (analysisdqn.py:162-176: head 1 on head 1);
 *   target_params != NULL : the next states go through `target_params` (compute_loss_tb).
 * losses[n_pairs or K], q_values / targets [B][n_pairs or K] (may be NULL). */
int isdqn_net_grad_on_batch(const isdqn_net_config* cfg, const float* params, const float* target_params,
                            const isdqn_batch* batch, int32_t online_head, int32_t target_head, int32_t n_pairs, float* grad_out,
                            float* losses, float* q_values, float* targets, void* workspace, void* stream);

/* iSDQN.shift_params (isdqn.py:111-125): head k <- head k+1 on the last Dense; moments untouched. */
int isdqn_net_shift_params(const isdqn_net_config* cfg, float* params, void* stream);

/* iSDQN.best_action (isdqn.py:127-135): forward one observation, argmax of head 1+idx_network. */
int isdqn_net_best_action(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                          int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t idx_network,
                          int32_t* out_action, void* workspace, void* stream);

/* best_action for `n_rows` observations at once (vectorised host environments: one forward, one argmax launch):
 * out_actions[i] = argmax_a of online head idx_networks[i] (device int32 arrays) of observation i.  n_rows <= 2 * batch_size.
 * flags: ISDQN_BATCH_MIRROR_CURRENT when the caller knows the workspace's weight mirror matches `params`;
 * ISDQN_ACT_MEAN_HEADS: out_actions[i] = first argmax_a of sum_h Q_h(row i, a) over all n_heads heads, the sum in fp32 in ascending h,
 * read from the "q" rows (REM's evaluation policy is the head average, and the sum has its argmax); idx_networks is ignored and may
 * be NULL. */
#define ISDQN_ACT_MEAN_HEADS 32
int isdqn_net_best_actions(const isdqn_net_config* cfg, const float* params, const uint8_t* frames, int64_t frame_stride,
                           const int32_t* frame_ids, const float* obs, int32_t n_rows, const int32_t* idx_networks,
                           int32_t* out_actions, int32_t flags, void* workspace, void* stream);

/* AnalysisNet.apply (slimdqn/utils/analysis_architecture.py:9-122) as eval_srank_and_dead_neurons uses it
 * (experiments/base/srank_and_dead_neurons.py:8-22): the network without its last layer on `n_rows` observations
 * (<= 2 * batch_size).  features_out [n_rows][width of the last hidden layer] = its post-ReLU activations (behind the last
 * BatchNorm when the network has them, as the reference returns them); scores_out = for every recorded layer in the reference's
 * order, the sum over the rows of its post-ReLU activations in the reference's feature order ((H, W, C) flattened for conv
 * layers) -- cnn: the three conv layers, impala: the two ReLU outputs of each residual block of each Stack and the flattened
 * torso output, then the hidden Dense layers; sizes from isdqn_net_analysis_layout (at most 32 entries).  BatchNorm networks
 * run on the batch statistics of these rows (the reference applies AnalysisNet with mutable batch_stats).  The srank (an SVD)
 * and the dead-neuron fraction are host arithmetic on these two arrays, as in the reference (utils/analysis.py:4-17). */
int isdqn_net_analysis_layout(const isdqn_net_config* cfg, int32_t* n_hidden, int64_t* sizes, int32_t max_sizes);
int isdqn_net_analysis(const isdqn_net_config* cfg, const float* params, const uint8_t* frames, int64_t frame_stride,
                       const int32_t* frame_ids, const float* obs, int32_t n_rows, float* features_out, float* scores_out,
                       void* workspace, void* stream);

/* ReDo: recycle dormant neurons (Sokar, Agarwal, Castro, Evci 2023, "The Dormant Neuron Phenomenon in Deep Reinforcement
 * Learning"; the reference has no counterpart -- it only measures them, utils/analysis.py:12-17).  On the device, in place,
 * stream-ordered, without a host synchronisation.
 * Recyclable layers: the hidden layers of the cnn and fc architectures in network order (every layer but the last Dense).  A
 * neuron of a conv layer is an output channel (n_neurons = cout, not npix * cout), of a Dense layer an output feature; the layout
 * call returns their number and widths (n_neurons may be NULL; at most max_layers entries are written).  scores_out / mask_out
 * hold sum(n_neurons) entries, the layers concatenated; n_recycled_out holds n_layers entries.
 * Score: the weight mirror is rebuilt and the network runs without its last layer on `n_rows` observations (1 <= n_rows <=
 * 2 * batch_size, inputs as in the forward call).  a_c = sum over rows and pixel positions of the post-ReLU activation of
 * neuron c, divided by n_rows * positions (fp32; fixed order: rows per position first, then positions in ascending order; no
 * atomics) -> scores_out.  mean_l = the fp32 mean of a over the layer in ascending c.  Neuron c of layer l is dormant iff
 * a_c <= tau * mean_l (a layer that is zero everywhere is dormant everywhere) -> mask_out (0 / 1), the count per layer ->
 * n_recycled_out.
 * Recycle, for every dormant neuron c of layer l, in the internal layout of the parameter layout call:
 *   - incoming: row c of layer l's kernel (the first convolution's [out][plane][ky][kx] form and padded input lanes included)
 *     and bias c are copied from the same offsets of `fresh_params` (a parameter buffer of the same layout, e.g. a new
 *     initialisation); with layer_norm also scale c and bias c of the LayerNorm behind layer l;
 *   - outgoing: every weight of layer l + 1 that reads neuron c is set to 0 -- [out][tap][c] for a convolution, columns
 *     p * c_pad + c for every position p of the first Dense behind the torso, column c of a Dense behind a Dense and of the last
 *     Dense (every head, action, bin or quantile) -- in every row, the padded ones too.  The outgoing zeros are written after
 *     the incoming copies: a weight from a dormant neuron into a dormant neuron ends up 0;
 *   - adam_m / adam_v (both NULL or both given) are set to 0 at every position written above.  The Adam step count is not an
 *     argument and is not touched.
 * Everything else -- other parameters, moments, padding lanes -- keeps its bits.  The call ends by rebuilding the weight mirror
 * from `params`: the mirror is current when it returns.  Without layer_norm and with tau = 0 the network's function on the
 * scored rows is unchanged (a dormant neuron's activations were exactly 0 and nothing reads it afterwards); with layer_norm
 * the recycled neuron changes the statistics of its layer's other channels.
 * ISDQN_ERR_UNSUPPORTED: arch impala (the residual adds make "outgoing" ambiguous), batch_norm (per-position statistics sit
 * between the layers).  ISDQN_ERR_ARG: a NULL params / fresh_params / scores_out / mask_out / n_recycled_out / workspace,
 * exactly one of adam_m / adam_v NULL, tau negative or not finite.  ISDQN_ERR_SHAPE: n_rows out of range. */
int isdqn_net_redo_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* n_neurons, int32_t max_layers);
int isdqn_net_redo(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, const float* fresh_params,
                   const uint8_t* frames, int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                   float tau, float* scores_out, int32_t* mask_out, int32_t* n_recycled_out, void* workspace, void* stream);

/* NoisyNet exploration: factorised noisy Dense layers (Fortunato et al., "Noisy Networks for Exploration", ICLR 2018; the reference has
 * no counterpart -- it explores with the epsilon schedule).  Built BESIDE the plan: no field of isdqn_net_config, no workspace region and no
 * launch of any existing entry point belongs to it; the caller owns the new buffers, and forward / loss / gradient run unchanged on a
 * composed "effective" parameter buffer.  On the device, stream-ordered, without a host synchronisation and without atomics.  The cost
 * of the extra passes over the parameters (one compose, one write and one read of the reduced gradient, one optimizer pass) is recorded
 * in docs/NOTEBOOK.md, not here.  THE definition:
 * Noisy layers: every Dense layer of the network, the hidden ones and the head (Fortunato's and Rainbow's choice).  Convolutions, LayerNorm
 * scale and bias are not noisy.
 * Buffers (device, caller-owned; "same layout" = isdqn_net_param_layout's, n_param_floats floats):
 *   mu       the ordinary parameter buffer;
 *   sigma    same layout.  Only the positions of Dense kernels and Dense biases mean anything; every other position is +0.0f and stays
 *            +0.0f, so that isdqn_net_shift_params and the tensor table work on sigma as they do on mu;
 *   m_sigma, v_sigma   Adam moments of sigma, same layout;     eff   the composed parameters, same layout;
 *   grad     n_param_floats floats: the reduced gradient of the step (the caller zeroes it once);
 *   noise    for noisy layer l in network order ein_l[in_p] then eout_l[out_p] -- the plan's internal widths, both multiples of 8 -- already
 *            transformed by f, the layers concatenated; isdqn_noisy_layout returns offsets[l] (of ein_l; eout_l follows at + in_widths[l]),
 *            the widths and the total.  ein is indexed by the INTERNAL input column (behind a conv torso: pixel * c_pad + channel);
 *   noise_count   one device int64.
 * Noise: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; round: (hi0, lo0) = M0 * c0,
 * (hi1, lo1) = M1 * c2, c <- {hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0}, then the key is bumped).  Element j of vector v (0 = in, 1 = out) of
 * noisy layer l: x = Philox(ctr = {j, (stream_id << 16) | (2 l + v), lo32(count), hi32(count)}, key = {lo32(seed), hi32(seed)}), count the
 * value of *noise_count when the kernel runs, stream_id 0 = online, 1 = target.  u1 = ((x0 >> 8) + 1/2) 2^-24 in (0, 1), u2 = (x1 >> 8) 2^-24;
 * z = sqrtf(-2 ln u1) * cospif(2 u2) with the full-precision device functions; the stored value is f(z) = copysignf(sqrtf(fabsf(z)), z).
 * u2 is exact in fp32; u1 has 25 significant bits from 1/2 on, so there ln u1 is evaluated as log1pf(-(1 - u1)), whose argument is exact
 * (below 1/2: logf(u1), exact argument).  A value depends on (seed, count, stream_id, l, v, j) alone, never on another layer's width.
 * isdqn_noisy_sample is one launch over all vectors and ends by storing count + 1: one thread, an ordinary store, in a launch of its
 * own behind the one that read the counter -- a captured graph advances the noise without a second capture.
 * Compose (isdqn_noisy_compose: one pass over the parameters), in fp32, in this order, uncontracted:
 *   Dense kernel element [o][i] at w_off + o * in_p + i:   n = eout[o] * ein[i],  t = sigma * n,  eff = mu + t
 *   Dense bias [o]:                                        eff = mu + sigma_b[o] * eout[o]
 *   every other element:                                   eff = mu, bit for bit
 * With `noise` all zero eff == mu bit for bit wherever sigma is finite: the evaluation network, selected by zeroing the noise buffer.
 * With a workspace the call also writes the weight mirror of eff, so that a following call on eff may pass ISDQN_BATCH_MIRROR_CURRENT
 * (acting: sample, compose with the workspace, isdqn_net_best_actions(..., eff, ..., ISDQN_BATCH_MIRROR_CURRENT, ...)).  NULL: eff alone.
 * Learn step (isdqn_noisy_learn_on_batch): compose eff and its mirror; the full gradient pass of isdqn_net_grad_on_batch on eff (n_pairs
 * = 0; eff_target != NULL: the DQN form, a second composed buffer the caller built from the target's mu, sigma and a stream_id = 1 draw)
 * -> grad = g, the reduced gradient w.r.t. eff exactly as a plain network holding eff would have fed it to Adam, masked under dueling as
 * grad_on_batch masks it; then one optimizer pass:
 *     g_mu = g;    g_sigma = fl32(g * n) on Dense kernels (n as in compose),  fl32(g * eout[o]) on Dense biases;  none elsewhere
 * Adam (the element update of learn_on_batch, the same learning_rate / adam_b1 / adam_b2 / adam_eps and the ONE shared adam_count,
 * incremented once) updates mu from g_mu everywhere and sigma from g_sigma on the Dense positions.  One draw serves both halves of the
 * concat(state, next_state) forward: iS-DQN and TF-DQN run one forward on one set of parameters -- a deviation from Fortunato's DQN,
 * which draws separate noise for the target forward (the *_target form does).  losses, losses_accum, q_values, targets, priorities,
 * priorities_ready, loss_weights and every target / loss option of cfg behave exactly as in isdqn_net_learn_on_batch on the composed
 * network.  Padding lanes and the structural zeros of a dueling head carry g = 0: their sigma stays +0.0f when it starts there.  The
 * weight mirror is NOT current for mu afterwards (every noisy call composes first).
 * ISDQN_ERR_UNSUPPORTED from all four entry points, behind the plan's own checks and in this order: batch_norm (running statistics
 * would be committed into eff), arch impala, max_grad_norm > 0 (the norm must cover g_sigma too: a follow-up).  ISDQN_ERR_ARG: a NULL
 * pointer other than workspace (compose) / eff_target / the optional outputs of learn_on_batch; stream_id outside {0, 1}.
 * isdqn_noisy_layout: host arithmetic on the plan.  *n_layers and *n_noise_floats are always written; offsets / in_widths / out_widths may
 * all be NULL (a query of the count and the total), otherwise max_layers must be at least *n_layers -- a smaller one is ISDQN_ERR_ARG,
 * nothing is truncated silently.  It refuses what the other three refuse, max_grad_norm > 0 included: a layout is handed out only for a
 * configuration the noisy step runs. */
int isdqn_noisy_layout(const isdqn_net_config* cfg, int32_t* n_layers, int64_t* offsets, int32_t* in_widths, int32_t* out_widths,
                       int32_t max_layers, int64_t* n_noise_floats);
int isdqn_noisy_sample(const isdqn_net_config* cfg, uint64_t seed, int32_t stream_id, int64_t* noise_count, float* noise, void* stream);
int isdqn_noisy_compose(const isdqn_net_config* cfg, const float* mu, const float* sigma, const float* noise, float* eff, void* workspace,
                        void* stream);
int isdqn_noisy_learn_on_batch(const isdqn_net_config* cfg, float* mu, float* sigma, float* m_mu, float* v_mu, float* m_sigma,
                               float* v_sigma, int32_t* adam_count, const float* noise, float* eff, const float* eff_target, float* grad,
                               const isdqn_batch* batch, float* losses, float* losses_accum, float* q_values, float* targets,
                               double* priorities, void* workspace, void* stream);

/* Periodic resets: re-initialise the top layers, shrink the rest towards a fresh initialisation, clear the optimizer state of what was
 * touched (Nikishin et al. 2022, "The Primacy Bias in Deep RL"; shrink and perturb: Ash & Adams 2020; D'Oro et al. 2023, SR-SPR; Schwarzer
 * et al. 2023, BBF).  The reference has no counterpart.  Built BESIDE the plan, like the noisy layers: no field of isdqn_net_config, no
 * workspace region, no launch of any existing entry point.  On the device, in place, stream-ordered, capturable, without a host
 * synchronisation, an allocation or an atomic.  Every configuration the plan accepts is accepted (cnn, impala, fc, layer_norm,
 * batch_norm, every head): there is no ISDQN_ERR_UNSUPPORTED of its own.  THE definition:
 * isdqn_net_reset_layout (host arithmetic on the plan, no GPU): *n_layers = the length of the layer list that isdqn_tensor_info::layer
 * indexes (the impala torso is ONE entry of it); *first_dense_layer = the index of the first Dense layer (0 for fc).  Either may be NULL.
 * isdqn_net_reset acts on every tensor isdqn_net_param_layout lists -- all kinds 0..8: kernels, biases, the LayerNorm tensors, the
 * BatchNorm "params" tensors and the running mean / var -- over each tensor's whole internal (padded) size.  Floats of the buffer that
 * belong to no tensor keep their bits.
 *   Class: a tensor is UPPER iff info.layer >= split_layer, else LOWER (the BatchNorm sites in front of and inside the impala torso
 *   carry negative layer numbers: always lower).  split_layer = 0: everything is upper; split_layer = n_layers: nothing is.
 *   Each class has a factor pair (s, q) = (shrink, perturb).  With p the parameter and f the value at the same offset of fresh_params (a
 *   buffer of the same layout, e.g. a new initialisation), fl32 the rounding to fp32:
 *     s == 1 && q == 0   the class is not touched: parameters AND moments keep their bits, nothing is read or written;
 *     s == 0             p' = fl32(q * f).  p is NOT read: a NaN or Inf parameter is replaced;
 *     otherwise          p' = fl32(fl32(s * p) + fl32(q * f)) -- two products and one sum, each rounded on its own, never contracted
 *                        into an FMA (a numpy float32 restatement gives the same bits).
 *   In the two writing cases adam_m and adam_v (both NULL or both given) are set to +0.0f over the same elements.
 *   With non-negative factors a position that is +0.0f in both params and fresh_params stays +0.0f: padding lanes and the structural
 *   zeros of a dueling head survive a reset.
 *   adam_count != NULL: *adam_count = 0, by an ordinary store in a launch of its own behind the element pass -- the next learn step runs
 *   with the bias corrections of step 1.  NULL leaves the count alone.
 *   workspace != NULL: the call ends by rebuilding the weight mirror from params (as isdqn_net_redo does): the mirror is current when
 *   it returns.  NULL is for buffers that are no engine's `params`: a target copy, a noisy engine's sigma (fresh: the initial sigma).
 *   Launches: one element launch over all written tensors through a table passed by value (at most 64 tensors per launch: the impala +
 *   batch_norm table is split), 16 bytes per lane where the buffers are 16-byte aligned and the tensor's offset and size are multiples
 *   of 4 floats, one element per lane otherwise; the grid is capped at 2048 workgroups and strides.
 *   ISDQN_ERR_ARG, nothing launched: NULL params / fresh_params; exactly one of adam_m / adam_v NULL; a factor that is negative or not
 *   finite; split_layer < 0 or > n_layers; fresh_params overlapping params (any byte of the two n_param_floats ranges).
 * EMA (Polyak) target: isdqn_net_ema covers all n_param_floats elements of two buffers of the parameter layout (parameters, or a noisy
 * engine's sigma buffers):    t' = fl32(fl32(omt * t) + fl32(tau * p)),   omt = fl32(1.0f - tau) computed once on the host
 * (optax.incremental_update), the three operations rounded separately, never contracted.  tau == 0 launches nothing; tau == 1 copies
 * the bits of `online` (a device-to-device copy: the sign of a zero and a non-finite target do not matter).  Plain loads and stores: the
 * next step reads both buffers again.  16 bytes per lane when both pointers are 16-byte aligned, one element per lane otherwise.
 * ISDQN_ERR_ARG: a NULL pointer, tau outside [0, 1] or NaN, target == online. */
int isdqn_net_reset_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* first_dense_layer);
int isdqn_net_reset(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, int32_t* adam_count,
                    const float* fresh_params, int32_t split_layer, float shrink_lower, float perturb_lower, float shrink_upper,
                    float perturb_upper, void* workspace, void* stream);
int isdqn_net_ema(const isdqn_net_config* cfg, float* target, const float* online, float tau, void* stream);

/* Soft head shift: iS-DQN's target is head 0 of the online parameters, so it has no target buffer an EMA could act on; the soft form of
 * iSDQN.shift_params moves every head towards its upper neighbour inside the parameter buffer, once per gradient step (K = 1: DQN's
 * Polyak target on a shared torso; larger K slides the whole window of heads continuously at rate tau per step).  The reference has no
 * counterpart.  Built BESIDE the plan, like the resets: no field of isdqn_net_config, no workspace region, no launch of any existing entry
 * point.  On the device, in place, stream-ordered, capturable, without a host synchronisation, an allocation or an atomic.  THE definition:
 * The last Dense holds n_heads = 1 + K head blocks of R rows each, R = (n_actions + dueling) * max(n_bins, n_quantiles, 1) -- the block
 * isdqn_net_shift_params moves.  For every head k = 0 .. K-1, every row of the block and every one of the in_p weight columns (the padded
 * ones too), and for the block's R biases:
 *     new[k] = fl32( fl32(omt * old[k]) + fl32(tau * old[k+1]) ),   omt = fl32(1.0f - tau) computed once on the host,
 * the two products and the sum rounded separately, never contracted into an FMA (isdqn_net_ema's arithmetic; a numpy float32 restatement
 * gives the same bits).  Every head reads the value its upper neighbour had BEFORE the call.  Head K, the padding rows behind the last
 * head, every other tensor, both Adam moments and the step count are neither arguments nor touched: they keep their bits.
 *   tau == 0 launches nothing.  tau == 1 is isdqn_net_shift_params (the call is routed there: a NaN and the sign of a zero behave as in
 *   the hard shift), followed by a rebuild of the mirror when a workspace is given.
 *   workspace == NULL: the fp32 master alone (a noisy engine's sigma, a copy).  With a workspace the same launch also stores the S8 weight
 *   mirror (region "wsplit", same offsets as the master) of every element it wrote, weights and biases, with the bits
 *   isdqn_net_refresh_mirror would produce from the new master: a mirror that was current before the call is current after it, so the
 *   steps of a captured update that run with ISDQN_BATCH_MIRROR_CURRENT stay one node longer on the same stream.
 *   One launch: a lane owns a row of the block and four consecutive columns (16 bytes) and walks the heads upward with old[k+1] kept in
 *   registers; every element of heads 0 .. K is loaded once and every element of heads 0 .. K-1 stored once; the grid is sized by
 *   positions, capped at 2048 workgroups, and strides.
 * ISDQN_ERR_ARG, nothing launched: NULL params; tau outside [0, 1] or NaN; n_heads < 2; params not 16-byte aligned (the lanes are 16
 * bytes wide: there is no scalar path, a view at an odd offset is refused). */
int isdqn_net_soft_shift(const isdqn_net_config* cfg, float* params, float tau, void* workspace, void* stream);

/* Gradual magnitude pruning (Zhu & Gupta 2017; Graesser et al. 2022; Obando-Ceron et al. 2024; the behaviour of JaxPruner's GMP): a bit
 * mask over the parameter buffer, chosen per tensor by magnitude and applied after every optimizer update; gradients and Adam moments stay
 * dense.  The reference has no counterpart.  Built BESIDE the plan, like the resets and the soft shift: no field of isdqn_net_config, no
 * workspace region, no launch of any existing entry point.  On the device, stream-ordered, capturable, without a host synchronisation or
 * an allocation; integer atomics only (sums of counts and disjoint bits of a word: the same result in every order).  THE definition:
 * Prunable tensors: every conv kernel and every Dense kernel (isdqn_tensor_info kinds 0 and 1) except the LAST Dense, in layout order (the
 *   head blocks of the last Dense are moved by isdqn_net_shift_params / isdqn_net_soft_shift, which a per-element mask would not survive).
 *   Only REAL elements count: out < the Flax output width, and the input lane inside its group of `in padded to 8` below the true input
 *   width (conv: in < cin of every tap; the first Dense behind a conv torso: c < cout of every pixel; any other Dense: in < in_f; Conv_0's
 *   [out][plane][ky][kx] form has no padded input lane).  Padding is never counted, never selected and never written.
 * Mask: one bit per float of the parameter buffer, bit (i & 31) of uint32 word (i >> 5), set = kept; mask_words = ceil(n_param_floats /
 *   32).  The caller initialises it to all ones.  The update rewrites the bits of real prunable elements and no other bit.
 * Selection of tensor i with n_i real elements and n_pruned[i] = k_i: the key of an element is 0 if its mask bit says pruned, otherwise
 *   1 + (bits of w & 0x7fffffff): float order on |w|, -0.0 as 0.0, denormals not flushed, NaN above inf.  The k_i elements with the smallest
 *   (key, flat internal index) are pruned (bit cleared), every other real element is kept (bit set): ties go to the lower index, masks are
 *   nested while k_i does not decrease, and the result is a pure function of (params, old mask, k).
 * Apply: wherever a bit is clear inside [offset of the first prunable tensor, end of the last one), the master element becomes +0.0f and,
 *   with a workspace, so does its half-group entry of the S8 weight mirror (region "wsplit": the bits isdqn_net_refresh_mirror would make
 *   of the new master).  Nothing is loaded from the parameters; every other element, lane and moment keeps its bits.  A mirror that was
 *   current before the call is current after it.
 * isdqn_net_prune_layout (host arithmetic on the plan, no GPU): *n_tensors = the number of prunable tensors; infos (may be NULL to query)
 *   receives for each of the first max_infos four int64: {index into isdqn_net_param_layout's table, offset, internal size, n_i};
 *   *mask_words as above; *scratch_bytes = what isdqn_net_prune_update needs (per tensor four histograms of 256 uint32 and one uint32 per
 *   chunk of 4096 floats; contents between calls do not matter).  Any output pointer may be NULL.
 * isdqn_net_prune_update: clears the scratch, six launches of the radix select over all tensors (four digit histograms of 8 bits, the
 *   tie counts, the mask bits), then the apply launch: mask, master and (with a workspace) mirror are final when it returns.
 * isdqn_net_prune_apply: the apply launch alone -- the node behind every gradient step; one lane per 16-byte position, grid capped at 2048
 *   workgroups, striding.
 * ISDQN_ERR_UNSUPPORTED, nothing launched: the impala torso and batch_norm.  ISDQN_ERR_ARG, nothing launched: a NULL cfg / params / mask /
 *   n_pruned / scratch; params not 16-byte aligned, mask or scratch not 4-byte aligned; a k_i outside [0, n_i]. */
int isdqn_net_prune_layout(const isdqn_net_config* cfg, int32_t* n_tensors, int64_t* infos, int32_t max_infos, int64_t* mask_words,
                           int64_t* scratch_bytes);
int isdqn_net_prune_update(const isdqn_net_config* cfg, float* params, const int32_t* n_pruned, uint32_t* mask, void* scratch,
                           void* workspace, void* stream);
int isdqn_net_prune_apply(const isdqn_net_config* cfg, float* params, const uint32_t* mask, void* workspace, void* stream);

/* Normalize-and-Project (NaP: Lyle, Zheng, Khetarpal, Martens, van Hasselt, Pascanu, Dabney, "Normalization and effective learning rates
 * in reinforcement learning", NeurIPS 2024): with a normalisation layer in front of every nonlinearity the function does not depend on
 * the scale of a weight matrix, the parameter norm grows freely under Adam and the effective learning rate decays as 1 / |W|^2; after
 * every optimizer update each layer's weights are therefore projected back to the norm they had at initialisation.  The reference has no
 * counterpart.  Built BESIDE the plan, like pruning: no field of isdqn_net_config, no workspace region, no launch of any existing entry
 * point.  On the device, stream-ordered, capturable, without a host synchronisation, an allocation or an atomic of any kind.  THE
 * definition:
 * Projected tensors: exactly the prunable tensors of isdqn_net_prune_layout -- every conv kernel and every Dense kernel (kinds 0 and 1)
 *   except the LAST Dense (no normalisation follows it: its scale is the scale of Q), in layout order.  Only REAL elements (the predicate
 *   of pruning, above) count and only real elements are written: padding rows and lanes keep their bits.  Biases, LayerNorm scales and
 *   biases, both Adam moments, the step count and every other tensor are neither read nor written.
 * Arithmetic: tensor i has real elements w_j (fp32) and a target norm rho_i = target_norms[i] (float64, device memory).
 *   S_i = sum_j (double)w_j * (double)w_j: the squares are exact in float64, the additions are float64 in an order that is the
 *   implementation's own but FIXED -- the same bits on every run, eager and captured, and in every workgroup that needs the sum.
 *   n_i = sqrt(S_i) in float64; s_i = (float)(rho_i / n_i): IEEE sqrt and division in float64, one rounding to fp32.
 *   If S_i is 0, inf or NaN, or rho_i is not finite or <= 0: s_i = 1.0f and nothing of the tensor is written.
 *   Otherwise every real element becomes fl32(w_j * s_i), one fp32 multiply (denormals are not flushed), and, with a workspace, its entry
 *   of the S8 weight mirror (region "wsplit") gets the bits isdqn_net_refresh_mirror would make of the new master: a mirror that was
 *   current before the call is current after it.  (Where s_i rounds to 1.0f the stores may be skipped: they would change no bit.)
 *   norms[i] = n_i (double), measured BEFORE the projection; scales[i] = s_i (float).
 * isdqn_net_project_layout (host arithmetic on the plan, no GPU): *n_tensors = the number of projected tensors; infos (may be NULL to
 *   query) receives for each of the first max_infos the four int64 of isdqn_net_prune_layout: {index into isdqn_net_param_layout's table,
 *   offset, internal size, real element count}; *scratch_bytes = what the two calls below need (one double per chunk of 4096 floats of
 *   every tensor; contents between calls do not matter).  Any output pointer may be NULL.
 * isdqn_net_project_norms: measures only -- norms[i] of `params`, in the bits isdqn_net_project_apply would report for the same buffer.
 *   Two launches: the chunk sums, then one workgroup per tensor.
 * isdqn_net_project_apply: the node behind every gradient step.  Two launches over one workgroup per chunk: the chunk sums into the
 *   scratch; then every workgroup adds up its tensor's chunk sums in one fixed order (so all of them derive the same s_i bit for bit),
 *   the tensor's first workgroup stores norms[i] and scales[i], and all of them scale their chunk.  workspace == NULL: the master alone.
 * ISDQN_ERR_UNSUPPORTED, nothing launched: the impala torso and batch_norm, as with pruning.  ISDQN_ERR_ARG, nothing launched: a NULL cfg /
 *   params / target_norms / norms / scales / scratch; params not 16-byte aligned; target_norms, norms or scratch not 8-byte aligned;
 *   scales not 4-byte aligned. */
int isdqn_net_project_layout(const isdqn_net_config* cfg, int32_t* n_tensors, int64_t* infos, int32_t max_infos, int64_t* scratch_bytes);
int isdqn_net_project_norms(const isdqn_net_config* cfg, const float* params, double* norms, void* scratch, void* stream);
int isdqn_net_project_apply(const isdqn_net_config* cfg, float* params, const double* target_norms, double* norms, float* scales,
                            void* scratch, void* workspace, void* stream);

/* Engine self-test: C[M][N] = A . B on the MFMA tile engine for every operand-layout
 * combination (a_tr/b_tr: 0 = operand stored [rows][K], 1 = stored [K][rows]).  Test hook. */
int isdqn_selftest_gemm(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int32_t a_tr,
                        int32_t b_tr, int32_t precision, int32_t split_k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISDQN_HIP_H */
