// Gradual magnitude pruning: what net_kernels.hip hands to the launchers of prune_kernels.hip, a translation unit of its own (its
// kernels are in no code object tests/golden/kernel_order.txt pins).  THE definition: include/isdqn_hip.h, isdqn_net_prune_layout /
// isdqn_net_prune_update / isdqn_net_prune_apply.  No kernel in this header.
#pragma once

#include "common.h"

namespace isdqn {

constexpr int PRUNE_MAX_TENSORS = 12;  // MAX_LAYERS of net_plan.h: at most one kernel per layer of a cnn / fc plan
constexpr int PRUNE_CHUNK = 4096;      // floats of the parameter buffer one workgroup of the selection walks: 128 whole mask words
constexpr int PRUNE_HIST_WORDS = 4 * 256;  // one histogram of 256 bins per 8-bit digit of the 32-bit key, most significant first

// One prunable tensor.  Element e < size of the internal form is REAL iff  e / row_len < rows_real  and  (e % row_len) % period < real_per
// (the padded rows behind the last output, the padded input lanes of every tap / pixel / row are not).
struct PruneTensor {
    int64_t offset;       // floats, a multiple of 8
    int32_t size;         // internal floats, a multiple of 8 (every index space of a plan is < 2^31)
    int32_t row_len, rows_real, period, real_per;
    int32_t n_real;       // rows_real * (row_len / period) * real_per
    int32_t k;            // elements to prune, 0 <= k <= n_real (the update alone reads it)
    int32_t first_chunk, n_chunks;  // the tensor's chunks in a launch of the selection: chunk c covers the PRUNE_CHUNK floats of the
                                    // buffer that start at (offset & ~31) + c * PRUNE_CHUNK -- whole mask words, shared with no other chunk
    int32_t pad_;
    int64_t scratch_off;  // in uint32 words of the scratch: PRUNE_HIST_WORDS histogram counters, then one tie count per chunk
    FastDiv d_row, d_per;
};
struct PruneTable {
    int32_t n, total_chunks;
    int64_t span_lo, span_hi;  // floats: [first prunable tensor's offset, end of the last one) -- what the apply pass walks
    int64_t hist_words;        // scratch words in use (what the update clears in front of the selection)
    PruneTensor t[PRUNE_MAX_TENSORS];
};
struct PruneArgs {
    float* p;          // the parameter buffer (16-byte aligned)
    float* mirror;     // workspace + wsplit_off (same offsets as the master, 32-byte aligned), or nullptr: the master alone
    uint32_t* mask;    // one bit per float of the buffer, bit (i & 31) of word (i >> 5); set = kept
    uint32_t* scratch; // the update alone
    PruneTable tab;
};

// Fills n_real / first_chunk / n_chunks / scratch_off / the dividers of every tensor and the table's totals from offset, size and the
// four geometry fields.  ISDQN_ERR_SHAPE: an offset or size that is no multiple of 8, a tensor of 2^31 floats or more.
int prune_table_finish(PruneTable& tab);
// Select (every t[i].k is read), write the mask, apply: the launches of one update on stream `st`.
int launch_prune_update(const PruneArgs& a, hipStream_t st);
// One launch on stream `st`: +0.0 to the master (and mirror) wherever the mask says pruned inside [span_lo, span_hi).
int launch_prune_apply(const PruneArgs& a, hipStream_t st);

}  // namespace isdqn
