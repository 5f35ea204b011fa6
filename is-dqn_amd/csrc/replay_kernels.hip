// Device-resident replay: byte/integer HBM-bound kernels for ReplayBuffer.sample
// (slimdqn/sample_collection/replay_buffer.py:198-213).
//
// HBM layout: frames[slot][h*w] uint8 (one single frame per env step, 7,056 B for Atari)
// and an element table in SoA form indexed by element slot.  A sampled batch is B rows of
// that table; the pixels themselves are never copied for the training step (the first
// convolution reads the frames through the id table).  `materialize` exists for callers
// that want the reference's (B, h, w, stack) arrays.
#include "common.h"

namespace isdqn {

__global__ __launch_bounds__(256) void gather_rows_kernel(const int* __restrict__ elem_frames,
                                                          const int* __restrict__ elem_action,
                                                          const float* __restrict__ elem_reward,
                                                          const uint8_t* __restrict__ elem_terminal, int stack2,
                                                          const int* __restrict__ index_to_slot,
                                                          const int* __restrict__ slots, int B,
                                                          int* __restrict__ out_ids, int* __restrict__ out_action,
                                                          float* __restrict__ out_reward,
                                                          uint8_t* __restrict__ out_terminal) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * stack2) return;
    int b = i / stack2, c = i - b * stack2;
    int slot = slots[b];
    if (index_to_slot != nullptr) slot = index_to_slot[slot];
    out_ids[i] = elem_frames[(int64_t)slot * stack2 + c];
    if (c == 0) {
        out_action[b] = elem_action[slot];
        out_reward[b] = elem_reward[slot];
        out_terminal[b] = elem_terminal[slot];
    }
}

// One workgroup per (sample, which): interleave `stack` planar frames into (h, w, stack).
// Reads: coalesced 4-byte words of each plane; writes: 4*stack bytes per thread, contiguous.
__global__ __launch_bounds__(256) void materialize_kernel(const uint8_t* __restrict__ frames, int64_t frame_stride,
                                                          int hw, int stack, const int* __restrict__ frame_ids,
                                                          uint8_t* __restrict__ out_state,
                                                          uint8_t* __restrict__ out_next) {
    const int b = blockIdx.x, which = blockIdx.y;
    const int* ids = frame_ids + ((int64_t)b * 2 + which) * stack;
    uint8_t* out = (which ? out_next : out_state) + (int64_t)b * hw * stack;
    for (int p = threadIdx.x; p < hw; p += blockDim.x) {
        for (int c = 0; c < stack; ++c) {
            int id = ids[c];
            out[(int64_t)p * stack + c] = id < 0 ? (uint8_t)0 : frames[(int64_t)id * frame_stride + p];
        }
    }
}

__global__ __launch_bounds__(256) void deinterleave_kernel(const uint8_t* __restrict__ state,
                                                           const uint8_t* __restrict__ next_state, int hw, int stack,
                                                           uint8_t* __restrict__ out_frames,
                                                           int* __restrict__ out_ids) {
    const int b = blockIdx.x, which = blockIdx.y;
    const uint8_t* in = (which ? next_state : state) + (int64_t)b * hw * stack;
    const int64_t first = ((int64_t)b * 2 + which) * stack;
    for (int p = threadIdx.x; p < hw; p += blockDim.x)
        for (int c = 0; c < stack; ++c) out_frames[(first + c) * hw + p] = in[(int64_t)p * stack + c];
    if (threadIdx.x < stack) out_ids[first + threadIdx.x] = (int)(first + threadIdx.x);
}

}  // namespace isdqn

using namespace isdqn;

// ReplayBuffer.add's device side (replay_buffer.py:185-196): everything the host accumulator changed since the last flush --
// new frames, rewritten element rows, moved sampler indices -- arrives in ONE staged buffer and is scattered by one launch.
// Workgroups [0, n_frames): one frame each (16-byte pieces); then the element rows; then the index -> slot pairs.
__global__ __launch_bounds__(256) void apply_staged_kernel(const uint8_t* __restrict__ st, const isdqn_staged_updates u, int row_blocks,
                                                           uint8_t* __restrict__ frames, int64_t frame_stride,
                                                           int* __restrict__ elem_frames, int* __restrict__ elem_action,
                                                           float* __restrict__ elem_reward, uint8_t* __restrict__ elem_terminal,
                                                           int* __restrict__ index_to_slot) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b < u.n_frames) {
        const int slot = reinterpret_cast<const int*>(st + u.off_frame_slots)[b];
        const uint8_t* src = st + u.off_frame_data + (int64_t)b * u.frame_bytes;
        uint8_t* dst = frames + (int64_t)slot * frame_stride;
        // 16-byte pieces only when both sides are 16-byte aligned for EVERY frame: frame size and stride multiples of 16 and
        // the bases of the staged frame block and of the frame store aligned (the host packer rounds its sections to 16 bytes,
        // but this is a public entry point); otherwise bytes
        const bool wide = ((u.frame_bytes | (int)(frame_stride & 15)) & 15) == 0 &&
                          ((reinterpret_cast<uintptr_t>(st + u.off_frame_data) | reinterpret_cast<uintptr_t>(frames)) & 15) == 0;
        const int n16 = wide ? u.frame_bytes / 16 : 0;
        for (int i = t; i < n16; i += 256) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (int i = n16 * 16 + t; i < u.frame_bytes; i += 256) dst[i] = src[i];
        return;
    }
    const int rb = b - u.n_frames;
    if (rb < row_blocks) {
        const int i = rb * 256 + t;
        if (i < u.n_rows * u.stack2) {
            const int r = i / u.stack2, c = i - r * u.stack2;
            const int row = reinterpret_cast<const int*>(st + u.off_rows)[r];
            elem_frames[(int64_t)row * u.stack2 + c] = reinterpret_cast<const int*>(st + u.off_row_frames)[i];
            if (c == 0) {
                elem_action[row] = reinterpret_cast<const int*>(st + u.off_row_action)[r];
                elem_reward[row] = reinterpret_cast<const float*>(st + u.off_row_reward)[r];
                elem_terminal[row] = (st + u.off_row_terminal)[r];
            }
        }
        return;
    }
    const int i = (rb - row_blocks) * 256 + t;
    if (i < u.n_index) index_to_slot[reinterpret_cast<const int*>(st + u.off_index_rows)[i]] = reinterpret_cast<const int*>(st + u.off_index_vals)[i];
}

extern "C" int isdqn_replay_apply_staged(const uint8_t* staged, const isdqn_staged_updates* u, uint8_t* frames, int64_t frame_stride,
                                         int32_t* elem_frames, int32_t* elem_action, float* elem_reward, uint8_t* elem_terminal,
                                         int32_t* index_to_slot, void* stream) {
    ISDQN_REQUIRE(staged && u, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(u->n_frames >= 0 && u->n_rows >= 0 && u->n_index >= 0 && u->stack2 >= 1 && u->frame_bytes >= 0, ISDQN_ERR_ARG, "negative count");
    ISDQN_REQUIRE(u->n_frames == 0 || frames, ISDQN_ERR_ARG, "null frame store");
    ISDQN_REQUIRE(u->n_rows == 0 || (elem_frames && elem_action && elem_reward && elem_terminal), ISDQN_ERR_ARG, "null element table");
    ISDQN_REQUIRE(u->n_index == 0 || index_to_slot, ISDQN_ERR_ARG, "null index table");
    // the int32 / float sections are read as such: 4-byte aligned offsets on a 4-byte aligned base
    ISDQN_REQUIRE((reinterpret_cast<uintptr_t>(staged) & 3) == 0 &&
                  ((u->off_frame_slots | u->off_rows | u->off_row_frames | u->off_row_action | u->off_row_reward | u->off_index_rows |
                    u->off_index_vals) & 3) == 0,
                  ISDQN_ERR_ARG, "staged int32/float sections must be 4-byte aligned");
    ISDQN_REQUIRE(u->off_frame_slots >= 0 && u->off_frame_data >= 0 && u->off_rows >= 0 && u->off_row_frames >= 0 && u->off_row_action >= 0 &&
                  u->off_row_reward >= 0 && u->off_row_terminal >= 0 && u->off_index_rows >= 0 && u->off_index_vals >= 0,
                  ISDQN_ERR_ARG, "negative section offset");
    ISDQN_REQUIRE(u->n_frames == 0 || frame_stride >= u->frame_bytes, ISDQN_ERR_SHAPE, "frame_stride < frame_bytes");
    const int row_blocks = (u->n_rows * u->stack2 + 255) / 256, idx_blocks = (u->n_index + 255) / 256;
    const int blocks = u->n_frames + row_blocks + idx_blocks;
    if (blocks == 0) return ISDQN_OK;
    hipLaunchKernelGGL(apply_staged_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, staged, *u, row_blocks, frames, frame_stride,
                       elem_frames, elem_action, elem_reward, elem_terminal, index_to_slot);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_replay_gather_rows(const int32_t* elem_frames, const int32_t* elem_action,
                                        const float* elem_reward, const uint8_t* elem_terminal, int32_t stack,
                                        const int32_t* index_to_slot, const int32_t* slots, int32_t B,
                                        int32_t* out_frame_ids, int32_t* out_action,
                                        float* out_reward, uint8_t* out_terminal, void* stream) {
    ISDQN_REQUIRE(elem_frames && elem_action && elem_reward && elem_terminal && slots, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(out_frame_ids && out_action && out_reward && out_terminal, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(stack >= 1 && B >= 0, ISDQN_ERR_SHAPE, "bad shape");
    if (B == 0) return ISDQN_OK;
    int total = B * 2 * stack;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, elem_frames,
                       elem_action, elem_reward, elem_terminal, 2 * stack, index_to_slot, slots, B, out_frame_ids, out_action,
                       out_reward, out_terminal);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_replay_materialize(const uint8_t* frames, int64_t frame_stride, int32_t h, int32_t w,
                                        int32_t stack, const int32_t* frame_ids, int32_t B, uint8_t* out_state,
                                        uint8_t* out_next_state, void* stream) {
    ISDQN_REQUIRE(frames && frame_ids && out_state && out_next_state, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(h > 0 && w > 0 && stack >= 1 && B >= 0 && frame_stride >= (int64_t)h * w, ISDQN_ERR_SHAPE,
                  "bad shape");
    if (B == 0) return ISDQN_OK;
    hipLaunchKernelGGL(materialize_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, frames, frame_stride, h * w,
                       stack, frame_ids, out_state, out_next_state);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_replay_deinterleave(const uint8_t* state, const uint8_t* next_state, int32_t h, int32_t w,
                                         int32_t stack, int32_t B, uint8_t* out_frames, int32_t* out_frame_ids,
                                         void* stream) {
    ISDQN_REQUIRE(state && next_state && out_frames && out_frame_ids, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(h > 0 && w > 0 && stack >= 1 && stack <= 256 && B >= 0, ISDQN_ERR_SHAPE, "bad shape");
    if (B == 0) return ISDQN_OK;
    hipLaunchKernelGGL(deinterleave_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, state, next_state, h * w,
                       stack, out_frames, out_frame_ids);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// The random-shift augmentation, last in this code object: tests/test_kernel_order_host.py holds every kernel to its place.
namespace isdqn {
#include "augment.h"
}  // namespace isdqn

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build (augment.h: this code object's own table): register the byte extents [lo[i], hi[i]) of every buffer
// the caller hands to the augmentation and clear the record; read back the first load that fell outside all of them (synchronises).
extern "C" int isdqn_debug_replay_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 16, ISDQN_ERR_ARG, "at most 16 regions");
    isdqn::ReplayBoundsTable t{};
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::replay_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_replay_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::ReplayBoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::replay_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif

// Random-shift augmentation of the frame stacks of n_rows sampled transitions into a scratch pool (include/isdqn_hip.h holds THE
// definition; augment.h the kernels).  Two launches: the shift, then the one-thread counter advance.
extern "C" int isdqn_replay_augment_shift(const uint8_t* frames, int64_t frame_stride, int32_t h, int32_t w, int32_t stack,
                                          const int32_t* frame_ids, int32_t n_rows, int32_t rows_per_step, int32_t pad, uint64_t seed,
                                          int64_t* aug_count, uint8_t* out_frames, int32_t* out_frame_ids, void* stream) {
    ISDQN_REQUIRE(frames && frame_ids && aug_count && out_frames && out_frame_ids, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(pad >= 0 && pad <= 127, ISDQN_ERR_ARG, "pad outside [0, 127]");
    ISDQN_REQUIRE(h >= 1 && w >= 1 && stack >= 1 && n_rows >= 1, ISDQN_ERR_ARG, "h, w, stack and n_rows must be positive");
    ISDQN_REQUIRE(rows_per_step >= 1 && n_rows % rows_per_step == 0, ISDQN_ERR_ARG, "rows_per_step must divide n_rows");
    ISDQN_REQUIRE((int64_t)h * w <= INT32_MAX && frame_stride >= (int64_t)h * w, ISDQN_ERR_ARG, "frame_stride < h * w");
    const int64_t n_out = (int64_t)n_rows * 2 * stack;
    ISDQN_REQUIRE(n_out <= INT32_MAX, ISDQN_ERR_ARG, "more than 2^31 - 1 output frames");
    ISDQN_REQUIRE((reinterpret_cast<uintptr_t>(frame_ids) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_frame_ids) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(aug_count) & 7) == 0, ISDQN_ERR_ARG, "misaligned id table or counter");
    // the pool must not overlap the store (a shifted frame would be read back as a source).  The store's extent is no argument: what the
    // call can tell is the store's base inside the pool, and the pool's base inside the store's first frame
    const uintptr_t fr = reinterpret_cast<uintptr_t>(frames), po = reinterpret_cast<uintptr_t>(out_frames);
    const uintptr_t pool_bytes = (uintptr_t)(n_out - 1) * (uintptr_t)frame_stride + (uintptr_t)h * w;
    ISDQN_REQUIRE(!(fr >= po && fr < po + pool_bytes) && !(po >= fr && po < fr + (uintptr_t)h * w), ISDQN_ERR_ARG,
                  "out_frames overlaps frames");
    // every workgroup reads its id and writes its output id: the two tables must be different memory
    const uintptr_t ti = reinterpret_cast<uintptr_t>(frame_ids), to = reinterpret_cast<uintptr_t>(out_frame_ids), tb = (uintptr_t)n_out * 4;
    ISDQN_REQUIRE(ti + tb <= to || to + tb <= ti, ISDQN_ERR_ARG, "out_frame_ids overlaps frame_ids");
    const int hw = h * w;
    const int wide = (hw & 15) == 0 && (frame_stride & 15) == 0 && ((fr | po) & 15) == 0 && hw <= AUG_MAX_LDS;
    hipLaunchKernelGGL(augment_shift_kernel, dim3((unsigned)n_out), dim3(AUG_THREADS), wide ? hw : 0, (hipStream_t)stream, frames, frame_stride,
                       h, w, FastDiv((uint32_t)w), stack, frame_ids, rows_per_step, pad, (uint32_t)seed, (uint32_t)(seed >> 32), aug_count,
                       out_frames, out_frame_ids, wide);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(augment_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, aug_count, (int64_t)(n_rows / rows_per_step));
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// Horizon windows (include/isdqn_hip.h, isdqn_replay_gather_horizon holds THE definition): an element row keeps the frame ids of its
// whole window [stack + n_max], its n_max per-step rewards and how many of them lie inside the trajectory; the gather cuts the window
// at a horizon m and sums the return at a discount that it reads from device memory, so a captured step changes both between replays.
// Appended behind the augmentation, as tests/golden/kernel_order.txt has them (tests/test_kernel_order_host.py).  Bounds sites 48 (gather), 49 (scatter).
namespace isdqn {

constexpr int HORIZON_MAX = 128;

// Lanes over the 2 * stack output ids of the B rows, as gather_rows_kernel; the lane of a row's first id also sums the row's return,
// sequentially and in float64 (one rounding per operation: -ffp-contract=off), and writes the row's scalars.
__global__ __launch_bounds__(256) void gather_horizon_kernel(const int* __restrict__ elem_window, const float* __restrict__ elem_steps,
                                                             const int* __restrict__ elem_len, const int* __restrict__ elem_action,
                                                             const uint8_t* __restrict__ elem_terminal, int stack, int n_max,
                                                             const int* __restrict__ index_to_slot, const int* __restrict__ slots, int B,
                                                             const int* __restrict__ horizon, const float* __restrict__ gamma,
                                                             int* __restrict__ out_ids, int* __restrict__ out_action,
                                                             float* __restrict__ out_reward, uint8_t* __restrict__ out_terminal,
                                                             float* __restrict__ out_discount) {
    const int stack2 = 2 * stack;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * stack2) return;
    const int b = i / stack2, c = i - b * stack2;
    ISDQN_BOUNDS_CHECK(slots + b, 4, 48);
    int slot = slots[b];
    if (index_to_slot != nullptr) {
        ISDQN_BOUNDS_CHECK(index_to_slot + slot, 4, 48);
        slot = index_to_slot[slot];
    }
    ISDQN_BOUNDS_CHECK(horizon, 4, 48);
    const int m = min(max(*horizon, 1), n_max);
    const int* __restrict__ win = elem_window + (int64_t)slot * (stack + n_max);
    const int col = c < stack ? c : m + (c - stack);  // state: window[0, stack); next state: window[m, m + stack)
    ISDQN_BOUNDS_CHECK(win + col, 4, 48);
    out_ids[i] = win[col];
    if (c != 0) return;
    ISDQN_BOUNDS_CHECK(elem_len + slot, 4, 48);
    ISDQN_BOUNDS_CHECK(gamma, 4, 48);
    const int len = elem_len[slot];
    const int me = min(m, len);
    const double G = (double)*gamma;
    const float* __restrict__ steps = elem_steps + (int64_t)slot * n_max;
    double g = 1.0, acc = 0.0;
    for (int t = 0; t < m; ++t) {
        if (t < me) {
            ISDQN_BOUNDS_CHECK(steps + t, 4, 48);
            acc = acc + (double)steps[t] * g;
        }
        g = g * G;
    }
    ISDQN_BOUNDS_CHECK(elem_action + slot, 4, 48);
    ISDQN_BOUNDS_CHECK(elem_terminal + slot, 1, 48);
    out_action[b] = elem_action[slot];
    out_reward[b] = (float)acc;
    out_discount[b] = (float)g;
    out_terminal[b] = (elem_terminal[slot] != 0 && m >= len) ? (uint8_t)1 : (uint8_t)0;
}

// The horizon tables' part of a flush: lanes over the stack + n_max window ids of the n_rows staged rows; a row's lanes below n_max
// also copy its step rewards, its first lane the length.
__global__ __launch_bounds__(256) void apply_staged_horizon_kernel(const uint8_t* __restrict__ st, int n_rows, int64_t off_rows,
                                                                   int64_t off_window, int64_t off_steps, int64_t off_len, int stack,
                                                                   int n_max, int* __restrict__ elem_window,
                                                                   float* __restrict__ elem_steps, int* __restrict__ elem_len) {
    const int wn = stack + n_max;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_rows * wn) return;
    const int r = (int)(i / wn), c = (int)(i - (int64_t)r * wn);
    ISDQN_BOUNDS_CHECK(reinterpret_cast<const int*>(st + off_rows) + r, 4, 49);
    ISDQN_BOUNDS_CHECK(reinterpret_cast<const int*>(st + off_window) + i, 4, 49);
    const int row = reinterpret_cast<const int*>(st + off_rows)[r];
    elem_window[(int64_t)row * wn + c] = reinterpret_cast<const int*>(st + off_window)[i];
    if (c < n_max) {
        ISDQN_BOUNDS_CHECK(reinterpret_cast<const float*>(st + off_steps) + (int64_t)r * n_max + c, 4, 49);
        elem_steps[(int64_t)row * n_max + c] = reinterpret_cast<const float*>(st + off_steps)[(int64_t)r * n_max + c];
    }
    if (c == 0) {
        ISDQN_BOUNDS_CHECK(reinterpret_cast<const int*>(st + off_len) + r, 4, 49);
        elem_len[row] = reinterpret_cast<const int*>(st + off_len)[r];
    }
}

}  // namespace isdqn

extern "C" int isdqn_replay_apply_staged_horizon(const uint8_t* staged, int32_t n_rows, int64_t off_rows, int64_t off_window,
                                                 int64_t off_steps, int64_t off_len, int32_t stack, int32_t n_max, int32_t* elem_window,
                                                 float* elem_steps, int32_t* elem_len, void* stream) {
    ISDQN_REQUIRE(staged && elem_window && elem_steps && elem_len, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(n_rows >= 0 && stack >= 1 && n_max >= 1 && n_max <= HORIZON_MAX, ISDQN_ERR_ARG, "n_rows < 0, stack < 1 or n_max outside [1, 128]");
    ISDQN_REQUIRE(off_rows >= 0 && off_window >= 0 && off_steps >= 0 && off_len >= 0, ISDQN_ERR_ARG, "negative section offset");
    ISDQN_REQUIRE((reinterpret_cast<uintptr_t>(staged) & 3) == 0 && ((off_rows | off_window | off_steps | off_len) & 3) == 0, ISDQN_ERR_ARG,
                  "staged int32/float sections must be 4-byte aligned");
    if (n_rows == 0) return ISDQN_OK;
    const int64_t total = (int64_t)n_rows * (stack + n_max);
    ISDQN_REQUIRE((total + 255) / 256 <= INT32_MAX, ISDQN_ERR_ARG, "too many rows");
    hipLaunchKernelGGL(apply_staged_horizon_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, staged, n_rows,
                       off_rows, off_window, off_steps, off_len, stack, n_max, elem_window, elem_steps, elem_len);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_replay_gather_horizon(const int32_t* elem_window, const float* elem_steps, const int32_t* elem_len,
                                           const int32_t* elem_action, const uint8_t* elem_terminal, int32_t stack, int32_t n_max,
                                           const int32_t* index_to_slot, const int32_t* slots, int32_t B, const int32_t* horizon,
                                           const float* gamma, int32_t* out_frame_ids, int32_t* out_action, float* out_reward,
                                           uint8_t* out_terminal, float* out_discount, void* stream) {
    ISDQN_REQUIRE(elem_window && elem_steps && elem_len && elem_action && elem_terminal && slots && horizon && gamma, ISDQN_ERR_ARG,
                  "null pointer");
    ISDQN_REQUIRE(out_frame_ids && out_action && out_reward && out_terminal && out_discount, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(B >= 1 && stack >= 1 && n_max >= 1 && n_max <= HORIZON_MAX, ISDQN_ERR_ARG, "B < 1, stack < 1 or n_max outside [1, 128]");
    const int64_t total = (int64_t)B * 2 * stack;
    ISDQN_REQUIRE(total <= INT32_MAX, ISDQN_ERR_ARG, "more than 2^31 - 1 output ids");
    hipLaunchKernelGGL(gather_horizon_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, elem_window, elem_steps,
                       elem_len, elem_action, elem_terminal, stack, n_max, index_to_slot, slots, B, horizon, gamma, out_frame_ids, out_action,
                       out_reward, out_terminal, out_discount);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}
