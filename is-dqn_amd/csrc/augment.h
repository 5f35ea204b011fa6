// DrQ random-shift augmentation of a sampled batch's frame stacks (Kostrikov, Yarats and Fergus 2020; DrQ(eps) of Agarwal et al. 2021).
// include/isdqn_hip.h, isdqn_replay_augment_shift holds THE definition.  Included by replay_kernels.hip inside namespace isdqn.
// Built beside the plan: the learn step reads frames + frame_stride + frame_ids and never the replay itself, so the shifted copies of a
// batch's frames go into a caller-owned scratch pool, an id table points into it, and no kernel of net_kernels.hip knows of the option.
//   augment_shift_kernel    one workgroup per output frame (B = 32, stack 4: 256 workgroups).  Every thread takes its stack's draw --
//                           Philox4x32-10 keyed by (seed, *aug_count + step of the row, row within the step, half) -- and writes
//                           out[y][x] = in[clamp(y + dy)][clamp(x + dx)].  `wide` (frame size, stride and both bases multiples of 16, frame
//                           within 64 KB): the source frame is staged in LDS with 16-byte loads, every lane assembles 16 output bytes from
//                           the clamped, shifted LDS columns and stores them as one piece.  Otherwise bytes, straight from global memory.
//   augment_advance_kernel  one thread, behind it: *aug_count += n_rows / rows_per_step with an ordinary store (the kernel boundary orders
//                           it behind every read, as noisy_advance_kernel's)
// No atomics.  Ids are the caller's (the row gather wrote them): as everywhere in this library they are trusted to name frames of the store.
#pragma once

#include "philox.h"

// Bounds-checked development build (-DISDQN_BOUNDS): the table of gemm_core.h is a static device variable of net_kernels.hip's code
// object (no relocatable device code), so this code object keeps one of its own behind its own pair of debug entry points
// (replay_kernels.hip: isdqn_debug_replay_bounds_set / _get); sites 43 (id table), 44 (counter), 45 (source frames)
#if defined(ISDQN_BOUNDS)
struct ReplayBoundsTable {
    int n, bad, bad_site, pad;
    unsigned long long bad_addr;
    unsigned long long lo[16], hi[16];
};
static __device__ ReplayBoundsTable replay_bounds;
__device__ __forceinline__ void replay_bounds_check(const void* p, int bytes, int site) {
    const unsigned long long a = (unsigned long long)p, b = a + (unsigned)bytes;
    const int n = replay_bounds.n;
    if (n <= 0) return;
    bool ok = false;
    for (int i = 0; i < n; ++i) ok |= (a >= replay_bounds.lo[i] && b <= replay_bounds.hi[i]);
    if (!ok && atomicCAS(&replay_bounds.bad, 0, 1) == 0) {
        replay_bounds.bad_addr = a;
        replay_bounds.bad_site = site;
    }
}
#define ISDQN_BOUNDS_CHECK(p, bytes, site) replay_bounds_check((const void*)(p), (int)(bytes), (site))
#else
#define ISDQN_BOUNDS_CHECK(p, bytes, site) ((void)0)
#endif

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_LDS = 65536;  // the wide path stages one frame; larger frames take the byte path

__device__ __forceinline__ int aug_clamp(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(AUG_THREADS) void augment_shift_kernel(const uint8_t* __restrict__ frames, int64_t frame_stride, int h, int w,
                                                                    FastDiv div_w, int stack, const int* __restrict__ frame_ids,
                                                                    int rows_per_step, int pad, uint32_t seed_lo, uint32_t seed_hi,
                                                                    const int64_t* __restrict__ aug_count, uint8_t* __restrict__ out_frames,
                                                                    int* __restrict__ out_frame_ids, int wide) {
    ISDQN_EMPTY_KERNEL_RETURN
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_src[];
    const int f = blockIdx.x;  // output frame r * 2*stack + k
    const int s2 = 2 * stack, r = f / s2, k = f - r * s2, tid = threadIdx.x;
    ISDQN_BOUNDS_CHECK(frame_ids + f, 4, 43);
    const int id = frame_ids[f];
    if (tid == 0) out_frame_ids[f] = id < 0 ? -1 : f;
    if (id < 0) return;  // the zero frame of the leading padding stays the zero frame; its scratch frame is not written
    ISDQN_BOUNDS_CHECK(aug_count, 8, 44);
    const uint64_t t = (uint64_t)*aug_count + (uint64_t)(r / rows_per_step);
    uint32_t x0, x1;
    philox4x32_10((uint32_t)(r % rows_per_step), 0x80000000u | (k >= stack ? 1u : 0u), (uint32_t)t, (uint32_t)(t >> 32), seed_lo, seed_hi, x0, x1);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    const int dx = (int)__umulhi(x0, span) - pad, dy = (int)__umulhi(x1, span) - pad;
    const uint8_t* __restrict__ src = frames + (int64_t)id * frame_stride;
    uint8_t* __restrict__ dst = out_frames + (int64_t)f * frame_stride;
    const int hw = h * w;
    if (wide) {
        const int n16 = hw >> 4;
        for (int i = tid; i < n16; i += AUG_THREADS) {
            ISDQN_BOUNDS_CHECK(src + 16 * i, 16, 45);
            reinterpret_cast<uint4*>(aug_src)[i] = reinterpret_cast<const uint4*>(src)[i];
        }
        __syncthreads();
        for (int i = tid; i < n16; i += AUG_THREADS) {
            uint32_t yq, xq;
            div_w.divmod((uint32_t)(16 * i), yq, xq);
            int y = (int)yq, x = (int)xq, row = aug_clamp(y + dy, h - 1) * w;
            uint32_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                word[j >> 2] |= (uint32_t)aug_src[row + aug_clamp(x + dx, w - 1)] << (8 * (j & 3));
                if (++x == w) {  // the piece runs on into the next row (84 is no multiple of 16)
                    x = 0;
                    ++y;
                    row = aug_clamp(y + dy, h - 1) * w;
                }
            }
            reinterpret_cast<uint4*>(dst)[i] = make_uint4(word[0], word[1], word[2], word[3]);
        }
        return;
    }
    for (int p = tid; p < hw; p += AUG_THREADS) {
        uint32_t y, x;
        div_w.divmod((uint32_t)p, y, x);
        const uint8_t* from = src + aug_clamp((int)y + dy, h - 1) * w + aug_clamp((int)x + dx, w - 1);
        ISDQN_BOUNDS_CHECK(from, 1, 45);
        dst[p] = *from;
    }
}

__global__ void augment_advance_kernel(int64_t* __restrict__ aug_count, int64_t n_steps) {
    ISDQN_EMPTY_KERNEL_RETURN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ISDQN_BOUNDS_CHECK(aug_count, 8, 44);
        *aug_count = *aug_count + n_steps;
    }
}
