// Periodic resets (Nikishin et al. 2022, "The Primacy Bias in Deep RL"; shrink and perturb: Ash & Adams 2020; SR-SPR, BBF) and EMA
// target networks (optax.incremental_update).  include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema hold THE definitions.  The reference
// has no counterpart.  Included by net_kernels.hip inside namespace isdqn, last of its headers: tests/test_kernel_order_host.py holds every
// kernel of the code object to its place in tests/golden/kernel_order.txt, these at the end.  Built beside the plan: no field of isdqn_net_config, no workspace region, nothing of build_plan.
//   reset_kernel       one launch over every tensor that is written, found through ResetTable (passed by value, as AdamTable): per
//                      tensor a factor pair (s, q) by its class; s == 0: p <- q * f without reading p, else p <- s * p + q * f, the two
//                      products and the sum rounded separately; both Adam moments <- +0.  A virtual block covers RESET_BLOCK_ELEMS
//                      consecutive elements of ONE tensor; 16 bytes per lane where the tensor's offset and size are multiples of 4
//                      floats (every tensor of every plan so far), a scalar path otherwise.  The grid is capped and strides.
//   reset_count_kernel one thread, behind it: *adam_count = 0 with an ordinary store (a kernel boundary orders it)
//   ema_kernel         t <- omt * t + tau * p over the flat buffer, 16 bytes per lane and a scalar tail, capped grid, plain loads and
//                      stores (the next step reads both buffers again: nothing is streamed past the caches)
// No atomics anywhere.  ISDQN_BOUNDS sites: 46 (reset), 47 (EMA) -- loads and stores alike.
#pragma once

constexpr int RESET_THREADS = 256;
constexpr int RESET_BLOCK_ELEMS = 4 * RESET_THREADS;  // elements of one virtual block: one float4 per lane
constexpr int RESET_MAX_ENTRIES = 64;                 // per launch (1.5 KB of kernel arguments); longer tables are split
constexpr int RESET_MAX_BLOCKS = 2048;                // 256 CUs x 8 workgroups: the rest of a launch is reached by the stride

struct ResetEntry {
    int64_t off, size;  // the tensor in the flat buffer (floats)
    int block_start;    // first virtual block of the tensor in this launch
    int mode;           // bit 0: the upper class' factors; bit 1: 16 bytes per lane
};
struct ResetTable {
    ResetEntry e[RESET_MAX_ENTRIES];
    int n, total_blocks;
    float s[2], q[2];  // [0] lower, [1] upper
};

// s == 0: the parameter is not an operand (a NaN or Inf is replaced)
__device__ __forceinline__ float reset_value(bool blend, float s, float q, float p, float f) {
    const float b = __fmul_rn(q, f);
    return blend ? __fadd_rn(__fmul_rn(s, p), b) : b;
}

__global__ __launch_bounds__(RESET_THREADS) void reset_kernel(const ResetTable tab, float* __restrict__ p, float* __restrict__ m,
                                                              float* __restrict__ v, const float* __restrict__ fresh) {
    ISDQN_EMPTY_KERNEL_RETURN
    int e = 0;
    for (int vb = (int)blockIdx.x; vb < tab.total_blocks; vb += (int)gridDim.x) {
        while (e + 1 < tab.n && vb >= tab.e[e + 1].block_start) ++e;
        const ResetEntry en = tab.e[e];
        const int c = en.mode & 1;
        const float s = tab.s[c], q = tab.q[c];
        const bool blend = s != 0.f;
        const int64_t i0 = (int64_t)(vb - en.block_start) * RESET_BLOCK_ELEMS;
        if (en.mode & 2) {
            const int64_t i = i0 + (int64_t)threadIdx.x * 4;
            if (i >= en.size) continue;
            const int64_t o = en.off + i;
            ISDQN_BOUNDS_CHECK(fresh + o, 16, 46);
            ISDQN_BOUNDS_CHECK(p + o, 16, 46);
            const float4 f = *reinterpret_cast<const float4*>(fresh + o);
            float4 x = float4{0.f, 0.f, 0.f, 0.f};
            if (blend) x = *reinterpret_cast<const float4*>(p + o);
            x.x = reset_value(blend, s, q, x.x, f.x);
            x.y = reset_value(blend, s, q, x.y, f.y);
            x.z = reset_value(blend, s, q, x.z, f.z);
            x.w = reset_value(blend, s, q, x.w, f.w);
            *reinterpret_cast<float4*>(p + o) = x;
            if (m != nullptr) {
                ISDQN_BOUNDS_CHECK(m + o, 16, 46);
                ISDQN_BOUNDS_CHECK(v + o, 16, 46);
                const float4 z = float4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<float4*>(m + o) = z;
                *reinterpret_cast<float4*>(v + o) = z;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + r * RESET_THREADS + (int)threadIdx.x;
                if (i >= en.size) break;
                const int64_t o = en.off + i;
                ISDQN_BOUNDS_CHECK(fresh + o, 4, 46);
                ISDQN_BOUNDS_CHECK(p + o, 4, 46);
                const float f = fresh[o];
                float x = 0.f;
                if (blend) x = p[o];
                p[o] = reset_value(blend, s, q, x, f);
                if (m != nullptr) {
                    ISDQN_BOUNDS_CHECK(m + o, 4, 46);
                    ISDQN_BOUNDS_CHECK(v + o, 4, 46);
                    m[o] = 0.f;
                    v[o] = 0.f;
                }
            }
        }
    }
}

__global__ void reset_count_kernel(int32_t* __restrict__ adam_count) {
    ISDQN_EMPTY_KERNEL_RETURN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ISDQN_BOUNDS_CHECK(adam_count, 4, 46);
        *adam_count = 0;
    }
}

__device__ __forceinline__ float ema_value(float omt, float tau, float t, float p) { return __fadd_rn(__fmul_rn(omt, t), __fmul_rn(tau, p)); }

// n4 float4 positions, then the n - 4 * n4 elements behind them one per lane (a buffer that is not 16-byte aligned: n4 = 0, everything).
// No __restrict__: the two buffers are distinct by contract, and a thread reads and writes the same positions only.  (Two positions in
// flight per lane, all loads in front of the first store, measured no faster inside a captured graph: docs/NOTEBOOK.md.)
__global__ __launch_bounds__(RESET_THREADS) void ema_kernel(float* t, const float* p, float omt, float tau, int64_t n4, int64_t n) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t stride = (int64_t)gridDim.x * RESET_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RESET_THREADS + threadIdx.x; i < n4; i += stride) {
        ISDQN_BOUNDS_CHECK(t + 4 * i, 16, 47);
        ISDQN_BOUNDS_CHECK(p + 4 * i, 16, 47);
        float4 a = *reinterpret_cast<const float4*>(t + 4 * i);
        const float4 b = *reinterpret_cast<const float4*>(p + 4 * i);
        a.x = ema_value(omt, tau, a.x, b.x);
        a.y = ema_value(omt, tau, a.y, b.y);
        a.z = ema_value(omt, tau, a.z, b.z);
        a.w = ema_value(omt, tau, a.w, b.w);
        *reinterpret_cast<float4*>(t + 4 * i) = a;
    }
    for (int64_t j = 4 * n4 + (int64_t)blockIdx.x * RESET_THREADS + threadIdx.x; j < n; j += stride) {
        ISDQN_BOUNDS_CHECK(t + j, 4, 47);
        ISDQN_BOUNDS_CHECK(p + j, 4, 47);
        t[j] = ema_value(omt, tau, t[j], p[j]);
    }
}
