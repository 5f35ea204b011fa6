// Soft head shift of iS-DQN on gfx950: head k of the last Dense moves towards head k + 1 at rate tau in every gradient step, instead of
// the hard copy of shift_kernel every T steps (K = 1: DQN's Polyak target on a shared torso).  THE definition is include/isdqn_hip.h,
// isdqn_net_soft_shift; the reference has no counterpart.  A translation unit of its own (build.SIDE_SOURCES): the four pinned code
// objects keep their kernels and their order.  Built beside the plan: no field of isdqn_net_config, no workspace region, nothing of
// build_plan; the entry point (net_kernels.hip, which holds the plan) fills SoftShiftArgs and calls launch_soft_shift.
//   soft_shift_kernel  a thread owns one position of the head block -- a row r < R and four consecutive columns, 16 bytes per lane;
//                      behind the R * in_p / 4 weight positions, the R bias positions, one element per lane -- and walks the heads
//                      upward: old[k + 1] is loaded once and stays in registers as the next iteration's old[k], new[k] is stored as a
//                      float4 and, with a workspace, as its half-group of the S8 weight mirror.  In place: every element of heads
//                      0 .. K is loaded once, every element of heads 0 .. K - 1 stored once.  A thread reads and writes its own
//                      positions only: no atomics, no LDS, no barrier.  The grid is sized by positions, capped, and strides.
//                      The launch is small against the chip (scalar heads at K = 9: 1152 lanes; 51 bins: 230 workgroups) and a lane's
//                      walk is a chain of memory round trips, so the loads of SOFT_SHIFT_AHEAD heads are issued together in front of
//                      the first store of the group (legal: a lane's stores never hit a position it has yet to load): one round trip
//                      per group instead of one per head (docs/NOTEBOOK.md has both timings).
// ISDQN_BOUNDS site: 51 -- loads and stores alike, the mirror's included -- against this object's own table (gemm_core.h keeps one per
// translation unit): isdqn_debug_soft_shift_bounds_set / _get below, after replay_kernels.hip's pair.
#include "soft_shift.h"

#include <string.h>

#include <algorithm>

#include "gemm_core.h"  // s8_store_quad / s8_store_elem, ISDQN_BOUNDS_CHECK and its table

namespace isdqn {

constexpr int SOFT_SHIFT_THREADS = 256;
constexpr int SOFT_SHIFT_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups: the rest of a launch is reached by the stride
constexpr int SOFT_SHIFT_AHEAD = 10;         // heads loaded in front of a group's first store: K = 9 (the headline shape) in one group

// the arithmetic of ema_value (reset.h): two products and one sum, each rounded on its own, never contracted
__device__ __forceinline__ float soft_shift_value(float omt, float tau, float lo, float up) { return __fadd_rn(__fmul_rn(omt, lo), __fmul_rn(tau, up)); }

template <bool MIRROR>
__global__ __launch_bounds__(SOFT_SHIFT_THREADS) void soft_shift_kernel(const SoftShiftArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    float* p = a.p;
    float* mirror = a.mirror;
    const int quads = a.in_p >> 2;
    const int K = a.K;
    const int64_t n_w = (int64_t)a.R * quads, n = n_w + a.R;
    const int64_t head_w = (int64_t)a.R * a.in_p;
    const float omt = a.omt, tau = a.tau;
    const int64_t stride = (int64_t)gridDim.x * SOFT_SHIFT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SOFT_SHIFT_THREADS + threadIdx.x; i < n; i += stride) {
        if (i < n_w) {
            const int r = (int)(i / quads), c0 = ((int)(i - (int64_t)r * quads)) << 2;
            int64_t row = a.w_off + (int64_t)r * a.in_p;  // the row of head k; w_off and in_p are multiples of 8
            ISDQN_BOUNDS_CHECK(p + row + c0, 16, 51);
            float4 lo = *reinterpret_cast<const float4*>(p + row + c0);
            for (int k0 = 0; k0 < K; k0 += SOFT_SHIFT_AHEAD) {
                float4 up[SOFT_SHIFT_AHEAD];
#pragma unroll
                for (int j = 0; j < SOFT_SHIFT_AHEAD; ++j)
                    if (k0 + j < K) {
                        ISDQN_BOUNDS_CHECK(p + row + (j + 1) * head_w + c0, 16, 51);
                        up[j] = *reinterpret_cast<const float4*>(p + row + (j + 1) * head_w + c0);
                    }
#pragma unroll
                for (int j = 0; j < SOFT_SHIFT_AHEAD; ++j)
                    if (k0 + j < K) {
                        float4 x;
                        x.x = soft_shift_value(omt, tau, lo.x, up[j].x);
                        x.y = soft_shift_value(omt, tau, lo.y, up[j].y);
                        x.z = soft_shift_value(omt, tau, lo.z, up[j].z);
                        x.w = soft_shift_value(omt, tau, lo.w, up[j].w);
                        *reinterpret_cast<float4*>(p + row + c0) = x;  // (checked as a load: the same 16 bytes)
                        if constexpr (MIRROR) {
                            ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(mirror + row + (c0 & ~7)) + (c0 & 4) * 2, 8, 51);
                            ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(mirror + row + (c0 & ~7)) + (c0 & 4) * 2 + 16, 8, 51);
                            s8_store_quad(mirror + row, c0, x.x, x.y, x.z, x.w);
                        }
                        lo = up[j];
                        row += head_w;
                    }
            }
        } else {
            const int j0 = (int)(i - n_w);
            int64_t o = a.b_off + j0;  // the bias of head k; b_off is a multiple of 8: the mirror's group of bias c is c & ~7
            ISDQN_BOUNDS_CHECK(p + o, 4, 51);
            float lo = p[o];
            for (int k0 = 0; k0 < K; k0 += SOFT_SHIFT_AHEAD) {
                float up[SOFT_SHIFT_AHEAD];
#pragma unroll
                for (int j = 0; j < SOFT_SHIFT_AHEAD; ++j)
                    if (k0 + j < K) {
                        ISDQN_BOUNDS_CHECK(p + o + (j + 1) * a.R, 4, 51);
                        up[j] = p[o + (j + 1) * a.R];
                    }
#pragma unroll
                for (int j = 0; j < SOFT_SHIFT_AHEAD; ++j)
                    if (k0 + j < K) {
                        const float x = soft_shift_value(omt, tau, lo, up[j]);
                        p[o] = x;
                        if constexpr (MIRROR) {
                            const int c = (int)(o - a.b_off);
                            ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(mirror + a.b_off + (c & ~7)) + (c & 7), 2, 51);
                            ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(mirror + a.b_off + (c & ~7)) + (c & 7) + 8, 2, 51);
                            s8_store_elem(mirror + a.b_off, c, x);
                        }
                        lo = up[j];
                        o += a.R;
                    }
            }
        }
    }
}

int launch_soft_shift(const SoftShiftArgs& a, hipStream_t st) {
    ISDQN_REQUIRE(a.p != nullptr, ISDQN_ERR_ARG, "soft head shift: null pointer");
    ISDQN_REQUIRE(a.R >= 1 && a.K >= 1 && a.in_p >= 8, ISDQN_ERR_SHAPE, "soft head shift: empty shape");
    // what the 16-byte lanes and the mirror's groups of 8 need
    ISDQN_REQUIRE(a.w_off >= 0 && a.b_off >= 0 && a.w_off % 8 == 0 && a.b_off % 8 == 0 && a.in_p % 8 == 0, ISDQN_ERR_SHAPE,
                  "soft head shift: the last Dense is not laid out in groups of 8");
    ISDQN_REQUIRE(((uintptr_t)a.p & 15) == 0, ISDQN_ERR_ARG, "soft head shift: params must be 16-byte aligned");
    ISDQN_REQUIRE(((uintptr_t)a.mirror & 31) == 0, ISDQN_ERR_ARG, "soft head shift: the workspace's weight mirror must be 32-byte aligned");
    const int64_t n = (int64_t)a.R * (a.in_p / 4) + a.R;
    const int64_t blocks = std::min<int64_t>((n + SOFT_SHIFT_THREADS - 1) / SOFT_SHIFT_THREADS, SOFT_SHIFT_MAX_BLOCKS);
    if (a.mirror != nullptr) hipLaunchKernelGGL(soft_shift_kernel<true>, dim3((unsigned)blocks), dim3(SOFT_SHIFT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(soft_shift_kernel<false>, dim3((unsigned)blocks), dim3(SOFT_SHIFT_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

}  // namespace isdqn

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build: the byte extents [lo[i], hi[i]) the soft shift may touch, and the first access outside all of them
// (scripts/soft_shift_bounds_check.py); this object's own table, as replay_kernels.hip has one.
extern "C" int isdqn_debug_soft_shift_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_soft_shift_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif
