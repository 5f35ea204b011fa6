// Random ensemble mixture (REM; Agarwal, Schuurmans, Norouzi, "An Optimistic Perspective on Offline Reinforcement Learning", ICML 2020):
// H scalar heads on one torso, trained on a fresh random convex combination of the heads at every gradient step, acting on their
// average.  THE definition is include/isdqn_hip.h (isdqn_mixture_draw, isdqn_batch_mixture, ISDQN_ACT_MEAN_HEADS).  A translation unit
// of its own (build.MIXTURE_SOURCES): the four pinned code objects keep their kernels and their order.  net_kernels.hip holds the plan
// and the entry points and calls the launchers of mixture.h.
//   mixture_draw_kernel      one workgroup: u_h from Philox4x32-10 keyed by (seed, *draw_count, h), their fp32 sum in ascending h by one
//                            thread, alpha_h = u_h / s.  mixture_advance_kernel stores count + 1 in a launch of its own behind it.
//   mix_td_kernel            td_kernel's place for a call that carries ISDQN_BATCH_MIXTURE: HeadLossArgs plus alpha and H, one regressed
//                            "pair" (K = 1).  td_kernel's row partition (TD_ROWS transitions per workgroup: loss_finalize_kernel and, at
//                            H = 1, every sum are td_kernel's, bit for bit), but a WAVE per transition instead of a lane: the lanes lie
//                            across the h * A + a columns of the transition's rows, so its 2 or 3 rows of H * A floats are read with
//                            coalesced loads (td_kernel's shape would read H = 200, A = 18 at a 14 KB stride per lane).  alpha is
//                            staged once in LDS.  No atomics, every sum in a fixed order: bit-identical from run to run.
//   argmax_mean_rows_kernel  argmax_rows_kernel on the sum of all heads: a wave per row, a lane per action, ascending h.
// The order of Qmix(x, a) = sum_h alpha_h Q_h(x, a), with G = 64 / A heads per pass (integer division; 1 when A > 64): partial g sums
// fl32(alpha_h * Q_h) over h = g, g + G, g + 2G, ... in ascending h, starting from the first product; the partials are then added in
// ascending g, starting from partial 0.  Products and adds are separate roundings (the build contracts nothing).
// ISDQN_BOUNDS sites 53 (the draw's count), 54 (alpha), 55 (the head-output rows), 56 (a row's discount), 57 (the "q" rows of the acting
// call), against this object's own table (gemm_core.h keeps one per translation unit): isdqn_debug_mixture_bounds_set / _get below.
#include "common.h"

#include <string.h>

#include "gemm_core.h"  // ISDQN_BOUNDS_CHECK and its table
#include "mixture.h"

namespace isdqn {

#include "philox.h"  // philox4x32_10, shared with noisy.h and augment.h

#include "td_loss.h"  // td_loss / td_dloss: td_kernel's own (at H = 1 the bits are its)

constexpr int MIX_THREADS = 1024;  // mix_td_kernel: 16 waves share the TD_ROWS transitions of a workgroup
constexpr int MIX_WAVES = MIX_THREADS / 64;
constexpr int MIX_ACT_THREADS = 256;
constexpr int TD_ROWS = 64;  // td_kernel's transitions per workgroup (row_kernels.h): the partition loss_and_finalize sizes n_blk by
constexpr uint32_t MIX_PHILOX_DOMAIN = 0x52454D00u;  // "REM\0": the second counter word of every draw

__global__ __launch_bounds__(MIX_MAX_HEADS) void mixture_draw_kernel(int H, uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ draw_count,
                                                                     float* __restrict__ alpha) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ float s_u[MIX_MAX_HEADS];
    __shared__ float s_sum;
    const int h = threadIdx.x;
    ISDQN_BOUNDS_CHECK(draw_count, 8, 53);
    const uint64_t count = (uint64_t)*draw_count;
    float u = 0.f;
    if (h < H) {
        uint32_t x0, x1;
        philox4x32_10((uint32_t)h, MIX_PHILOX_DOMAIN, (uint32_t)count, (uint32_t)(count >> 32), seed_lo, seed_hi, x0, x1);
        u = (float)((x0 >> 8) + 1u) * 0x1p-24f;  // exact: an integer in [1, 2^24] times a power of two, in (0, 1]
        s_u[h] = u;
    }
    __syncthreads();
    if (h == 0) {
        float s = 0.f;
        for (int i = 0; i < H; ++i) s += s_u[i];  // ascending h, one thread: THE order
        s_sum = s;
    }
    __syncthreads();
    if (h < H) alpha[h] = u / s_sum;  // (IEEE division: the build keeps hipcc's correctly rounded fp32 divide)
}

// Lane `lane` <- Qmix(row[r], a0 + lane) for lane < min(64, A - a0) (A <= 64: a0 = 0) of NR rows at once, in the order above; the other
// lanes hold nothing of use.  Every lane of the wave calls it (the shuffles are the wave's).  The trip count is the wave's
// (ceil(H / G) passes; a lane whose head of the last pass is past H - 1 loads head H - 1 again and adds nothing), and the loads of
// MIX_BATCH passes of all NR rows are requested before the first of them is used: the kernel lives off loads in flight.
constexpr int MIX_BATCH = 8;
template <int NR>
__device__ __forceinline__ void mix_chunk(const float* const (&row)[NR], const float* s_alpha, int a0, int A, int H, int lane, float (&m)[NR]) {
    const bool grouped = A <= 64;
    const int G = grouped ? 64 / A : 1;
    const int width = grouped ? A : min(64, A - a0);
    const int g = grouped ? lane / A : 0;
    const bool live = grouped ? g < G : lane < width;
    const int ge = live ? g : 0, col = a0 + (live ? lane - g * A : 0);
    const int n_it = (H + G - 1) / G;
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    for (int it0 = 0; it0 < n_it; it0 += MIX_BATCH) {
        float v[NR][MIX_BATCH], al[MIX_BATCH];
        bool ok[MIX_BATCH];
#pragma unroll
        for (int u = 0; u < MIX_BATCH; ++u) {
            const int h = (it0 + u) * G + ge;
            const int hc = min(h, H - 1);
            ok[u] = live && h < H;
            al[u] = s_alpha[hc];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float* p = row[r] + (int64_t)hc * A + col;
                ISDQN_BOUNDS_CHECK(p, 4, 55);
                v[r][u] = *p;
            }
        }
#pragma unroll
        for (int u = 0; u < MIX_BATCH; ++u)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float t = al[u] * v[r][u];
                // (the first product starts the partial; a masked pass leaves it alone, so that a lone -0.0 stays -0.0)
                acc[r] = (it0 + u == 0) ? (ok[u] ? t : 0.f) : (ok[u] ? acc[r] + t : acc[r]);
            }
    }
    // partial g of action a sits in lane a + g * A
    const int src = lane < width ? lane : 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float x = __shfl(acc[r], src);
        for (int k = 1; k < G && k < H; ++k) x += __shfl(acc[r], src + k * A);
        m[r] = x;
    }
}
__device__ __forceinline__ float mix_chunk(const float* __restrict__ row, const float* s_alpha, int a0, int A, int H, int lane) {
    const float* const rows[1] = {row};
    float m[1];
    mix_chunk<1>(rows, s_alpha, a0, A, H, lane, m);
    return m[0];
}

// (v, i) of every lane -> the largest v and, among equals, the lowest i, as lane 0 ends up holding them (a NaN can leave the lanes
// disagreeing: lane 0's answer is the wave's); lanes without a candidate pass -inf and INT_MAX
__device__ __forceinline__ void wave_argmax_first(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    v = __shfl(v, 0);
    i = __shfl(i, 0);
}

// Qmix(row, a) for one action, on every lane
__device__ __forceinline__ float mix_at(const float* __restrict__ row, const float* s_alpha, int a, int A, int H, int lane) {
    const int a0 = A <= 64 ? 0 : (a / 64) * 64;
    return __shfl(mix_chunk(row, s_alpha, a0, A, H, lane), (a - a0) & 63);
}

// first argmax_a Qmix(row, a) and its value, on every lane (strict >: the lowest index wins, across the chunks of A > 64 too)
__device__ __forceinline__ void mix_argmax(const float* __restrict__ row, const float* s_alpha, int A, int H, int lane, float& best_v, int& best_i) {
    best_v = 0.f;
    best_i = 0;
    for (int a0 = 0; a0 < A; a0 += 64) {
        const float m = mix_chunk(row, s_alpha, a0, A, H, lane);
        const bool has = lane < min(64, A - a0);
        float v = has ? m : -INFINITY;
        int i = has ? a0 + lane : 0x7fffffff;
        wave_argmax_first(v, i);
        i = min(max(i, 0), A - 1);
        if (a0 == 0 || v > best_v) { best_v = v; best_i = i; }
    }
}

__global__ __launch_bounds__(MIX_THREADS) void mix_td_kernel(const HeadLossArgs args, const float* __restrict__ alpha, int H) {
    ISDQN_EMPTY_KERNEL_RETURN
    const float *__restrict__ q = args.out, *__restrict__ vq = args.val, *__restrict__ sq = args.sel;
    const int B = args.B, A = args.A, pitch = args.pitch, sq_pitch = args.sel_pitch;
    const float huber_delta = args.huber_delta;
    float *__restrict__ dout = args.dout, *__restrict__ q_values = args.q_values, *__restrict__ targets = args.targets;
    float *__restrict__ loss_part = args.loss_part, *__restrict__ dbh_part = args.dbh_part;
    double* __restrict__ priorities = args.priorities;
    extern __shared__ float s_alpha[];                           // [H]
    __shared__ float s_g[TD_ROWS], s_td[TD_ROWS], s_lw[TD_ROWS];  // l'(d) w / B; l(d), unweighted; l(d) w  (rows past B: zeros)
    __shared__ int s_action[TD_ROWS];                             // (rows past B: -1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * TD_ROWS;
    const int rows = min(TD_ROWS, B - b0);
    const float inv_b = 1.f / (float)B;
    for (int h = tid; h < H; h += MIX_THREADS) {
        ISDQN_BOUNDS_CHECK(alpha + h, 4, 54);
        s_alpha[h] = alpha[h];
    }
    if (tid < TD_ROWS) {
        s_g[tid] = 0.f; s_td[tid] = 0.f; s_lw[tid] = 0.f;
        s_action[tid] = -1;
    }
    __syncthreads();
    for (int bl = wave; bl < rows; bl += MIX_WAVES) {  // a wave per transition
        const int b = b0 + bl;
        const int a = args.action[b];
        const float r = args.reward[b], nt = 1.f - (float)args.terminal[b];
        const float w = args.loss_weights != nullptr ? args.loss_weights[b] : 1.f;
        float gamma_n = args.gamma_n;
        if (args.discount != nullptr) {
            ISDQN_BOUNDS_CHECK(args.discount + b, 4, 56);
            gamma_n = args.discount[b];
        }
        const float* oq = q + (int64_t)b * pitch;
        const float* nq = vq + (int64_t)b * pitch;
        const float* sel = sq != nullptr ? sq + (int64_t)b * sq_pitch : nullptr;
        float qv, mx;
        int best;
        if (A <= 64) {  // one pass over the transition's two or three rows together
            float sv;
            if (sel != nullptr) {  // double_q: the selector rows pick under the same alpha, the value rows are read at that action
                const float* const rows[3] = {oq, nq, sel};
                float m[3];
                mix_chunk<3>(rows, s_alpha, 0, A, H, lane, m);
                qv = m[0]; mx = m[1]; sv = m[2];
            } else {
                const float* const rows[2] = {oq, nq};
                float m[2];
                mix_chunk<2>(rows, s_alpha, 0, A, H, lane, m);
                qv = m[0]; mx = sv = m[1];
            }
            qv = __shfl(qv, a & 63);
            sv = lane < A ? sv : -INFINITY;
            best = lane < A ? lane : 0x7fffffff;
            wave_argmax_first(sv, best);
            best = min(max(best, 0), A - 1);
            mx = __shfl(mx, best);
        } else {
            qv = mix_at(oq, s_alpha, a, A, H, lane);
            if (sel != nullptr) {
                float sv;
                mix_argmax(sel, s_alpha, A, H, lane, sv, best);
                mx = mix_at(nq, s_alpha, best, A, H, lane);
            } else {
                mix_argmax(nq, s_alpha, A, H, lane, mx, best);
            }
        }
        const float tg = r + nt * gamma_n * mx;
        const float d = qv - tg;
        const float td = td_loss(d, huber_delta);
        if (lane == 0) {
            if (q_values) q_values[b] = qv;
            if (targets) targets[b] = tg;
            s_g[bl] = td_dloss(d, huber_delta) * inv_b * w;
            s_td[bl] = td;  // unweighted: the priorities are the raw TD error
            s_lw[bl] = td * w;
            s_action[bl] = a;
        }
    }
    __syncthreads();  // s_g / s_td / s_lw / s_action complete
    if (wave == 0) {  // td_kernel's sum of its 64 lanes
        float sum = s_lw[lane];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) loss_part[blockIdx.x] = sum;
    }
    if (dout != nullptr) {
        // every element of the workgroup's dout rows is written once: fl32(alpha_h * g_b) on the taken action of each head, zero elsewhere
        for (int bl = wave; bl < rows; bl += MIX_WAVES) {
            const int a = s_action[bl];
            const float g = s_g[bl];
            for (int c = lane; c < pitch; c += 64) {
                const int h = c / A, aa = c - h * A;
                dout[(int64_t)(b0 + bl) * pitch + c] = (h < H && aa == a) ? s_alpha[h] * g : 0.f;
            }
        }
        // column sums over the workgroup's rows in ascending row, as td_kernel forms them
        for (int c = tid; c < pitch; c += MIX_THREADS) {
            const int h = c / A, aa = c - h * A;
            float sum = 0.f;
            if (h < H) {
                const float al = s_alpha[h];
                for (int bl = 0; bl < rows; ++bl) sum += (s_action[bl] == aa) ? al * s_g[bl] : 0.f;  // (the rows past B would add +0)
            }
            dbh_part[(int64_t)blockIdx.x * pitch + c] = sum;
        }
    }
    if (priorities != nullptr && tid < rows) priorities[b0 + tid] = sqrt((double)(s_td[tid] / 1.f) + 1e-10);
}

// isdqn_net_best_actions with ISDQN_ACT_MEAN_HEADS: row i -> first argmax_a of sum_h q[i][h * A + a], fp32 in ascending h.  Four waves
// per workgroup, a wave per row, a lane per action (A > 64: in chunks of 64, lowest index kept across them).
__global__ __launch_bounds__(MIX_ACT_THREADS) void argmax_mean_rows_kernel(const float* __restrict__ q, int n_rows, int nha_p, int A, int H,
                                                                          int* __restrict__ out) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (MIX_ACT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_rows) return;  // (wave-uniform)
    const float* __restrict__ row = q + (int64_t)i * nha_p;
    float best_v = 0.f;
    int best_i = 0;
    for (int a0 = 0; a0 < A; a0 += 64) {
        const bool has = a0 + lane < A;
        float s = 0.f;
        if (has)
            for (int h = 0; h < H; ++h) {
                ISDQN_BOUNDS_CHECK(row + (int64_t)h * A + a0 + lane, 4, 57);
                s += row[(int64_t)h * A + a0 + lane];
            }
        float v = has ? s : -INFINITY;
        int idx = has ? a0 + lane : 0x7fffffff;
        wave_argmax_first(v, idx);
        idx = min(max(idx, 0), A - 1);
        if (a0 == 0 || v > best_v) { best_v = v; best_i = idx; }
    }
    if (lane == 0) out[i] = best_i;
}

__global__ void mixture_advance_kernel(int64_t* __restrict__ draw_count) {
    ISDQN_EMPTY_KERNEL_RETURN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ISDQN_BOUNDS_CHECK(draw_count, 8, 53);
        *draw_count = *draw_count + 1;
    }
}

int launch_mixture_draw(int H, uint64_t seed, int64_t* draw_count, float* alpha, hipStream_t st) {
    hipLaunchKernelGGL(mixture_draw_kernel, dim3(1), dim3(MIX_MAX_HEADS), 0, st, H, (uint32_t)seed, (uint32_t)(seed >> 32), (const int64_t*)draw_count,
                       alpha);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mixture_advance_kernel, dim3(1), dim3(64), 0, st, draw_count);  // (count + 1: one thread, an ordinary store, behind the reader)
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_mix_td(const HeadLossArgs& a, int n_blk, const float* alpha, int H, hipStream_t st) {
    ISDQN_REQUIRE(H >= 1 && H <= MIX_MAX_HEADS && n_blk == ceil_div(a.B, TD_ROWS) && (int64_t)H * a.A <= a.pitch, ISDQN_ERR_SHAPE,
                  "mixture: heads, row partition or row pitch outside what the kernel walks");
    hipLaunchKernelGGL(mix_td_kernel, dim3(n_blk), dim3(MIX_THREADS), (size_t)H * sizeof(float), st, a, alpha, H);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_argmax_mean(const float* q, int n_rows, int nha_p, int A, int H, int* out, hipStream_t st) {
    ISDQN_REQUIRE(n_rows >= 1 && (int64_t)H * A <= nha_p, ISDQN_ERR_SHAPE, "mean-heads argmax: the heads' columns exceed the row pitch");
    hipLaunchKernelGGL(argmax_mean_rows_kernel, dim3(ceil_div(n_rows, MIX_ACT_THREADS / 64)), dim3(MIX_ACT_THREADS), 0, st, q, n_rows, nha_p, A, H, out);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

}  // namespace isdqn

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build: the byte extents [lo[i], hi[i]) the mixture's kernels may read, and the first load outside all of
// them (tests/test_gpu_mixture_bounds.py); this object's own table, as prune_kernels.hip has one.
extern "C" int isdqn_debug_mixture_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_mixture_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif
