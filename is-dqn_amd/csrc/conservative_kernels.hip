// The conservative (CQL) term beside the head losses, on gfx950 (Kumar et al., "Conservative Q-Learning for Offline Reinforcement
// Learning", NeurIPS 2020); THE definition is include/isdqn_hip.h, isdqn_batch_conservative:
//   c_bk = m + log(sum_a exp(Q_a - m)) - Q_{a_b},  dL/d(output of (h, a')) += alpha w_b / B (softmax_a Q - 1{a' = a_b}) dQ_a'/d(output).
// A translation unit of its own: the four pinned code objects keep their kernels and their order.  loss_and_finalize (net_launch.h)
// calls launch_conservative behind the loss kernel of a call and in front of loss_finalize_kernel, with that loss kernel's row
// partition, so a workgroup here owns the dout rows, the loss_part row and the dbh_part row the same workgroup of the loss kernel
// wrote: one owner per address, read-modify-write in a fixed order, no atomics, bit-identical from run to run.
//   cql_scalar_kernel  scalar heads: the 64 transitions of td_kernel's workgroup along the lanes, wave w takes pairs k = w, w + 4, ...;
//                      a lane walks the A values of its row three times (maximum, sum of exponentials, gradient): no shuffle but the
//                      loss sum's butterfly.
//   cql_dist_kernel    quantile / histogram heads: one wave per (transition, pair), lanes along the outputs of one action
//                      (lane + 64 t), the A action values of the pair staged in the wave's own slot of LDS.
// Both end with the column sums of the workgroup's NEW dout rows over the regressed heads, rows ascending: the head-bias gradient is
// the column sum of what the head's weight gradient multiplies.
#include "conservative.h"

#ifndef ISDQN_BOUNDS_CHECK
#define ISDQN_BOUNDS_CHECK(p, bytes, site) ((void)0)  // (gemm_core.h's checked loads are the four pinned objects')
#endif
#include "head_loss.h"  // wave_sum / wave_max, MAX_ROWS, MAX_GROUP, PER_LANE

namespace isdqn {

constexpr int CQL_SCALAR_ROWS = 64;   // td_kernel's TD_ROWS: one transition per lane
constexpr int CQL_WAVES = 16;         // cql_dist_kernel: a pair is a chain of A dependent reductions, as in qr_loss_kernel
constexpr int CQL_THREADS = 64 * CQL_WAVES;
constexpr int CQL_DIST_MAX_ACTIONS = 960;  // 16 waves x 960 action values: 60 KB of LDS beside s_c

// column sums of the workgroup's dout rows over the regressed heads' `width` columns from column `c0` on, rows ascending
template <int THREADS>
__device__ __forceinline__ void cql_column_sums(const float* dout, float* __restrict__ dbh_part, int b0, int rows, int pitch, int c0, int width) {
    for (int c = threadIdx.x; c < width; c += THREADS) {
        float sum = 0.f;
        for (int bl = 0; bl < rows; ++bl) sum += dout[(int64_t)(b0 + bl) * pitch + c0 + c];
        dbh_part[(int64_t)blockIdx.x * pitch + c0 + c] = sum;
    }
}

__global__ __launch_bounds__(256) void cql_scalar_kernel(const ConservativeArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    const float* __restrict__ q = a.out;
    float* dout = a.dout;
    float* __restrict__ loss_part = a.loss_part;
    const int B = a.B, K = a.K, A = a.A, pitch = a.pitch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * a.rows_per_blk;
    const int rows = min(a.rows_per_blk, B - b0);
    const bool on = lane < rows;
    const int b = b0 + lane;
    int act = 0;
    float w = 1.f;
    if (on) {
        act = a.action[b];
        if (a.loss_weights != nullptr) w = a.loss_weights[b];
    }
    const float aw = __fmul_rn(a.alpha, w);
    const float coef = aw / (float)B;
    for (int k = wave; k < K; k += 4) {
        float lc = 0.f;
        if (on) {
            const int64_t off = (int64_t)b * pitch + (int64_t)(a.on0 + k) * A;
            const float* __restrict__ row = q + off;
            float m = row[0];
            for (int j = 1; j < A; ++j) m = fmaxf(m, row[j]);
            float s = 0.f;
            for (int j = 0; j < A; ++j) s += expf(row[j] - m);
            const float c = (m + logf(s)) - row[act];
            lc = __fmul_rn(aw, c);
            if (dout != nullptr) {
                float* d = dout + off;
                for (int j = 0; j < A; ++j) {
                    const float pi = expf(row[j] - m) / s;
                    const float t = __fmul_rn(coef, pi - (j == act ? 1.f : 0.f));
                    d[j] = __fadd_rn(d[j], t);
                }
            }
        }
        lc = wave_sum(lc);  // (lanes past the workgroup's rows: 0)
        if (lane == 0) loss_part[(int64_t)blockIdx.x * K + k] = __fadd_rn(loss_part[(int64_t)blockIdx.x * K + k], lc);
    }
    if (dout == nullptr) return;
    __syncthreads();  // every wave's dout rows are written
    cql_column_sums<256>(dout, a.dbh_part, b0, rows, pitch, a.on0 * A, K * A);
}

// Q of one action of a quantile head: qr_reduce's order (the lane's own values in ascending t, the butterfly, one division)
__device__ __forceinline__ float cql_quantile_mean(const float* __restrict__ th, int N, int lane) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int i = lane + 64 * t;
        s += i < N ? th[i] : 0.f;
    }
    return wave_sum(s) / (float)N;
}
// Q of one action of a histogram head, hl_softmax_parts' order: e[t] = exp(l_j - max) (0 past nb), *sum = sum_j e_j; returns
// sum_j e_j z_j / sum_j e_j with z_j = vmin + (j + 1/2) eta.  Every lane ends with the same values.
__device__ __forceinline__ float cql_histogram_q(const float* __restrict__ l, int nb, int lane, float vmin, float eta, float (&e)[PER_LANE],
                                                 float* sum) {
    float v[PER_LANE];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int j = lane + 64 * t;
        v[t] = j < nb ? l[j] : -INFINITY;
        m = fmaxf(m, v[t]);
    }
    m = wave_max(m);
    float s = 0.f, ws = 0.f;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int j = lane + 64 * t;
        e[t] = j < nb ? expf(v[t] - m) : 0.f;
        s += e[t];
        ws += e[t] * (vmin + ((float)j + 0.5f) * eta);
    }
    *sum = wave_sum(s);
    return wave_sum(ws) / *sum;
}

template <bool QR>
__global__ __launch_bounds__(CQL_THREADS) void cql_dist_kernel(const ConservativeArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    extern __shared__ float s_q[];                     // [CQL_WAVES][A]: the action values of the pair a wave is at
    __shared__ float s_c[MAX_ROWS * CQL_MAX_PAIRS];    // [R][K]: alpha w_b c_bk (0 on padded rows)
    const float* __restrict__ out = a.out;
    float* dout = a.dout;
    float* __restrict__ loss_part = a.loss_part;
    const int B = a.B, R = a.rows_per_blk, K = a.K, A = a.A, nb = a.nb, pitch = a.pitch;
    const float vmin = a.vmin, eta = a.eta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const int ldk = A * nb;  // outputs of one head
    float* sq = s_q + wave * A;
    for (int pr = wave; pr < R * K; pr += CQL_WAVES) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) s_c[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const int act = a.action[b];
        const float w = a.loss_weights != nullptr ? a.loss_weights[b] : 1.f;
        const float aw = __fmul_rn(a.alpha, w);
        const int64_t off = (int64_t)b * pitch + (int64_t)(a.on0 + k) * ldk;
        const float* __restrict__ hrow = out + off;
        float e[PER_LANE], se;
        for (int a2 = 0; a2 < A; ++a2) {
            const float qv = QR ? cql_quantile_mean(hrow + (int64_t)a2 * nb, nb, lane) : cql_histogram_q(hrow + (int64_t)a2 * nb, nb, lane, vmin, eta, e, &se);
            if (lane == 0) sq[a2] = qv;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float m = -INFINITY;
        for (int j = lane; j < A; j += 64) m = fmaxf(m, sq[j]);
        m = wave_max(m);
        float s = 0.f;
        for (int j = lane; j < A; j += 64) s += expf(sq[j] - m);
        s = wave_sum(s);
        const float c = (m + logf(s)) - sq[act];
        if (lane == 0) s_c[pr] = __fmul_rn(aw, c);
        if (dout != nullptr) {
            const float coef = aw / (float)B;
            float* d = dout + off;
            for (int a2 = 0; a2 < A; ++a2) {
                const float qa = sq[a2];
                const float pi = expf(qa - m) / s;
                const float g = __fmul_rn(coef, pi - (a2 == act ? 1.f : 0.f));
                if (QR) {
                    const float t = g / (float)nb;
#pragma unroll
                    for (int tt = 0; tt < PER_LANE; ++tt) {
                        const int i = lane + 64 * tt;
                        if (i < nb) d[(int64_t)a2 * nb + i] = __fadd_rn(d[(int64_t)a2 * nb + i], t);
                    }
                } else {
                    cql_histogram_q(hrow + (int64_t)a2 * nb, nb, lane, vmin, eta, e, &se);  // (the bits of the first pass)
#pragma unroll
                    for (int tt = 0; tt < PER_LANE; ++tt) {
                        const int j = lane + 64 * tt;
                        if (j < nb) {
                            const float z = vmin + ((float)j + 0.5f) * eta;
                            const float dq = __fmul_rn(e[tt] / se, z - qa);
                            d[(int64_t)a2 * nb + j] = __fadd_rn(d[(int64_t)a2 * nb + j], __fmul_rn(g, dq));
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the slot is read out before the wave's next pair overwrites it
    }
    __syncthreads();  // s_c complete, every wave's dout rows written
    for (int k = threadIdx.x; k < K; k += CQL_THREADS) {
        float sum = 0.f;
        for (int bl = 0; bl < R; ++bl) sum += s_c[bl * K + k];
        loss_part[(int64_t)blockIdx.x * K + k] = __fadd_rn(loss_part[(int64_t)blockIdx.x * K + k], sum);
    }
    if (dout != nullptr) cql_column_sums<CQL_THREADS>(dout, a.dbh_part, b0, rows, pitch, a.on0 * ldk, K * ldk);
}

int launch_conservative(const ConservativeArgs& a, hipStream_t st) {
    ISDQN_REQUIRE(a.out && a.loss_part && a.action && (a.dout == nullptr || a.dbh_part != nullptr), ISDQN_ERR_ARG, "conservative term: null pointer");
    ISDQN_REQUIRE(a.alpha > 0.f && a.alpha <= 3.4028234e38f, ISDQN_ERR_ARG, "conservative term: cql_alpha must be finite and > 0 here");
    ISDQN_REQUIRE(a.B >= 1 && a.K >= 1 && a.A >= 1 && a.on0 >= 0 && a.nb >= 0 && a.rows_per_blk >= 1 && a.n_blk >= 1, ISDQN_ERR_SHAPE,
                  "conservative term: empty shape");
    ISDQN_REQUIRE(a.K <= CQL_MAX_PAIRS, ISDQN_ERR_UNSUPPORTED, "the conservative term is built for at most 64 regressed pairs");
    const int width = a.nb > 0 ? a.nb : 1;
    // every row and column the grid touches lies inside what the plan reports
    ISDQN_REQUIRE((int64_t)a.n_blk * a.rows_per_blk >= a.B && (int64_t)(a.n_blk - 1) * a.rows_per_blk < a.B, ISDQN_ERR_SHAPE,
                  "conservative term: the row partition does not cover the batch exactly");
    ISDQN_REQUIRE((int64_t)(a.on0 + a.K) * a.A * width <= a.pitch, ISDQN_ERR_SHAPE, "conservative term: regressed heads outside the head-output rows");
    ISDQN_REQUIRE(a.dout == nullptr || (int64_t)a.B * a.pitch <= a.dout_floats, ISDQN_ERR_SHAPE, "conservative term: rows outside the dout region");
    ISDQN_REQUIRE((int64_t)a.n_blk * ((int64_t)a.K + a.pitch) <= a.part_floats, ISDQN_ERR_SHAPE,
                  "conservative term: partial rows outside the loss_partials region");
    ISDQN_REQUIRE(a.dbh_part == nullptr || a.dbh_part == a.loss_part + (int64_t)a.n_blk * a.K, ISDQN_ERR_SHAPE,
                  "conservative term: dbh_part does not follow loss_part");
    if (a.nb == 0) {
        ISDQN_REQUIRE(a.rows_per_blk <= CQL_SCALAR_ROWS, ISDQN_ERR_UNSUPPORTED, "conservative term: more than 64 transitions per workgroup");
        hipLaunchKernelGGL(cql_scalar_kernel, dim3(a.n_blk), dim3(256), 0, st, a);
    } else {
        ISDQN_REQUIRE(a.rows_per_blk <= MAX_ROWS && a.nb <= MAX_GROUP, ISDQN_ERR_UNSUPPORTED,
                      "conservative term: more transitions per workgroup or outputs per action than the distributional kernels take");
        ISDQN_REQUIRE(a.A <= CQL_DIST_MAX_ACTIONS, ISDQN_ERR_UNSUPPORTED, "conservative term on histogram / quantile heads: at most 960 actions");
        const size_t lds = (size_t)CQL_WAVES * a.A * sizeof(float);
        if (a.quantile) hipLaunchKernelGGL(cql_dist_kernel<true>, dim3(a.n_blk), dim3(CQL_THREADS), lds, st, a);
        else hipLaunchKernelGGL(cql_dist_kernel<false>, dim3(a.n_blk), dim3(CQL_THREADS), lds, st, a);
    }
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

}  // namespace isdqn
