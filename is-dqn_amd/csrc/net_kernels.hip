// iS-DQN Q-network on gfx950: forward over the 1+K shared heads, iterated Bellman target, squared TD
// loss, backward and Adam.  Reference: slimdqn/networks/architectures/dqn.py:47-103 and
// slimdqn/networks/isdqn.py:82-135.  Contractions run on the MFMA tile engine (gemm_core.h,
// net_problems.h); the row-wise kernels below are the HBM-bound remainder.
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>
#include <atomic>

#include "conv_img.h"
#include "conv_u8_pair.h"
#include "conv_s8_pair.h"
#include "head_loss.h"
#include "munchausen.h"
#include "hl_gauss.h"
#include "quantile.h"
#include "categorical.h"
#include "redo.h"
#include "dueling.h"
#include "net_plan.h"
#include "net_problems.h"

namespace isdqn {

// b^t for the Adam bias corrections 1 - b^t (optax.adam, isdqn.py:46): exponentiation by squaring, at most 62 double
// multiplies (relative error ~1e-15).  The library pow() is thousands of instructions on ONE lane -- 10-20 us -- and
// the kernel that owns the step counter lasts as long as that lane.
__device__ inline double pow_int(double b, int t) {
    double r = 1.0, x = b;
    for (unsigned u = (unsigned)t; u != 0; u >>= 1) {
        if (u & 1u) r *= x;
        x *= x;
    }
    return r;
}

// =============================================================================================
// Row-wise kernels
// =============================================================================================

// Dense layer tail (dqn.py:96-99): sum the split-K slabs, add the bias, LayerNorm over the row,
// ReLU.  One workgroup per row; the row is staged in LDS between the two passes.
__global__ __launch_bounds__(256) void dense_post_kernel(const float* __restrict__ slabs, int n_slabs,
                                                         int64_t slab_stride, int64_t row_pitch, int rows, int F, int Fp,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int has_relu,
                                                         float* __restrict__ act, float* __restrict__ z, int z_rows, int act_s8) {
    extern __shared__ float s_row[];  // [3][Fp]: the summed row, gamma, beta
    __shared__ float s_red[2][4];
    const int row = blockIdx.x, tid = threadIdx.x;
    float* s_g = s_row + Fp;
    float* s_b = s_row + 2 * Fp;
    float s1 = 0.f, s2 = 0.f;
    // two adjacent columns per thread (Fp is a multiple of 8: 8-byte loads), 16 slabs in flight, fixed summation order.
    // bias / gamma / beta of the two columns are requested FIRST and travel under the slab loads: a workgroup lives
    // for a few microseconds, and three dependent round trips behind the sums were a third of that.
    for (int c = 2 * tid; c < Fp; c += 512) {
        float par[3][2];
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const float* src = w == 0 ? bias : w == 1 ? gamma : beta;
#pragma unroll
            for (int e = 0; e < 2; ++e)
            {
                ISDQN_BOUNDS_CHECK((src != nullptr && c + e < F) ? src + c + e : zero_chunk(), 4, 28);
                par[w][e] = *(const ISDQN_GLOBAL float*)((src != nullptr && c + e < F) ? src + c + e : zero_chunk());
            }
        }
        float v0 = 0.f, v1 = 0.f;
        const float* p = slabs + (int64_t)row * row_pitch + c;
        int s = 0;
        for (; s + 16 <= n_slabs; s += 16) {
            float2 t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = *reinterpret_cast<const float2*>(p + (int64_t)(s + u) * slab_stride);
#pragma unroll
            for (int u = 0; u < 16; ++u) { v0 += t[u].x; v1 += t[u].y; }
        }
        if (s < n_slabs) {
            float2 t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)  // tail: clamped to the last slab, masked in the sum
                t[u] = *reinterpret_cast<const float2*>(p + (int64_t)min(s + u, n_slabs - 1) * slab_stride);
#pragma unroll
            for (int u = 0; u < 16; ++u) { v0 += (s + u < n_slabs) ? t[u].x : 0.f; v1 += (s + u < n_slabs) ? t[u].y : 0.f; }
        }
        v0 = c < F ? v0 + par[0][0] : 0.f;
        v1 = c + 1 < F ? v1 + par[0][1] : 0.f;
        s_row[c] = v0;
        s_row[c + 1] = v1;
        s_g[c] = par[1][0]; s_g[c + 1] = par[1][1];
        s_b[c] = par[2][0]; s_b[c + 1] = par[2][1];
        s1 += v0 + v1;
        s2 += v0 * v0 + v1 * v1;
    }
    float mean = 0.f, rstd = 1.f;
    if (gamma != nullptr) {
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
        }
        if ((tid & 63) == 0) {
            s_red[0][tid >> 6] = s1;
            s_red[1][tid >> 6] = s2;
        }
        __syncthreads();
        s1 = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        s2 = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        mean = s1 / (float)F;
        float var = fmaxf(s2 / (float)F - mean * mean, 0.f);
        rstd = rsqrtf(var + 1e-6f);
    }
    for (int c0 = 2 * tid; c0 < Fp; c0 += 512) {
        float y2[2], v2[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = c0 + e;
            const float v = s_row[c];  // (row, gamma, beta: written by this same thread)
            float y = v;
            if (gamma != nullptr && c < F) y = (v - mean) * (rstd * s_g[c]) + s_b[c];
            if (has_relu) y = fmaxf(y, 0.f);
            if (c >= F) y = 0.f;
            y2[e] = y; v2[e] = v;
        }
        if (act_s8) s8_store_pair(act + (int64_t)row * Fp, c0, y2[0], y2[1]);  // hidden activations: S8; the head's q stays fp32
        else *reinterpret_cast<float2*>(act + (int64_t)row * Fp + c0) = make_float2(y2[0], y2[1]);
        if (row < z_rows) *reinterpret_cast<float2*>(z + (int64_t)row * Fp + c0) = make_float2(v2[0], v2[1]);
    }
}

// LayerNorm + ReLU backward over the last axis (rows x C, C <= 4*TPR), TPR lanes per row, float4 per lane.
//   xhat = (z-mean)*rstd ; y = xhat*gamma+beta ; dy = da*[y>0] ; dgamma += dy*xhat ; dbeta += dy
//   g = dy*gamma ; dz = rstd*(g - mean(g) - xhat*mean(g*xhat)) ; dbias += dz
// Per-workgroup partial sums go to part[block][3][Cp] (deterministic; reduced by the Adam kernel).
template <int TPR>
__global__ __launch_bounds__(256) void ln_bwd_small_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int rows, int C, int Cp,
                                                           float* __restrict__ dz, float* __restrict__ part) {
    constexpr int RPB = 256 / TPR;
    __shared__ float s_part[RPB][3][4 * TPR];
    const int tid = threadIdx.x, grp = tid / TPR, sub = tid % TPR;
    const int ch0 = sub * 4;
    const bool lane_on = ch0 < Cp;
    float ga[4], be[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bool ok = lane_on && (ch0 + r) < C;
        ga[r] = (ok && gamma) ? gamma[ch0 + r] : 1.f;
        be[r] = (ok && gamma) ? beta[ch0 + r] : 0.f;
    }
    float dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0}, dbias[4] = {0, 0, 0, 0};
    const float inv_c = 1.f / (float)C;
    for (int row0 = blockIdx.x * RPB; row0 < rows; row0 += gridDim.x * RPB) {
        const int row = row0 + grp;
        const bool on = lane_on && row < rows;
        float zv[4] = {0, 0, 0, 0}, dv[4] = {0, 0, 0, 0};
        if (on) {
            float4 a = *reinterpret_cast<const float4*>(z + (int64_t)row * Cp + ch0);
            float4 b = *reinterpret_cast<const float4*>(da + (int64_t)row * Cp + ch0);
            zv[0] = a.x; zv[1] = a.y; zv[2] = a.z; zv[3] = a.w;
            dv[0] = b.x; dv[1] = b.y; dv[2] = b.z; dv[3] = b.w;
        }
        float out[4];
        if (gamma != nullptr) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool ok = (ch0 + r) < C;
                s1 += ok ? zv[r] : 0.f;
                s2 += ok ? zv[r] * zv[r] : 0.f;
            }
#pragma unroll
            for (int off = TPR / 2; off > 0; off >>= 1) {
                s1 += __shfl_xor(s1, off);
                s2 += __shfl_xor(s2, off);
            }
            float mean = s1 * inv_c;
            float rstd = rsqrtf(fmaxf(s2 * inv_c - mean * mean, 0.f) + 1e-6f);
            float xh[4], gg[4], m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool ok = on && (ch0 + r) < C;
                xh[r] = (zv[r] - mean) * rstd;
                float y = xh[r] * ga[r] + be[r];
                float dy = (ok && y > 0.f) ? dv[r] : 0.f;
                dg[r] += dy * xh[r];
                db[r] += dy;
                gg[r] = dy * ga[r];
                m1 += gg[r];
                m2 += gg[r] * xh[r];
            }
#pragma unroll
            for (int off = TPR / 2; off > 0; off >>= 1) {
                m1 += __shfl_xor(m1, off);
                m2 += __shfl_xor(m2, off);
            }
            m1 *= inv_c;
            m2 *= inv_c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool ok = on && (ch0 + r) < C;
                out[r] = ok ? rstd * (gg[r] - m1 - xh[r] * m2) : 0.f;
                dbias[r] += out[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool ok = on && (ch0 + r) < C;
                out[r] = (ok && zv[r] > 0.f) ? dv[r] : 0.f;
                dbias[r] += out[r];
            }
        }
        if (on) s8_store_quad(dz + (int64_t)row * Cp, ch0, out[0], out[1], out[2], out[3]);  // dz: S8
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s_part[grp][0][ch0 + r] = dg[r];
        s_part[grp][1][ch0 + r] = db[r];
        s_part[grp][2][ch0 + r] = dbias[r];
    }
    __syncthreads();
    for (int i = tid; i < 3 * Cp; i += 256) {
        int which = i / Cp, c = i % Cp;
        float s = 0.f;
        for (int g2 = 0; g2 < RPB; ++g2) s += s_part[g2][which][c];
        part[((int64_t)blockIdx.x * 3 + which) * Cp + c] = s;
    }
}

// Same, wide rows (dense layers): one workgroup per row at a time, columns strided over the threads.
constexpr int LN_WIDE_MAX_COLS = 16;  // per thread: widths up to 4096
__global__ __launch_bounds__(256) void ln_bwd_wide_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int rows, int C, int Cp,
                                                          float* __restrict__ dz, float* __restrict__ part) {
    __shared__ float s_red[4][4];
    const int tid = threadIdx.x;
    float dg[LN_WIDE_MAX_COLS], db[LN_WIDE_MAX_COLS], dbias[LN_WIDE_MAX_COLS];
#pragma unroll
    for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) dg[i] = db[i] = dbias[i] = 0.f;
    const float inv_c = 1.f / (float)C;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* zr = z + (int64_t)row * Cp;
        const float* dr = da + (int64_t)row * Cp;
        float* outr = dz + (int64_t)row * Cp;
        if (gamma != nullptr) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) {
                int c = tid + i * 256;
                if (c < C) {
                    float v = zr[c];
                    s1 += v;
                    s2 += v * v;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                s1 += __shfl_xor(s1, off);
                s2 += __shfl_xor(s2, off);
            }
            __syncthreads();
            if ((tid & 63) == 0) { s_red[0][tid >> 6] = s1; s_red[1][tid >> 6] = s2; }
            __syncthreads();
            s1 = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
            s2 = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
            float mean = s1 * inv_c;
            float rstd = rsqrtf(fmaxf(s2 * inv_c - mean * mean, 0.f) + 1e-6f);
            float m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) {
                int c = tid + i * 256;
                if (c < C) {
                    float xh = (zr[c] - mean) * rstd;
                    float y = xh * gamma[c] + beta[c];
                    float dy = y > 0.f ? dr[c] : 0.f;
                    dg[i] += dy * xh;
                    db[i] += dy;
                    float g2 = dy * gamma[c];
                    m1 += g2;
                    m2 += g2 * xh;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                m1 += __shfl_xor(m1, off);
                m2 += __shfl_xor(m2, off);
            }
            if ((tid & 63) == 0) { s_red[2][tid >> 6] = m1; s_red[3][tid >> 6] = m2; }
            __syncthreads();
            m1 = (s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3]) * inv_c;
            m2 = (s_red[3][0] + s_red[3][1] + s_red[3][2] + s_red[3][3]) * inv_c;
#pragma unroll
            for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) {
                int c = tid + i * 256;
                if (c < Cp) {
                    float o = 0.f;
                    if (c < C) {
                        float xh = (zr[c] - mean) * rstd;
                        float y = xh * gamma[c] + beta[c];
                        float dy = y > 0.f ? dr[c] : 0.f;
                        o = rstd * (dy * gamma[c] - m1 - xh * m2);
                    }
                    dbias[i] += o;
                    s8_store_elem(outr, c, o);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) {
                int c = tid + i * 256;
                if (c < Cp) {
                    float o = (c < C && zr[c] > 0.f) ? dr[c] : 0.f;
                    dbias[i] += o;
                    s8_store_elem(outr, c, o);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < LN_WIDE_MAX_COLS; ++i) {
        int c = tid + i * 256;
        if (c < Cp) {
            float* p = part + (int64_t)blockIdx.x * 3 * Cp;
            p[c] = dg[i];
            p[Cp + c] = db[i];
            p[2 * Cp + c] = dbias[i];
        }
    }
}

// Iterated Bellman target + squared TD loss (isdqn.py:92-109); the arguments and THE contract of what it writes: head_loss.h.
//   q_k(s,a) from head 1+k of the online rows, target_k = r + (1-terminal)*gamma^n*max_a' Q_k(s',a')
//   from head k of the next-state rows (same parameters, stop-gradient), td = (q - target)^2.
// One workgroup per 64 transitions, wave w takes heads k = w, w+4, ...  Emits dL/dq rows (dout),
// q_values/targets/priorities and per-workgroup partials of the per-head loss sums and of the head
// bias gradient (column sums of dout); loss_finalize_kernel reduces them in a fixed order.
// `vq` (args.val): the value rows of the B next states (pitch nha_p; rows [B, 2B) of `q`, or the target network's own rows).  `sq` != null:
// Double Q-learning (isdqn_net_config::double_q) -- the value is taken at the first argmax of head sh + k of the selector rows
// (pitch sq_pitch; they may come from another forward than the value rows); null: the max form.  `mq` != null: Munchausen targets
// (munchausen.h) -- the value head th + k (mh + k in `mq`) of the STATE rows `mq` (pitch mq_pitch; rows [0, B) of `q`, or the target
// network's own rows) supplies the bonus, and the bootstrap value is the soft value of the value rows; null: off.
// Per-element loss and its derivative w.r.t. q for d = q - target: squared error (the reference, isdqn.py:102) or, with
// huber_delta > 0, the Huber loss (0.5 d^2 inside, delta (|d| - delta / 2) outside; derivative clip(d, -delta, delta)).
__device__ __forceinline__ float td_loss(float d, float huber_delta) {
    const float a = fabsf(d);
    return huber_delta > 0.f ? (a <= huber_delta ? 0.5f * d * d : huber_delta * (a - 0.5f * huber_delta)) : d * d;
}
__device__ __forceinline__ float td_dloss(float d, float huber_delta) {
    return huber_delta > 0.f ? fminf(fmaxf(d, -huber_delta), huber_delta) : 2.f * d;
}
// first index attaining the maximum of v[0..n): strict >, the lowest index wins (argmax_kernel's rule)
__device__ __forceinline__ int argmax_first(const float* v, int n) {
    int best = 0;
    float bv = v[0];
    for (int j = 1; j < n; ++j) {
        const float x = v[j];
        if (x > bv) { bv = x; best = j; }
    }
    return best;
}
constexpr int TD_ROWS = 64;
__global__ __launch_bounds__(256) void td_kernel(const HeadLossArgs args) {
    const float *__restrict__ q = args.out, *__restrict__ vq = args.val, *__restrict__ sq = args.sel, *mq = args.mun;
    const int sq_pitch = args.sel_pitch, sh = args.sel_head, mq_pitch = args.mun_pitch, mh = args.mun_head;
    const Munchausen mu = args.mu;
    const int B = args.B, K = args.K, oh = args.on0, th = args.tg0, A = args.A, nha_p = args.pitch;
    const int* __restrict__ action = args.action;
    const uint8_t* __restrict__ terminal = args.terminal;
    const float *__restrict__ reward = args.reward, *__restrict__ loss_weights = args.loss_weights;
    const float* __restrict__ discount = args.discount;
    const float huber_delta = args.huber_delta;
    float *__restrict__ dout = args.dout, *__restrict__ q_values = args.q_values, *__restrict__ targets = args.targets;
    float *__restrict__ loss_part = args.loss_part, *__restrict__ dbh_part = args.dbh_part;
    double* __restrict__ priorities = args.priorities;
    extern __shared__ float s_d[];  // [TD_ROWS][K] : 2*(q-target)/B ; then [TD_ROWS][K] td
    __shared__ int s_action[TD_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * TD_ROWS;
    const int b = b0 + lane;
    const bool on = b < B;
    float* s_td = s_d + TD_ROWS * K;
    const float inv_b = 1.f / (float)B;
    if (dout != nullptr) {
        const int rows = min(TD_ROWS, B - b0);
        for (int i = tid; i < rows * nha_p; i += 256) dout[(int64_t)b0 * nha_p + i] = 0.f;
    }
    int a = 0;
    float r = 0.f, nt = 0.f, w = 1.f;  // w: importance-sampling weight of the transition (isdqn_batch.loss_weights; none: 1)
    float gamma_n = args.gamma_n;      // the transition's discount (isdqn_batch_discount::discount; none: cfg->gamma_n)
    if (on) {
        a = action[b];
        r = reward[b];
        nt = 1.f - (float)terminal[b];
        if (loss_weights != nullptr) w = loss_weights[b];
        if (discount != nullptr) {
            ISDQN_BOUNDS_CHECK(discount + b, 4, 50);
            gamma_n = discount[b];
        }
    }
    if (wave == 0) s_action[lane] = on ? a : -1;
    for (int k = wave; k < K; k += 4) {
        float d = 0.f, td = 0.f;
        if (on) {
            float qv = q[(int64_t)b * nha_p + (oh + k) * A + a];
            const float* nq = vq + (int64_t)b * nha_p + (th + k) * A;
            float mx = nq[0];
            if (sq != nullptr) {
                const float* sel = sq + (int64_t)b * sq_pitch + (sh + k) * A;
                ISDQN_BOUNDS_CHECK(sel, 4 * A, 30);
                ISDQN_BOUNDS_CHECK(nq, 4 * A, 30);
                mx = nq[argmax_first(sel, A)];
            } else {
                for (int j = 1; j < A; ++j) mx = fmaxf(mx, nq[j]);
            }
            float tg = r + nt * gamma_n * mx;
            if (mq != nullptr) {
                const float* sv = mq + (int64_t)b * mq_pitch + (mh + k) * A;
                ISDQN_BOUNDS_CHECK(sv, 4 * A, 31);
                ISDQN_BOUNDS_CHECK(nq, 4 * A, 31);
                tg = munchausen_target(r, nt, gamma_n, sv[a], soft_value(sv, A, mu.tau), soft_value(nq, A, mu.tau), mu);
            }
            d = qv - tg;
            td = td_loss(d, huber_delta);
            if (q_values) q_values[(int64_t)b * K + k] = qv;
            if (targets) targets[(int64_t)b * K + k] = tg;
        }
        s_d[lane * K + k] = td_dloss(d, huber_delta) * inv_b * w;
        s_td[lane * K + k] = td;  // unweighted: the priorities are the raw TD error
        float sum = td * w;
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) loss_part[(int64_t)blockIdx.x * K + k] = sum;
    }
    __syncthreads();  // dout zero-fill (this workgroup's rows) and s_d / s_td complete
    if (dout != nullptr) {
        for (int i = tid; i < TD_ROWS * K; i += 256) {
            int bl = i / K, k = i - bl * K;
            if (b0 + bl < B) dout[(int64_t)(b0 + bl) * nha_p + (oh + k) * A + s_action[bl]] = s_d[i];
        }
        // column sums over this workgroup's rows: column (oh+k)*A + a' collects rows whose action is a'
        // (round 3: the regressed heads start at `oh`, which is 0 for the single-head baselines -- the test `head >= 1` left the
        // head-bias gradient of DQN / of TF-DQN off the head chain at zero)
        for (int c = tid; c < nha_p; c += 256) {
            float sum = 0.f;
            int head = c / A, aa = c - head * A;
            if (head >= oh && head < oh + K)
                for (int bl = 0; bl < TD_ROWS; ++bl) sum += (s_action[bl] == aa) ? s_d[bl * K + head - oh] : 0.f;
            dbh_part[(int64_t)blockIdx.x * nha_p + c] = sum;
        }
    }
    if (priorities != nullptr && tid < TD_ROWS && b0 + tid < B) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s_td[tid * K + k];
        priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }
}

// ---------------------------------------------------------------------------------------------
// Head chain (learn path).  Everything between the last hidden activation and the gradient w.r.t. that
// layer's pre-activation is per-transition work on a few hundred floats, so one kernel does it for S
// transitions per workgroup instead of five latency-bound launches:
//   q = a W_head^T + b           (dqn.py:100-103; online rows 0..S-1 and next-state rows S..2S-1 form one
//                                  16-row MFMA tile, the waves split the contraction and reduce through LDS)
//   iterated Bellman target, squared TD loss, dL/dq   (isdqn.py:92-109, as td_kernel)
//   da = dL/dq W_head            (dL/dq has one non-zero per head and transition: K fp32 row-AXPYs, exact)
//   dz = backward of a = relu(LN(z)) over the hidden row (as ln_bwd_wide_kernel), partial (dgamma, dbeta,
//        dbias) sums per workgroup to part[wg][3][Fp]
// Workgroup 0 also advances the Adam step counter (it used to ride on loss_finalize_kernel, which now runs
// off the critical path).
// ---------------------------------------------------------------------------------------------
struct HeadChainParams {
    // hidden dense layer, finished inside this kernel for the rows a workgroup owns (dense_post_kernel's work)
    const float* slabs;     // [2B][n_slabs][Fp] split-K partial products of the hidden layer (row-interleaved)
    int n_slabs;
    int64_t slab_stride, row_pitch;  // Fp, n_slabs * Fp
    const float* hbias;     // [F] hidden bias
    float* act;             // [2B][Fp] post-activation rows (rows [0,B): states, [B,2B): next states), written here
    float* z;               // [B][Fp]  pre-LayerNorm rows of the states, written here
    const float* W;     // [O][Fp]
    const float* bias;  // [O]
    const float* gamma; // hidden LayerNorm scale / bias, or null
    const float* beta;
    int B, S, F, Fp, O, Op, K, A, oh;  // oh: online head k + oh is regressed on head k (1: iS-DQN, 0: single head)
    const int* action;
    const float* reward;
    const uint8_t* terminal;
    const float* loss_weights;  // [B] importance-sampling weights, or null (weight 1)
    const float* discount;      // [B] per-transition discounts in gamma_n's place, or null (isdqn_batch_discount::discount)
    float gamma_n, huber_delta;
    int double_q;       // isdqn_net_config::double_q: head oh + k of the next-state row selects, head k values
    Munchausen mu;      // isdqn_net_config::munchausen_*: head k of the state row gives the bonus, of the next-state row the soft value
    float* dout;        // [B][Op]  dL/dq
    float* dz;          // [B][Fp]
    float* part;        // [n_wg][3][Fp]
    float* q_values;    // [B][K]
    float* targets;     // [B][K]
    double* priorities; // [B] or null
    float* loss_part;   // [n_wg][K]
    float* dbh_part;    // [n_wg][Op]
    int* adam_count;
    float b1, b2;
    float* adam_consts;
    long long* stamps;  // profiling only (isdqn_debug_set_stamps "head_chain"): [workgroup][8] phase boundaries
};

// Transitions per workgroup (template parameter SMAX = 1, 2 or 4; HC_MAX_S in net_plan.h is the largest).  The kernel
// is instruction-issue bound (a few thousand instructions executed once per wave), and the target / data-gradient /
// LayerNorm phases scale with S, so few transitions on many workgroups win -- until every one of too many workgroups
// streams the whole head matrix from L2: S = 1 at B = 256 (20 us; S = 2: 23 us; S = 4 on 256 threads: 22 us before the
// dense_post fusion), S = 4 at B = 1024 (head_chain_plan picks about 256 workgroups).
constexpr int HC_MAX_COLS = 4;  // hidden width up to HC_THREADS * 4 (columns per thread: template parameter COLS)
// Eight waves: the kernel executes a few thousand instructions ONCE per wave, so it is bound by instruction issue and
// its dependency stalls; two waves per SIMD interleave, and each owns half the K-steps / columns.
constexpr int HC_THREADS = 512, HC_WAVES = HC_THREADS / 64;
constexpr int HC_KU = 16 / HC_WAVES;  // K-steps per wave and work item (an item covers 16 K-steps)

__host__ __device__ inline int head_chain_pitch(int Fp) { return (Fp + 31) / 32 * 32 + 8; }
static inline int head_chain_lds_bytes(int Fp, int Op, int K, int passes, int S) {
    const int PA = head_chain_pitch(Fp);
    return (passes >= 2 ? 2 : 1) * 16 * PA * 2 + (HC_WAVES * 16 * Op + 16 * Op + S * Op + Op + 4 + 2 * S * Fp) * 4 + S * K * 12 +
           HC_WAVES * 2 * S * 2 * 4 + 64;
}

template <int PASSES, int COLS, int SMAX>
__global__ __launch_bounds__(HC_THREADS) void head_chain_kernel(const HeadChainParams p) {
    ISDQN_EMPTY_KERNEL_RETURN
    extern __shared__ __attribute__((aligned(16))) char hc_smem[];
    const int PA = head_chain_pitch(p.Fp);
    constexpr int A_PLANES = PASSES >= 2 ? 2 : 1;
    __bf16* a_hi = reinterpret_cast<__bf16*>(hc_smem);
    __bf16* a_lo = a_hi + 16 * PA;
    float* qpart = reinterpret_cast<float*>(a_hi + A_PLANES * 16 * PA);  // [HC_WAVES][16][Op]
    float* s_q = qpart + HC_WAVES * 16 * p.Op;                                  // [16][Op]
    float* s_dq = s_q + 16 * p.Op;                                       // [SMAX][Op]
    float* s_d = s_dq + SMAX * p.Op;                                 // [SMAX][K]
    float* s_td = s_d + SMAX * p.K;                                  // TD loss per (transition, head): the priorities
    float* s_wtd = s_td + SMAX * p.K;                                // the same times the transition's weight: the loss partials
    float* s_red = s_wtd + SMAX * p.K;                               // [HC_WAVES][2 * SMAX][2]
    float* s_bias = s_red + HC_WAVES * 2 * SMAX * 2;                 // [Op]
    float* s_pre = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(s_bias + p.Op) + 15) & ~(uintptr_t)15);  // [2 * SMAX][Fp] hidden pre-activations, 16-B aligned

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if defined(ISDQN_DEV)
#define HC_STAMP(i)                                                                                     \
    if (p.stamps != nullptr && threadIdx.x == 0) {                                                     \
        p.stamps[(int64_t)blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memtime();              \
        if ((i) == 0) p.stamps[(int64_t)blockIdx.x * 8 + 7] = (long long)__builtin_amdgcn_s_memrealtime(); \
    }
#else
#define HC_STAMP(i)
#endif
    HC_STAMP(0);
    const int S = p.S, b0 = (int)blockIdx.x * S;
    const int Fp = p.Fp, Op = p.Op, K = p.K, A = p.A;

    if (blockIdx.x == 0 && tid == 0) {
        int t = *p.adam_count + 1;
        *p.adam_count = t;
        p.adam_consts[0] = (float)(1.0 - pow_int((double)p.b1, t));
        p.adam_consts[1] = (float)(1.0 - pow_int((double)p.b2, t));
    }

    // Global loads are requested a phase before they are needed, and nothing touches a loaded register where it is
    // requested (the data were last written from other XCDs: a first touch costs ~4000 cycles).
    // ---- operands of the later phases (raw: converted where they are used) ----
    int act[SMAX];  // action of the S transitions (selects the head rows the data gradient reads)
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        ISDQN_BOUNDS_CHECK((s < S && b0 + s < p.B) ? (const void*)(p.action + b0 + s) : zero_chunk(), 4, 20);
        act[s] = *(const ISDQN_GLOBAL int*)((s < S && b0 + s < p.B) ? (const void*)(p.action + b0 + s) : zero_chunk());
    }
    float td_r, td_w, td_g;  // reward, importance-sampling weight, discount, terminal flag of this thread's (transition, head) pair
    uint8_t td_term;
    {
        const int s = tid / K;
        const bool ok = tid < S * K && b0 + s < p.B;
        const bool okw = ok && p.loss_weights != nullptr;
        ISDQN_BOUNDS_CHECK(okw ? (const void*)(p.loss_weights + b0 + s) : zero_chunk(), 4, 29);
        td_w = *(const ISDQN_GLOBAL float*)(okw ? (const void*)(p.loss_weights + b0 + s) : zero_chunk());
        const bool okg = ok && p.discount != nullptr;
        ISDQN_BOUNDS_CHECK(okg ? (const void*)(p.discount + b0 + s) : zero_chunk(), 4, 50);
        td_g = *(const ISDQN_GLOBAL float*)(okg ? (const void*)(p.discount + b0 + s) : zero_chunk());
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.reward + b0 + s) : zero_chunk(), 4, 21);
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.terminal + b0 + s) : zero_chunk(), 1, 22);
        td_r = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.reward + b0 + s) : zero_chunk());
        td_term = *(const ISDQN_GLOBAL uint8_t*)(ok ? (const void*)(p.terminal + b0 + s) : zero_chunk());
    }
    ISDQN_BOUNDS_CHECK(tid < p.O ? (const void*)(p.bias + tid) : zero_chunk(), 4, 23);
    const float bias_v = *(const ISDQN_GLOBAL float*)(tid < p.O ? (const void*)(p.bias + tid) : zero_chunk());
    float ga[COLS], be[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
        const int c = tid + j * HC_THREADS;
        const bool ok = p.gamma != nullptr && c < p.F;
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.gamma + c) : zero_chunk(), 4, 24);
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.beta + c) : zero_chunk(), 4, 24);
        ga[j] = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.gamma + c) : zero_chunk());
        be[j] = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.beta + c) : zero_chunk());
    }

    // ---- the hidden dense layer is finished HERE for the 2S rows of this workgroup (dqn.py:96-99; what
    //      dense_post_kernel does in the forward-only path): split-K slabs summed in slab order, + bias, LayerNorm, ReLU.
    //      The rows go to HBM once (act: the head's weight gradient reads the state rows; z: debug / tests), to LDS as
    //      bf16 hi/lo for the head GEMM, and the pre-LayerNorm values stay in registers for the backward below.
    //      Tile rows 2S..15 are not staged: MFMA output rows depend on their own A row only, and nothing reads the q
    //      rows of those tile rows ----
    constexpr int R2 = 2 * SMAX;
    constexpr int TPR = HC_THREADS / R2;  // threads per tile row (two waves): 16-byte loads, one row per thread
    constexpr int SB = 32;                // slabs per batch = loads in flight per thread
    static_assert(TPR % 64 == 0, "a wave must not straddle two rows");
    float m1 = 0.f, m2 = 0.f;  // LayerNorm sums of this thread's row (over its columns)
    {
        const int r = tid / TPR, q = tid - r * TPR;
        const int smp = r < S ? r : r - S;
        const bool row_ok = r < 2 * S && b0 + smp < p.B;
        const int64_t grow = r < S ? (int64_t)(b0 + smp) : (int64_t)p.B + b0 + smp;
        for (int c0 = q * 4; c0 < Fp; c0 += TPR * 4) {  // (one pass up to 512 columns)
            float hb4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ISDQN_BOUNDS_CHECK(c0 + e < p.F ? (const void*)(p.hbias + c0 + e) : zero_chunk(), 4, 25);
                hb4[e] = *(const ISDQN_GLOBAL float*)(c0 + e < p.F ? (const void*)(p.hbias + c0 + e) : zero_chunk());
            }
            const ISDQN_GLOBAL f32x4* base = (const ISDQN_GLOBAL f32x4*)(row_ok ? (const void*)(p.slabs + grow * p.row_pitch + c0) : zero_chunk());
            const int64_t strd = row_ok ? p.slab_stride / 4 : 0;  // (Fp is a multiple of 8)
            f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < p.n_slabs; s0 += SB) {
                f32x4 t[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    ISDQN_BOUNDS_CHECK((const void*)(base + min(s0 + u, p.n_slabs - 1) * strd), 16, 26);
                    t[u] = base[min(s0 + u, p.n_slabs - 1) * strd];  // tail: clamped, masked in the sum
                }
#pragma unroll
                for (int u = 0; u < SB; ++u)
                    if (s0 + u < p.n_slabs) sum += t[u];  // (uniform condition; slab order)
            }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = c0 + e < p.F ? sum[e] + hb4[e] : 0.f;
                m1 += v[e];
                m2 += v[e] * v[e];
            }
            *reinterpret_cast<float4*>(s_pre + r * Fp + c0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }

    HC_STAMP(6);  // slab sums of this thread's row done
    // ---- q = a W^T work items, see below; the first batch of W fragments travels under the LayerNorm ----
    const int nkt = (PA - 8) / 32, NT = (Op + 15) / 16;
    const int nks = (nkt + 15) / 16, n_items = ((NT + 1) / 2) * nks;
    const int kg8 = (lane >> 4) * 8;
    const int arow = (lane & 15) * PA + kg8;
    auto issue_w = [&](float (&v)[2][HC_KU][8], int item) {
        const int pair = item / nks, ksb = wave + 16 * (item - pair * nks);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < HC_KU; ++u) {
                const int o = (pair * 2 + t) * 16 + (lane & 15), ks = ksb + HC_WAVES * u;
                const bool ok = item < n_items && o < p.O && ks < nkt && ks * 32 + kg8 < Fp;
                load8_aligned(ok ? p.W + (int64_t)o * Fp + ks * 32 + kg8 : zero_chunk(), v[t][u]);
            }
    };
    float wv0[2][HC_KU][8], wv1[2][HC_KU][8];
    issue_w(wv0, 0);

    float zv[SMAX][COLS];  // pre-LayerNorm values of the state rows (zero outside the row / the transition range)
    {
        for (int off = 32; off > 0; off >>= 1) {
            m1 += __shfl_xor(m1, off);
            m2 += __shfl_xor(m2, off);
        }
        if (lane == 0) {
            s_red[wave * 2] = m1;
            s_red[wave * 2 + 1] = m2;
        }
        __syncthreads();  // row sums and the pre-activation rows (s_pre) are visible
        constexpr int WPR = TPR / 64;  // waves per row
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            float a1 = s_red[r * WPR * 2], a2 = s_red[r * WPR * 2 + 1];
#pragma unroll
            for (int w = 1; w < WPR; ++w) {  // fixed order
                a1 += s_red[(r * WPR + w) * 2];
                a2 += s_red[(r * WPR + w) * 2 + 1];
            }
            const float mean = a1 / (float)p.F;
            const float rstd = rsqrtf(fmaxf(a2 / (float)p.F - mean * mean, 0.f) + 1e-6f);
            const int smp = r < S ? r : r - S;
            const bool row_ok = r < 2 * S && b0 + smp < p.B;
            const int64_t grow = r < S ? (int64_t)(b0 + smp) : (int64_t)p.B + b0 + smp;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int c = tid + j * HC_THREADS;
                const float v = c < Fp ? s_pre[r * Fp + c] : 0.f;
                float y = v;
                if (p.gamma != nullptr && c < p.F) y = (v - mean) * (rstd * ga[j]) + be[j];
                y = fmaxf(y, 0.f);  // (the head chain requires a ReLU hidden layer)
                if (c >= p.F) y = 0.f;
                if (row_ok && c < Fp) {
                    s8_store_elem(p.act + grow * Fp, c, y);  // hidden activations: S8 (read back by the head weight gradient)
                    if (r < S) p.z[grow * Fp + c] = v;
                }
                if (r < 2 * S && c < PA - 8) {
                    const float ys = row_ok ? y : 0.f;
                    const __bf16 h = (__bf16)ys;
                    a_hi[r * PA + c] = h;
                    if constexpr (PASSES >= 2) a_lo[r * PA + c] = (__bf16)(ys - (float)h);
                }
                if (r < SMAX) zv[r < SMAX ? r : 0][j] = (row_ok && r < S && c < p.F) ? v : 0.f;
            }
        }
    }
    for (int i = tid; i < SMAX * Op; i += HC_THREADS) s_dq[i] = 0.f;
    if (tid < Op) s_bias[tid] = bias_v;
    for (int o = tid + HC_THREADS; o < Op; o += HC_THREADS) s_bias[o] = o < p.O ? p.bias[o] : 0.f;  // (more outputs than threads)
    __syncthreads();  // hidden rows staged
    HC_STAMP(1);  // hidden rows staged

    // ---- q = a W^T : wave w takes K-steps w, w+16, ... of every pair of 16-column tiles.  A work item is (tile pair,
    //      K-step group): its W fragments (two tiles x four K-steps) are one batch of loads, and the batch of the NEXT
    //      item is in flight while this one is multiplied ----
    {
        f32x4 acc[2];
        auto run_item = [&](float (&v)[2][HC_KU][8], int item) {
            const int pair = item / nks, ksi = item - pair * nks, ksb = wave + 16 * ksi;
            if (ksi == 0) {
                acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < HC_KU; ++u) {
                const int ks = min(ksb + HC_WAVES * u, nkt - 1);  // past the end: B is zero, A only has to be finite
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + arow + ks * 32);
                bf16x8 al;
                if constexpr (PASSES >= 2) al = *reinterpret_cast<const bf16x8*>(a_lo + arow + ks * 32);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    bf16x8 bh, bl;
                    if constexpr (PASSES >= 2) {
                        split8(v[t][u], bh, bl);
                        if constexpr (PASSES >= 3)
                            mfma_acc(acc[t], ah, bl);
                        mfma_acc(acc[t], al, bh);
                    } else {
                        round8(v[t][u], bh);
                    }
                    mfma_acc(acc[t], ah, bh);
                }
            }
            const bool last = ksi + 1 == nks;
            if (last) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int o = (pair * 2 + t) * 16 + (lane & 15);
                    if (o < Op) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) qpart[(wave * 16 + (lane >> 4) * 4 + r) * Op + o] = acc[t][r];
                    }
                }
            }
        };
        for (int item = 0; item < n_items; item += 2) {
            issue_w(wv1, item + 1);  // (past the last item: zero block)
            run_item(wv0, item);
            issue_w(wv0, item + 2);
            if (item + 1 < n_items) run_item(wv1, item + 1);
        }
    }

    // ---- data-gradient rows: head row (1 + k) * A + action of every (transition, head), four heads per batch; the
    //      first batch is requested here and travels under the target / TD phase ----
    auto issue_rows = [&](float (&w)[SMAX][4][COLS], int k0) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool on = s < S && k0 + u < K;
                const float* wr = p.W + (int64_t)(on ? (p.oh + k0 + u) * A + act[s] : 0) * Fp;
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    ISDQN_BOUNDS_CHECK(wr + (c < p.F ? c : 0), 4, 27);
                    w[s][u][j] = *(const ISDQN_GLOBAL float*)(wr + (c < p.F ? c : 0));
                }
            }
    };
    HC_STAMP(2);  // head GEMM done (this wave)
    float wr0[SMAX][4][COLS], wr1[SMAX][4][COLS];
    issue_rows(wr0, 0);
    __syncthreads();
    for (int i = tid; i < 2 * S * Op; i += HC_THREADS) {  // (tile rows 2S..15 are nobody's)
        const int o = i % Op;
        float v = qpart[i];
#pragma unroll
        for (int w = 1; w < HC_WAVES; ++w) v += qpart[w * 16 * Op + i];  // fixed order
        s_q[i] = o < p.O ? v + s_bias[o] : 0.f;
    }
    __syncthreads();

    // ---- iterated Bellman target, TD, dL/dq (isdqn.py:92-109) ----
    const float inv_b = 1.f / (float)p.B;
    if (tid < S * K) {
        const int s = tid / K, k = tid - s * K;
        const int b = b0 + s;
        float d = 0.f, td = 0.f;
        int a = 0;
        if (b < p.B) {
            a = act[0];
#pragma unroll
            for (int i = 1; i < SMAX; ++i) a = s == i ? act[i] : a;
            const float qv = s_q[s * Op + (p.oh + k) * A + a];
            const float* nq = s_q + (S + s) * Op + k * A;
            float mx = nq[0];
            if (p.double_q) {
                mx = nq[argmax_first(nq + p.oh * A, A)];
            } else {
                for (int j = 1; j < A; ++j) mx = fmaxf(mx, nq[j]);
            }
            const float gamma_n = p.discount != nullptr ? td_g : p.gamma_n;
            float tg = td_r + (1.f - (float)td_term) * gamma_n * mx;
            if (p.mu.tau > 0.f) {  // the value head's own row of the state: head k, not oh + k
                const float* sv = s_q + s * Op + k * A;
                tg = munchausen_target(td_r, 1.f - (float)td_term, gamma_n, sv[a], soft_value(sv, A, p.mu.tau), soft_value(nq, A, p.mu.tau), p.mu);
            }
            d = qv - tg;
            td = td_loss(d, p.huber_delta);
            if (p.q_values) p.q_values[(int64_t)b * K + k] = qv;
            if (p.targets) p.targets[(int64_t)b * K + k] = tg;
        }
        const float w = p.loss_weights != nullptr ? td_w : 1.f;
        const float dd = td_dloss(d, p.huber_delta) * inv_b * w;
        s_d[tid] = dd;
        s_td[tid] = td;
        s_wtd[tid] = td * w;
        s_dq[s * Op + (p.oh + k) * A + a] = dd;
    }
    __syncthreads();
    for (int i = tid; i < S * Op; i += HC_THREADS) {
        const int s = i / Op;
        if (b0 + s < p.B) p.dout[(int64_t)b0 * Op + i] = s_dq[i];
    }
    for (int c = tid; c < Op; c += HC_THREADS) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += s_dq[s * Op + c];
        p.dbh_part[(int64_t)blockIdx.x * Op + c] = sum;
    }
    if (tid < K) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += s_wtd[s * K + tid];
        p.loss_part[(int64_t)blockIdx.x * K + tid] = sum;
    }
    if (p.priorities != nullptr && tid < S && b0 + tid < p.B) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s_td[tid * K + k];
        p.priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }

    HC_STAMP(3);  // targets / TD / small stores issued
    // ---- da = dL/dq W (K row-AXPYs per transition, heads in ascending order), then the LayerNorm/ReLU backward of
    //      the hidden row ----
    float da[SMAX][COLS];
#pragma unroll
    for (int s = 0; s < SMAX; ++s)
#pragma unroll
        for (int j = 0; j < COLS; ++j) da[s][j] = 0.f;
    auto axpy_rows = [&](const float (&w)[SMAX][4][COLS], int k0) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool on = s < S && k0 + u < K;
                const float dd = on ? s_d[s * K + k0 + u] : 0.f;
#pragma unroll
                for (int j = 0; j < COLS; ++j) da[s][j] += dd * w[s][u][j];
            }
    };
    for (int k0 = 0; k0 < K; k0 += 8) {  // 4 heads x S transitions x COLS columns of W rows per batch, two batches in flight
        issue_rows(wr1, k0 + 4);
        axpy_rows(wr0, k0);
        issue_rows(wr0, k0 + 8);
        if (k0 + 4 < K) axpy_rows(wr1, k0 + 4);
    }
    HC_STAMP(4);  // data-gradient rows accumulated
    float dg[COLS], db[COLS], dbias[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) dg[j] = db[j] = dbias[j] = 0.f;
    if (p.gamma != nullptr) {
        const float inv_c = 1.f / (float)p.F;
        float r1[SMAX], r2[SMAX];
        auto block_sum2 = [&]() {  // r1[s], r2[s] summed over the workgroup
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                for (int off = 32; off > 0; off >>= 1) {
                    r1[s] += __shfl_xor(r1[s], off);
                    r2[s] += __shfl_xor(r2[s], off);
                }
            __syncthreads();
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < SMAX; ++s) {
                    s_red[(wave * SMAX + s) * 2] = r1[s];
                    s_red[(wave * SMAX + s) * 2 + 1] = r2[s];
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                r1[s] = s_red[s * 2];
                r2[s] = s_red[s * 2 + 1];
#pragma unroll
                for (int w = 1; w < HC_WAVES; ++w) {  // fixed order
                    r1[s] += s_red[(w * SMAX + s) * 2];
                    r2[s] += s_red[(w * SMAX + s) * 2 + 1];
                }
            }
        };
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            r1[s] = r2[s] = 0.f;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {  // zv is zero outside the row / the transition range
                r1[s] += zv[s][j];
                r2[s] += zv[s][j] * zv[s][j];
            }
        }
        block_sum2();
        float mean[SMAX], rstd[SMAX];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            mean[s] = r1[s] * inv_c;
            rstd[s] = rsqrtf(fmaxf(r2[s] * inv_c - mean[s] * mean[s], 0.f) + 1e-6f);
            r1[s] = r2[s] = 0.f;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int c = tid + j * HC_THREADS;
                const bool ok = c < p.F && s < S && b0 + s < p.B;
                const float xh = (zv[s][j] - mean[s]) * rstd[s];
                const float y = xh * ga[j] + be[j];
                const float dy = (ok && y > 0.f) ? da[s][j] : 0.f;
                dg[j] += dy * xh;
                db[j] += dy;
                const float g2 = dy * ga[j];
                da[s][j] = g2;   // keep g
                zv[s][j] = ok ? xh : 0.f;  // keep xhat
                r1[s] += g2;
                r2[s] += g2 * zv[s][j];
            }
        }
        block_sum2();
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            const float m1 = r1[s] * inv_c, m2 = r2[s] * inv_c;
            if (s < S && b0 + s < p.B) {
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    if (c < Fp) {
                        const float o = c < p.F ? rstd[s] * (da[s][j] - m1 - zv[s][j] * m2) : 0.f;
                        dbias[j] += o;
                        s8_store_elem(p.dz + (int64_t)(b0 + s) * Fp, c, o);  // dz: S8
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            if (s < S && b0 + s < p.B) {
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    if (c < Fp) {
                        const float o = (c < p.F && zv[s][j] > 0.f) ? da[s][j] : 0.f;
                        dbias[j] += o;
                        s8_store_elem(p.dz + (int64_t)(b0 + s) * Fp, c, o);  // dz: S8
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
        const int c = tid + j * HC_THREADS;
        if (c < Fp) {
            float* pp = p.part + (int64_t)blockIdx.x * 3 * Fp;
            pp[c] = dg[j];
            pp[Fp + c] = db[j];
            pp[2 * Fp + c] = dbias[j];
        }
    }
    HC_STAMP(5);  // LayerNorm backward done, stores issued
#undef HC_STAMP
}

// losses[k] = mean_b td (isdqn.py:103), optional running sum (update_online_params' cumulated_losses,
// isdqn.py:62, kept on the device), head-bias gradient, Adam step counter and bias corrections.
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ loss_part,
                                                            const float* __restrict__ dbh_part, int n_blk, int B, int K,
                                                            int nha_p, float* __restrict__ losses,
                                                            float* __restrict__ loss_accum, float* __restrict__ dbh,
                                                            int* adam_count, float b1, float b2,
                                                            float* __restrict__ adam_consts) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    // One workgroup per 16 outputs (blocks [0, ceil(K/16)): losses, the rest: head-bias columns).  16 lanes share one
    // output: strided partial sums (eight loads in flight, added in index order), then a fixed shuffle tree.
    const int nkb = (K + 15) / 16;
    const bool is_loss = (int)blockIdx.x < nkb;
    const int col = (is_loss ? (int)blockIdx.x : (int)blockIdx.x - nkb) * 16 + grp;
    const int ncol = is_loss ? K : nha_p;
    const float* src = is_loss ? loss_part : dbh_part;
    if (!is_loss && dbh == nullptr) return;
    float s = 0.f;
    if (col < ncol)
        for (int i0 = sub; i0 < n_blk; i0 += 8 * 16) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 16;
                v[u] = i < n_blk ? src[(int64_t)i * ncol + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (col < ncol && sub == 0) {
        if (is_loss) {
            s /= (float)B;
            losses[col] = s;
            if (loss_accum != nullptr) loss_accum[col] += s;
        } else {
            dbh[col] = s;
        }
    }
    if (blockIdx.x != 0) return;
    if (adam_count != nullptr && tid == 0) {
        int t = *adam_count + 1;
        *adam_count = t;
        adam_consts[0] = (float)(1.0 - pow_int((double)b1, t));
        adam_consts[1] = (float)(1.0 - pow_int((double)b2, t));
    }
}

// Adam (optax.adam, isdqn.py:46, 85-86) over the flat parameter buffer; the gradient of every
// tensor is the sum of its slabs (split-K partials / LayerNorm-backward partials), so gradients
// are reduced here and never stored in reduced form.
struct AdamEntry {
    int64_t p_off, size, slab_stride;
    const float* g;
    int n_slabs, block_start;
};
constexpr int ADAM_MAX_ENTRIES = 4 * MAX_LAYERS;
struct AdamTable {
    AdamEntry e[ADAM_MAX_ENTRIES];
    int n, total_blocks;
};
// The slab reduction of one float4 position, shared by adam_kernel and grad_reduce_sq_kernel (grad_clip.h) so that both form the
// reduced gradient in the same order: slab lane `sl` of 16 adds up the slabs sl, sl + 16, ... (adam_slab_lane_sum), the 16 lane sums
// go through LDS and are added in ascending lane order (adam_slab_combine).
__device__ __forceinline__ float4 adam_slab_lane_sum(const AdamEntry& en, int64_t i, int sl) {
    float4 g = float4{0.f, 0.f, 0.f, 0.f};
    int s = sl;
    // (eight slabs in flight per thread first: the first layer's weight gradient leaves one slab per image at B = 256 -- 16 dependent
    // loads per thread in batches of four were four round trips at the tail of the side queue)
#if !defined(ISDQN_ADAM_4_IN_FLIGHT)
    for (; s + 7 * 16 < en.n_slabs; s += 8 * 16) {
        float4 h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = *reinterpret_cast<const float4*>(en.g + (int64_t)(s + u * 16) * en.slab_stride + i);
#pragma unroll
        for (int u = 0; u < 8; ++u) { g.x += h[u].x; g.y += h[u].y; g.z += h[u].z; g.w += h[u].w; }
    }
#endif
    for (; s + 3 * 16 < en.n_slabs; s += 4 * 16) {
        float4 h[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) h[u] = *reinterpret_cast<const float4*>(en.g + (int64_t)(s + u * 16) * en.slab_stride + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) { g.x += h[u].x; g.y += h[u].y; g.z += h[u].z; g.w += h[u].w; }
    }
    for (; s < en.n_slabs; s += 16) {
        float4 h = *reinterpret_cast<const float4*>(en.g + (int64_t)s * en.slab_stride + i);
        g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    return g;
}
__device__ __forceinline__ float4 adam_slab_combine(const float4 (*s_g)[16], int pos) {
    float4 g = s_g[0][pos];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const float4 h = s_g[k][pos];
        g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    return g;
}
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable tab, float* __restrict__ p, float* __restrict__ m,
                                                   float* __restrict__ v, const float* __restrict__ consts, float lr,
                                                   float b1, float b2, float eps, float* __restrict__ grad_out,
                                                   float* __restrict__ mirror, int update) {
    ISDQN_EMPTY_KERNEL_RETURN
    // A workgroup covers 16 float4 positions; 16 "slab lanes" per position split the slab reduction (up to a
    // few hundred split-K / per-image-group slabs for the conv kernels) and combine through LDS in a fixed
    // order, so the reduction is deterministic and never a long serial chain of dependent loads.
    __shared__ float4 s_g[16][16];
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].block_start) ++e;
    const AdamEntry en = tab.e[e];
    const float c1 = consts[0], c2 = consts[1];  // 1 - b1^t, 1 - b2^t (loss_finalize_kernel)
    const int pos = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t i = ((int64_t)(blockIdx.x - en.block_start) * 16 + pos) * 4;
    const bool on = i < en.size;
    float4 g = float4{0.f, 0.f, 0.f, 0.f};
    // the updating lanes request their moments and parameters now: they arrive under the slab reduction
    const int64_t o = en.p_off + i;
    float4 pm = g, pv = g, pp = g;
    if (on && sl == 0) {
        pm = *reinterpret_cast<const float4*>(m + o);
        pv = *reinterpret_cast<const float4*>(v + o);
        pp = *reinterpret_cast<const float4*>(p + o);
    }
    if (on) g = adam_slab_lane_sum(en, i, sl);
    s_g[sl][pos] = g;
    __syncthreads();
    if (sl != 0 || !on) return;
    g = adam_slab_combine(s_g, pos);
    if (grad_out != nullptr) *reinterpret_cast<float4*>(grad_out + o) = g;
    if (!update) return;  // gradient only (isdqn_net_grad_on_batch)
    float* gp = &g.x; float* mp = &pm.x; float* vp = &pv.x; float* xp = &pp.x;
    const float inv_c1 = 1.f / c1, inv_c2 = 1.f / c2;
#pragma unroll
    for (int r = 0; r < 4; ++r) xp[r] = adam_element(mp[r], vp[r], xp[r], gp[r], b1, b2, lr, eps, inv_c1, inv_c2);
    *reinterpret_cast<float4*>(m + o) = pm;
    *reinterpret_cast<float4*>(v + o) = pv;
    *reinterpret_cast<float4*>(p + o) = pp;
    s8_store_quad(mirror, (int)o, pp.x, pp.y, pp.z, pp.w);  // S8 mirror of the updated parameters (read by the next step's MFMA stages)
}

#include "grad_clip.h"  // (inside namespace isdqn, behind the Adam table and the slab reduction it shares)

// shift_params (isdqn.py:111-125): rows [0, nha-A) <- rows [A, nha) of the last Dense ([out][in] layout).  (Histogram heads: called
// with the logit width and A * n_bins, so that whole histograms move.)
__global__ __launch_bounds__(256) void shift_kernel(float* __restrict__ w, float* __restrict__ bias, int nha, int A,
                                                    int in_p) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < in_p)
        for (int r = 0; r + A < nha; ++r) w[(int64_t)r * in_p + f] = w[(int64_t)(r + A) * in_p + f];
    if (f == in_p)
        for (int r = 0; r + A < nha; ++r) bias[r] = bias[r + A];
}

// best_action (isdqn.py:127-135): first argmax over the actions of head 1+idx.
__global__ void argmax_kernel(const float* __restrict__ q, int A, int head, int* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float* r = q + head * A;
        int best = 0;
        for (int a = 1; a < A; ++a)
            if (r[a] > r[best]) best = a;
        *out = best;
    }
}

// AnalysisNet (slimdqn/utils/analysis_architecture.py:46-122): per-neuron sums over the rows of one hidden layer's post-ReLU
// activations (S8 storage, [n_rows][pitch], `cpp` padded channels per pixel of which `c` are real), optionally also the
// activations themselves as fp32 [n_rows][feat_ld] in the reference's (unpadded) feature order.  A workgroup owns 32 groups
// of 8 elements; 8 row lanes stride over the rows and combine through LDS in a fixed order (deterministic).
__global__ __launch_bounds__(256) void act_rowsum_kernel(const float* __restrict__ act, int n_rows, int pitch, int cpp, int c,
                                                         float* __restrict__ scores, float* __restrict__ feat, int feat_ld) {
    __shared__ float s_sum[8][32][8];
    const int gl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int e0 = ((int)blockIdx.x * 32 + gl) * 8;
    const bool on = e0 < pitch;
    const int pix = on ? e0 / cpp : 0, ch0 = on ? e0 % cpp : 0;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    if (on)
        for (int r = rl; r < n_rows; r += 8) {
            const float* src = act + (int64_t)r * pitch + e0;
            const f32x4 h = *reinterpret_cast<const f32x4*>(src), l = *reinterpret_cast<const f32x4*>(src + 4);
            const bf16x8 hi = __builtin_bit_cast(bf16x8, h), lo = __builtin_bit_cast(bf16x8, l);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = (float)hi[i] + (float)lo[i];
                acc[i] += v;
                if (feat != nullptr && ch0 + i < c) feat[(int64_t)r * feat_ld + pix * c + ch0 + i] = v;
            }
        }
#pragma unroll
    for (int i = 0; i < 8; ++i) s_sum[rl][gl][i] = acc[i];
    __syncthreads();
    if (rl == 0 && on) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += s_sum[k][gl][i];
            if (ch0 + i < c) scores[pix * c + ch0 + i] = t;
        }
    }
}

// batched form: row i -> first argmax of head oh + idx[i] of its own q row
__global__ __launch_bounds__(64) void argmax_rows_kernel(const float* __restrict__ q, int n_rows, int nha_p, int A, int oh, int K,
                                                         const int* __restrict__ idx, int* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_rows) return;
    int head = idx[i];
    head = oh + (head < 0 ? 0 : head >= K ? K - 1 : head);
    const float* r = q + (int64_t)i * nha_p + head * A;
    int best = 0;
    for (int a = 1; a < A; ++a)
        if (r[a] > r[best]) best = a;
    out[i] = best;
}

// =============================================================================================
// Host orchestration
// =============================================================================================
// profiling hook (not in the public header): phase stamps of the image-resident forward kernel of one layer
#if defined(ISDQN_DEV)
static long long* g_stamps = nullptr;
static int g_stamp_layer = -1;
static char g_stamp_name[32] = "";
extern "C" int isdqn_debug_set_stamps(void* buf, const char* layer_name) {
    g_stamps = (long long*)buf;
    g_stamp_layer = buf ? 0 : -1;
    snprintf(g_stamp_name, sizeof(g_stamp_name), "%s", layer_name ? layer_name : "");
    return ISDQN_OK;
}
static long long* stamps_for(const char* kernel_tag) {
    return (g_stamp_layer >= 0 && strcmp(kernel_tag, g_stamp_name) == 0) ? g_stamps : nullptr;
}
#else
static long long* stamps_for(const char*) { return nullptr; }
#endif

// fp32 master parameters -> S8 mirror (gemm_core.h): every 32-byte group of 8 values becomes 8 hi + 8 lo bf16.  The
// MFMA consumers of the weights stage the mirror by copy.  Run at the head of every entry point that takes `params`:
// the master is caller-owned memory (imports, head shifts, target copies happen outside this library).
__global__ __launch_bounds__(256) void split_params_kernel(const float* __restrict__ p, float* __restrict__ mirror, int64_t n_groups) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    float v[8];
    load8_aligned(p + g * 8, v);
    s8_store_group(mirror + g * 8, v);
}
static int refresh_mirror(const Plan& P, const float* params, float* ws, hipStream_t st) {
    const int64_t n_groups = P.n_params / 8;  // every tensor size is a multiple of 8 (padded widths)
    hipLaunchKernelGGL(split_params_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, params, ws + P.wsplit_off, n_groups);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static ConvGeom conv_geom(const Layer& l) {
    ConvGeom g;
    g.hin = l.hin; g.win = l.win; g.cin_p = l.cin_p; g.hout = l.hout; g.wout = l.wout;
    g.cout = l.cout; g.cout_p = l.cout_p; g.ksz = l.ksz; g.stride = l.stride; g.pad = l.pad;
    g.npix = l.npix; g.K = l.K;
    g.stride_sh = l.stride == 4 ? 2 : l.stride == 2 ? 1 : 0;
    g.d_npix = FastDiv(l.npix); g.d_wout = FastDiv(l.wout); g.d_cinp = FastDiv(l.cin_p);
    g.d_ksz = FastDiv(l.ksz); g.d_coutp = FastDiv(l.cout_p);
    return g;
}

// Storage of the pre-activation gradients dz of hidden layers (bit 0 of the S8 operand masks below): S8, written so
// by every producer (head chain, LayerNorm-backward epilogues and kernels); the head's dL/dq stays fp32
constexpr int DZ_S8 = 1;

struct NetInput {
    const uint8_t* frames; int64_t frame_stride; const int* frame_ids; int paired_B;  // cnn
    const float* obs; const float* obs2; int obs_split;                             // fc
    int id_pitch = 0, id_off = 0;                                                   // cnn, unpaired: see FrameSrc
};

template <int BM, int PASSES, bool U8>
static int launch_conv_fwd(const Layer& l, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                           int z_img, float* act, float* z, hipStream_t st) {
    ConvFwd<BM, PASSES, U8> p;
    p.g = conv_geom(l);
    p.W = MatSrc{wmir + l.w_off, l.K, l.cout_p, l.K, 1};
    p.in = act_in;
    p.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    p.bias = params + l.b_off;
    p.gamma = l.has_ln ? params + l.g_off : nullptr;
    p.beta = l.has_ln ? params + l.be_off : nullptr;
    p.scale = U8 ? (1.0f / 255.0f) : 1.0f;
    p.act = act; p.z = z;
    p.n_pix_total = n_img * l.npix;
    p.z_pix = z_img * l.npix;
    return launch_gemm(p, ceil_div(p.n_pix_total, 128), st);
}

// image-resident forward convolution (conv_img.h) when the input tile fits in LDS; generic engine otherwise
static int conv_fwd_img(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                        int z_img, float* act, float* z, hipStream_t st, bool* done) {
    *done = false;
    // The image-resident kernels store `act` unconditionally (only the `z` store is guarded, by z_img): a caller without an activation
    // output -- the impala Stacks pass act == nullptr for the convolutions whose output is only needed pre-activation -- must take the
    // generic engine.  (Round 3's uncommitted experiment that routed the impala convolutions here faulted on exactly that store:
    // "Memory access fault ... on address 0x9000" = null + the first image tile's offset, gpurun_out/imp1.log)
    if (act == nullptr || (z == nullptr && z_img > 0)) return ISDQN_OK;
    ConvImgParams ip;
    ip.g = conv_geom(l);
    // (two channel tiles: the kernel then alternates two accumulator sets, see conv_fwd_img_kernel)
    const int mt = l.cout_p <= 32 ? 2 : 4;
    const int passes = x3 ? (l.is_u8 ? 2 : 3) : 1;
    // pixel pitch: +8 / +16 elements so that the 16 pixels of an MFMA column tile do not share LDS banks
    // (128-byte pixel rows put them 4-5 deep on the same banks; measured model in DESIGN.md)
    ip.PP = l.is_u8 ? 0 : l.cin_p + (l.cin_p % 64 == 0 ? 16 : 8);
    int lds = conv_img_geometry(ip.g, l.is_u8, l.cin, passes >= 3 ? 2 : 1, mt, passes >= 2 ? 2 : 1, ip.R, ip.Wp,
                                ip.plane_elems, ip.PP);
    constexpr int LDS_LIMIT = 158 * 1024;  // of the 160 KB, minus the kernels' static arrays
    if (lds > LDS_LIMIT || (l.is_u8 && (l.win < 8 || l.cin > 4))) return ISDQN_OK;  // (frame ids of a stack live in 4 registers)
    if (!l.is_u8 && l.cin_p < 16) return ISDQN_OK;  // (8-channel S8 inputs -- the BatchNorm networks' first convolution -- take the generic engine)
    // A row pitch of wout (mod 8) pixels keeps the bank pattern of a fragment's pixel columns going across the end of an
    // image row (conv_img.h, PixelOrder: the short last strip of every row is where the conflicts are left); taken when it
    // costs no workgroup per CU (11-pixel rows of the stride-2 layer: 24 -> 27 columns, conflict factor 1.75 -> 1.0).
    if (!l.is_u8 && l.npix <= 128) {
        const int want = ip.Wp + (((l.wout - ip.Wp) % 8) + 8) % 8;
        const int planes = passes >= 3 ? 2 : 1;
        const int lds2 = lds + planes * ip.R * (want - ip.Wp) * ip.PP * 2;
        const int stage2 = (passes >= 2 ? 2 : 1) * (mt * 16) * 48 * 2 * 2;  // the second K group's stages (see kg2 below)
        const int old_total = lds > 80 * 1024 ? lds + stage2 : lds, new_total = lds2 > 80 * 1024 ? lds2 + stage2 : lds2;
        if (want != ip.Wp && new_total <= LDS_LIMIT && (old_total <= 80 * 1024) == (new_total <= 80 * 1024)) {
            ip.Wp = want;
            ip.plane_elems = ip.R * want * ip.PP;
            lds = lds2;
        }
    }
    ip.W = MatSrc{wmir + l.w_off, l.K, l.cout_p, l.K, 1};
    ip.in = act_in;
    ip.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    ip.bias = params + l.b_off;
    ip.gamma = l.has_ln ? params + l.g_off : nullptr;
    ip.beta = l.has_ln ? params + l.be_off : nullptr;
    ip.scale = l.is_u8 ? (1.0f / 255.0f) : 1.0f;
    ip.act = act; ip.z = z; ip.n_img = n_img; ip.z_img = z_img;
    ip.tiles_per_img = ceil_div(l.npix, 128);
    ip.d_chunk = FastDiv((uint32_t)(l.is_u8 ? ip.Wp / 8 : l.cin_p / 8));
    ip.d_Wp = FastDiv((uint32_t)ip.Wp);
    ip.d_R = FastDiv((uint32_t)ip.R);
    ip.order = PixelOrder(l.hout, l.wout, !l.is_u8 && ip.tiles_per_img == 1);
    ip.stamps = stamps_for(l.name);
    ip.ablate = 0;
#if defined(ISDQN_DEV)
    if (const char* e = getenv("ISDQN_ABLATE")) ip.ablate = atoi(e);
#endif
    *done = true;
    if (l.is_u8) {
#if !defined(ISDQN_NO_U8_PAIR)
        // two pixel tiles per workgroup, the second one's frame rows prefetched into registers (conv_u8_pair.h): the tile image
        // must be one batch of 2 x 256 positions, the frame ids four at most
        // (four stacked frames: K = 256, eight K steps as straight-line code)
        if (mt == 2 && ip.tiles_per_img % 2 == 0 && ip.R * (ip.Wp / 8) <= U8P_PB * GEMM_THREADS && l.cin == 4 && l.K == 256 && ip.ablate == 0)
            return passes == 2 ? launch_conv_fwd_u8_pair<2, 8>(ip, st) : launch_conv_fwd_u8_pair<1, 8>(ip, st);
#endif
        if (passes == 2) return mt == 2 ? launch_conv_fwd_img<2, 2, true>(ip, st) : launch_conv_fwd_img<4, 2, true>(ip, st);
        return mt == 2 ? launch_conv_fwd_img<2, 1, true>(ip, st) : launch_conv_fwd_img<4, 1, true>(ip, st);
    }
    // An image that leaves room for one workgroup per CU only (more than half of the 160 KB) runs with two K groups of
    // four waves, if the second pair of weight stages still fits and the accumulator exchange fits the image area.
    const int stage_bytes = (passes >= 2 ? 2 : 1) * (mt * 16) * 48 * 2 * 2;  // two stages of one K group
    static const bool no_kg = ISDQN_DEV_ENV("ISDQN_NO_KGROUPS");
    const bool kg2 = !no_kg && mt == 4 && lds > 80 * 1024 && lds + stage_bytes <= LDS_LIMIT &&
                     mt * 16 * 128 * 4 <= lds - stage_bytes && l.K >= 8 * GEMM_BK;
#if !defined(ISDQN_NO_U8_PAIR)
    // two images per workgroup, the second one prefetched into registers (conv_s8_pair.h): the one-workgroup-per-CU layer with 16 K steps
    if (passes == 3 && mt == 4 && kg2 && ip.tiles_per_img == 1 && l.K == 512 && n_img % 2 == 0 && ip.ablate == 0 && ip.stamps == nullptr &&
        ip.R * ip.Wp * (l.cin_p / 8) <= S8P_BATCH * GEMM_THREADS * 2)
        return launch_conv_fwd_s8_pair<8>(ip, st);
#endif
    if (passes == 3) return mt == 2 ? launch_conv_fwd_img<2, 3, false>(ip, st)
                          : kg2 ? launch_conv_fwd_img<4, 3, false, 2>(ip, st) : launch_conv_fwd_img<4, 3, false>(ip, st);
    return mt == 2 ? launch_conv_fwd_img<2, 1, false>(ip, st)
         : kg2 ? launch_conv_fwd_img<4, 1, false, 2>(ip, st) : launch_conv_fwd_img<4, 1, false>(ip, st);
}

static int conv_fwd(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                    int z_img, float* act, float* z, hipStream_t st) {
    bool done = false;
    int rc = conv_fwd_img(l, x3, params, wmir, in, act_in, n_img, z_img, act, z, st, &done);
    if (rc || done) return rc;
    const bool small = l.cout_p <= 32;
    if (l.is_u8) {
        if (x3) return small ? launch_conv_fwd<32, 2, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                             : launch_conv_fwd<64, 2, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
        return small ? launch_conv_fwd<32, 1, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                     : launch_conv_fwd<64, 1, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
    }
    if (x3) return small ? launch_conv_fwd<32, 3, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                         : launch_conv_fwd<64, 3, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
    return small ? launch_conv_fwd<32, 1, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                 : launch_conv_fwd<64, 1, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
}

// number of slabs launch_plain writes for (K, splits); *steps_per_split: the K steps of each
static int effective_splits(int K, int splits, int* steps_per_split = nullptr) {
    int ksteps = ceil_div(K, GEMM_BK);
    if (splits < 1) splits = 1;
    if (splits > ksteps) splits = ksteps;
    int sps = ceil_div(ksteps, splits);
    if (steps_per_split) *steps_per_split = sps;
    return ceil_div(ksteps, sps);
}

// C[split][M][N] = A . B^T over row-major sources.  a_tr/b_tr: the operand is stored [K][rows].
template <int BM, int BN, int WM, int WN, bool ATR, bool BTR, int PASSES, bool AL, bool A2PART, bool ADAM = false, int S8M = 0>
static int launch_plain(const MatSrc& A, const float* A2, int a_split, const MatSrc& B, float* C, int ldc, int M,
                        int N, int K, int splits, int64_t slab_stride, hipStream_t st,
                        const AdamFuse* adam = nullptr) {
    PlainGemm<BM, BN, WM, WN, ATR, BTR, PASSES, AL, A2PART, ADAM, S8M> p;
    if (adam) p.adam = *adam;
    p.A = A; p.B = B; p.A2 = A2; p.a_split = a_split; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
    p.tiles_m = ceil_div(M, BM); p.tiles_n = ceil_div(N, BN);
    p.splits = effective_splits(K, splits, &p.steps_per_split);
    p.slab_stride = slab_stride;
    return launch_gemm(p, p.tiles_m * p.tiles_n * p.splits, st);
}

template <bool ATR, bool BTR, bool AL = true, bool A2PART = false, int S8M = 0>
static int plain_big(bool x3, const MatSrc& A, const float* A2, int a_split, const MatSrc& B, float* C, int ldc,
                     int M, int N, int K, int splits, int64_t slab_stride, hipStream_t st) {
    if (x3)
        return launch_plain<128, 128, 2, 2, ATR, BTR, 3, AL, A2PART, false, S8M>(A, A2, a_split, B, C, ldc, M, N, K, splits,
                                                                                 slab_stride, st);
    return launch_plain<128, 128, 2, 2, ATR, BTR, 1, AL, A2PART, false, S8M>(A, A2, a_split, B, C, ldc, M, N, K, splits,
                                                                             slab_stride, st);
}

// 128 x 64 tiles: twice the workgroups of plain_big for GEMMs whose 128 x 128 grid cannot fill 256 CUs
template <bool ATR, bool BTR, int S8M = 0>
static int plain_narrow(bool x3, const MatSrc& A, const MatSrc& B, float* C, int ldc, int M, int N, int K, int splits,
                        int64_t slab_stride, hipStream_t st) {
    if (x3) return launch_plain<128, 64, 2, 2, ATR, BTR, 3, true, false, false, S8M>(A, nullptr, 0, B, C, ldc, M, N, K, splits, slab_stride, st);
    return launch_plain<128, 64, 2, 2, ATR, BTR, 1, true, false, false, S8M>(A, nullptr, 0, B, C, ldc, M, N, K, splits, slab_stride, st);
}

// `skip_post`: leave the split-K slabs as they are (the head chain kernel finishes the layer for its own rows)
static int dense_fwd(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int rows,
                     int z_rows, float* slab, float* act, float* z, hipStream_t st, bool skip_post = false) {
    MatSrc A, B;
    const float* A2 = nullptr;
    int a_split = 0;
    if (l.in_unpadded_ld) {  // fc first layer: caller's [rows][obs] matrices
        A = MatSrc{in.obs, l.in_unpadded_ld, rows, l.in_f, 0};
        if (in.obs2) { A2 = in.obs2; a_split = in.obs_split; }
    } else {
        A = MatSrc{act_in, l.in_p, rows, l.in_p, 1};
    }
    B = MatSrc{wmir + l.w_off, l.in_p, l.out_f, l.in_p, 1};  // weights: S8 mirror (rows padded to in_p with zeros)
    // split-K partial products, row-interleaved: slab s of row m at slab[(m * ns + s) * out_p].  The ns partial rows of
    // one output row are one contiguous block (64 KB at the headline size) for whoever sums them; in [slab][row]
    // order they sit 1 MB apart, 32 pages per reader.
    const int ns = effective_splits(l.in_unpadded_ld ? l.in_f : l.K, l.fwd_splits);
    const int64_t slab_stride = l.out_p;
    const int ldc = ns * l.out_p;
    int rc;
    if (l.in_unpadded_ld) {
        // caller-provided observations: no alignment promise; MatSrc bounds use the true widths
        // (the observation operand bounds its own chunks to in_f; the mirror rows are read in whole aligned groups)
        rc = A2 ? plain_big<false, false, false, true, 2>(x3, A, A2, a_split, B, slab, ldc, rows, l.out_f, l.in_f,
                                                          l.fwd_splits, slab_stride, st)
                : plain_big<false, false, false, false, 2>(x3, A, nullptr, 0, B, slab, ldc, rows, l.out_f, l.in_f,
                                                           l.fwd_splits, slab_stride, st);
    } else if (l.fwd_narrow) {  // few row tiles: 128 x 64 tiles reach the workgroup count with half the split-K slabs
        rc = plain_narrow<false, false, 3>(x3, A, B, slab, ldc, rows, l.out_f, l.K, l.fwd_splits, slab_stride, st);
    } else {
        rc = plain_big<false, false, true, false, 3>(x3, A, nullptr, 0, B, slab, ldc, rows, l.out_f, l.K, l.fwd_splits, slab_stride,
                                                     st);  // activations and weights both S8
    }
    if (rc || skip_post) return rc;
    hipLaunchKernelGGL(dense_post_kernel, dim3(rows), dim3(256), 3 * l.out_p * sizeof(float), st, slab, ns, slab_stride,
                       (int64_t)ldc, rows, l.out_f, l.out_p, params + l.b_off, l.has_ln ? params + l.g_off : nullptr,
                       l.has_ln ? params + l.be_off : nullptr, l.has_relu, act, z, z_rows, l.is_head ? 0 : 1);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static int impala_forward(const Plan& P, bool x3, const float* params, const float* wmir, const NetInput& in, int n_img, int z_img,
                          float* ws, hipStream_t st, int bn_mode = 0);  // impala.h

static int bn_forward(const Plan& P, bool x3, const float* params, const NetInput& in, int n_img, int z_img, float* ws, float* q_out, bool running,
                      hipStream_t st);  // batchnorm.h

// Dueling heads: the raw rows ("head_raw" / "head_raw_target") that belong to the head-output rows `q_out` points at -- rows of the
// "q" / "logits" region or of their *_target twin (null: neither)
static float* duel_raw_rows(const Plan& P, float* ws, const float* q_out) {
    const int64_t o = q_out - ws;
    if (o >= P.out_off && o < P.out_off + (int64_t)P.N2 * P.nlog_p) return ws + P.raw_off + (o - P.out_off) / P.nlog_p * P.raw_p;
    if (P.out_t_off >= 0 && o >= P.out_t_off && o < P.out_t_off + (int64_t)P.qt_rows * P.nlog_p)
        return ws + P.raw_t_off + (o - P.out_t_off) / P.nlog_p * P.raw_p;
    return nullptr;
}
// raw rows -> the combined head-output rows every consumer reads (dueling.h)
static int duel_combine(const Plan& P, const float* raw, float* out, int n_rows, hipStream_t st) {
    const int64_t threads = (int64_t)n_rows * P.n_heads * (P.head_nb > 0 ? P.head_nb : 1);
    hipLaunchKernelGGL(duel_combine_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, st, raw, P.raw_p, out,
                       P.nlog_p, n_rows, P.n_heads, P.n_actions, P.head_nb > 0 ? P.head_nb : 1);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// forward over n_img images; hidden activations -> ws act regions, head output -> q_out [n_img][nha_p] (histogram / quantile heads:
// [n_img][nlog_p]; dueling heads: the combined rows, the head Dense's own output goes to the raw rows behind them)
static int net_forward(const Plan& P, bool x3, const float* params, const NetInput& in, int n_img, int z_img,
                       float* ws, float* q_out, hipStream_t st, int n_run = -1, int skip_post_layer = -1) {
    if (P.bn) {  // BatchNorm networks outside a learn step: the running averages (isdqn.py:130, use_running_average=True)
        ISDQN_REQUIRE(n_run < 0 && skip_post_layer < 0, ISDQN_ERR_UNSUPPORTED, "partial forward passes are not built for BatchNorm networks");
        return bn_forward(P, x3, params, in, n_img, z_img, ws, q_out, true, st);
    }
    const float* prev = nullptr;
    const float* wmir = ws + P.wsplit_off;  // refreshed by the caller (refresh_mirror) from `params`
    if (n_run < 0) n_run = P.n_layers;
    for (int i = 0; i < n_run; ++i) {
        const Layer& l = P.L[i];
        float* act = l.is_head ? q_out : ws + l.act_off;
        float* z = l.is_head ? nullptr : ws + l.z_off;
        int rc;
        if (l.is_head && P.dueling) {
            act = duel_raw_rows(P, ws, q_out);
            ISDQN_REQUIRE(act != nullptr, ISDQN_ERR_ARG, "dueling heads: the head output must go to the workspace's head rows");
        }
        if (l.kind == 2)
            rc = impala_forward(P, x3, params, wmir, in, n_img, z_img, ws, st);
        else if (l.kind == 0)
            rc = conv_fwd(l, x3, params, wmir, in, prev, n_img, z_img, act, z, st);
        else
            rc = dense_fwd(l, x3, params, wmir, in, prev, n_img, l.is_head ? 0 : z_img, ws + P.slab_off, act, z, st,
                           i == skip_post_layer);
        if (rc) return rc;
        if (l.is_head && P.dueling) {
            rc = duel_combine(P, act, q_out, n_img, st);
            if (rc) return rc;
        }
        prev = act;
    }
    return ISDQN_OK;
}

static int ln_bwd(const Layer& l, const float* params, const float* da, const float* z, int rows, float* dz,
                  float* part, int* n_blocks_out, hipStream_t st) {
    const float* gamma = l.has_ln ? params + l.g_off : nullptr;
    const float* beta = l.has_ln ? params + l.be_off : nullptr;
    const int C = l.out_f, Cp = l.out_p;
    int nb;
#define LAUNCH_SMALL(TPR)                                                                                          \
    do {                                                                                                           \
        nb = ceil_div(rows, 256 / TPR);                                                                            \
        if (nb > LN_MAX_BLOCKS) nb = LN_MAX_BLOCKS;                                                                \
        hipLaunchKernelGGL(ln_bwd_small_kernel<TPR>, dim3(nb), dim3(256), 0, st, da, z, gamma, beta, rows, C, Cp,  \
                           dz, part);                                                                              \
    } while (0)
    if (Cp <= 32) LAUNCH_SMALL(8);
    else if (Cp <= 64) LAUNCH_SMALL(16);
    else if (Cp <= 128) LAUNCH_SMALL(32);
    else if (Cp <= 256) LAUNCH_SMALL(64);
    else {
        ISDQN_REQUIRE(Cp <= 256 * LN_WIDE_MAX_COLS, ISDQN_ERR_UNSUPPORTED, "hidden dense width above 4096");
        nb = rows < LN_MAX_BLOCKS ? rows : LN_MAX_BLOCKS;
        hipLaunchKernelGGL(ln_bwd_wide_kernel, dim3(nb), dim3(256), 0, st, da, z, gamma, beta, rows, C, Cp, dz, part);
    }
#undef LAUNCH_SMALL
    ISDQN_HIP_CHECK(hipGetLastError());
    *n_blocks_out = nb;
    return ISDQN_OK;
}

template <int BM, int PASSES>
static int launch_conv_dgrad(const Layer& l, const float* wmir, const float* dz, float* da, int n_img,
                             hipStream_t st) {
    ConvDgrad<BM, PASSES> p;
    p.g = conv_geom(l);
    p.W = wmir + l.w_off;
    p.dz = dz; p.da = da; p.n_img = n_img;
    p.T = l.ksz / l.stride;
    p.Kc = p.T * p.T * l.cout_p;
    p.n_classes = l.stride * l.stride;
    int acc = 0;
    for (int c = 0; c < p.n_classes; ++c) {
        int cy = c / l.stride, cx = c % l.stride;
        int Ha = (l.hin - cy + l.stride - 1) / l.stride, Wb = (l.win - cx + l.stride - 1) / l.stride;
        p.tile_start[c] = acc;
        p.cls_d_hw[c] = FastDiv((uint32_t)(Ha * Wb));
        p.cls_d_w[c] = FastDiv((uint32_t)Wb);
        acc += ceil_div(n_img * Ha * Wb, 128);
    }
    p.tile_start[p.n_classes] = acc;
    return launch_gemm(p, acc, st);
}

template <int PASSES, bool U8>
static int launch_conv_wgrad(const Layer& l, const NetInput& in, const float* act_in, const float* dz, float* slabs,
                             int n_img, hipStream_t st) {
    ConvWgrad<PASSES, U8> p;
    p.g = conv_geom(l);
    p.n_pix = n_img * l.npix;
    p.DZ = MatSrc{dz, l.cout_p, p.n_pix, l.cout_p, 1};
    p.in = act_in;
    p.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    p.slabs = slabs;
    p.scale = U8 ? (1.0f / 255.0f) : 1.0f;
    p.tiles_n = ceil_div(l.K, 64);
    int ksteps = ceil_div(p.n_pix, GEMM_BK);
    p.steps_per_split = ceil_div(ksteps, l.gw_slabs);
    p.splits = ceil_div(ksteps, p.steps_per_split);
    return launch_gemm(p, p.tiles_n * p.splits, st);
}
// image-resident weight gradient (conv_img.h); *slabs_out = 0 when the layer does not qualify
static int conv_wgrad_img(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, float* slabs,
                          int n_img, hipStream_t st, int* slabs_out) {
    *slabs_out = 0;
    if (!l.wgi_ntw || n_img != 0 && ceil_div(n_img, l.wgi_G) > l.gw_slabs) return ISDQN_OK;
    ConvWgradImgParams wp;
    wp.g = conv_geom(l);
    const int passes = x3 ? (l.is_u8 ? 2 : 3) : 1;
    const int mt = l.cout_p <= 32 ? 2 : 4;
    int lds_unused_R, Wp, plane;
    conv_img_geometry(wp.g, l.is_u8, l.cin, 1, mt, 1, lds_unused_R, Wp, plane);
    wp.R = l.stride * (l.hout - 1) + l.ksz;  // the whole image
    wp.Wp = Wp;
    // pixel pitches: an odd multiple of 32 bytes between consecutive contraction pixels (dz rows: PA; input: stride * PPin)
    wp.PPin = l.cin_p;
    for (int pad = 0; pad <= 24; pad += 8)
        if ((l.stride * (l.cin_p + pad)) % 32 == 16) { wp.PPin = l.cin_p + pad; break; }
    wp.in_plane = l.is_u8 ? l.cin * wp.R * Wp : wp.R * Wp * wp.PPin;
    wp.PA = l.cout_p + (l.cout_p % 32 == 0 ? 16 : 8);
    wp.npix_pad = round_up(l.npix, 32);
    wp.dz_plane = wp.npix_pad * wp.PA;
    const int lds = ((passes >= 2 ? 2 : 1) * wp.dz_plane + (passes >= 3 ? 2 : 1) * wp.in_plane) * 2;
    if (lds > 150 * 1024 || (l.is_u8 && (l.win < 8 || l.cin > 4))) return ISDQN_OK;
    wp.d_chunk = FastDiv((uint32_t)(l.is_u8 ? Wp / 8 : l.cin_p / 8));
    wp.d_Wp = FastDiv((uint32_t)Wp);
    wp.d_R = FastDiv((uint32_t)wp.R);
    wp.d_dzchunk = FastDiv((uint32_t)(l.cout_p / 8));
    wp.d_npixpad = FastDiv((uint32_t)wp.npix_pad);
    wp.dz = dz; wp.in = act_in;
    wp.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    wp.slabs = slabs;
    wp.scale = l.is_u8 ? (1.0f / 255.0f) : 1.0f;
    wp.n_img = n_img; wp.G = l.wgi_G;
    wp.NC = 64 * l.wgi_ntw;
    wp.n_col_groups = l.K / wp.NC;
    wp.d_ncg = FastDiv((uint32_t)wp.n_col_groups);
    {
        char tag[32];
        snprintf(tag, sizeof(tag), "wgrad:%s", l.name);
        wp.stamps = stamps_for(tag);
    }
    const int groups = ceil_div(n_img, l.wgi_G);
    *slabs_out = groups;
#define WGI(MT_, NTW_, P_, U_) return launch_conv_wgrad_img<MT_, NTW_, P_, U_>(wp, groups, st)
#define WGI8(MT_, NTW_, P_, U_) return launch_conv_wgrad_img<MT_, NTW_, P_, U_, 8>(wp, groups, st)
    if (l.is_u8) {
        if (mt == 2) { if (l.wgi_ntw == 4) { if (passes == 2) WGI(2, 4, 2, true); else WGI(2, 4, 1, true); }
                       if (l.wgi_ntw == 2) { if (passes == 2) WGI(2, 2, 2, true); else WGI(2, 2, 1, true); } }
        else         { if (l.wgi_ntw == 4) { if (passes == 2) WGI(4, 4, 2, true); else WGI(4, 4, 1, true); }
                       if (l.wgi_ntw == 2) { if (passes == 2) WGI(4, 2, 2, true); else WGI(4, 2, 1, true); } }
    } else {
        if (mt == 2) { if (l.wgi_ntw == 4) { if (passes == 3) WGI(2, 4, 3, false); else WGI(2, 4, 1, false); }
                       if (l.wgi_ntw == 3) { if (passes == 3) WGI(2, 3, 3, false); else WGI(2, 3, 1, false); }
                       if (l.wgi_ntw == 2) { if (passes == 3) WGI(2, 2, 3, false); else WGI(2, 2, 1, false); } }
        else         { // full-width tiles: 32 column tiles on eight waves (25.7 -> 21 us); the 36 tiles of a 3x3x64 layer stay on four
                       // (six or eight waves re-read the dz fragments too often: 33.5 -> 37 us)
                       static const bool w4 = ISDQN_DEV_ENV("ISDQN_WGRAD_4WAVES");
                       if (l.wgi_ntw == 8 && !w4) { if (passes == 3) WGI8(4, 4, 3, false); else WGI8(4, 4, 1, false); }
                       if (l.wgi_ntw == 9) { if (passes == 3) WGI(4, 9, 3, false); else WGI(4, 9, 1, false); }
                       if (l.wgi_ntw == 8) { if (passes == 3) WGI(4, 8, 3, false); else WGI(4, 8, 1, false); }
                       if (l.wgi_ntw == 4) { if (passes == 3) WGI(4, 4, 3, false); else WGI(4, 4, 1, false); }
                       if (l.wgi_ntw == 3) { if (passes == 3) WGI(4, 3, 3, false); else WGI(4, 3, 1, false); }
                       if (l.wgi_ntw == 2) { if (passes == 3) WGI(4, 2, 3, false); else WGI(4, 2, 1, false); } }
    }
#undef WGI
#undef WGI8
    *slabs_out = 0;  // (u8 with NTW 3 is not instantiated)
    return ISDQN_OK;
}

// image-resident data gradient of conv layer `l` fused with the LayerNorm/ReLU backward of layer `below`:
// writes dz of `below` and the reduced (dgamma, dbeta, dbias) row of `below`.  *done = false: not applicable.
static void add_reduce_job(ReduceJobs& jobs, const float* part, int n_rows, int width, float* out) {
    const int i = jobs.n++;
    jobs.part[i] = part; jobs.out[i] = out; jobs.n_rows[i] = n_rows; jobs.width[i] = width;
    jobs.block_start[i + 1] = jobs.block_start[i] + ceil_div(width, 8);
}

static int conv_dgrad_img(const Layer& l, const Layer& below, bool x3, const float* params, const float* wmir, const float* dz, float* ws,
                          int n_img, hipStream_t st, bool* done, ReduceJobs* jobs) {
    *done = false;
    if (!l.dgi_tiles || below.part_rows < n_img * l.dgi_tiles) return ISDQN_OK;
    ConvDgradImgParams dp;
    dp.g = conv_geom(l);
    dp.W = wmir + l.w_off;
    dp.dz = dz;
    dp.z_in = ws + below.z_off;
    dp.gamma = below.has_ln ? params + below.g_off : nullptr;
    dp.beta = below.has_ln ? params + below.be_off : nullptr;
    dp.c_in = below.out_f;
    dp.dz_in = ws + below.dz_off;
    dp.part = ws + below.part_off;
    dp.n_img = n_img;
    dp.T = l.ksz / l.stride;
    dp.Kc = dp.T * dp.T * l.cout_p;
    // top / left zero border of the dz image: the taps of a class reach dz rows (iy + pad - py) / stride - jy, jy < T, i.e. down
    // to pad / stride - (T - 1).  (Round 1 took T - 1 rows whatever the padding; for the 3x3 / 1 layer that is one row and one
    // column too many -- a 14 x 14 instead of a 13 x 13 image, 83 KB of LDS instead of 75: ONE workgroup per CU instead of two.)
#if defined(ISDQN_DGRAD_WIDE_BORDER)
    dp.bt = dp.T - 1;
#else
    dp.bt = dp.T - 1 - l.pad / l.stride > 0 ? dp.T - 1 - l.pad / l.stride : 0;
#endif
    const int need_h = (l.hin - 1 + l.pad) / l.stride + 1, need_w = (l.win - 1 + l.pad) / l.stride + 1;
    dp.Hd = dp.bt + (l.hout > need_h ? l.hout : need_h);
    dp.Wd = dp.bt + (l.wout > need_w ? l.wout : need_w);
    // pixel pitch with (pitch bytes / 16) = 2 (mod 4): conflict-free ds_read_b128 of 16 consecutive pixels (conv_img.h)
    dp.PPd = l.cout_p + ((16 - l.cout_p % 32) + 32) % 32;
    dp.dz_plane = dp.Hd * dp.Wd * dp.PPd;
    dp.d_chunk = FastDiv((uint32_t)(l.cout_p / 8));
    dp.d_Wd = FastDiv((uint32_t)dp.Wd);
    dp.d_T = FastDiv((uint32_t)dp.T);
    {
        char tag[32];
        snprintf(tag, sizeof(tag), "dgrad:%s", l.name);
        dp.stamps = stamps_for(tag);
    }
    dp.n_classes = l.stride * l.stride;
    int acc = 0;
    for (int c = 0; c < dp.n_classes; ++c) {
        int cy = c / l.stride, cx = c % l.stride;
        int Ha = (l.hin - cy + l.stride - 1) / l.stride, Wb = (l.win - cx + l.stride - 1) / l.stride;
        dp.cls_tile_start[c] = acc;
        dp.cls_order[c] = PixelOrder(Ha, Wb, Ha * Wb <= 128);  // (a class of several tiles keeps row-major tiles)
        acc += ceil_div(Ha * Wb, l.dgi_tile_pix);
    }
    dp.cls_tile_start[dp.n_classes] = acc;
    dp.tiles_per_img = acc;
    const int mt = l.cin_p <= 32 ? 2 : 4;
    const int passes = x3 ? 3 : 1;
    const int lds = (2 * (passes >= 2 ? 2 : 1) * 32 * (mt * 16 + 16) + (passes >= 3 ? 2 : 1) * dp.dz_plane) * 2;  // TileGeom<.., true>
    if (lds > 150 * 1024) return ISDQN_OK;
    int rc;
    ISDQN_REQUIRE(acc == l.dgi_tiles, ISDQN_ERR_ARG, "data-gradient tiling differs from the plan's");
#if ISDQN_DGRAD_TILE64_BELOW > 0
    if (l.dgi_tile_pix == 64) {
        if (passes == 3) rc = mt == 2 ? launch_conv_dgrad_img<2, 3, 1>(dp, st) : launch_conv_dgrad_img<4, 3, 1>(dp, st);
        else rc = mt == 2 ? launch_conv_dgrad_img<2, 1, 1>(dp, st) : launch_conv_dgrad_img<4, 1, 1>(dp, st);
    } else
#endif
    if (passes == 3) rc = mt == 2 ? launch_conv_dgrad_img<2, 3>(dp, st) : launch_conv_dgrad_img<4, 3>(dp, st);
    else rc = mt == 2 ? launch_conv_dgrad_img<2, 1>(dp, st) : launch_conv_dgrad_img<4, 1>(dp, st);
    if (rc) return rc;
    add_reduce_job(*jobs, ws + below.part_off, n_img * dp.tiles_per_img, 3 * below.out_p, ws + below.red_off);
    *done = true;
    return ISDQN_OK;
}

static int conv_wgrad_slabs(const Layer& l, int n_img) {
    int ksteps = ceil_div(n_img * l.npix, GEMM_BK);
    int sps = ceil_div(ksteps, l.gw_slabs);
    return ceil_div(ksteps, sps);
}

// (batchnorm.h, used by the impala torso's BatchNorm sites)
static inline const BnSite* bn_site_of(const Plan& P, int layer);
static int bn_site_forward(const BnSite& b, const float* params, float* ws, int rows, bool running, hipStream_t st);
static int bn_site_backward(const BnSite& b, const float* params, float* ws, float* dy, int rows, bool apply, hipStream_t st);
// Which heads a loss regresses (default: the plan's iterated pairs, online head oh + k on target head k, k < K).  The analysis
// agents evaluate single-pair losses on the multi-head network: online head 1 on target head 1 (analysisdqn.py:156-183).
struct HeadSel {
    int on0, tg0, K;
};

// ---- launch helpers shared by the three learn paths (plain / LayerNorm below, BatchNorm in batchnorm.h, the torso in impala.h) ----
// `rows`: the rows the gradient flows through (B, or all 2B rows of a BatchNorm network)

// The tensors one stream's optimizer launches update, in launch order: adam_kernel once per ADAM_MAX_ENTRIES of them.
struct AdamList {
    std::vector<AdamEntry> e;
    AdamList() { e.reserve(ADAM_MAX_ENTRIES); }
    void add(int64_t p_off, int64_t size, const float* g, int n_slabs, int64_t stride) {
        e.push_back(AdamEntry{p_off, size, stride, g, n_slabs, 0});
    }
    // entries [e0, e0 + ADAM_MAX_ENTRIES) as one launch's table; `per_block`: elements a workgroup of the launch covers
    AdamTable table(size_t e0, int per_block = 64) const {
        AdamTable tab;
        tab.n = 0;
        tab.total_blocks = 0;
        for (size_t k = e0; k < e.size() && k < e0 + ADAM_MAX_ENTRIES; ++k) {
            AdamEntry& t = tab.e[tab.n++];
            t = e[k];
            t.block_start = tab.total_blocks;
            tab.total_blocks += (int)((t.size + per_block - 1) / per_block);
        }
        return tab;
    }
    int launch(hipStream_t st, const Plan& P, const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, float* ws, float* grad_out,
               bool update) const {
        for (size_t e0 = 0; e0 < e.size(); e0 += ADAM_MAX_ENTRIES) {
            const AdamTable tab = table(e0);
            hipLaunchKernelGGL(adam_kernel, dim3(tab.total_blocks), dim3(256), 0, st, tab, params, adam_m, adam_v, ws + P.adam_tab_off, cfg->learning_rate,
                               cfg->adam_b1, cfg->adam_b2, cfg->adam_eps, grad_out, ws + P.wsplit_off, update ? 1 : 0);
            ISDQN_HIP_CHECK(hipGetLastError());
        }
        return ISDQN_OK;
    }
};

// per-head loss sums and the head-bias gradient (`width` columns) of the P.B transitions from the `n_blk` partial rows a loss kernel left
// in the workspace; `adam_count` non-null: also the step count and Adam's bias corrections
static int loss_finalize(const Plan& P, const isdqn_net_config* cfg, float* ws, int n_blk, int K, int width, float* losses, float* loss_accum,
                         bool head_bias_grad, int32_t* adam_count, hipStream_t st) {
    float* loss_part = ws + P.lpart_off;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(ceil_div(K, 16) + ceil_div(width, 16)), dim3(256), 0, st, loss_part, loss_part + (int64_t)n_blk * K, n_blk,
                       P.B, K, width, losses, loss_accum, head_bias_grad ? ws + P.dbh_off : nullptr, adam_count, cfg->adam_b1, cfg->adam_b2,
                       ws + P.adam_tab_off);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// targets, per-transition loss and dL/d(head output) of rows [0, B) from the head outputs of a finished forward (TD loss on the Q rows, or
// the HL-Gauss or the categorical projection loss on the logit rows, the quantile-regression loss on the quantile rows), then loss_finalize over the head layer's width (nlog_p: nha_p without histogram heads).
// `val_rows`: head-output rows [B][nlog_p] of the next states that supply the bootstrap value (null: rows [B, 2B) of the forward);
// `double_q`: selector head on0 + k of rows [B, 2B) of the forward -- the online parameters on the next states -- picks the action;
// Munchausen targets (cfg->munchausen_tau > 0): `state_val_rows`, head-output rows [B][nlog_p] of the states from the network that
// supplies the value (null: rows [0, B) of the forward)
// The per-transition discounts behind a batch that says it has them (include/isdqn_hip.h, isdqn_batch_discount), else null.
static inline const float* batch_discount(const isdqn_batch* batch) {
    return (batch->flags & ISDQN_BATCH_DISCOUNT) ? reinterpret_cast<const isdqn_batch_discount*>(batch)->discount : nullptr;
}

static int loss_and_finalize(const Plan& P, const isdqn_net_config* cfg, float* ws, const isdqn_batch* batch, int K, int on0, int tg0, bool learn,
                             int32_t* adam_count, float* qv, float* tg, double* priorities, float* losses, float* loss_accum, hipStream_t st,
                             bool double_q = false, const float* val_rows = nullptr, const float* state_val_rows = nullptr) {
    const int B = P.B;
    const Munchausen mu{cfg->munchausen_tau, cfg->munchausen_alpha, cfg->munchausen_clip};
    if (state_val_rows == nullptr) state_val_rows = ws + P.out_off;
    const float* mun_rows = mu.tau > 0.f ? state_val_rows : nullptr;
    const float* next_rows = ws + P.out_off + (int64_t)B * P.nlog_p;
    if (val_rows == nullptr) val_rows = next_rows;
    const float* sel_rows = double_q ? next_rows : nullptr;
    const int R = P.head_nb > 0 ? rows_per_wg(K, P.head_nb) : 0;  // distributional kernels: transitions per workgroup
    const int n_blk = R ? ceil_div(B, R) : ceil_div(B, TD_ROWS);
    float* loss_part = ws + P.lpart_off;
    HeadLossArgs a{};  // (head_loss.h)
    a.out = ws + P.out_off;
    a.val = val_rows;
    a.sel = sel_rows; a.sel_pitch = P.nlog_p; a.sel_head = on0;
    a.mun = mun_rows; a.mun_pitch = P.nlog_p; a.mun_head = tg0; a.mu = mu;
    a.B = B; a.R = R; a.K = K; a.on0 = on0; a.tg0 = tg0; a.A = P.n_actions;
    a.nb = P.head_nb; a.pitch = P.nlog_p;
    a.vmin = P.hl_min; a.eta = P.head_nb > 0 ? (P.hl_max - P.hl_min) / (float)P.head_nb : 0.f; a.sigma = P.hl_sigma;
    a.huber_delta = cfg->huber_delta;
    a.action = batch->action; a.reward = batch->reward; a.terminal = batch->terminal; a.loss_weights = batch->loss_weights;
    a.discount = batch_discount(batch); a.gamma_n = cfg->gamma_n;
    a.dout = learn ? ws + P.dout_off : nullptr;
    a.q_values = qv; a.targets = tg; a.priorities = priorities;
    a.loss_part = loss_part; a.dbh_part = loss_part + (int64_t)n_blk * K;
    auto launch = [&](auto kern, int threads, size_t dyn_lds) { hipLaunchKernelGGL(kern, dim3(n_blk), dim3(threads), dyn_lds, st, a); };
    const size_t dl_bytes = (size_t)R * K * P.head_nb * sizeof(float);  // s_dl of head_loss.h
    // NT = 64-value groups of a (head, action) a lane owns: the quantile and the categorical kernels are instantiated per count
    auto with_nt = [&](auto f) {
        switch (ceil_div(P.head_nb, 64)) {
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            case 3: f(std::integral_constant<int, 3>{}); break;
            default: f(std::integral_constant<int, 4>{}); break;
        }
    };
    if (P.qr)  // quantile heads (quantile.h): kappa = cfg->huber_delta (0: the plain pinball loss)
        with_nt([&](auto nt) {
            if (cfg->huber_delta > 0.f) launch(qr_loss_kernel<decltype(nt)::value, true>, QR_THREADS, dl_bytes);
            else launch(qr_loss_kernel<decltype(nt)::value, false>, QR_THREADS, dl_bytes);
        });
    else if (P.c51)  // categorical projection loss on the histogram heads (categorical.h)
        with_nt([&](auto nt) { launch(c51_loss_kernel<decltype(nt)::value>, C51_THREADS, dl_bytes); });
    else if (R)
        launch(hl_loss_kernel, 256, dl_bytes);
    else
        launch(td_kernel, 256, 2 * TD_ROWS * K * sizeof(float));
    ISDQN_HIP_CHECK(hipGetLastError());
    return loss_finalize(P, cfg, ws, n_blk, K, P.nlog_p, losses, loss_accum, learn, adam_count, st);
}

// LayerNorm scale / bias and layer bias of `l` from `n_rows` partial rows of (dgamma, dbeta, dbias) at `part`
static void add_ln_bias_entries(AdamList& adam, const Layer& l, const float* part, int n_rows, int64_t stride) {
    if (l.has_ln) {
        adam.add(l.g_off, l.out_p, part, n_rows, stride);
        adam.add(l.be_off, l.out_p, part + l.out_p, n_rows, stride);
    }
    if (l.b_off >= 0) adam.add(l.b_off, l.out_p, part + 2 * l.out_p, n_rows, stride);  // (the impala torso has no bias of its own)
}

// generic data gradient of conv layer `l`: da [rows][hin][win][cin_p] fp32
static int conv_dgrad(const Layer& l, bool x3, const float* wmir, const float* dz, float* da, int rows, hipStream_t st) {
    const bool small = l.cin_p <= 32;
    if (x3) return small ? launch_conv_dgrad<32, 3>(l, wmir, dz, da, rows, st) : launch_conv_dgrad<64, 3>(l, wmir, dz, da, rows, st);
    return small ? launch_conv_dgrad<32, 1>(l, wmir, dz, da, rows, st) : launch_conv_dgrad<64, 1>(l, wmir, dz, da, rows, st);
}

// data gradient of dense layer `l`: da[b][in_p] = sum_o dz[b][o] * W[o][in_p]  (dz: the fp32 dL/dq of the head, S8 for a hidden layer)
// `narrow`: 128 x 64 tiles
static int dense_dgrad(const Layer& l, bool x3, const float* wmir, const float* dz, int dz_ld, float* da, int rows, bool narrow, hipStream_t st) {
    MatSrc A{dz, dz_ld, rows, l.out_p, 1};
    MatSrc Bm{wmir + l.w_off, l.in_p, l.out_f, l.in_p, 1};
    if (l.is_head)
        return narrow ? plain_narrow<false, true, 2>(x3, A, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st)
                      : plain_big<false, true, true, false, 2>(x3, A, nullptr, 0, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st);
    return narrow ? plain_narrow<false, true, DZ_S8 | 2>(x3, A, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st)
                  : plain_big<false, true, true, false, DZ_S8 | 2>(x3, A, nullptr, 0, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st);
}

// weight gradient of conv layer `l` into its slabs (image-resident kernel where the layer qualifies); *n_slabs: the slabs written
// (l.is_u8 only on the first layer of a cnn without BatchNorm, net_plan.h)
static int conv_wgrad(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, float* slabs, int rows, hipStream_t st,
                      int* n_slabs) {
    int rc = conv_wgrad_img(l, x3, in, act_in, dz, slabs, rows, st, n_slabs);
    if (rc || *n_slabs) return rc;
    *n_slabs = conv_wgrad_slabs(l, rows);
    if (l.is_u8) return x3 ? launch_conv_wgrad<2, true>(l, in, act_in, dz, slabs, rows, st) : launch_conv_wgrad<1, true>(l, in, act_in, dz, slabs, rows, st);
    return x3 ? launch_conv_wgrad<3, false>(l, in, act_in, dz, slabs, rows, st) : launch_conv_wgrad<1, false>(l, in, act_in, dz, slabs, rows, st);
}

// weight gradient of dense layer `l` into its effective_splits(rows, l.gw_slabs) slabs:
// dW[out][in_p] = sum_b dz[b][out] * a[b][in_p], both operands stored [K = b][rows]
static int dense_wgrad(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, int dz_ld, float* slabs, int rows,
                       hipStream_t st) {
    const MatSrc A{dz, dz_ld, rows, l.out_p, 1};
    const MatSrc Bm = l.in_unpadded_ld ? MatSrc{in.obs, l.in_unpadded_ld, rows, l.in_f, 0} : MatSrc{act_in, l.in_p, rows, l.in_p, 1};
    if (l.in_unpadded_ld)  // fc first layer: caller's fp32 observations
        return plain_big<true, true, false, false, DZ_S8>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
    if (l.is_head)  // dL/dq is fp32, the hidden activations are S8
        return plain_big<true, true, true, false, 2>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
    return plain_big<true, true, true, false, DZ_S8 | 2>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
}

#include "impala.h"
#include "batchnorm.h"

}  // namespace isdqn

using namespace isdqn;

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build (gemm_core.h: ISDQN_BOUNDS_CHECK): register the byte extents of every tensor the caller hands to
// the library -- [lo[i], hi[i]) -- and clear the record; read back the first load that fell outside all of them (synchronises).
extern "C" int isdqn_debug_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int isdqn_net_param_layout(const isdqn_net_config* cfg, int64_t* n_param_floats, isdqn_tensor_info* infos,
                                      int32_t max_infos, int32_t* n_infos) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    if (n_param_floats) *n_param_floats = P.n_params;
    int n = 0;
    for_each_param_tensor(P, [&](const isdqn_tensor_info& t) {
        if (infos && n < max_infos) memcpy(&infos[n], &t, sizeof(t));
        ++n;
    });
    if (n_infos) *n_infos = n;
    return ISDQN_OK;
}

extern "C" int isdqn_net_workspace_bytes(const isdqn_net_config* cfg, int64_t* bytes) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(bytes != nullptr, ISDQN_ERR_ARG, "null pointer");
    *bytes = P.ws_bytes;
    return ISDQN_OK;
}

extern "C" int isdqn_net_workspace_region(const isdqn_net_config* cfg, const char* name, int64_t* offset_bytes,
                                          int64_t* size_bytes) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(name != nullptr, ISDQN_ERR_ARG, "null name");
    for (auto& r : P.regions)
        if (r.first == name) {
            if (offset_bytes) *offset_bytes = r.second.first;
            if (size_bytes) *size_bytes = r.second.second;
            return ISDQN_OK;
        }
    set_last_error("unknown workspace region '%s'", name);
    return ISDQN_ERR_ARG;
}

// Histogram / quantile heads: Q rows `q` [n_rows][nha_p] <- expectations of the logit rows / means of the quantile rows `rows`
// [n_rows][nlog_p] (no-op for scalar heads).
static int head_expect_rows(const Plan& P, const float* rows, int n_rows, float* q, hipStream_t st) {
    if (P.head_nb == 0) return ISDQN_OK;
    const int64_t waves = (int64_t)n_rows * P.nha;
    if (P.qr)
        hipLaunchKernelGGL(qr_expect_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rows, n_rows, P.nha, P.head_nb, P.nlog_p,
                           P.nha_p, q);
    else
        hipLaunchKernelGGL(hl_expect_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rows, n_rows, P.nha, P.head_nb,
                           P.nlog_p, P.nha_p, P.hl_min, (P.hl_max - P.hl_min) / (float)P.head_nb, q);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}
// the rows the forward left in the "logits" region -> the "q" region
static int head_expect(const Plan& P, float* ws, int n_rows, hipStream_t st) {
    return head_expect_rows(P, ws + P.logits_off, n_rows, ws + P.q_off, st);
}

static int check_input(const isdqn_net_config* cfg, const uint8_t* frames, int64_t frame_stride,
                       const int32_t* frame_ids, const float* obs) {
    if (cfg->arch != ISDQN_ARCH_FC) {
        ISDQN_REQUIRE(frames && frame_ids, ISDQN_ERR_ARG, "cnn / impala need frames and frame_ids");
        ISDQN_REQUIRE(frame_stride >= (int64_t)cfg->obs_h * cfg->obs_w, ISDQN_ERR_SHAPE, "frame_stride < h*w");
    } else {
        ISDQN_REQUIRE(obs != nullptr, ISDQN_ERR_ARG, "fc needs obs");
    }
    return ISDQN_OK;
}

extern "C" int isdqn_net_forward(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                 int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                                 float* q_out, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && q_out && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2*batch_size]");
    rc = check_input(cfg, frames, frame_stride, frame_ids, obs);
    if (rc) return rc;
    NetInput in{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    rc = refresh_mirror(P, params, ws, st);
    if (rc) return rc;
    rc = net_forward(P, cfg->precision == ISDQN_PRECISION_BF16X3, params, in, n_rows, 0, ws, ws + P.out_off, st);
    if (rc) return rc;
    rc = head_expect(P, ws, n_rows, st);
    if (rc) return rc;
    // q_out is the unpadded (n_rows, nha) view
    ISDQN_HIP_CHECK(hipMemcpy2DAsync(q_out, (size_t)P.nha * 4, ws + P.q_off, (size_t)P.nha_p * 4, (size_t)P.nha * 4,
                                     n_rows, hipMemcpyDeviceToDevice, st));
    return ISDQN_OK;
}

// Side stream for the weight gradients.  The backward's critical path is dgrad -> LayerNorm-backward -> dgrad ...;
// every weight gradient only needs its layer's dz and is needed again by Adam at the very end, so they run on a
// second HIP stream and share the CUs with the data-gradient chain (both sides are partly latency bound and
// their workgroups co-reside).  One stream + event pool per device, created on first use, never destroyed.
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2 * MAX_LAYERS + 4];
    int n_ev = 0;
    std::atomic<unsigned> next{0};  // several agents / host threads of one process may share a device's pool
    std::atomic<int> state{0};      // 0 = not created, 1 = being created, 2 = ready, -1 = unavailable
};
static SideStream* side_stream() {
    static SideStream per_dev[ISDQN_MAX_DEVICES];
    if (ISDQN_DEV_ENV("ISDQN_SINGLE_STREAM")) return nullptr;
    SideStream& s = per_dev[current_device_slot()];
    int st = s.state.load(std::memory_order_acquire);
    if (st == 2) return &s;
    if (st == -1) return nullptr;
    int expected = 0;
    if (s.state.compare_exchange_strong(expected, 1)) {
        bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
        s.n_ev = 2 * MAX_LAYERS + 4;
        for (int i = 0; ok && i < s.n_ev; ++i) ok = hipEventCreateWithFlags(&s.ev[i], hipEventDisableTiming) == hipSuccess;
        s.state.store(ok ? 2 : -1, std::memory_order_release);
        return ok ? &s : nullptr;
    }
    while ((st = s.state.load(std::memory_order_acquire)) == 1) {}  // another thread is creating it
    return st == 2 ? &s : nullptr;
}
static hipEvent_t next_event(SideStream* ss) { return ss->ev[ss->next.fetch_add(1, std::memory_order_relaxed) % (unsigned)ss->n_ev]; }
// make `waiter` wait for everything enqueued so far on `signaller`
static int chain(SideStream* ss, hipStream_t signaller, hipStream_t waiter) {
    hipEvent_t e = next_event(ss);
    ISDQN_HIP_CHECK(hipEventRecord(e, signaller));
    ISDQN_HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
    return ISDQN_OK;
}

// What a learn / loss / gradient-only call on a network without BatchNorm fixes before its first launch (learn_or_loss).
struct LearnCtx {
    const Plan& P;
    const isdqn_net_config* cfg;
    const isdqn_batch* batch;
    float *params, *adam_m, *adam_v;
    int32_t* adam_count;
    const float* target_params;
    float *losses, *loss_accum, *qv, *tg;  // qv / tg: the caller's q_values / targets, or their workspace regions
    double* priorities;
    float* ws;
    float* grad_out;
    hipStream_t st;  // the caller's stream
    bool learn, update, x3;
    int B, K, on0, tg0;
    NetInput in;
    SideStream* ss = nullptr;   // learn steps: the weight-gradient stream (nullptr: everything runs on the caller's stream)
    hipStream_t wst = nullptr;  // stream of the weight gradients: ss->stream, or st
    bool double_q = false;      // Double Q-learning targets (cfg->double_q, unless selector and value are the same head of the same rows)
    bool munchausen = false;    // Munchausen targets (cfg->munchausen_tau > 0); excludes double_q (build_plan)
    int hc_S = 0, hc_wg = 0;    // head chain (head_chain_plan): transitions per workgroup, workgroups; 0 = generic loss and head backward
    const float* wmir() const { return ws + P.wsplit_off; }
    const Layer& hid() const { return P.L[P.n_layers >= 2 ? P.n_layers - 2 : 0]; }
    const Layer& head() const { return P.L[P.n_layers - 1]; }
};

// head chain eligibility (learn steps on the plan's own heads): last hidden layer dense + ReLU, widths within the kernel's limits
static void head_chain_plan(LearnCtx& c, bool plan_heads) {
    const Plan& P = c.P;
    const Layer& hid = c.hid();
    static const bool hc_disabled = ISDQN_DEV_ENV("ISDQN_NO_HEAD_CHAIN");
    // (histogram and quantile heads take the generic backward: head GEMMs at the logit width; the head chain is built for scalar heads)
    // (dueling heads too: the chain multiplies by the head kernel itself and knows no combine)
    if (P.dueling) return;
    if (!(c.learn && c.update && plan_heads && !hc_disabled && c.target_params == nullptr && P.head_nb == 0 && P.n_layers >= 2 && hid.kind == 1 &&
          !hid.is_head && hid.has_relu && hid.out_p <= HC_THREADS * HC_MAX_COLS && hid.out_p % 8 == 0))
        return;
    // transitions per workgroup: the per-transition phases scale with S (the kernel is instruction-issue bound) while
    // every workgroup streams the whole head matrix from L2, so S follows the batch: about 256 workgroups
    const int S = c.B >= 1024 ? 4 : c.B >= 512 ? 2 : 1;
    const int n_wg = ceil_div(c.B, S);
    if (n_wg <= hid.part_rows && S * c.K <= HC_THREADS && head_chain_lds_bytes(hid.out_p, P.nha_p, c.K, c.x3 ? 3 : 1, S) <= 150 * 1024) {
        c.hc_S = S;
        c.hc_wg = n_wg;
    }
}

static int learn_forward(const LearnCtx& c) {
    const Plan& P = c.P;
    const isdqn_batch* batch = c.batch;
    float* ws = c.ws;
    const int B = c.B;
    int rc;
    if (c.target_params != nullptr && c.munchausen) {
        // Munchausen DQN: the target parameters value the states too, so they run over concat(state, next_state) (2B rows of head
        // output -> "q_target" / "logits_target", states first); then the online parameters over the B states, as the DQN form below
        const int stack = c.cfg->arch != ISDQN_ARCH_FC ? c.cfg->obs_c : 0;
        rc = refresh_mirror(P, c.target_params, ws, c.st);
        if (rc) return rc;
        rc = net_forward(P, c.x3, c.target_params, c.in, P.N2, 0, ws, ws + P.out_t_off, c.st);
        if (rc) return rc;
        if (P.head_nb > 0) {
            rc = head_expect_rows(P, ws + P.logits_t_off, P.N2, ws + P.qt_off, c.st);
            if (rc) return rc;
        }
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
        NetInput on{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->state, nullptr, 0, 2 * stack, 0};
        return net_forward(P, c.x3, c.params, on, B, B, ws, ws + P.out_off, c.st);
    }
    if (c.target_params != nullptr && c.double_q) {
        // Double DQN: the target parameters value the B next states (head output -> "q_target" / "logits_target"), then ONE forward
        // of the online parameters over concat(state, next_state) as the iS-DQN path runs it: its next-state rows select
        const int stack = c.cfg->arch != ISDQN_ARCH_FC ? c.cfg->obs_c : 0;
        NetInput nx{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->next_state, nullptr, 0, 2 * stack, stack};
        rc = refresh_mirror(P, c.target_params, ws, c.st);
        if (rc) return rc;
        rc = net_forward(P, c.x3, c.target_params, nx, B, 0, ws, ws + P.out_t_off, c.st);
        if (rc) return rc;
        if (P.head_nb > 0) {
            rc = head_expect_rows(P, ws + P.logits_t_off, B, ws + P.qt_off, c.st);
            if (rc) return rc;
        }
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
        return net_forward(P, c.x3, c.params, c.in, P.N2, B, ws, ws + P.out_off, c.st);
    }
    if (c.target_params != nullptr) {
        // DQN (dqn.py:74-88): the next states go through the TARGET parameters, the states through the online ones: two
        // forwards of B images each over the same workspace, q rows [B, 2B) first, then rows [0, B) (+ z of every layer)
        const int stack = c.cfg->arch != ISDQN_ARCH_FC ? c.cfg->obs_c : 0;
        NetInput nx{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->next_state, nullptr, 0, 2 * stack, stack};
        rc = refresh_mirror(P, c.target_params, ws, c.st);
        if (rc) return rc;
        rc = net_forward(P, c.x3, c.target_params, nx, B, 0, ws, ws + P.out_off + (int64_t)B * P.nlog_p, c.st);
        if (rc) return rc;
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
        NetInput on{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->state, nullptr, 0, 2 * stack, 0};
        return net_forward(P, c.x3, c.params, on, B, B, ws, ws + P.out_off, c.st);
    }
    // The optimizer writes the updated parameters in both forms, so a learn step leaves the mirror current; a caller
    // that chains learn steps on one workspace with nothing else writing `params` in between says so
    // (ISDQN_BATCH_MIRROR_CURRENT: the captured multi-step graphs) and the refresh is skipped.
    if (!(batch->flags & ISDQN_BATCH_MIRROR_CURRENT)) {
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
    }
    // forward on concat(state, next_state) (isdqn.py:95); the head chain takes over at the last hidden layer's split-K slabs
    return net_forward(P, c.x3, c.params, c.in, P.N2, B, ws, ws + P.out_off, c.st, c.hc_S ? P.n_layers - 1 : -1, c.hc_S ? P.n_layers - 2 : -1);
}

static int launch_head_chain(const LearnCtx& c) {
    const Plan& P = c.P;
    const Layer &hid = c.hid(), &head = c.head();
    float* ws = c.ws;
    HeadChainParams hp;
    hp.act = ws + hid.act_off; hp.z = ws + hid.z_off;
    hp.slabs = ws + P.slab_off;
    hp.n_slabs = effective_splits(hid.in_unpadded_ld ? hid.in_f : hid.K, hid.fwd_splits);
    hp.slab_stride = hid.out_p;
    hp.row_pitch = (int64_t)hp.n_slabs * hid.out_p;
    hp.hbias = c.params + hid.b_off;
    hp.W = c.params + head.w_off; hp.bias = c.params + head.b_off;
    hp.gamma = hid.has_ln ? c.params + hid.g_off : nullptr;
    hp.beta = hid.has_ln ? c.params + hid.be_off : nullptr;
    hp.B = c.B; hp.S = c.hc_S; hp.F = hid.out_f; hp.Fp = hid.out_p; hp.O = P.nha; hp.Op = P.nha_p; hp.K = c.K; hp.oh = P.oh;
    hp.A = P.n_actions;
    hp.action = c.batch->action; hp.reward = c.batch->reward; hp.terminal = c.batch->terminal;
    hp.loss_weights = c.batch->loss_weights; hp.discount = batch_discount(c.batch);
    hp.gamma_n = c.cfg->gamma_n; hp.huber_delta = c.cfg->huber_delta;
    hp.double_q = c.double_q ? 1 : 0;
    hp.mu = Munchausen{c.cfg->munchausen_tau, c.cfg->munchausen_alpha, c.cfg->munchausen_clip};
    hp.dout = ws + P.dout_off; hp.dz = ws + hid.dz_off; hp.part = ws + hid.part_off;
    hp.q_values = c.qv; hp.targets = c.tg; hp.priorities = c.priorities;
    hp.loss_part = ws + P.lpart_off; hp.dbh_part = hp.loss_part + (int64_t)c.hc_wg * c.K;
    hp.adam_count = c.adam_count; hp.b1 = c.cfg->adam_b1; hp.b2 = c.cfg->adam_b2; hp.adam_consts = ws + P.adam_tab_off;
    hp.stamps = stamps_for("head_chain");
    const int lds = head_chain_lds_bytes(hid.out_p, P.nha_p, c.K, c.x3 ? 3 : 1, c.hc_S);
    const int cols = ceil_div(hid.out_p, HC_THREADS) <= 1 ? 1 : ceil_div(hid.out_p, HC_THREADS) <= 2 ? 2 : 4;
    auto launch_hc = [&](auto kern, int slot) -> int {
        static LdsConfigured configured[18];
        if (int rc2 = ensure_dynamic_lds(kern, lds, configured[slot])) return rc2;
        ISDQN_REPORT_OCCUPANCY(kern, HC_THREADS, lds, c.hc_wg);
        hipLaunchKernelGGL(kern, dim3(c.hc_wg), dim3(HC_THREADS), lds, c.st, hp);
        ISDQN_HIP_CHECK(hipGetLastError());
        return ISDQN_OK;
    };
    auto by_cols = [&](auto passes_c, auto s_c, int base) -> int {
        constexpr int PS = decltype(passes_c)::value, SS = decltype(s_c)::value;
        return cols == 1 ? launch_hc(&head_chain_kernel<PS, 1, SS>, base) : cols == 2 ? launch_hc(&head_chain_kernel<PS, 2, SS>, base + 1)
                                                                        : launch_hc(&head_chain_kernel<PS, 4, SS>, base + 2);
    };
    auto by_s = [&](auto passes_c, int base) -> int {
        return c.hc_S == 1 ? by_cols(passes_c, std::integral_constant<int, 1>{}, base)
             : c.hc_S == 2 ? by_cols(passes_c, std::integral_constant<int, 2>{}, base + 3)
                           : by_cols(passes_c, std::integral_constant<int, 4>{}, base + 6);
    };
    return c.x3 ? by_s(std::integral_constant<int, 3>{}, 0) : by_s(std::integral_constant<int, 1>{}, 9);
}

// The two small kernels that only need the head chain's outputs: the loss / head-bias sums of its per-workgroup partials, and the
// head's weight gradient (dL/dq fp32, hidden activations S8)
static int head_chain_sums(const LearnCtx& c, hipStream_t s) {
    return loss_finalize(c.P, c.cfg, c.ws, c.hc_wg, c.K, c.P.nha_p, c.losses, c.loss_accum, true, nullptr, s);
}
static int head_chain_tail(const LearnCtx& c, hipStream_t s) {
    if (int rc = head_chain_sums(c, s)) return rc;
    const Layer& head = c.head();
    return dense_wgrad(head, c.x3, c.in, c.ws + c.hid().act_off, c.ws + c.P.dout_off, c.P.nlog_p, c.ws + head.gw_off, c.B, s);
}

// targets, loss, dL/dq: q_values / targets / priorities / per-head loss partials are final behind it
static int learn_loss(const LearnCtx& c) {
    // the target network's own head output ("q_target" / "logits_target": next states; Munchausen: states, then next states)
    const bool tnet = (c.double_q || c.munchausen) && c.target_params != nullptr;
    if (!c.hc_S) {
        // (adam_count in a gradient-only pass: null from grad_on_batch; the noisy learn step hands its own, because its optimizer
        // launch follows the pass and reads the step count's bias corrections from the same place)
        int rc = loss_and_finalize(c.P, c.cfg, c.ws, c.batch, c.K, c.on0, c.tg0, c.learn, c.learn ? c.adam_count : nullptr, c.qv, c.tg,
                                   c.priorities, c.losses, c.loss_accum, c.st, c.double_q,
                                   tnet ? c.ws + c.P.out_t_off + (c.munchausen ? (int64_t)c.B * c.P.nlog_p : 0) : nullptr,
                                   (tnet && c.munchausen) ? c.ws + c.P.out_t_off : nullptr);
        if (rc || !(c.learn && c.P.dueling)) return rc;
        // dueling heads: dL/d(combined rows) and the reduced head-bias gradient -> the raw head's (dueling.h), where the backward starts
        const Plan& P = c.P;
        const int w = P.head_nb > 0 ? P.head_nb : 1;
        const int64_t threads = (int64_t)(c.B + 1) * P.n_heads * w;
        hipLaunchKernelGGL(duel_backward_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, c.st,
                           (const float*)(c.ws + P.dout_off), P.nlog_p, c.ws + P.dout_raw_off, P.raw_p, (const float*)(c.ws + P.dbh_off),
                           c.ws + P.dbh_raw_off, c.B, P.n_heads, P.n_actions, w);
        ISDQN_HIP_CHECK(hipGetLastError());
        return ISDQN_OK;
    }
    if (int rc = launch_head_chain(c)) return rc;
    // with a weight-gradient stream the sums leave the critical path: BackwardSchedule enqueues head_chain_tail() there
    return c.ss ? ISDQN_OK : head_chain_sums(c, c.st);
}

// One layer's weight gradient as the schedule sees it (plain data: a deferred one waits in BackwardSchedule)
struct WgradJob {
    int layer = -1;  // -1: none
    hipStream_t stream = nullptr;
    hipEvent_t wait = nullptr;  // deferred: the fork recorded on the caller's stream behind the layer's data gradient
    const float* dz = nullptr;  // gradient w.r.t. the layer's pre-activation output
    int dz_ld = 0;
};

// dense weight gradient straight into Adam: one workgroup holds the whole contraction
// (a gradient-only pass runs the same kernel with the stores of p / m / v switched off)
static int dense_wgrad_fused_adam(const LearnCtx& c, const Layer& l, const float* act_in, const WgradJob& j) {
    const MatSrc A{j.dz, j.dz_ld, c.B, l.out_p, 1};
    const MatSrc Bm{act_in, l.in_p, c.B, l.in_p, 1};
    AdamFuse af{c.params + l.w_off, c.adam_m + l.w_off, c.adam_v + l.w_off, c.ws + c.P.adam_tab_off,
                c.cfg->learning_rate, c.cfg->adam_b1, c.cfg->adam_b2, c.cfg->adam_eps,
                c.grad_out ? c.grad_out + l.w_off : nullptr, c.ws + c.P.wsplit_off + l.w_off, c.update ? 1 : 0};
    // 64x64 tiles: the contraction is only B deep, the kernel lives off streaming p/m/v through the Adam
    // epilogue, and 128x128 tiles would leave 100 workgroups for 256 CUs
    // (operands: dz of a hidden layer -- or the fp32 dL/dq of the head -- and the S8 activations below it)
    if (l.is_head)
        return c.x3 ? launch_plain<64, 64, 2, 2, true, true, 3, true, false, true, 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1, 0,
                                                                                      j.stream, &af)
                    : launch_plain<64, 64, 2, 2, true, true, 1, true, false, true, 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1, 0,
                                                                                      j.stream, &af);
    return c.x3 ? launch_plain<64, 64, 2, 2, true, true, 3, true, false, true, DZ_S8 | 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1,
                                                                                          0, j.stream, &af)
                : launch_plain<64, 64, 2, 2, true, true, 1, true, false, true, DZ_S8 | 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1,
                                                                                          0, j.stream, &af);
}

// weight gradient -> slabs and an entry in the optimizer list of its stream, or straight into Adam
// `adam`: [0] caller's stream, [1] weight-gradient stream
static int weight_gradient(const LearnCtx& c, const WgradJob& j, AdamList* adam) {
    const Layer& l = c.P.L[j.layer];
    float* ws = c.ws;
    const float* act_in = j.layer > 0 ? ws + c.P.L[j.layer - 1].act_off : nullptr;
    int w_slabs, rc;
    if (l.is_head && c.hc_S && c.ss) {  // enqueued by head_chain_tail()
        w_slabs = effective_splits(c.B, l.gw_slabs);
    } else if (l.kind == 0) {
        rc = conv_wgrad(l, c.x3, c.in, act_in, j.dz, ws + l.gw_off, c.B, j.stream, &w_slabs);
        if (rc) return rc;
    } else {
        w_slabs = effective_splits(c.B, l.gw_slabs);
        // (gradient clipping: no parameter may move before the norm of the whole gradient is known -- the one slab goes to "gw/")
        if (w_slabs == 1 && !l.in_unpadded_ld && !c.P.grad_clip) return dense_wgrad_fused_adam(c, l, act_in, j);
        rc = dense_wgrad(l, c.x3, c.in, act_in, j.dz, j.dz_ld, ws + l.gw_off, c.B, j.stream);
        if (rc) return rc;
    }
    adam[c.ss && j.stream == c.wst ? 1 : 0].add(l.w_off, l.w_size, ws + l.gw_off, w_slabs, l.w_size);
    return ISDQN_OK;
}

#if !defined(ISDQN_FORK_LATE_MAX_B)
#define ISDQN_FORK_LATE_MAX_B 768
#endif
// The side-stream policy of one learn step's backward pass: which stream a weight gradient runs on, where the caller's stream
// forks, and in which order the kernels behind a fork are created.  Without a side stream (c.ss == nullptr) nothing forks and
// every kernel is enqueued in line on the caller's stream.
//
//  * Streams.  Weight gradients of the middle layers go to the side stream.  Every fork costs the main stream an event record
//    (a ~6 us bubble), so the head's tiny weight gradient and the first layer's (nothing is left to overlap with) stay on the
//    main stream, and a dense layer (its Adam may be fused: an in-place update) forks once, AFTER its data gradient: dz is final
//    and the data gradient, which reads W, is enqueued, so the update on the side stream cannot overtake it.
//  * Tail swap.  With at least three layers the last two weight gradients swap streams: layer 1's follows its data gradient on
//    the caller's stream, layer 0's (which only needs that data gradient's output) runs beside it.
//  * Head chain.  Its loss / head-bias sums and the head's weight gradient (head_chain_tail) leave the critical path: they are
//    enqueued on the side stream behind the first fork the backward pass makes anyway (no fork is spent on these two small
//    kernels alone), or in line when no layer forked.
//  * The caller's event (batch->priorities_ready: q_values / targets / priorities are final behind the loss) is likewise
//    recorded at the first point that forks the caller's stream anyway, else at the end of the backward (no side stream: at once).
//  * Which queue the replayed graph gives a kernel: a node's FIRST-created successor stays on its queue, the others move to
//    another one and start ~12 us late.  Round 4's order (fork_late; c2 +1.2 %, c3 +7.5 %;
//    -DISDQN_FORK_LATE_MAX_B=0 keeps round 3's):
//      - the data-gradient chain is created first behind every fork, so it stays on the capturing queue all the way: a layer
//        that forks after its data gradient records the fork there, but its side-stream kernels are created (`deferred`, flush)
//        only after the NEXT layer's data gradient has been enqueued on the caller's stream;
//      - the two head kernels become successors of the HEAD CHAIN on the side stream (head_event) -- created behind the dense
//        data gradient, which therefore stays the head chain's first successor -- and run under the dense data gradient; the new
//        queue's late start is hidden there, and it is what lets the first convolution data gradient become resident before the
//        fused-Adam GEMM's 968 workgroups ask for the CUs.
//    Large batches keep round 3's order: at B = 1024 every kernel is several rounds of workgroups, which queue gets the CUs first
//    no longer matters and the new order measured 0.6 % slower (profiles/round4/ab_fork_c5.txt; ab_thresholds.txt: +2.0 % at
//    B = 32, +1.7 % at 128, +1.5 % at 512, +2.0 % at 768).
//  * Two optimizer lists: tensors whose gradient is produced on the side stream are updated there, the others on the caller's
//    stream, so the step ends with two short Adam launches side by side instead of join -> reduce -> one Adam.  The side
//    stream may update its own tensors only when every reader of the weights is behind it (adam_on_side): with the tail swap
//    its last kernel (layer 0's weight gradient) waited for the last data gradient of the caller's stream.
struct BackwardSchedule {
    const LearnCtx& c;
    AdamList* const adam;  // [0] caller's stream, [1] side stream
    const bool tail_swap, fork_late;
    bool prio_pending, head_pending;  // priorities_ready / head_chain_tail() still to be enqueued
    hipEvent_t head_event = nullptr;  // fork_late: the head chain's end on the caller's stream
    bool forked = false, layer0_chained = false;
    WgradJob deferred;  // the side-stream work of the layer above, held back until this layer's data gradient is enqueued

    BackwardSchedule(const LearnCtx& ctx, AdamList* lists)
        : c(ctx), adam(lists), tail_swap(ctx.ss && ctx.P.n_layers >= 3 && !ctx.P.L[1].is_head),
          fork_late(ctx.ss != nullptr && ctx.P.L[0].kind != 2 && ctx.B <= ISDQN_FORK_LATE_MAX_B),
          prio_pending(ctx.batch->priorities_ready != nullptr), head_pending(ctx.hc_S && ctx.ss) {}

    bool wgrad_on_side(int i) const { return c.ss && !c.P.L[i].is_head && (tail_swap ? i != 1 : i > 0); }
    // (the head's weight gradient behind a head chain: head_chain_tail() on the side stream)
    hipStream_t wgrad_stream(int i) const { return wgrad_on_side(i) || (c.P.L[i].is_head && c.hc_S) ? c.wst : c.st; }
    bool forks_after_dgrad(int i) const { return wgrad_on_side(i) && c.P.L[i].kind == 1 && i > 0; }
    // dz of the layer is final on the main stream (layer 0 with the tail swap: chain_layer0() already forked)
    bool forks_before_dgrad(int i) const { return wgrad_on_side(i) && !forks_after_dgrad(i) && !(i == 0 && layer0_chained); }
    // (gradient clipping: never -- both streams join in front of the norm, learn_optimizer)
    bool adam_on_side() const { return c.ss && forked && tail_swap && !c.P.grad_clip; }

    int signal_priorities() {
        if (prio_pending) {
            prio_pending = false;
            ISDQN_HIP_CHECK(hipEventRecord((hipEvent_t)c.batch->priorities_ready, c.st));
        }
        return ISDQN_OK;
    }
    int run_head_tail(hipStream_t s) {
        if (!head_pending) return ISDQN_OK;
        head_pending = false;
        return head_chain_tail(c, s);
    }
    // behind the loss, in front of the first layer
    int begin() {
        if (!c.ss)
            if (int rc = signal_priorities()) return rc;
        if (fork_late && head_pending) {
            head_event = next_event(c.ss);
            ISDQN_HIP_CHECK(hipEventRecord(head_event, c.st));
        }
        return ISDQN_OK;
    }
    // fork in front of a layer's data gradient
    int fork(hipStream_t side) {
        if (int rc = chain(c.ss, c.st, side)) return rc;
        if (int rc = signal_priorities()) return rc;
        forked = true;
        // (held-back side work of the layer above enqueues the two head kernels itself, behind this layer's data gradient)
        return deferred.layer < 0 ? run_head_tail(side) : ISDQN_OK;
    }
    // fork behind a layer's data gradient; *defer: the job's kernels wait (as `deferred`) for the next layer's data gradient
    int fork_after_dgrad(WgradJob& job, bool* defer) {
        if (!fork_late) {
            if (int rc = chain(c.ss, c.st, job.stream)) return rc;
            if (int rc = signal_priorities()) return rc;
            forked = true;
            return run_head_tail(job.stream);
        }
        if (head_event != nullptr && head_pending) {  // (the dense data gradient is enqueued: the head chain keeps it as first successor)
            ISDQN_HIP_CHECK(hipStreamWaitEvent(job.stream, head_event, 0));
            if (int rc = run_head_tail(job.stream)) return rc;
        }
        job.wait = next_event(c.ss);
        ISDQN_HIP_CHECK(hipEventRecord(job.wait, c.st));
        *defer = true;
        forked = true;
        return signal_priorities();
    }
    // tail swap, behind layer 1's fused data gradient: layer 0's dz is final, its weight gradient may start beside layer 1's
    int chain_layer0() {
        if (int rc = chain(c.ss, c.st, c.wst)) return rc;
        forked = layer0_chained = true;
        return run_head_tail(c.wst);
    }
    // the held-back side-stream work, now that the data gradient it yields to is enqueued
    int flush() {
        if (deferred.layer < 0) return ISDQN_OK;
        const WgradJob j = deferred;
        deferred.layer = -1;
        ISDQN_HIP_CHECK(hipStreamWaitEvent(j.stream, j.wait, 0));
        if (int rc = run_head_tail(j.stream)) return rc;
        return weight_gradient(c, j, adam);
    }
    // behind the last layer
    int finish() {
        if (int rc = flush()) return rc;
        if (int rc = run_head_tail(c.st)) return rc;  // no layer forked: keep the two kernels in line
        return signal_priorities();
    }
};

// first dense layer over a 64-channel conv output: data gradient + LN/ReLU backward of the layer below in one kernel
static bool dense_dgrad_ln_applies(const Layer& l, const Layer& below, int B) {
    return l.kind == 1 && below.kind != 1 && below.cout_p == 64 && !l.in_unpadded_ld && below.part_rows >= ceil_div(B, 128) * below.npix;
}
static int dense_dgrad_ln(const LearnCtx& c, const Layer& l, const Layer& below, const float* dz, int dz_ld, ReduceJobs* red) {
    float* ws = c.ws;
    const int B = c.B;
    auto launch = [&](auto prob) {
        prob.A = MatSrc{dz, dz_ld, B, l.out_p, 1};
        prob.B = MatSrc{c.wmir() + l.w_off, l.in_p, l.out_f, l.in_p, 1};
        prob.z = ws + below.z_off;
        prob.gamma = below.has_ln ? c.params + below.g_off : nullptr;
        prob.beta = below.has_ln ? c.params + below.be_off : nullptr;
        prob.dz_out = ws + below.dz_off;
        prob.part = ws + below.part_off;
        prob.ldc = l.in_p; prob.M = B; prob.N = l.in_p; prob.K = l.out_p; prob.c_in = below.out_f;
        prob.tiles_m = ceil_div(B, decltype(prob)::BM); prob.tiles_n = l.in_p / 64;
        return launch_gemm(prob, prob.tiles_m * prob.tiles_n, c.st);
    };
    // 128-row tiles (8 accumulators per wave).  64-row tiles fill the chip better (196 workgroups, -3 us)
    // but are a four-accumulator kernel, and those are not run-to-run stable on gfx950
    // at most one workgroup per CU (242 at the headline size): two K groups of four waves (gemm_core.h)
    static const bool no_kg = ISDQN_DEV_ENV("ISDQN_NO_KGROUPS");
    const bool kg2 = !no_kg && ceil_div(B, 128) * (l.in_p / 64) <= 256 && l.out_p % 64 == 0;
    int rc;
    // ISDQN_DGRAD64 (development): 64-row tiles, one K group
#if defined(ISDQN_DGRAD64)
    (void)kg2;
    rc = c.x3 ? launch(DenseDgradLN<3, 64>{}) : launch(DenseDgradLN<1, 64>{});
    constexpr int DG_BM = 64;
#else
    if (kg2) rc = c.x3 ? launch(DenseDgradLN<3, 128, 2>{}) : launch(DenseDgradLN<1, 128, 2>{});
    else rc = c.x3 ? launch(DenseDgradLN<3, 128>{}) : launch(DenseDgradLN<1, 128>{});
    constexpr int DG_BM = 128;
#endif
    if (rc) return rc;
    add_reduce_job(*red, ws + below.part_off, ceil_div(B, DG_BM) * (l.in_p / 64), 3 * below.out_p, ws + below.red_off);
    return ISDQN_OK;
}

// data gradient of layer i > 0 for the layer below.  *dz_fused: a fused kernel also ran the LN/ReLU backward of the layer below (its dz
// is written, the partial rows of its parameter gradients are a job in `red`); otherwise da (w.r.t. that layer's activation) is in ws+da_off
static int data_gradient(const LearnCtx& c, int i, const float* dz, int dz_ld, bool* dz_fused, ReduceJobs* red) {
    const Layer &l = c.P.L[i], &below = c.P.L[i - 1];
    float* da = c.ws + c.P.da_off;
    *dz_fused = false;
    if (l.is_head && c.hc_S) return ISDQN_OK;  // dz of the hidden layer came from the head chain
    if (l.kind == 0) {
        int rc = conv_dgrad_img(l, below, c.x3, c.params, c.wmir(), dz, c.ws, c.B, c.st, dz_fused, red);
        if (rc || *dz_fused) return rc;
        return conv_dgrad(l, c.x3, c.wmir(), dz, da, c.B, c.st);
    }
    if (dense_dgrad_ln_applies(l, below, c.B)) {
        *dz_fused = true;
        return dense_dgrad_ln(c, l, below, dz, dz_ld, red);
    }
    const bool narrow = ceil_div(c.B, 128) * ceil_div(l.in_p, 128) < 200;
    return dense_dgrad(l, c.x3, c.wmir(), dz, dz_ld, da, c.B, narrow, c.st);
}

// backward (online rows only: the next-state half has a zero cotangent, isdqn.py:99), top layer first.  Per layer: parameter-gradient
// entries -> maybe fork -> data gradient for the layer below -> what the layer above deferred -> fork after the data gradient, or
// defer -> weight gradient
static int learn_backward(const LearnCtx& c, BackwardSchedule& sched, AdamList* adam, ReduceJobs* red) {
    const Plan& P = c.P;
    float* ws = c.ws;
    const int B = c.B;
    int rc;
    // gradient w.r.t. the current layer's pre-activation output (dueling heads: of the raw head, "dout_raw" / "dbh_raw")
    const float* dz_cur = ws + (P.dueling ? P.dout_raw_off : P.dout_off);
    int dz_ld = P.dueling ? P.raw_p : P.nlog_p;
    bool dz_fused = false;  // dz of layer i was already produced by the fused data gradient of layer i+1
    for (int i = P.n_layers - 1; i >= 0; --i) {
        const Layer& l = P.L[i];
        if (l.is_head) {
            adam[c.hc_S && c.ss ? 1 : 0].add(l.b_off, l.out_p, ws + (P.dueling ? P.dbh_raw_off : P.dbh_off), 1, 0);  // loss_finalize_kernel's stream
        } else {
            dz_cur = ws + l.dz_off;
            dz_ld = l.out_p;
            if (c.hc_S && i == P.n_layers - 2) {  // dz and the partial sums came from the head chain
                add_ln_bias_entries(adam[0], l, ws + l.part_off, c.hc_wg, 3 * (int64_t)l.out_p);
            } else if (dz_fused) {  // (reduce_rows_kernel, in front of Adam)
                add_ln_bias_entries(adam[0], l, ws + l.red_off, 1, 0);
            } else {
                // da (w.r.t. this layer's activation) was left in ws+da_off by layer i+1's data-gradient
                int nb = 0;
                rc = ln_bwd(l, c.params, ws + P.da_off, ws + l.z_off, l.kind != 1 ? B * l.npix : B, ws + l.dz_off, ws + l.part_off, &nb, c.st);
                if (rc) return rc;
                add_ln_bias_entries(adam[0], l, ws + l.part_off, nb, 3 * (int64_t)l.out_p);
            }
        }
        if (l.kind == 2) {  // the impala torso: its own backward (generic engine + row-wise kernels) and optimizer launches, on the caller's stream
            rc = impala_backward(P, c.cfg, c.x3, c.params, c.adam_m, c.adam_v, c.wmir(), ws, B, c.grad_out, c.update, c.st);
            if (rc) return rc;
            continue;
        }
        WgradJob job;
        job.layer = i; job.stream = sched.wgrad_stream(i); job.dz = dz_cur; job.dz_ld = dz_ld;
        if (sched.forks_before_dgrad(i)) {
            rc = sched.fork(job.stream);
            if (rc) return rc;
        }
        // data gradient for the layer below first: it reads this layer's weights, which the fused-Adam
        // weight-gradient epilogue below updates in place
        dz_fused = false;
        if (i > 0) {
            rc = data_gradient(c, i, dz_cur, dz_ld, &dz_fused, red);
            if (rc) return rc;
        }
        rc = sched.flush();
        if (rc) return rc;
        bool defer = false;
        if (sched.forks_after_dgrad(i)) {
            rc = sched.fork_after_dgrad(job, &defer);
            if (rc) return rc;
        }
        if (sched.tail_swap && i == 1 && dz_fused) {
            rc = sched.chain_layer0();
            if (rc) return rc;
        }
        if (defer) {
            sched.deferred = job;
        } else {
            rc = weight_gradient(c, job, adam);
            if (rc) return rc;
        }
    }
    return sched.finish();
}

// Gradient clipping (cfg->max_grad_norm > 0; grad_clip.h), on the caller's stream behind the join of both streams and behind
// reduce_rows_kernel.  The entries of both lists in two tables: those with several slabs -> grad_reduce_sq_kernel (the reduced
// gradient over slab 0, one float64 sum of squares per workgroup), those whose one slab IS the reduced gradient (the Dense kernels
// that would have been fused into Adam, the reduced rows, the head bias) -> grad_flat_sq_kernel, 1024 elements per workgroup; the
// dueling head's structural zeros leave the gradient in whichever of the two holds the head kernel.  Then grad_clip_finalize_kernel
// (norm, scale, accumulators -> "grad_clip") and one adam_flat_kernel over every entry at its slab 0, multiplied by the scale.  A
// gradient-only pass runs all of them: the Adam launch is what writes grad_out
static int clipped_adam(const LearnCtx& c, const AdamList* adam) {
    const Plan& P = c.P;
    AdamList multi, single, all;
    for (int k = 0; k < 2; ++k)
        for (const AdamEntry& t : adam[k].e) {
            (t.n_slabs > 1 ? multi : single).e.push_back(t);
            all.add(t.p_off, t.size, t.g, 1, 0);
        }
    ISDQN_REQUIRE(all.e.size() <= (size_t)ADAM_MAX_ENTRIES, ISDQN_ERR_UNSUPPORTED, "gradient clipping: more tensors than one optimizer table holds");
    const AdamTable tab_m = multi.table(0), tab_s = single.table(0, GC_FLAT_ELEMS), tab_a = all.table(0, GC_FLAT_ELEMS);
    const int n_part = tab_m.total_blocks + tab_s.total_blocks;
    ISDQN_REQUIRE(n_part <= P.gc_part_cap, ISDQN_ERR_SHAPE, "gradient clipping: more workgroups than the partials region holds");
    GradClipMask dm{-1, 0, 0, 0, 0, 0, 0};
    if (P.dueling) dm = GradClipMask{c.head().w_off, c.head().in_p, P.raw, P.n_actions, P.head_nb > 0 ? P.head_nb : 1, P.duel_f2, P.duel_f};
    double* partials = reinterpret_cast<double*>(c.ws + P.gc_part_off);
    float* gc = c.ws + P.gc_off;
    if (tab_m.total_blocks > 0) {
        hipLaunchKernelGGL(grad_reduce_sq_kernel, dim3(tab_m.total_blocks), dim3(256), 0, c.st, tab_m, dm, partials);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (tab_s.total_blocks > 0) {
        hipLaunchKernelGGL(grad_flat_sq_kernel, dim3(tab_s.total_blocks), dim3(GC_FLAT_THREADS), 0, c.st, tab_s, dm, partials + tab_m.total_blocks);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(GC_FIN_THREADS), 0, c.st, (const double*)partials, n_part, c.cfg->max_grad_norm, gc,
                       c.update ? 1 : 0);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(adam_flat_kernel, dim3(tab_a.total_blocks), dim3(GC_FLAT_THREADS), 0, c.st, tab_a, c.params, c.adam_m, c.adam_v,
                       (const float*)(c.ws + P.adam_tab_off), c.cfg->learning_rate, c.cfg->adam_b1, c.cfg->adam_b2, c.cfg->adam_eps, c.grad_out,
                       c.ws + P.wsplit_off, c.update ? 1 : 0, (const float*)(gc + 1));
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// the partial-row reductions the fused data gradients left, and the optimizer launches of both streams; the call is complete on
// the caller's stream behind it (and the next call may touch the workspace)
static int learn_optimizer(const LearnCtx& c, const BackwardSchedule& sched, const AdamList* adam, const ReduceJobs& red) {
    auto run_adam = [&](const AdamList& list, hipStream_t s) {
        return list.launch(s, c.P, c.cfg, c.params, c.adam_m, c.adam_v, c.ws, c.grad_out, c.update);
    };
    int rc;
    if (sched.adam_on_side()) {
        rc = run_adam(adam[1], c.wst);
        if (rc) return rc;
    } else if (c.ss) {  // all weight gradients done before Adam
        rc = chain(c.ss, c.wst, c.st);
        if (rc) return rc;
    }
    if (red.n > 0) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(red.block_start[red.n]), dim3(256), 0, c.st, red);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (c.P.grad_clip) {  // (adam_on_side() is false: the side stream was joined above, every gradient of the step is final here)
        rc = clipped_adam(c, adam);
    } else {
        rc = run_adam(adam[0], c.st);
        if (rc) return rc;
        rc = sched.adam_on_side() ? chain(c.ss, c.wst, c.st) : run_adam(adam[1], c.st);
    }
    if (rc || !c.P.dueling) return rc;
    // dueling heads: behind the head's Adam the structural zeros of the head kernel are written again (Adam is per element: this equals
    // a masked gradient exactly).  What orders the launch: without a head chain BackwardSchedule keeps the head's weight gradient --
    // fused into Adam, or reduced by run_adam(adam[0]) above -- and its bias entry on the caller's stream, and whatever the side stream
    // updates is joined into the caller's stream by chain(c.ss, c.wst, c.st), in front of Adam or in the line above; so every optimizer
    // launch of the step is behind this point on c.st.  A schedule that moves the head's update to the side stream has to keep that
    // join in front of this launch.  A gradient-only pass masks grad_out alone
    const Plan& P = c.P;
    const Layer& head = c.head();
    const int64_t threads = (int64_t)P.raw * P.duel_f2;
    float* const none = nullptr;
    hipLaunchKernelGGL(duel_mask_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, c.st,
                       c.update ? c.params : none, c.update ? c.adam_m : none, c.update ? c.adam_v : none, c.update ? c.ws + P.wsplit_off : none,
                       c.grad_out, head.w_off, head.in_p, P.raw, P.n_actions, P.head_nb > 0 ? P.head_nb : 1, P.duel_f2);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static int learn_or_loss(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, int32_t* adam_count,
                         const isdqn_batch* batch, float* losses, float* loss_accum, float* q_values, float* targets,
                         double* priorities, void* workspace, void* stream, bool learn, float* grad_out,
                         const float* target_params = nullptr, const HeadSel* sel = nullptr, bool update = true) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && batch && losses && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(batch->B == P.B, ISDQN_ERR_SHAPE, "batch->B != cfg->batch_size");
    ISDQN_REQUIRE(batch->action && batch->reward && batch->terminal, ISDQN_ERR_ARG, "null batch field");
    rc = check_input(cfg, batch->frames, batch->frame_stride, batch->frame_ids, batch->state);
    if (rc) return rc;
    if (cfg->arch == ISDQN_ARCH_FC) ISDQN_REQUIRE(batch->next_state != nullptr, ISDQN_ERR_ARG, "fc needs next_state");
    if (learn && update) ISDQN_REQUIRE(adam_m && adam_v && adam_count, ISDQN_ERR_ARG, "null optimizer state");
    if (learn && !update) {
        ISDQN_REQUIRE(grad_out != nullptr, ISDQN_ERR_ARG, "a gradient-only pass needs grad_out");
        // the optimizer kernels request p / m / v before they know whether they update: a gradient-only pass has no moments, so
        // those (unused) loads read the parameters instead of a null pointer
        adam_m = params;
        adam_v = params;
    }
    if (P.bn) {  // BatchNorm: the layer-by-layer form over all 2B rows (batchnorm.h)
        ISDQN_REQUIRE(target_params == nullptr || (learn && !update), ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: separate target parameters only in gradient-only passes (the reference's DQN cannot run with "
                      "batch_norm, dqn.py:86)");
        ISDQN_REQUIRE(target_params == nullptr || cfg->double_q == 0, ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: double_q with separate target parameters is not defined (no statistics for an online forward "
                      "of the next states)");
        ISDQN_REQUIRE(target_params == nullptr || !P.munchausen, ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: Munchausen targets with separate target parameters are not defined (no statistics for a target "
                      "forward of the states)");
        return bn_learn_or_loss(cfg, P, params, adam_m, adam_v, adam_count, batch, losses, loss_accum, q_values, targets, priorities,
                                (float*)workspace, (hipStream_t)stream, learn, grad_out, update, target_params, sel);
    }
    const int B = P.B, K = sel ? sel->K : P.K;
    const int on0 = sel ? sel->on0 : P.oh, tg0 = sel ? sel->tg0 : 0;
    if (sel) ISDQN_REQUIRE(sel->K >= 1 && on0 >= 0 && tg0 >= 0 && on0 + K <= P.n_heads && tg0 + K <= P.n_heads && K <= P.K, ISDQN_ERR_ARG,
                           "head selection outside the network's heads");
    float* ws = (float*)workspace;
    LearnCtx c{P, cfg, batch, params, adam_m, adam_v, adam_count, target_params, losses, loss_accum,
               q_values ? q_values : ws + P.qv_off, targets ? targets : ws + P.tg_off, priorities, ws, grad_out, (hipStream_t)stream,
               learn, update, cfg->precision == ISDQN_PRECISION_BF16X3, B, K, on0, tg0,
               NetInput{batch->frames, batch->frame_stride, batch->frame_ids, B, batch->state, batch->next_state, B}};
    // (same head of the same rows selecting and valuing -- TF-DQN -- is the max form: Q[argmax Q] == max Q)
    c.double_q = cfg->double_q != 0 && !(target_params == nullptr && on0 == tg0);
    c.munchausen = P.munchausen;
    head_chain_plan(c, sel == nullptr);
    c.ss = learn ? side_stream() : nullptr;
    c.wst = c.ss ? c.ss->stream : c.st;

    rc = learn_forward(c);
    if (rc) return rc;
    rc = learn_loss(c);
    if (rc) return rc;
    if (!learn) {
        if (batch->priorities_ready != nullptr) ISDQN_HIP_CHECK(hipEventRecord((hipEvent_t)batch->priorities_ready, c.st));
        return ISDQN_OK;
    }
    AdamList adam[2];  // [0] caller's stream, [1] weight-gradient stream
    ReduceJobs red;    // partial-row reductions left by the fused data gradients (one launch before Adam)
    red.n = 0;
    red.block_start[0] = 0;
    BackwardSchedule sched(c, adam);
    rc = sched.begin();
    if (rc) return rc;
    rc = learn_backward(c, sched, adam, &red);
    if (rc) return rc;
    return learn_optimizer(c, sched, adam, red);
}

extern "C" int isdqn_net_learn_on_batch(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v,
                                        int32_t* adam_count, const isdqn_batch* batch, float* losses,
                                        float* losses_accum, float* q_values, float* targets, double* priorities,
                                        void* workspace, void* stream) {
    return learn_or_loss(cfg, params, adam_m, adam_v, adam_count, batch, losses, losses_accum, q_values, targets,
                         priorities, workspace, stream, true, nullptr);
}

// Test hook (not in the public header): learn_on_batch that also writes the reduced gradient (internal layout).
extern "C" int isdqn_net_learn_on_batch_debug(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v,
                                              int32_t* adam_count, const isdqn_batch* batch, float* losses,
                                              float* losses_accum, float* q_values, float* targets, double* priorities,
                                              void* workspace, void* stream, float* grad_out) {
    return learn_or_loss(cfg, params, adam_m, adam_v, adam_count, batch, losses, losses_accum, q_values, targets,
                         priorities, workspace, stream, true, grad_out);
}

extern "C" int isdqn_net_loss_on_batch(const isdqn_net_config* cfg, const float* params, const isdqn_batch* batch,
                                       float* losses, float* q_values, float* targets, void* workspace, void* stream) {
    return learn_or_loss(cfg, const_cast<float*>(params), nullptr, nullptr, nullptr, batch, losses, nullptr, q_values,
                         targets, nullptr, workspace, stream, false, nullptr);
}

// Gradient of a TD loss without an update (the diagnostics of AnalysisDQN, analysisdqn.py:156-219): `n_pairs` > 0 regresses
// online heads online_head + k on target heads target_head + k (k < n_pairs) instead of the plan's iterated pairs;
// `target_params` != NULL takes the next states through those parameters (the target-based loss).
extern "C" int isdqn_net_grad_on_batch(const isdqn_net_config* cfg, const float* params, const float* target_params,
                                       const isdqn_batch* batch, int32_t online_head, int32_t target_head, int32_t n_pairs,
                                       float* grad_out, float* losses, float* q_values, float* targets, void* workspace,
                                       void* stream) {
    ISDQN_REQUIRE(grad_out != nullptr, ISDQN_ERR_ARG, "null grad_out");
    HeadSel sel{online_head, target_head, n_pairs};
    return learn_or_loss(cfg, const_cast<float*>(params), nullptr, nullptr, nullptr, batch, losses, nullptr, q_values, targets, nullptr,
                         workspace, stream, true, grad_out, target_params, n_pairs > 0 ? &sel : nullptr, false);
}

extern "C" int isdqn_net_refresh_mirror(const isdqn_net_config* cfg, const float* params, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(params != nullptr && workspace != nullptr, ISDQN_ERR_ARG, "null pointer");
    return refresh_mirror(*Pp, params, (float*)workspace, (hipStream_t)stream);
}

extern "C" int isdqn_net_bn_commit_running(const isdqn_net_config* cfg, float* params, const void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(params != nullptr && workspace != nullptr, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(Pp->bn, ISDQN_ERR_ARG, "not a BatchNorm network");
    return bn_commit_running(*Pp, params, (const float*)workspace, (hipStream_t)stream);
}

// DQN.learn_on_batch / loss_on_batch (dqn.py:59-83): separate target parameters for the next states.
extern "C" int isdqn_net_learn_on_batch_target(const isdqn_net_config* cfg, float* params, const float* target_params,
                                               float* adam_m, float* adam_v, int32_t* adam_count, const isdqn_batch* batch,
                                               float* losses, float* losses_accum, float* q_values, float* targets,
                                               double* priorities, void* workspace, void* stream) {
    ISDQN_REQUIRE(target_params != nullptr, ISDQN_ERR_ARG, "null target_params");
    return learn_or_loss(cfg, params, adam_m, adam_v, adam_count, batch, losses, losses_accum, q_values, targets,
                         priorities, workspace, stream, true, nullptr, target_params);
}

extern "C" int isdqn_net_loss_on_batch_target(const isdqn_net_config* cfg, const float* params, const float* target_params,
                                              const isdqn_batch* batch, float* losses, float* q_values, float* targets,
                                              void* workspace, void* stream) {
    ISDQN_REQUIRE(target_params != nullptr, ISDQN_ERR_ARG, "null target_params");
    return learn_or_loss(cfg, const_cast<float*>(params), nullptr, nullptr, nullptr, batch, losses, nullptr, q_values,
                         targets, nullptr, workspace, stream, false, nullptr, target_params);
}

extern "C" int isdqn_net_shift_params(const isdqn_net_config* cfg, float* params, void* stream) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(params != nullptr, ISDQN_ERR_ARG, "null pointer");
    const Layer& l = P.L[P.n_layers - 1];
    hipLaunchKernelGGL(shift_kernel, dim3(ceil_div(l.in_p + 1, 256)), dim3(256), 0, (hipStream_t)stream,
                       params + l.w_off, params + l.b_off, P.dueling ? P.raw : P.nlog,
                       (P.n_actions + (P.dueling ? 1 : 0)) * (P.head_nb > 0 ? P.head_nb : 1), l.in_p);  // (dueling: the value rows move with their head)
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_net_best_action(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                     int64_t frame_stride, const int32_t* frame_ids, const float* obs,
                                     int32_t idx_network, int32_t* out_action, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && out_action && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(idx_network >= 0 && idx_network < P.K, ISDQN_ERR_ARG, "idx_network out of range");
    rc = check_input(cfg, frames, frame_stride, frame_ids, obs);
    if (rc) return rc;
    NetInput in{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    rc = refresh_mirror(P, params, ws, st);
    if (rc) return rc;
    rc = net_forward(P, cfg->precision == ISDQN_PRECISION_BF16X3, params, in, 1, 0, ws, ws + P.out_off, st);
    if (rc) return rc;
    rc = head_expect(P, ws, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(64), 0, st, ws + P.q_off, P.n_actions, P.oh + idx_network, out_action);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// best_action for n observations in one forward (vectorised environments: n host envs, one launch chain), with the
// "weight mirror is current" promise of ISDQN_BATCH_MIRROR_CURRENT as a flag.
extern "C" int isdqn_net_best_actions(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                      int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                                      const int32_t* idx_networks, int32_t* out_actions, int32_t flags, void* workspace,
                                      void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && idx_networks && out_actions && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
    rc = check_input(cfg, frames, frame_stride, frame_ids, obs);
    if (rc) return rc;
    NetInput in{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (!(flags & ISDQN_BATCH_MIRROR_CURRENT)) {
        rc = refresh_mirror(P, params, ws, st);
        if (rc) return rc;
    }
    rc = net_forward(P, cfg->precision == ISDQN_PRECISION_BF16X3, params, in, n_rows, 0, ws, ws + P.out_off, st);
    if (rc) return rc;
    rc = head_expect(P, ws, n_rows, st);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, st, ws + P.q_off, n_rows, P.nha_p, P.n_actions,
                       P.oh, P.K, idx_networks, out_actions);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// eval_srank_and_dead_neurons' device part (experiments/base/srank_and_dead_neurons.py:8-22): the torso on n_rows observations.
extern "C" int isdqn_net_analysis_layout(const isdqn_net_config* cfg, int32_t* n_hidden, int64_t* sizes, int32_t max_sizes) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(n_hidden != nullptr, ISDQN_ERR_ARG, "null pointer");
    int n = 0;
    auto put = [&](int64_t v) {
        if (sizes != nullptr && n < max_sizes) sizes[n] = v;
        ++n;
    };
    if (P.L[0].kind == 2)  // impala: the two ReLU outputs of each residual block of each Stack (analysis_architecture.py:27-40)
        for (int s = 0; s < IMP_STACKS; ++s)
            for (int k = 0; k < 4; ++k) put((int64_t)P.imp[s].Hp * P.imp[s].Wp * P.imp[s].C);
    for (int i = 0; i < P.n_layers - 1; ++i) {
        const Layer& l = P.L[i];
        put(l.kind != 1 ? (int64_t)l.npix * l.cout : (int64_t)l.out_f);
    }
    *n_hidden = n;
    return ISDQN_OK;
}

extern "C" int isdqn_net_analysis(const isdqn_net_config* cfg, const float* params, const uint8_t* frames, int64_t frame_stride,
                                  const int32_t* frame_ids, const float* obs, int32_t n_rows, float* features_out,
                                  float* scores_out, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && features_out && scores_out && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
    ISDQN_REQUIRE(P.n_layers >= 2, ISDQN_ERR_SHAPE, "no hidden layer");
    rc = check_input(cfg, frames, frame_stride, frame_ids, obs);
    if (rc) return rc;
    NetInput in{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const bool x3 = cfg->precision == ISDQN_PRECISION_BF16X3;
    rc = refresh_mirror(P, params, ws, st);
    if (rc) return rc;
    // BatchNorm networks: as the reference applies AnalysisNet (srank_and_dead_neurons.py:17: mutable batch_stats, use_running_average
    // left False) -- the batch statistics of the analysed rows; the whole network runs (its head output is not used)
    if (P.bn) rc = bn_forward(P, x3, params, in, n_rows, 0, ws, ws + P.q_off, /*running=*/false, st);
    else rc = net_forward(P, x3, params, in, n_rows, 0, ws, ws + P.q_off, st, P.n_layers - 1);
    if (rc) return rc;
    int64_t off = 0;
    auto rowsum = [&](const float* act_s8, int elems_p, int cpp, int c, int64_t width, float* feat) -> int {
        hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(elems_p, 256)), dim3(256), 0, st, act_s8, n_rows, elems_p, cpp, c, scores_out + off, feat,
                           feat ? (int)width : 0);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += width;
        return ISDQN_OK;
    };
    if (P.L[0].kind == 2)
        for (int s = 0; s < IMP_STACKS; ++s) {
            const ImpalaStack& S = P.imp[s];
            const int elems_p = S.Hp * S.Wp * S.C_p;
            for (int b = 0; b < 2; ++b) {  // relu([LN](r)) in front of the block's BatchNorm, relu(conv) behind its first convolution
                if ((rc = rowsum(ws + S.a1_off[b], elems_p, S.C_p, S.C, (int64_t)S.Hp * S.Wp * S.C, nullptr))) return rc;
                if ((rc = rowsum(ws + S.a2_off[b], elems_p, S.C_p, S.C, (int64_t)S.Hp * S.Wp * S.C, nullptr))) return rc;
            }
        }
    for (int i = 0; i < P.n_layers - 1; ++i) {
        const Layer& l = P.L[i];
        const int cpp = l.kind != 1 ? l.cout_p : l.out_p, c = l.kind != 1 ? l.cout : l.out_f;
        const bool last = i == P.n_layers - 2;
        const int64_t width = l.kind != 1 ? (int64_t)l.npix * l.cout : (int64_t)l.out_f;
        // the sums are those of the ReLU output (in front of a BatchNorm); the feature matrix leaves the network behind the last
        // BatchNorm (analysis_architecture.py:115-122): a second pass over that site's output, sums discarded into the head's q rows
        if ((rc = rowsum(ws + l.act_off, l.out_elems_p, cpp, c, width, (last && !P.bn) ? features_out : nullptr))) return rc;
        if (last && P.bn) {
            const BnSite* b = bn_site_of(P, i);
            hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(l.out_elems_p, 256)), dim3(256), 0, st, (const float*)(ws + b->out_off), n_rows,
                               l.out_elems_p, cpp, c, ws + P.slab_off, features_out, (int)width);
            ISDQN_HIP_CHECK(hipGetLastError());
        }
    }
    return ISDQN_OK;
}

// ReDo (Sokar et al. 2023; csrc/redo.h): the recyclable layers are the hidden ones, in network order.
static int redo_supported(const isdqn_net_config* cfg, const Plan& P) {
    ISDQN_REQUIRE(cfg->arch != ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED,
                  "ReDo is not built for the impala torso: its residual adds make a neuron's outgoing weights ambiguous");
    ISDQN_REQUIRE(!P.bn, ISDQN_ERR_UNSUPPORTED, "ReDo is not built for BatchNorm networks: per-position statistics sit between the layers");
    ISDQN_REQUIRE(P.n_layers >= 2, ISDQN_ERR_SHAPE, "no hidden layer");
    return ISDQN_OK;
}

extern "C" int isdqn_net_redo_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* n_neurons, int32_t max_layers) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    if ((rc = redo_supported(cfg, P))) return rc;
    ISDQN_REQUIRE(n_layers != nullptr, ISDQN_ERR_ARG, "null pointer");
    for (int i = 0; i < P.n_layers - 1 && n_neurons != nullptr && i < max_layers; ++i) n_neurons[i] = P.L[i].out_f;
    *n_layers = P.n_layers - 1;
    return ISDQN_OK;
}

extern "C" int isdqn_net_redo(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, const float* fresh_params,
                              const uint8_t* frames, int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                              float tau, float* scores_out, int32_t* mask_out, int32_t* n_recycled_out, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    if ((rc = redo_supported(cfg, P))) return rc;
    ISDQN_REQUIRE(params && fresh_params && scores_out && mask_out && n_recycled_out && workspace, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE((adam_m == nullptr) == (adam_v == nullptr), ISDQN_ERR_ARG, "adam_m and adam_v must be both null or both given");
    ISDQN_REQUIRE(std::isfinite(tau) && tau >= 0.f, ISDQN_ERR_ARG, "tau must be finite and >= 0");
    ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
    rc = check_input(cfg, frames, frame_stride, frame_ids, obs);
    if (rc) return rc;
    NetInput in{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int n_hidden = P.n_layers - 1;
    rc = refresh_mirror(P, params, ws, st);
    if (rc) return rc;
    rc = net_forward(P, cfg->precision == ISDQN_PRECISION_BF16X3, params, in, n_rows, 0, ws, ws + P.q_off, st, n_hidden);
    if (rc) return rc;
    // score: per-position sums over the rows into scratch (the data-gradient region: the forward does not touch it, and it holds a
    // batch of the widest input any layer above the first reads, so one image of any hidden layer's output), then one workgroup
    float* possum = ws + P.da_off;
    int64_t off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        const int npix = l.kind == 0 ? l.npix : 1;
        ISDQN_REQUIRE((int64_t)npix * l.out_f <= P.da_floats && l.out_f <= REDO_MAX_WIDTH, ISDQN_ERR_UNSUPPORTED, "ReDo: hidden layer too wide");
        hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(l.out_elems_p, 256)), dim3(256), 0, st, (const float*)(ws + l.act_off), n_rows,
                           l.out_elems_p, l.out_p, l.out_f, possum, (float*)nullptr, 0);
        ISDQN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(redo_score_kernel, dim3(1), dim3(256), 0, st, (const float*)possum, npix, l.out_f, (float)((int64_t)n_rows * npix), tau,
                           scores_out + off, mask_out + off, n_recycled_out + i);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    // recycle: every incoming side first, then every outgoing side -- where a dormant neuron reads a dormant neuron the weight is 0
    off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        hipLaunchKernelGGL(redo_incoming_kernel, dim3(ceil_div(l.K, 1024), l.out_f), dim3(256), 0, st, params, adam_m, adam_v, fresh_params,
                           (const int*)(mask_out + off), l.w_off, l.K, l.b_off, l.g_off, l.be_off);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        const Layer& nx = P.L[i + 1];
        hipLaunchKernelGGL(redo_outgoing_kernel, dim3(ceil_div(nx.K / 8, 256), nx.out_p), dim3(256), 0, st, params, adam_m, adam_v,
                           (const int*)(mask_out + off), l.out_f, l.out_p, nx.w_off, nx.K);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    return refresh_mirror(P, params, ws, st);
}

// ---- noisy Dense layers (noisy.h; include/isdqn_hip.h, isdqn_noisy_layout) ----
namespace isdqn {
#include "noisy.h"  // (behind every kernel of the learn step)
}  // namespace isdqn
// the plan behind its own checks, then the three refusals of the noisy entry points in their documented order
static const Plan* noisy_plan(const isdqn_net_config* cfg, int* rc) {
    const Plan* Pp = cached_plan(cfg, rc);
    if (!Pp) return nullptr;
    auto refuse = [&](const char* msg) -> const Plan* {
        set_last_error("%s", msg);
        *rc = ISDQN_ERR_UNSUPPORTED;
        return nullptr;
    };
    if (cfg->batch_norm) return refuse("noisy layers are not built for BatchNorm networks: running statistics would be committed into the composed parameters");
    if (cfg->arch == ISDQN_ARCH_IMPALA) return refuse("noisy layers are not built for the impala torso");
    if (cfg->max_grad_norm > 0.f)
        return refuse("noisy layers with max_grad_norm > 0 are a follow-up: the global norm must cover the gradient of sigma too");
    return Pp;
}
// noise layout: per noisy layer ein[in_p] then eout[out_p], the layers concatenated in network order
static int64_t noisy_tables(const Plan& P, NoisyTable* tab, NoisyVecTable* vecs) {
    int64_t off = 0;
    int l_noisy = 0;
    if (tab) tab->n = 0;
    if (vecs) { vecs->n = 0; vecs->total_blocks = 0; }
    for (int i = 0; i < P.n_layers; ++i) {
        const Layer& l = P.L[i];
        if (l.kind != 1) continue;
        const int64_t ein = off, eout = off + l.in_p;
        if (tab) {
            tab->e[tab->n++] = NoisyEntry{l.w_off, l.w_size, ein, eout, l.in_p, FastDiv((uint32_t)l.in_p)};
            tab->e[tab->n++] = NoisyEntry{l.b_off, (int64_t)l.out_p, ein, eout, 0, FastDiv()};
        }
        if (vecs) {
            const int widths[2] = {l.in_p, l.out_p};
            const int64_t offs[2] = {ein, eout};
            for (int v = 0; v < 2; ++v) {
                vecs->v[vecs->n++] = NoisyVec{offs[v], widths[v], 2 * l_noisy + v, vecs->total_blocks, 0};
                vecs->total_blocks += ceil_div(widths[v], NOISY_THREADS);
            }
        }
        off += l.in_p + l.out_p;
        ++l_noisy;
    }
    return off;
}

extern "C" int isdqn_noisy_layout(const isdqn_net_config* cfg, int32_t* n_layers, int64_t* offsets, int32_t* in_widths, int32_t* out_widths,
                                  int32_t max_layers, int64_t* n_noise_floats) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    int n = 0;
    int64_t total = 0;
    for (int i = 0; i < Pp->n_layers; ++i)
        if (Pp->L[i].kind == 1) {
            ++n;
            total += Pp->L[i].in_p + Pp->L[i].out_p;
        }
    if (n_layers) *n_layers = n;
    if (n_noise_floats) *n_noise_floats = total;
    if (!offsets && !in_widths && !out_widths) return ISDQN_OK;  // a query of the count and the total
    // (the arrays must hold every layer: nothing is truncated silently)
    ISDQN_REQUIRE(max_layers >= n, ISDQN_ERR_ARG, "isdqn_noisy_layout: max_layers is smaller than the number of noisy layers (returned in *n_layers)");
    int k = 0;
    int64_t off = 0;
    for (int i = 0; i < Pp->n_layers; ++i) {
        const Layer& l = Pp->L[i];
        if (l.kind != 1) continue;
        if (offsets) offsets[k] = off;
        if (in_widths) in_widths[k] = l.in_p;
        if (out_widths) out_widths[k] = l.out_p;
        off += l.in_p + l.out_p;
        ++k;
    }
    return ISDQN_OK;
}

extern "C" int isdqn_noisy_sample(const isdqn_net_config* cfg, uint64_t seed, int32_t stream_id, int64_t* noise_count, float* noise, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(noise_count != nullptr && noise != nullptr, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(stream_id == 0 || stream_id == 1, ISDQN_ERR_ARG, "stream_id must be 0 (online) or 1 (target)");
    NoisyVecTable vecs;
    noisy_tables(*Pp, nullptr, &vecs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noisy_sample_kernel, dim3(vecs.total_blocks), dim3(NOISY_THREADS), 0, st, vecs, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)stream_id, (const int64_t*)noise_count, noise);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(noisy_advance_kernel, dim3(1), dim3(64), 0, st, noise_count);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static int noisy_compose(const Plan& P, const NoisyTable& tab, const float* mu, const float* sigma, const float* noise, float* eff, float* ws,
                         hipStream_t st) {
    const int64_t quads = P.n_params / 4;  // (every tensor size is a multiple of 8)
    hipLaunchKernelGGL(noisy_compose_kernel, dim3((unsigned)((quads + NOISY_THREADS - 1) / NOISY_THREADS)), dim3(NOISY_THREADS), 0, st, tab, mu, sigma,
                       noise, eff, ws ? ws + P.wsplit_off : nullptr, P.n_params);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_noisy_compose(const isdqn_net_config* cfg, const float* mu, const float* sigma, const float* noise, float* eff,
                                   void* workspace, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(mu && sigma && noise && eff, ISDQN_ERR_ARG, "null pointer");
    NoisyTable tab;
    noisy_tables(*Pp, &tab, nullptr);
    return noisy_compose(*Pp, tab, mu, sigma, noise, eff, (float*)workspace, (hipStream_t)stream);
}

extern "C" int isdqn_noisy_learn_on_batch(const isdqn_net_config* cfg, float* mu, float* sigma, float* m_mu, float* v_mu, float* m_sigma,
                                          float* v_sigma, int32_t* adam_count, const float* noise, float* eff, const float* eff_target,
                                          float* grad, const isdqn_batch* batch, float* losses, float* losses_accum, float* q_values,
                                          float* targets, double* priorities, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(mu && sigma && m_mu && v_mu && m_sigma && v_sigma && adam_count && noise && eff && grad && batch && workspace, ISDQN_ERR_ARG,
                  "null pointer");
    NoisyTable tab;
    noisy_tables(P, &tab, nullptr);
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    rc = noisy_compose(P, tab, mu, sigma, noise, eff, ws, st);
    if (rc) return rc;
    // the full two-stream gradient pass on eff: its optimizer launches write the reduced gradient (masked under dueling) and update
    // nothing; loss_finalize_kernel advances adam_count and leaves the bias corrections in the workspace, as in a plain learn step
    isdqn_batch_discount b{*batch, batch_discount(batch)};  // (the copy keeps the discounts that may follow the caller's batch)
    b.batch.flags |= ISDQN_BATCH_MIRROR_CURRENT;  // (compose wrote the mirror of eff; the *_target form rebuilds both mirrors itself)
    rc = learn_or_loss(cfg, eff, nullptr, nullptr, adam_count, &b.batch, losses, losses_accum, q_values, targets, priorities, workspace, stream, true, grad,
                       eff_target, nullptr, false);
    if (rc) return rc;
    const int64_t quads = P.n_params / 4;
    hipLaunchKernelGGL(noisy_adam_kernel, dim3((unsigned)((quads + NOISY_THREADS - 1) / NOISY_THREADS)), dim3(NOISY_THREADS), 0, st, tab, (const float*)grad,
                       noise, mu, m_mu, v_mu, sigma, m_sigma, v_sigma, (const float*)(ws + P.adam_tab_off), cfg->learning_rate, cfg->adam_b1, cfg->adam_b2,
                       cfg->adam_eps, P.n_params);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// ---- periodic resets and EMA targets (reset.h; include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema) ----
namespace isdqn {
#include "reset.h"  // (behind every kernel the library had)
}  // namespace isdqn

extern "C" int isdqn_net_reset_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* first_dense_layer) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    int first = Pp->n_layers;
    for (int i = Pp->n_layers - 1; i >= 0; --i)
        if (Pp->L[i].kind == 1) first = i;
    if (n_layers) *n_layers = Pp->n_layers;
    if (first_dense_layer) *first_dense_layer = first;
    return ISDQN_OK;
}

extern "C" int isdqn_net_reset(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, int32_t* adam_count,
                               const float* fresh_params, int32_t split_layer, float shrink_lower, float perturb_lower, float shrink_upper,
                               float perturb_upper, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && fresh_params, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE((adam_m == nullptr) == (adam_v == nullptr), ISDQN_ERR_ARG, "adam_m and adam_v must be both null or both given");
    const float fac[4] = {shrink_lower, perturb_lower, shrink_upper, perturb_upper};
    for (float f : fac) ISDQN_REQUIRE(std::isfinite(f) && f >= 0.f, ISDQN_ERR_ARG, "every shrink / perturb factor must be finite and >= 0");
    ISDQN_REQUIRE(split_layer >= 0 && split_layer <= P.n_layers, ISDQN_ERR_ARG, "split_layer must be in [0, n_layers]");
    {
        const uintptr_t a = (uintptr_t)params, b = (uintptr_t)fresh_params, bytes = (uintptr_t)P.n_params * 4;
        ISDQN_REQUIRE(a + bytes <= b || b + bytes <= a, ISDQN_ERR_ARG, "fresh_params overlaps params");
    }
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = (((uintptr_t)params | (uintptr_t)fresh_params | (uintptr_t)adam_m | (uintptr_t)adam_v) & 15) == 0;
    const bool touch[2] = {!(shrink_lower == 1.f && perturb_lower == 0.f), !(shrink_upper == 1.f && perturb_upper == 0.f)};
    ResetTable tab;
    tab.s[0] = shrink_lower; tab.q[0] = perturb_lower; tab.s[1] = shrink_upper; tab.q[1] = perturb_upper;
    tab.n = 0;
    tab.total_blocks = 0;
    int launch_rc = ISDQN_OK;
    auto flush = [&]() {
        if (tab.n == 0 || launch_rc) return;
        hipLaunchKernelGGL(reset_kernel, dim3(std::min(tab.total_blocks, RESET_MAX_BLOCKS)), dim3(RESET_THREADS), 0, st, tab, params, adam_m, adam_v,
                           fresh_params);
        if (hipGetLastError() != hipSuccess) {
            set_last_error("isdqn_net_reset: kernel launch failed");
            launch_rc = ISDQN_ERR_HIP;
        }
        tab.n = 0;
        tab.total_blocks = 0;
    };
    for_each_param_tensor(P, [&](const isdqn_tensor_info& t) {
        const int upper = t.layer >= split_layer ? 1 : 0;
        if (!touch[upper] || t.size <= 0) return;
        // one launch per tensor would do for a tensor of 2^31 * RESET_BLOCK_ELEMS elements; the plan's tensors hold fewer than 2^31
        const int vec = (aligned && t.offset % 4 == 0 && t.size % 4 == 0) ? 2 : 0;
        const int blocks = (int)((t.size + RESET_BLOCK_ELEMS - 1) / RESET_BLOCK_ELEMS);
        if (tab.n == RESET_MAX_ENTRIES) flush();
        tab.e[tab.n++] = ResetEntry{t.offset, t.size, tab.total_blocks, upper | vec};
        tab.total_blocks += blocks;
    });
    flush();
    if (launch_rc) return launch_rc;
    if (adam_count != nullptr) {
        hipLaunchKernelGGL(reset_count_kernel, dim3(1), dim3(64), 0, st, adam_count);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (workspace != nullptr) return refresh_mirror(P, params, (float*)workspace, st);
    return ISDQN_OK;
}

extern "C" int isdqn_net_ema(const isdqn_net_config* cfg, float* target, const float* online, float tau, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(target && online, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(tau >= 0.f && tau <= 1.f, ISDQN_ERR_ARG, "tau must be in [0, 1]");  // (NaN fails both comparisons)
    ISDQN_REQUIRE(target != online, ISDQN_ERR_ARG, "target and online are the same buffer");
    if (tau == 0.f) return ISDQN_OK;
    const int64_t n = Pp->n_params;
    hipStream_t st = (hipStream_t)stream;
    if (tau == 1.f) {  // the bits of `online`, a NaN target and the sign of a zero included
        ISDQN_HIP_CHECK(hipMemcpyAsync(target, online, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        return ISDQN_OK;
    }
    const bool aligned = (((uintptr_t)target | (uintptr_t)online) & 15) == 0;
    const int64_t n4 = aligned ? n / 4 : 0;
    const int64_t work = std::max<int64_t>(n4, n - 4 * n4);
    const int64_t blocks = std::min<int64_t>((work + RESET_THREADS - 1) / RESET_THREADS, RESET_MAX_BLOCKS);
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(RESET_THREADS), 0, st, target, online, 1.0f - tau, tau, n4, n);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_selftest_gemm(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K,
                                   int32_t a_tr, int32_t b_tr, int32_t precision, int32_t split_k, void* stream) {
    ISDQN_REQUIRE(A && B && C, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(M > 0 && N > 0 && K > 0, ISDQN_ERR_SHAPE, "bad shape");
    const bool x3 = precision == ISDQN_PRECISION_BF16X3;
    hipStream_t st = (hipStream_t)stream;
    // ROW operand: [rows][K] ; TR operand: [K][rows].  No alignment promises (self-test shapes are arbitrary).
    MatSrc a = a_tr ? MatSrc{A, M, K, M, 0} : MatSrc{A, K, M, K, 0};
    MatSrc b = b_tr ? MatSrc{B, N, K, N, 0} : MatSrc{B, K, N, K, 0};
    const int64_t slab = (int64_t)M * N;
    if (!a_tr && !b_tr) return plain_big<false, false, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    if (!a_tr && b_tr) return plain_big<false, true, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    if (a_tr && !b_tr) return plain_big<true, false, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    return plain_big<true, true, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
}
