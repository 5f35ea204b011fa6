// The row-wise kernels of the forward, the LayerNorm backward and the TD loss -- the HBM-bound remainder beside the MFMA tile engine:
// dense_post_kernel, ln_bwd_small_kernel / ln_bwd_wide_kernel, td_kernel (and pow_int for Adam's bias corrections).  Included by
// net_kernels.hip inside namespace isdqn, first of its own headers: tests/test_kernel_order_host.py holds every kernel to its place.
#pragma once
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
#include "td_loss.h"  // td_loss / td_dloss, shared with mix_td_kernel (mixture_kernels.hip)
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
