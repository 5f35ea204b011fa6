// HL-Gauss histogram value loss ("Stop Regressing", Farebrother et al. 2024) on the Q-network heads: the flags of the
// reference's add_histogram_loss_parameters (experiments/base/parser_argument.py:199-228), which the reference defines but never
// uses; the loss is this project's (include/isdqn_hip.h, isdqn_net_config::n_bins).  With n_bins = nb > 0 the head layer has
// n_heads * A * nb outputs, logit ((h * A) + a) * nb + j being bin j of action a of head h over the support [v_min, v_max]:
//   eta = (v_max - v_min) / nb, edges e_i = v_min + i eta (i = 0..nb), centres c_j = v_min + (j + 1/2) eta;
//   Q_h(s, a) = sum_j softmax(l_{h,a})_j c_j.
// Two kernels, both one wave per (row, head / action) with the lanes over the bins, fp32 with max subtraction, every sum a fixed
// __shfl_xor butterfly (bit-identical from run to run, no atomics):
//   hl_expect_kernel: logits rows -> Q rows (forward / best_action / best_actions, in front of the argmax kernels);
//   hl_loss_kernel:   where td_kernel runs for scalar heads (learn / loss / grad, every head selection).
#pragma once

namespace isdqn {

constexpr int HL_MAX_BINS = 256;
constexpr int HL_PER_LANE = HL_MAX_BINS / 64;
constexpr int HL_MAX_ROWS = 4;  // transitions per workgroup of hl_loss_kernel

__device__ __forceinline__ float hl_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float hl_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// The nb logits at `l` (one action of one head) in the lanes' registers: lane owns bins lane + 64 t.  Returns the row maximum and
// fills e[t] = exp(l_j - max) (0 past nb), *sum = sum_j e_j, *wsum = sum_j e_j c_j.  Every lane ends with the same values.
__device__ __forceinline__ float hl_softmax_parts(const float* __restrict__ l, int nb, int lane, float vmin, float eta,
                                                  float (&v)[HL_PER_LANE], float (&e)[HL_PER_LANE], float* sum, float* wsum) {
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < HL_PER_LANE; ++t) {
        const int j = lane + 64 * t;
        v[t] = j < nb ? l[j] : -INFINITY;
        m = fmaxf(m, v[t]);
    }
    m = hl_wave_max(m);
    float s = 0.f, w = 0.f;
#pragma unroll
    for (int t = 0; t < HL_PER_LANE; ++t) {
        const int j = lane + 64 * t;
        e[t] = j < nb ? expf(v[t] - m) : 0.f;
        s += e[t];
        w += e[t] * (vmin + ((float)j + 0.5f) * eta);
    }
    *sum = hl_wave_sum(s);
    *wsum = hl_wave_sum(w);
    return m;
}

__device__ __forceinline__ float hl_expectation(const float* __restrict__ l, int nb, int lane, float vmin, float eta) {
    float v[HL_PER_LANE], e[HL_PER_LANE], s, w;
    hl_softmax_parts(l, nb, lane, vmin, eta, v, e, &s, &w);
    return w / s;
}

// Soft value tau log(sum_a exp(Q_a / tau)) of the A expectations of one head's logits at `row` (munchausen.h: the maximum is
// subtracted first); *picked = the expectation of action a_pick.  One pass over the actions, every expectation computed once: the
// running sum is rescaled whenever the running maximum moves (exponents stay <= 0, so tau = 0.03 with |Q| in the hundreds neither
// overflows nor returns -inf; the first action finds s = 0, m = -inf and leaves s = 1).
__device__ __forceinline__ float hl_soft_value(const float* __restrict__ row, int A, int nb, int lane, float vmin, float eta, float tau,
                                               int a_pick, float* picked) {
    float m = -INFINITY, s = 0.f;
    for (int a2 = 0; a2 < A; ++a2) {
        const float x = hl_expectation(row + (int64_t)a2 * nb, nb, lane, vmin, eta);
        if (a2 == a_pick) *picked = x;
        if (x > m) {
            s = s * expf((m - x) / tau) + 1.f;
            m = x;
        } else {
            s += expf((x - m) / tau);
        }
    }
    return m + tau * logf(s);
}

// q[row][c] = Q of column c = h * A + a (c < nha) from logits[row][c * nb .. c * nb + nb); the padding columns of q are not written.
__global__ __launch_bounds__(256) void hl_expect_kernel(const float* __restrict__ logits, int n_rows, int nha, int nb, int nlog_p,
                                                        int nha_p, float vmin, float eta, float* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)n_rows * nha) return;  // (whole waves: the shuffles below see every lane of theirs)
    const int row = (int)(item / nha), c = (int)(item - (int64_t)row * nha);
    const float qv = hl_expectation(logits + (int64_t)row * nlog_p + (int64_t)c * nb, nb, lane, vmin, eta);
    if (lane == 0) q[(int64_t)row * nha_p + c] = qv;
}

// Iterated Bellman target on expectations + HL-Gauss cross-entropy.  Workgroup = R <= HL_MAX_ROWS transitions; wave w takes the
// (transition, k) pairs w, w + 4, ...: online head on0 + k at the taken action is regressed on head tg0 + k of the next-state rows.
//   target = r + (1 - terminal) gamma^n max_a' Q_{tg0+k}(s', a');  y = clamp(target, v_min, v_max)
//   u_i = erf((e_i - y) / (sqrt(2) sigma)),  p_j = (u_{j+1} - u_j) / (u_nb - u_0)   (the clamp keeps u_nb - u_0 away from 0/0)
//   CE = w_b (logsumexp(l) - sum_j p_j l_j),  dL/dl_j = w_b (softmax(l)_j - p_j) / B on the taken action's nb logits, 0 elsewhere
//   (w_b: isdqn_batch.loss_weights, 1 without).
// `vlogits`: the value rows of the B next states (pitch nlog_p).  `slogits` != null (isdqn_net_config::double_q): max_a' becomes the
// value head's expectation at the first argmax of the expectations of head sh + k of the selector rows (pitch s_pitch).
// `mlogits` != null (isdqn_net_config::munchausen_tau > 0, munchausen.h): the target is the Munchausen one on the expectations of
// the value head -- head mh + k of the STATE rows `mlogits` (pitch m_pitch) for the bonus, the soft value of the value rows.
// Writes q_values / targets [B][K] (expectation, unclamped scalar target), priorities[B] = sqrt(mean_k (q - target)^2 + 1e-10) --
// the expectations' TD error, not the CE (which never falls below the target histogram's entropy) -- per-workgroup partials of the
// per-pair CE sums (loss_part [n_blk][K]) and, with `dout`, the dL/dlogits rows (zero-filled) and their column sums over the
// workgroup's rows (dbh_part [n_blk][nlog_p], the head-bias gradient); loss_finalize_kernel reduces both in a fixed order.
// Dynamic LDS: R * K * nb floats of dL/dl.
__global__ __launch_bounds__(256) void hl_loss_kernel(const float* __restrict__ logits, const float* __restrict__ vlogits,
                                                      const float* __restrict__ slogits, int s_pitch, int sh, const float* mlogits, int m_pitch,
                                                      int mh, Munchausen mu, int B, int R, int K, int on0, int tg0, int A,
                                                      int nb, int nlog_p, float vmin, float eta, float sigma,
                                                      const int* __restrict__ action, const float* __restrict__ reward,
                                                      const uint8_t* __restrict__ terminal, const float* __restrict__ loss_weights,
                                                      float gamma_n, float* __restrict__ dout,
                                                      float* __restrict__ q_values, float* __restrict__ targets,
                                                      double* __restrict__ priorities, float* __restrict__ loss_part,
                                                      float* __restrict__ dbh_part) {
    extern __shared__ float s_dl[];  // [R][K][nb]
    __shared__ int s_action[HL_MAX_ROWS];
    __shared__ float s_r[HL_MAX_ROWS], s_nt[HL_MAX_ROWS], s_w[HL_MAX_ROWS];  // s_w: importance-sampling weights (none: 1)
    __shared__ float s_ce[HL_MAX_ROWS * 64], s_td2[HL_MAX_ROWS * 64];  // [R][K], K <= 64 (checked by the host)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const float inv_b = 1.f / (float)B;
    const int ldk = A * nb;  // logits of one head
    if (dout != nullptr)
        for (int i = tid; i < rows * nlog_p; i += 256) dout[(int64_t)b0 * nlog_p + i] = 0.f;
    if (tid < R) {
        const bool on = tid < rows;
        s_action[tid] = on ? action[b0 + tid] : -1;
        s_r[tid] = on ? reward[b0 + tid] : 0.f;
        s_nt[tid] = on ? 1.f - (float)terminal[b0 + tid] : 0.f;
        s_w[tid] = (on && loss_weights != nullptr) ? loss_weights[b0 + tid] : 1.f;
    }
    __syncthreads();
    const float inv_s = 1.f / (1.41421356237309515f * sigma);
    for (int pr = wave; pr < R * K; pr += 4) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) s_ce[pr] = s_td2[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const float* nrow = vlogits + (int64_t)b * nlog_p + (int64_t)(tg0 + k) * ldk;
        float mx = -INFINITY;
        float tg_m = 0.f;
        if (mlogits != nullptr) {  // Munchausen: bonus from the value head's state row, soft value of its next-state row
            const float* srow = mlogits + (int64_t)b * m_pitch + (int64_t)(mh + k) * ldk;
            ISDQN_BOUNDS_CHECK(srow + min(lane, ldk - 1), 4, 31);
            ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 31);
            float qa = 0.f, unused;
            const float vs = hl_soft_value(srow, A, nb, lane, vmin, eta, mu.tau, s_action[bl], &qa);
            const float vn = hl_soft_value(nrow, A, nb, lane, vmin, eta, mu.tau, -1, &unused);
            tg_m = munchausen_target(s_r[bl], s_nt[bl], gamma_n, qa, vs, vn, mu);
            mx = 0.f;
        } else if (slogits != nullptr) {  // Double Q-learning: first argmax of the selector head's expectations, valued by the value head
            const float* srow = slogits + (int64_t)b * s_pitch + (int64_t)(sh + k) * ldk;
            ISDQN_BOUNDS_CHECK(srow + min(lane, ldk - 1), 4, 30);
            ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 30);
            int best = 0;
            float bv = hl_expectation(srow, nb, lane, vmin, eta);
            for (int a2 = 1; a2 < A; ++a2) {
                const float x = hl_expectation(srow + (int64_t)a2 * nb, nb, lane, vmin, eta);
                if (x > bv) { bv = x; best = a2; }
            }
            mx = hl_expectation(nrow + (int64_t)best * nb, nb, lane, vmin, eta);
        } else {
            for (int a2 = 0; a2 < A; ++a2) mx = fmaxf(mx, hl_expectation(nrow + (int64_t)a2 * nb, nb, lane, vmin, eta));
        }
        const float tg = mlogits != nullptr ? tg_m : s_r[bl] + s_nt[bl] * gamma_n * mx;
        float v[HL_PER_LANE], e[HL_PER_LANE], s, w;
        const float m = hl_softmax_parts(logits + (int64_t)b * nlog_p + (int64_t)(on0 + k) * ldk + (int64_t)s_action[bl] * nb, nb, lane,
                                         vmin, eta, v, e, &s, &w);
        const float qv = w / s;
        const float y = fminf(fmaxf(tg, vmin), vmin + (float)nb * eta);
        const float u0 = erff((vmin - y) * inv_s), un = erff((vmin + (float)nb * eta - y) * inv_s);
        const float inv_norm = 1.f / (un - u0), inv_sum = 1.f / s;
        float pl = 0.f;
#pragma unroll
        for (int t = 0; t < HL_PER_LANE; ++t) {
            const int j = lane + 64 * t;
            if (j < nb) {
                const float p = (erff((vmin + (float)(j + 1) * eta - y) * inv_s) - erff((vmin + (float)j * eta - y) * inv_s)) * inv_norm;
                pl += p * v[t];
                s_dl[(int64_t)pr * nb + j] = (e[t] * inv_sum - p) * inv_b * s_w[bl];
            }
        }
        pl = hl_wave_sum(pl);
        if (lane == 0) {
            s_ce[pr] = (m + logf(s) - pl) * s_w[bl];  // (s_td2 stays unweighted: the priorities are the raw TD error)
            s_td2[pr] = (qv - tg) * (qv - tg);
            if (q_values) q_values[(int64_t)b * K + k] = qv;
            if (targets) targets[(int64_t)b * K + k] = tg;
        }
    }
    __syncthreads();  // dout zero-fill (this workgroup's rows), s_dl / s_ce / s_td2 complete
    for (int k = tid; k < K; k += 256) {
        float sum = 0.f;
        for (int bl = 0; bl < R; ++bl) sum += s_ce[bl * K + k];
        loss_part[(int64_t)blockIdx.x * K + k] = sum;
    }
    if (dout != nullptr) {
        for (int i = tid; i < rows * K * nb; i += 256) {
            const int pr = i / nb, j = i - pr * nb;
            const int bl = pr / K, k = pr - bl * K;
            dout[(int64_t)(b0 + bl) * nlog_p + (int64_t)(on0 + k) * ldk + (int64_t)s_action[bl] * nb + j] = s_dl[i];
        }
        // column c = (h * A + a) * nb + j collects the rows whose action is a, for the regressed heads h in [on0, on0 + K)
        for (int c = tid; c < nlog_p; c += 256) {
            const int h = c / ldk, rem = c - h * ldk, a = rem / nb, j = rem - a * nb;
            float sum = 0.f;
            if (h >= on0 && h < on0 + K)
                for (int bl = 0; bl < R; ++bl) sum += (s_action[bl] == a) ? s_dl[((int64_t)bl * K + h - on0) * nb + j] : 0.f;
            dbh_part[(int64_t)blockIdx.x * nlog_p + c] = sum;
        }
    }
    if (priorities != nullptr && tid < rows) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s_td2[tid * K + k];
        priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }
}

// Transitions per workgroup of hl_loss_kernel: HL_MAX_ROWS while the dL/dl staging stays within 32 KB of LDS.
static inline int hl_rows_per_wg(int K, int nb) {
    int R = (8192 / (K * nb));
    return R < 1 ? 1 : R > HL_MAX_ROWS ? HL_MAX_ROWS : R;
}

}  // namespace isdqn
