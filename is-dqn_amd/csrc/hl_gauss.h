// HL-Gauss histogram value loss ("Stop Regressing", Farebrother et al. 2024) on the Q-network heads: the flags of the
// reference's add_histogram_loss_parameters (experiments/base/parser_argument.py:199-228), which the reference defines but never
// uses; the loss is this project's (include/isdqn_hip.h, isdqn_net_config::n_bins).  With n_bins = nb > 0 the head layer has
// n_heads * A * nb outputs, logit ((h * A) + a) * nb + j being bin j of action a of head h over the support [v_min, v_max]:
//   eta = (v_max - v_min) / nb, edges e_i = v_min + i eta (i = 0..nb), centres c_j = v_min + (j + 1/2) eta;
//   Q_h(s, a) = sum_j softmax(l_{h,a})_j c_j.
// Two kernels, both one wave per (row, head / action) with the lanes over the bins, fp32 with max subtraction, every sum a fixed
// __shfl_xor butterfly (bit-identical from run to run, no atomics):
//   hl_expect_kernel: logits rows -> Q rows (forward / best_action / best_actions, in front of the argmax kernels);
//   hl_loss_kernel:   where td_kernel runs for scalar heads (learn / loss / grad, every head selection; head_loss.h).
#pragma once

namespace isdqn {

// The nb logits at `l` (one action of one head) in the lanes' registers: lane owns bins lane + 64 t.  Returns the row maximum and
// fills e[t] = exp(l_j - max) (0 past nb), *sum = sum_j e_j, *wsum = sum_j e_j c_j.  Every lane ends with the same values.
__device__ __forceinline__ float hl_softmax_parts(const float* __restrict__ l, int nb, int lane, float vmin, float eta,
                                                  float (&v)[PER_LANE], float (&e)[PER_LANE], float* sum, float* wsum) {
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int j = lane + 64 * t;
        v[t] = j < nb ? l[j] : -INFINITY;
        m = fmaxf(m, v[t]);
    }
    m = wave_max(m);
    float s = 0.f, w = 0.f;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int j = lane + 64 * t;
        e[t] = j < nb ? expf(v[t] - m) : 0.f;
        s += e[t];
        w += e[t] * (vmin + ((float)j + 0.5f) * eta);
    }
    *sum = wave_sum(s);
    *wsum = wave_sum(w);
    return m;
}

__device__ __forceinline__ float hl_expectation(const float* __restrict__ l, int nb, int lane, float vmin, float eta) {
    float v[PER_LANE], e[PER_LANE], s, w;
    hl_softmax_parts(l, nb, lane, vmin, eta, v, e, &s, &w);
    return w / s;
}

// First argmax of the expectations of the A actions at a head's logit row: strict >, the lowest index wins (argmax_kernel's rule).
__device__ __forceinline__ int hl_argmax_first(const float* __restrict__ row, int A, int nb, int lane, float vmin, float eta) {
    int best = 0;
    float bv = hl_expectation(row, nb, lane, vmin, eta);
    for (int a2 = 1; a2 < A; ++a2) {
        const float x = hl_expectation(row + (int64_t)a2 * nb, nb, lane, vmin, eta);
        if (x > bv) { bv = x; best = a2; }
    }
    return best;
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

// The butterfly of wave_sum on doubles, for the one place that needs a normaliser without float32's rounding (hl_loss_kernel's dL/dl).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
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

// Iterated Bellman target on expectations + HL-Gauss cross-entropy, in the frame of head_loss.h (THE contract: there).  Wave w of 4 takes
// the (transition, k) pairs w, w + 4, ...
//   target = r + (1 - terminal) gamma^n max_a' Q_{tg0+k}(s', a');  y = clamp(target, v_min, v_max)
//   u_i = erf((e_i - y) / (sqrt(2) sigma)),  p_j = (u_{j+1} - u_j) / (u_nb - u_0)   (the clamp keeps u_nb - u_0 away from 0/0)
//   CE = w_b (logsumexp(l) - sum_j p_j l_j),  dL/dl_j = w_b (softmax(l)_j - p_j) / B on the taken action's nb logits, 0 elsewhere.
// dL/dl is rounded once: softmax(l)_j - p_j is formed in double from the float32 e_j and u_i, each histogram divided by the double sum of
// its own float32 terms, so both sum to one to 1e-16 and the nb entries of a pair sum to zero within nb 2^-24 of the largest -- also
// where the two histograms nearly agree (at two bins both are near 1/2, and float32 roundings of each would be what is left of their
// difference).  The loss, q_values, targets and priorities keep their float32 arithmetic and their bits.
// a.sel != null: max_a' becomes the value head's expectation at the first argmax of the expectations of the selector head.
// a.mun != null: the target is the Munchausen one on the expectations of the value head -- its state row for the bonus, the soft
// value of its next-state row.  q_values / targets: the expectation and the unclamped scalar target.
// Dynamic LDS: R * K * nb floats of dL/dl.
__global__ __launch_bounds__(256) void hl_loss_kernel(const HeadLossArgs a) {
    extern __shared__ float s_dl[];  // [R][K][nb]
    __shared__ LossStage st;
    const float *__restrict__ logits = a.out, *__restrict__ vlogits = a.val, *__restrict__ slogits = a.sel, *mlogits = a.mun;
    float *__restrict__ q_values = a.q_values, *__restrict__ targets = a.targets;
    const int B = a.B, R = a.R, K = a.K, A = a.A, nb = a.nb, nlog_p = a.pitch;
    const float vmin = a.vmin, eta = a.eta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const float inv_b = 1.f / (float)B;
    const int ldk = A * nb;  // logits of one head
    loss_prologue<256>(a, st);
    __syncthreads();
    const float inv_s = 1.f / (1.41421356237309515f * a.sigma);
    for (int pr = wave; pr < R * K; pr += 4) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) st.loss[pr] = st.td2[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const float* nrow = vlogits + (int64_t)b * nlog_p + (int64_t)(a.tg0 + k) * ldk;
        float mx = -INFINITY;
        float tg_m = 0.f;
        if (mlogits != nullptr) {  // Munchausen: bonus from the value head's state row, soft value of its next-state row
            const float* srow = mlogits + (int64_t)b * a.mun_pitch + (int64_t)(a.mun_head + k) * ldk;
            ISDQN_BOUNDS_CHECK(srow + min(lane, ldk - 1), 4, 31);
            ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 31);
            float qa = 0.f, unused;
            const float vs = hl_soft_value(srow, A, nb, lane, vmin, eta, a.mu.tau, st.action[bl], &qa);
            const float vn = hl_soft_value(nrow, A, nb, lane, vmin, eta, a.mu.tau, -1, &unused);
            tg_m = munchausen_target(st.r[bl], st.nt[bl], st.g[bl], qa, vs, vn, a.mu);
            mx = 0.f;
        } else if (slogits != nullptr) {  // Double Q-learning: the selector head decides, the value head supplies the value
            const float* srow = slogits + (int64_t)b * a.sel_pitch + (int64_t)(a.sel_head + k) * ldk;
            ISDQN_BOUNDS_CHECK(srow + min(lane, ldk - 1), 4, 30);
            ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 30);
            const int best = hl_argmax_first(srow, A, nb, lane, vmin, eta);
            mx = hl_expectation(nrow + (int64_t)best * nb, nb, lane, vmin, eta);
        } else {
            for (int a2 = 0; a2 < A; ++a2) mx = fmaxf(mx, hl_expectation(nrow + (int64_t)a2 * nb, nb, lane, vmin, eta));
        }
        const float tg = mlogits != nullptr ? tg_m : st.r[bl] + st.nt[bl] * st.g[bl] * mx;
        float v[PER_LANE], e[PER_LANE], s, w;
        const float m = hl_softmax_parts(logits + (int64_t)b * nlog_p + (int64_t)(a.on0 + k) * ldk + (int64_t)st.action[bl] * nb, nb, lane,
                                         vmin, eta, v, e, &s, &w);
        const float qv = w / s;
        const float y = fminf(fmaxf(tg, vmin), vmin + (float)nb * eta);
        const float u0 = erff((vmin - y) * inv_s), un = erff((vmin + (float)nb * eta - y) * inv_s);
        const float inv_norm = 1.f / (un - u0);
        double es = 0.0;
#pragma unroll
        for (int t = 0; t < PER_LANE; ++t) es += (double)e[t];  // (0 past nb)
        const double inv_sum_d = 1.0 / wave_sum_f64(es), inv_norm_d = 1.0 / ((double)un - (double)u0);
        const double scale_d = (double)inv_b * (double)st.w[bl];
        float pl = 0.f;
#pragma unroll
        for (int t = 0; t < PER_LANE; ++t) {
            const int j = lane + 64 * t;
            if (j < nb) {
                const float uh = erff((vmin + (float)(j + 1) * eta - y) * inv_s), ul = erff((vmin + (float)j * eta - y) * inv_s);
                const float p = (uh - ul) * inv_norm;
                pl += p * v[t];
                // (uh of bin j is ul of bin j + 1 bit for bit: the double differences telescope to un - u0)
                s_dl[(int64_t)pr * nb + j] = (float)(((double)e[t] * inv_sum_d - ((double)uh - (double)ul) * inv_norm_d) * scale_d);
            }
        }
        pl = wave_sum(pl);
        if (lane == 0) {
            st.loss[pr] = (m + logf(s) - pl) * st.w[bl];  // (st.td2 stays unweighted: the priorities are the raw TD error)
            st.td2[pr] = (qv - tg) * (qv - tg);
            if (q_values) q_values[(int64_t)b * K + k] = qv;
            if (targets) targets[(int64_t)b * K + k] = tg;
        }
    }
    __syncthreads();  // dout zero-fill (this workgroup's rows), s_dl / st.loss / st.td2 complete
    loss_epilogue<256>(a, st, s_dl);
}

}  // namespace isdqn
