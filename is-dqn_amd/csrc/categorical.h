// C51 categorical projection loss (Bellemare, Dabney and Munos, "A Distributional Perspective on Reinforcement Learning", ICML 2017) on the
// histogram heads; THE definition is include/isdqn_hip.h, isdqn_net_config::categorical.  The heads are those of n_bins = nb (hl_gauss.h:
// same layout, same expectation, atoms z_j = the bin centres c_j); only the loss differs: the value head's whole distribution at the greedy
// action is pushed through r + gamma^n z and projected back on the support,
//   m_i = sum_j p_j max(0, 1 - |b_j - i|),  b_j = (clamp(r + g z_j, z_0, z_{nb-1}) - z_0) / eta
// -- the projection as a gather: no l == u case (an atom landing exactly on a support point keeps its mass) and no atomics.
// One kernel, the shape of qr_loss_kernel (quantile.h): one wave per (transition, pair), C51_WAVES waves per workgroup, lane owns atoms
// i = lane + 64 t, fp32 with max subtraction, every sum a fixed __shfl_xor butterfly or the j loop in ascending j: bit-identical from run to
// run.
//   c51_loss_kernel: where hl_loss_kernel runs for histogram heads without the option (learn / loss / grad, every head selection).
#pragma once

namespace isdqn {

// Waves per workgroup: a (transition, pair) is a chain of dependent steps (A softmaxes, each three butterflies, then the nb-step broadcast
// loop), so a wave's time is the number of pairs it takes in turn -- as QR_WAVES (quantile.h).
constexpr int C51_WAVES = 16;
constexpr int C51_THREADS = 64 * C51_WAVES;

// The projection of one (transition, pair): the lanes hold p[t2] / bpos[t2] of atoms j = lane + 64 t2 and broadcast them one j at a time,
// ascending j, without a branch; leaves m_i of the lane's atoms i = lane + 64 t (t < NT) in m[t].
template <int NT>
__device__ __forceinline__ void c51_project(const float (&p)[PER_LANE], const float (&bpos)[PER_LANE], int nb, int lane,
                                            float (&m)[PER_LANE]) {
    float fi[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        fi[t] = (float)(lane + 64 * t);
        m[t] = 0.f;
    }
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
        const int nj = min(64, nb - 64 * t2);
        for (int jj = 0; jj < nj; ++jj) {
            const float pj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[t2]), jj));
            const float bj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bpos[t2]), jj));
#pragma unroll
            for (int t = 0; t < NT; ++t) m[t] += pj * fmaxf(0.f, 1.f - fabsf(bj - fi[t]));
        }
    }
}

// Iterated categorical Bellman target + cross-entropy, in the frame of head_loss.h (THE contract: there).  Wave w of C51_WAVES takes the
// (transition, k) pairs w, w + C51_WAVES, ...
//   a* = first argmax_a of the expectations of the value head (a.sel != null: of the selector head);
//   p = softmax(l^val(s', a*));  g = (1 - terminal) gamma^n;  m = the projection of (p, r + g z) above
//   CE = w_b (logsumexp(l) - sum_i m_i l_i),  dL/dl_i = w_b (softmax(l)_i - m_i) / B on the taken action's nb logits, 0 elsewhere.
// q_values / targets: the online expectation and the unclamped scalar r + g Q^val(s', a*).
// Dynamic LDS: R * K * nb floats of dL/dl.
template <int NT>
__global__ __launch_bounds__(C51_THREADS) void c51_loss_kernel(const HeadLossArgs a) {
    extern __shared__ float s_dl[];  // [R][K][nb]
    __shared__ LossStage st;
    const float *__restrict__ logits = a.out, *__restrict__ vlogits = a.val, *__restrict__ slogits = a.sel;
    float *__restrict__ q_values = a.q_values, *__restrict__ targets = a.targets;
    const int B = a.B, R = a.R, K = a.K, A = a.A, nb = a.nb, nlog_p = a.pitch;
    const float vmin = a.vmin, eta = a.eta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const float inv_b = 1.f / (float)B;
    const int ldk = A * nb;  // logits of one head
    loss_prologue<C51_THREADS>(a, st);
    __syncthreads();
    const float z0 = vmin + 0.5f * eta, zl = vmin + ((float)(nb - 1) + 0.5f) * eta;  // the end atoms, as hl_softmax_parts forms them
    for (int pr = wave; pr < R * K; pr += C51_WAVES) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) st.loss[pr] = st.td2[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const float* nrow = vlogits + (int64_t)b * nlog_p + (int64_t)(a.tg0 + k) * ldk;
        const float* drow = nrow;  // the deciding head's row
        if (slogits != nullptr) {  // Double Q-learning: the selector head decides, the value head supplies the distribution
            drow = slogits + (int64_t)b * a.sel_pitch + (int64_t)(a.sel_head + k) * ldk;
            ISDQN_BOUNDS_CHECK(drow + min(lane, ldk - 1), 4, 34);
        }
        ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 35);
        const int best = hl_argmax_first(drow, A, nb, lane, vmin, eta);
        // p_j = softmax(l^val(s', a*))_j and the position b_j of the pushed atom on the support, in the lanes that own j
        float v[PER_LANE], e[PER_LANE], p[PER_LANE], bpos[PER_LANE], mi[PER_LANE], s, w;
        hl_softmax_parts(nrow + (int64_t)best * nb, nb, lane, vmin, eta, v, e, &s, &w);
        const float disc = st.nt[bl] * st.g[bl];
        const float tg = st.r[bl] + disc * (w / s);
#pragma unroll
        for (int t = 0; t < PER_LANE; ++t) {
            const float z = vmin + ((float)(lane + 64 * t) + 0.5f) * eta;
            p[t] = e[t] / s;  // (0 past nb)
            bpos[t] = (fminf(fmaxf(st.r[bl] + disc * z, z0), zl) - z0) / eta;
        }
        c51_project<NT>(p, bpos, nb, lane, mi);
        const float m = hl_softmax_parts(logits + (int64_t)b * nlog_p + (int64_t)(a.on0 + k) * ldk + (int64_t)st.action[bl] * nb, nb, lane,
                                         vmin, eta, v, e, &s, &w);
        const float qv = w / s;
        const float inv_sum = 1.f / s;
        float pl = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int i = lane + 64 * t;
            if (i < nb) {
                pl += mi[t] * v[t];
                s_dl[(int64_t)pr * nb + i] = (e[t] * inv_sum - mi[t]) * inv_b * st.w[bl];
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
    loss_epilogue<C51_THREADS>(a, st, s_dl);
}

}  // namespace isdqn
