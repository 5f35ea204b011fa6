// QR-DQN quantile-regression heads (Dabney et al., "Distributional Reinforcement Learning with Quantile Regression", AAAI 2018) on the
// Q-network heads; THE definition is include/isdqn_hip.h, isdqn_net_config::n_quantiles.  With n_quantiles = N > 0 the head layer has
// n_heads * A * N outputs, output ((h * A) + a) * N + i being theta_i of action a of head h, the quantile at tau_i = (i + 1/2) / N;
//   Q_h(s, a) = (1 / N) sum_i theta_i.
// Two kernels, both one wave per (row, head / action) or (transition, pair) with the lanes over the quantiles (lane owns theta_i for
// i = lane + 64 t), fp32, every sum in a fixed order (a lane's own values in ascending t, then a __shfl_xor butterfly; the j loop of the
// pairwise loss in ascending j): bit-identical from run to run, no atomics.
//   qr_expect_kernel: quantile rows -> Q rows (forward / best_action / best_actions and the DQN-form target rows, where
//                     hl_expect_kernel runs for histogram heads);
//   qr_loss_kernel:   where hl_loss_kernel runs for histogram heads (learn / loss / grad, every head selection; head_loss.h).
#pragma once

namespace isdqn {

// Waves per workgroup of qr_loss_kernel.  A (transition, pair) is a chain of dependent steps -- A row loads, each followed by a butterfly,
// then the N x N loop -- so a wave's time is the number of pairs it takes in turn: 16 waves share the R * K pairs of a workgroup (9 each
// with 4 waves at K = 9, 98.8 us measured at B = 256; 3 each with 16), and the partial rows the workgroup leaves stay as many.
constexpr int QR_WAVES = 16;
constexpr int QR_THREADS = 64 * QR_WAVES;
constexpr int QR_AHEAD = 4;  // actions whose rows are requested before the first of them is reduced

// The N quantile values at `th` (one action of one head) into the lanes' registers (0 past N) ...
__device__ __forceinline__ void qr_load(const float* __restrict__ th, int N, int lane, float (&v)[PER_LANE]) {
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int i = lane + 64 * t;
        v[t] = i < N ? th[i] : 0.f;
    }
}
// ... and their mean: the lane's own values in ascending t, the butterfly, one division -- the same bits in every lane and wherever
// it is called.
__device__ __forceinline__ float qr_reduce(const float (&v)[PER_LANE], int N) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) s += v[t];
    return wave_sum(s) / (float)N;
}
__device__ __forceinline__ float qr_mean(const float* __restrict__ th, int N, int lane, float (&v)[PER_LANE]) {
    qr_load(th, N, lane, v);
    return qr_reduce(v, N);
}

// q[row][c] = mean of the quantile values of column c = h * A + a (c < nha) at rows[row][c * N .. c * N + N); the padding columns of
// q are not written.
__global__ __launch_bounds__(256) void qr_expect_kernel(const float* __restrict__ rows, int n_rows, int nha, int N, int nlog_p, int nha_p,
                                                        float* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)n_rows * nha) return;  // (whole waves: the shuffles below see every lane of theirs)
    const int row = (int)(item / nha), c = (int)(item - (int64_t)row * nha);
    float v[PER_LANE];
    const float qv = qr_mean(rows + (int64_t)row * nlog_p + (int64_t)c * N, N, lane, v);
    if (lane == 0) q[(int64_t)row * nha_p + c] = qv;
}

// The N x N pairwise sums of one (transition, pair): the lane's online quantiles th[t] (i = lane + 64 t, t < NT) against the target
// atoms tv[t2] (j = lane + 64 t2, held by the lanes and broadcast one at a time, ascending j).  Leaves in g[t] / ls[t] the sums over j
// of |tau_i - 1{u < 0}| * clip(u, -kappa, kappa) and |tau_i - 1{u < 0}| * L_kappa(u) (HUBER), or * sign(u) and * |u| (kappa = 0),
// u = t_j - theta_i.  The indicator is a select and h' a clamp: the loop body has no branch.
template <int NT, bool HUBER>
__device__ __forceinline__ void qr_pairwise(const float (&th)[PER_LANE], const float (&tv)[PER_LANE], int N, int lane, float kappa,
                                            float (&g)[PER_LANE], float (&ls)[PER_LANE]) {
    float tau[NT], omt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        tau[t] = ((float)(lane + 64 * t) + 0.5f) / (float)N;
        // 1 - tau_i from its own exact numerator: 1.f - tau[t] would carry tau's rounding, N ulps of 1 - tau at the last quantile
        omt[t] = ((float)(N - 1 - (lane + 64 * t)) + 0.5f) / (float)N;
        g[t] = ls[t] = 0.f;
    }
#pragma unroll
    for (int t2 = 0; t2 < NT; ++t2) {
        const int nj = min(64, N - 64 * t2);
        for (int jj = 0; jj < nj; ++jj) {
            const float tj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tv[t2]), jj));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float u = tj - th[t];
                const float wgt = u < 0.f ? omt[t] : tau[t];
                const float au = fabsf(u);
                float c, L;
                if (HUBER) {
                    c = fminf(fmaxf(u, -kappa), kappa);
                    L = au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa);
                } else {
                    c = (u > 0.f ? 1.f : 0.f) - (u < 0.f ? 1.f : 0.f);
                    L = au;
                }
                g[t] += wgt * c;
                ls[t] += wgt * L;
            }
        }
    }
}

// Iterated Bellman target atoms + quantile-regression (Huber) loss, in the frame of head_loss.h (THE contract: there).  Wave w of
// QR_WAVES takes the (transition, k) pairs w, w + QR_WAVES, ...; kappa = a.huber_delta.
//   a* = first argmax_a of the means of the value head (a.sel != null: of the selector head);
//   t_j = r + ((1 - terminal) gamma^n) theta^val_j(s', a*);  u_ij = t_j - theta_i(s, a_b)
//   l = sum_i (1 / N) sum_j |tau_i - 1{u_ij < 0}| h_kappa(u_ij),  dL/dtheta_i = -(w_b / (B N)) sum_j |tau_i - 1{u_ij < 0}| h'_kappa(u_ij)
//   on the taken action's N outputs, 0 elsewhere.
// q_values / targets: the online mean and r + (1 - terminal) gamma^n * mean of the value row at a*.
// The selection below is this kernel's own, not hl_argmax_first's shape: QR_AHEAD rows are requested before the first is reduced (a
// measured optimisation), and the loop also captures the winning row's quantiles.
// Dynamic LDS: R * K * N floats of dL/dtheta.
template <int NT, bool HUBER>
__global__ __launch_bounds__(QR_THREADS) void qr_loss_kernel(const HeadLossArgs a) {
    extern __shared__ float s_dl[];  // [R][K][N]
    __shared__ LossStage st;
    const float *__restrict__ logits = a.out, *__restrict__ vlogits = a.val, *__restrict__ slogits = a.sel;
    float *__restrict__ q_values = a.q_values, *__restrict__ targets = a.targets;
    const int B = a.B, R = a.R, K = a.K, A = a.A, N = a.nb, nlog_p = a.pitch;
    const float kappa = a.huber_delta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const int ldk = A * N;  // outputs of one head
    loss_prologue<QR_THREADS>(a, st);
    __syncthreads();
    const float inv_n = 1.f / (float)N;
    for (int pr = wave; pr < R * K; pr += QR_WAVES) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) st.loss[pr] = st.td2[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const float* nrow = vlogits + (int64_t)b * nlog_p + (int64_t)(a.tg0 + k) * ldk;
        // a*: first argmax of the deciding head's means (strict >: the lowest index wins); tv: the value head's quantiles at a*
        const float* drow = nrow;
        if (slogits != nullptr) {  // Double Q-learning: the selector head decides, the value head supplies the atoms
            drow = slogits + (int64_t)b * a.sel_pitch + (int64_t)(a.sel_head + k) * ldk;
            ISDQN_BOUNDS_CHECK(drow + min(lane, ldk - 1), 4, 32);
        }
        ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 33);
        float tv[PER_LANE], x[QR_AHEAD][PER_LANE];
        int best = 0;
        float mx = -INFINITY;
        for (int a0 = 0; a0 < A; a0 += QR_AHEAD) {  // QR_AHEAD rows in flight, reduced and compared in ascending a
#pragma unroll
            for (int d = 0; d < QR_AHEAD; ++d) qr_load(drow + (int64_t)min(a0 + d, A - 1) * N, N, lane, x[d]);
#pragma unroll
            for (int d = 0; d < QR_AHEAD; ++d) {
                const float m = qr_reduce(x[d], N);
                if (a0 + d < A && (m > mx || a0 + d == 0)) {
                    mx = m;
                    best = a0 + d;
#pragma unroll
                    for (int t = 0; t < PER_LANE; ++t) tv[t] = x[d][t];
                }
            }
        }
        if (slogits != nullptr) mx = qr_mean(nrow + (int64_t)best * N, N, lane, tv);
        const float disc = st.nt[bl] * st.g[bl];
        const float tg = st.r[bl] + disc * mx;
#pragma unroll
        for (int t = 0; t < PER_LANE; ++t) tv[t] = st.r[bl] + disc * tv[t];  // the target atoms t_j, j = lane + 64 t
        float th[PER_LANE], g[PER_LANE], ls[PER_LANE];
        const float qv = qr_mean(logits + (int64_t)b * nlog_p + (int64_t)(a.on0 + k) * ldk + (int64_t)st.action[bl] * N, N, lane, th);
        qr_pairwise<NT, HUBER>(th, tv, N, lane, kappa, g, ls);
        const float scale = st.w[bl] / (float)(B * N);
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int i = lane + 64 * t;
            if (i < N) {
                const float gs = HUBER ? g[t] / kappa : g[t];
                l += (HUBER ? ls[t] / kappa : ls[t]) * inv_n;
                s_dl[(int64_t)pr * N + i] = -(scale * gs);
            }
        }
        l = wave_sum(l);
        if (lane == 0) {
            st.loss[pr] = l * st.w[bl];  // (st.td2 stays unweighted: the priorities are the raw TD error)
            st.td2[pr] = (qv - tg) * (qv - tg);
            if (q_values) q_values[(int64_t)b * K + k] = qv;
            if (targets) targets[(int64_t)b * K + k] = tg;
        }
    }
    __syncthreads();  // dout zero-fill (this workgroup's rows), s_dl / st.loss / st.td2 complete
    loss_epilogue<QR_THREADS>(a, st, s_dl);
}

}  // namespace isdqn
