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

constexpr int C51_MAX_ROWS = 4;  // transitions per workgroup
// Waves per workgroup: a (transition, pair) is a chain of dependent steps (A softmaxes, each three butterflies, then the nb-step broadcast
// loop), so a wave's time is the number of pairs it takes in turn -- as QR_WAVES (quantile.h).
constexpr int C51_WAVES = 16;
constexpr int C51_THREADS = 64 * C51_WAVES;

// The projection of one (transition, pair): the lanes hold p[t2] / bpos[t2] of atoms j = lane + 64 t2 and broadcast them one j at a time,
// ascending j, without a branch; leaves m_i of the lane's atoms i = lane + 64 t (t < NT) in m[t].
template <int NT>
__device__ __forceinline__ void c51_project(const float (&p)[HL_PER_LANE], const float (&bpos)[HL_PER_LANE], int nb, int lane,
                                            float (&m)[HL_PER_LANE]) {
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

// Iterated categorical Bellman target + cross-entropy.  Workgroup = R <= C51_MAX_ROWS transitions; wave w of C51_WAVES takes the
// (transition, k) pairs w, w + C51_WAVES, ...: online head on0 + k at the taken action is regressed on head tg0 + k of the next-state rows.
//   a* = first argmax_a of the expectations of the value head (`slogits` != null, isdqn_net_config::double_q: of head sh + k of the selector
//        rows, pitch s_pitch);  p = softmax(l^val(s', a*));  g = (1 - terminal) gamma^n;  m = the projection of (p, r + g z) above
//   CE = w_b (logsumexp(l) - sum_i m_i l_i),  dL/dl_i = w_b (softmax(l)_i - m_i) / B on the taken action's nb logits, 0 elsewhere
//   (w_b: isdqn_batch.loss_weights, 1 without).
// `vlogits`: the value rows of the B next states (pitch nlog_p).  Writes q_values / targets [B][K] (online expectation, the unclamped scalar
// r + g Q^val(s', a*)), priorities[B] = sqrt(mean_k (q - target)^2 + 1e-10) on those scalars, per-workgroup partials of the per-pair CE
// sums (loss_part [n_blk][K]) and, with `dout`, the dL/dlogits rows (zero-filled) and their column sums over the workgroup's rows
// (dbh_part [n_blk][nlog_p], the head-bias gradient); loss_finalize_kernel reduces both in a fixed order.
// Dynamic LDS: R * K * nb floats of dL/dl.
template <int NT>
__global__ __launch_bounds__(C51_THREADS) void c51_loss_kernel(const float* __restrict__ logits, const float* __restrict__ vlogits,
                                                               const float* __restrict__ slogits, int s_pitch, int sh, int B, int R, int K,
                                                               int on0, int tg0, int A, int nb, int nlog_p, float vmin, float eta,
                                                               const int* __restrict__ action, const float* __restrict__ reward,
                                                               const uint8_t* __restrict__ terminal, const float* __restrict__ loss_weights,
                                                               float gamma_n, float* __restrict__ dout, float* __restrict__ q_values,
                                                               float* __restrict__ targets, double* __restrict__ priorities,
                                                               float* __restrict__ loss_part, float* __restrict__ dbh_part) {
    extern __shared__ float s_dl[];  // [R][K][nb]
    __shared__ int s_action[C51_MAX_ROWS];
    __shared__ float s_r[C51_MAX_ROWS], s_nt[C51_MAX_ROWS], s_w[C51_MAX_ROWS];  // s_w: importance-sampling weights (none: 1)
    __shared__ float s_ce[C51_MAX_ROWS * 64], s_td2[C51_MAX_ROWS * 64];  // [R][K], K <= 64 (checked by the host)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * R;
    const int rows = min(R, B - b0);
    const float inv_b = 1.f / (float)B;
    const int ldk = A * nb;  // logits of one head
    if (dout != nullptr)
        for (int i = tid; i < rows * nlog_p; i += C51_THREADS) dout[(int64_t)b0 * nlog_p + i] = 0.f;
    if (tid < R) {
        const bool on = tid < rows;
        s_action[tid] = on ? action[b0 + tid] : -1;
        s_r[tid] = on ? reward[b0 + tid] : 0.f;
        s_nt[tid] = on ? 1.f - (float)terminal[b0 + tid] : 0.f;
        s_w[tid] = (on && loss_weights != nullptr) ? loss_weights[b0 + tid] : 1.f;
    }
    __syncthreads();
    const float z0 = vmin + 0.5f * eta, zl = vmin + ((float)(nb - 1) + 0.5f) * eta;  // the end atoms, as hl_softmax_parts forms them
    for (int pr = wave; pr < R * K; pr += C51_WAVES) {
        const int bl = pr / K, k = pr - bl * K;
        if (bl >= rows) {
            if (lane == 0) s_ce[pr] = s_td2[pr] = 0.f;
            continue;
        }
        const int b = b0 + bl;
        const float* nrow = vlogits + (int64_t)b * nlog_p + (int64_t)(tg0 + k) * ldk;
        // a*: first argmax of the deciding head's expectations (strict >: the lowest index wins)
        const float* drow = nrow;
        if (slogits != nullptr) {  // Double Q-learning: the selector head decides, the value head supplies the distribution
            drow = slogits + (int64_t)b * s_pitch + (int64_t)(sh + k) * ldk;
            ISDQN_BOUNDS_CHECK(drow + min(lane, ldk - 1), 4, 34);
        }
        ISDQN_BOUNDS_CHECK(nrow + min(lane, ldk - 1), 4, 35);
        int best = 0;
        float bv = hl_expectation(drow, nb, lane, vmin, eta);
        for (int a2 = 1; a2 < A; ++a2) {
            const float x = hl_expectation(drow + (int64_t)a2 * nb, nb, lane, vmin, eta);
            if (x > bv) { bv = x; best = a2; }
        }
        // p_j = softmax(l^val(s', a*))_j and the position b_j of the pushed atom on the support, in the lanes that own j
        float v[HL_PER_LANE], e[HL_PER_LANE], p[HL_PER_LANE], bpos[HL_PER_LANE], mi[HL_PER_LANE], s, w;
        hl_softmax_parts(nrow + (int64_t)best * nb, nb, lane, vmin, eta, v, e, &s, &w);
        const float disc = s_nt[bl] * gamma_n;
        const float tg = s_r[bl] + disc * (w / s);
#pragma unroll
        for (int t = 0; t < HL_PER_LANE; ++t) {
            const float z = vmin + ((float)(lane + 64 * t) + 0.5f) * eta;
            p[t] = e[t] / s;  // (0 past nb)
            bpos[t] = (fminf(fmaxf(s_r[bl] + disc * z, z0), zl) - z0) / eta;
        }
        c51_project<NT>(p, bpos, nb, lane, mi);
        const float m = hl_softmax_parts(logits + (int64_t)b * nlog_p + (int64_t)(on0 + k) * ldk + (int64_t)s_action[bl] * nb, nb, lane,
                                         vmin, eta, v, e, &s, &w);
        const float qv = w / s;
        const float inv_sum = 1.f / s;
        float pl = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int i = lane + 64 * t;
            if (i < nb) {
                pl += mi[t] * v[t];
                s_dl[(int64_t)pr * nb + i] = (e[t] * inv_sum - mi[t]) * inv_b * s_w[bl];
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
    for (int k = tid; k < K; k += C51_THREADS) {
        float sum = 0.f;
        for (int bl = 0; bl < R; ++bl) sum += s_ce[bl * K + k];
        loss_part[(int64_t)blockIdx.x * K + k] = sum;
    }
    if (dout != nullptr) {
        for (int i = tid; i < rows * K * nb; i += C51_THREADS) {
            const int pr = i / nb, j = i - pr * nb;
            const int bl = pr / K, k = pr - bl * K;
            dout[(int64_t)(b0 + bl) * nlog_p + (int64_t)(on0 + k) * ldk + (int64_t)s_action[bl] * nb + j] = s_dl[i];
        }
        // column c = (h * A + a) * nb + j collects the rows whose action is a, for the regressed heads h in [on0, on0 + K)
        for (int c = tid; c < nlog_p; c += C51_THREADS) {
            const int h = c / ldk, rem = c - h * ldk, a = rem / nb, j = rem - a * nb;
            float sum = 0.f;
            if (h >= on0 && h < on0 + K)
                for (int bl = 0; bl < rows; ++bl) sum += (s_action[bl] == a) ? s_dl[((int64_t)bl * K + h - on0) * nb + j] : 0.f;
            dbh_part[(int64_t)blockIdx.x * nlog_p + c] = sum;
        }
    }
    if (priorities != nullptr && tid < rows) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s_td2[tid * K + k];
        priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }
}

// Transitions per workgroup of c51_loss_kernel: C51_MAX_ROWS while the dL/dl staging stays within 32 KB of LDS.
static inline int c51_rows_per_wg(int K, int nb) {
    int R = (8192 / (K * nb));
    return R < 1 ? 1 : R > C51_MAX_ROWS ? C51_MAX_ROWS : R;
}

}  // namespace isdqn
