// Munchausen targets (Vieillard, Pietquin, Geist 2020; include/isdqn_hip.h, isdqn_net_config::munchausen_tau holds THE definition):
//   V(x)   = m + tau log(sum_a exp((Q(x, a) - m) / tau)),  m = max_a Q(x, a)       the soft value of the value head
//   target = r + alpha clip(Q(s, a_b) - V(s), l0, 0) + (1 - terminal) gamma^n V(s')
// Scalar per-(transition, pair) arithmetic shared by td_kernel, head_chain_kernel and hl_loss_kernel: fp32 with full-accuracy
// expf / logf.  The maximum is subtracted before the division by tau, so tau = 0.03 with |Q| in the hundreds neither overflows
// nor returns -inf: every exponent is <= 0 and the sum is >= 1.
#pragma once

namespace isdqn {

struct Munchausen {
    float tau, alpha, clip;  // tau == 0: off
};

__device__ __forceinline__ float soft_value(const float* v, int n, float tau) {
    float m = v[0];
    for (int j = 1; j < n; ++j) m = fmaxf(m, v[j]);
    float s = 0.f;
    for (int j = 0; j < n; ++j) s += expf((v[j] - m) / tau);
    return m + tau * logf(s);
}

// qa: Q(s, a_b) of the value head, vs / vn: its soft values on the state and on the next state, nt: 1 - terminal
__device__ __forceinline__ float munchausen_target(float r, float nt, float gamma_n, float qa, float vs, float vn, Munchausen mu) {
    const float bonus = mu.alpha * fminf(fmaxf(qa - vs, mu.clip), 0.f);
    return r + bonus + nt * gamma_n * vn;
}

}  // namespace isdqn
