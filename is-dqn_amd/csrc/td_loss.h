// The per-element TD loss of the scalar heads, shared by td_kernel (row_kernels.h, net_kernels.hip) and mix_td_kernel
// (mixture_kernels.hip); included inside namespace isdqn by both, as philox.h is.  No kernel in this header.
#pragma once

// Per-element loss and its derivative w.r.t. q for d = q - target: squared error (the reference, isdqn.py:102) or, with
// huber_delta > 0, the Huber loss (0.5 d^2 inside, delta (|d| - delta / 2) outside; derivative clip(d, -delta, delta)).
__device__ __forceinline__ float td_loss(float d, float huber_delta) {
    const float a = fabsf(d);
    return huber_delta > 0.f ? (a <= huber_delta ? 0.5f * d * d : huber_delta * (a - 0.5f * huber_delta)) : d * d;
}
__device__ __forceinline__ float td_dloss(float d, float huber_delta) {
    return huber_delta > 0.f ? fminf(fmaxf(d, -huber_delta), huber_delta) : 2.f * d;
}
