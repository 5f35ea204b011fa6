// The small kernels of the entry points beside the learn step: shift_kernel, argmax_kernel / argmax_rows_kernel, act_rowsum_kernel.
// Included by net_kernels.hip inside namespace isdqn, behind grad_clip.h.
#pragma once
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
