// ReDo: recycling dormant neurons (Sokar, Agarwal, Castro, Evci 2023, "The Dormant Neuron Phenomenon in Deep Reinforcement
// Learning"; include/isdqn_hip.h, isdqn_net_redo holds THE definition).  The reference has no counterpart.
//   a_c     = mean over rows and pixel positions of the post-ReLU activation of neuron c (conv: an output channel)
//   dormant = a_c <= tau * mean_c' a_c'                                                   (per layer, fp32)
//   recycle = incoming weights, bias [, LayerNorm scale / bias] of c <- fresh parameters; every weight of the next layer that
//             reads c <- 0; Adam moments <- 0 wherever a parameter was written
// Three kernels, no atomics, every sum in a fixed order: the score of one layer from the per-position sums act_rowsum_kernel
// left in scratch, the row copy and the column zeroing.  All of them index the internal layout of isdqn_net_param_layout.
#pragma once

namespace isdqn {

constexpr int REDO_MAX_WIDTH = 8192;  // widest hidden layer the plan accepts (net_plan.h: dense widths <= 8192, conv <= 64)

// One workgroup per layer.  possum [npix][c]: the sums over the rows per (pixel, channel) in the reference's feature order.
// Lanes run along c (contiguous); every channel adds its pixels in ascending order, thread 0 adds the channels in ascending
// order for the layer mean.  scores / mask [c], n_recycled [1].
__global__ __launch_bounds__(256) void redo_score_kernel(const float* __restrict__ possum, int npix, int c, float count, float tau,
                                                         float* __restrict__ scores, int* __restrict__ mask, int* __restrict__ n_recycled) {
    __shared__ float s_a[REDO_MAX_WIDTH];
    __shared__ int s_cnt[256];
    __shared__ float s_thr;
    const int tid = threadIdx.x;
    for (int ch = tid; ch < c; ch += 256) {
        float t = 0.f;
        for (int p = 0; p < npix; ++p) t += possum[(int64_t)p * c + ch];
        const float a = t / count;
        s_a[ch] = a;
        scores[ch] = a;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int ch = 0; ch < c; ++ch) t += s_a[ch];
        s_thr = tau * (t / (float)c);
    }
    __syncthreads();
    const float thr = s_thr;
    int n = 0;
    for (int ch = tid; ch < c; ch += 256) {
        const int d = s_a[ch] <= thr ? 1 : 0;  // (a layer that is zero everywhere: 0 <= 0, dormant everywhere)
        mask[ch] = d;
        n += d;
    }
    s_cnt[tid] = n;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int k = 0; k < 256; ++k) t += s_cnt[k];
        *n_recycled = t;
    }
}

// Incoming side of the dormant neurons of one layer: grid (ceil(K / 1024), neurons).  Row c of the layer's kernel [out_p][K]
// (K % 4 == 0: Conv_0's [plane][ky * 8 + kx] form, [tap][in_p] and [in_p] alike, padded input lanes included), bias c and, when the
// layer has a LayerNorm, its scale c and bias c are copied from `fresh`; the moments of all of them are cleared (m, v: both or none).
__global__ __launch_bounds__(256) void redo_incoming_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ fresh, const int* __restrict__ mask, int64_t w_off,
                                                            int K, int64_t b_off, int64_t g_off, int64_t be_off) {
    const int c = blockIdx.y;
    if (!mask[c]) return;
    const int k = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (k < K) {
        const int64_t i = w_off + (int64_t)c * K + k;
        *reinterpret_cast<f32x4*>(p + i) = *reinterpret_cast<const f32x4*>(fresh + i);
        if (m != nullptr) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(m + i) = z;
            *reinterpret_cast<f32x4*>(v + i) = z;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        const int64_t i = (threadIdx.x == 0 ? b_off : threadIdx.x == 1 ? g_off : be_off);
        if (i >= 0) {
            p[i + c] = fresh[i + c];
            if (m != nullptr) {
                m[i + c] = 0.f;
                v[i + c] = 0.f;
            }
        }
    }
}

// Outgoing side: the kernel [rows][K] of the NEXT layer, grid (ceil(K / 8 / 256), rows) with every row, the padded ones too.
// Column k reads neuron k % cpp of the layer below (cpp: its padded width -- [tap][c_p], [p * c_p + c] behind the last convolution
// and [in_p] are the same formula); lanes run along k, the contiguous axis of both the weights and the mask lookup, in groups of
// 8 columns that never straddle a pixel (cpp % 8 == 0).  Only dormant columns are stored to.
__global__ __launch_bounds__(256) void redo_outgoing_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                            const int* __restrict__ mask, int c, int cpp, int64_t w_off, int K) {
    const int k0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 8;
    if (k0 >= K) return;
    const int ci0 = k0 % cpp;
    const int64_t i0 = w_off + (int64_t)blockIdx.y * K + k0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (ci0 + i < c && mask[ci0 + i]) {
            p[i0 + i] = 0.f;
            if (m != nullptr) {
                m[i0 + i] = 0.f;
                v[i0 + i] = 0.f;
            }
        }
    }
}

}  // namespace isdqn
