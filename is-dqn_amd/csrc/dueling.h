// Dueling value / advantage heads (Wang et al. 2016; include/isdqn_hip.h, isdqn_net_config::dueling holds THE definition).
//   raw row     [H][A + 1][w]: per head the A advantage rows, then the value row, w components each (w = 1: scalar heads)
//   combine     out[h][a][j] = raw[h][A][j] + (raw[h][a][j] - (sum_a raw[h][a][j]) / A)
//   backward    draw[h][A][j] = sum_a d[h][a][j],  draw[h][a][j] = d[h][a][j] - draw[h][A][j] / A
//   mask        the structural zeros of the head kernel [R][in_p]: columns [F2, F) of a value row, [0, F2) of an advantage row
// Three row-wise kernels, bandwidth-trivial (at most 2B x R floats; they count through their launches): one thread per (row, head, j)
// looping over the actions in ascending order, so neighbouring lanes read neighbouring j when w > 1.  Every sum is in a fixed order,
// no atomics, no LDS: bit-identical from run to run.  The padded columns behind the last real one are written as zeros, as
// dense_post_kernel and the loss kernels leave them.  The loops over the actions stay scalar (DUEL_SCALAR_LOOP): the loop vectoriser
// would pair two actions into negated packed fp32 adds, the form scripts/isa_lint.py (rule R3) keeps out of the
// library.
#pragma once

namespace isdqn {

constexpr int DUEL_THREADS = 256;
#define DUEL_SCALAR_LOOP _Pragma("clang loop vectorize(disable) interleave(disable)")

// raw [n_rows][raw_pitch] -> out [n_rows][pitch]
__global__ __launch_bounds__(DUEL_THREADS) void duel_combine_kernel(const float* __restrict__ raw, int raw_pitch, float* __restrict__ out, int pitch,
                                                                    int n_rows, int H, int A, int w) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t t = (int64_t)blockIdx.x * DUEL_THREADS + threadIdx.x;
    const int hw = H * w;
    if (t >= (int64_t)n_rows * hw) return;
    const int row = (int)(t / hw), r = (int)(t - (int64_t)row * hw);
    const int h = r / w, j = r - h * w;
    const float* __restrict__ src = raw + (int64_t)row * raw_pitch + (int64_t)h * (A + 1) * w + j;
    float* __restrict__ dst = out + (int64_t)row * pitch + (int64_t)h * A * w + j;
    ISDQN_BOUNDS_CHECK(src, 4, 36);
    ISDQN_BOUNDS_CHECK(src + (int64_t)A * w, 4, 36);
    float s = 0.f;
    DUEL_SCALAR_LOOP
    for (int a = 0; a < A; ++a) s += src[(int64_t)a * w];
    const float mean = s / (float)A;
    const float v = src[(int64_t)A * w];
    DUEL_SCALAR_LOOP
    for (int a = 0; a < A; ++a) dst[(int64_t)a * w] = v + (src[(int64_t)a * w] - mean);
    if (r == 0)
        for (int c = H * A * w; c < pitch; ++c) out[(int64_t)row * pitch + c] = 0.f;
}

// dout [B][pitch] -> draw [B][raw_pitch]; row B of the grid: the reduced head-bias gradient dbh [pitch] -> dbh_raw [raw_pitch]
__global__ __launch_bounds__(DUEL_THREADS) void duel_backward_kernel(const float* __restrict__ dout, int pitch, float* __restrict__ draw, int raw_pitch,
                                                                     const float* __restrict__ dbh, float* __restrict__ dbh_raw, int B, int H, int A,
                                                                     int w) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t t = (int64_t)blockIdx.x * DUEL_THREADS + threadIdx.x;
    const int hw = H * w;
    if (t >= (int64_t)(B + 1) * hw) return;
    const int row = (int)(t / hw), r = (int)(t - (int64_t)row * hw);
    const int h = r / w, j = r - h * w;
    const float* __restrict__ src = (row < B ? dout + (int64_t)row * pitch : dbh) + (int64_t)h * A * w + j;
    float* base = row < B ? draw + (int64_t)row * raw_pitch : dbh_raw;
    float* __restrict__ dst = base + (int64_t)h * (A + 1) * w + j;
    ISDQN_BOUNDS_CHECK(src, 4, 37);
    ISDQN_BOUNDS_CHECK(src + (int64_t)(A - 1) * w, 4, 37);
    float s = 0.f;
    DUEL_SCALAR_LOOP
    for (int a = 0; a < A; ++a) s += src[(int64_t)a * w];
    const float m = s / (float)A;
    DUEL_SCALAR_LOOP
    for (int a = 0; a < A; ++a) dst[(int64_t)a * w] = src[(int64_t)a * w] - m;
    dst[(int64_t)A * w] = s;
    if (r == 0)
        for (int c = H * (A + 1) * w; c < raw_pitch; ++c) base[c] = 0.f;
}

// Re-zero the structural entries of the head kernel at w_off ([R][in_p], R = H * (A + 1) * w rows) in every buffer given (null: left
// alone): the parameters, both Adam moments, both halves of the S8 weight mirror (gemm_core.h: a group of 8 values is 8 bf16 hi, then
// 8 bf16 lo) and a gradient buffer.  One thread per structural entry, lanes along the hidden units.
__global__ __launch_bounds__(DUEL_THREADS) void duel_mask_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                 float* __restrict__ mirror, float* __restrict__ grad, int64_t w_off, int in_p, int R,
                                                                 int A, int w, int F2) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t t = (int64_t)blockIdx.x * DUEL_THREADS + threadIdx.x;
    if (t >= (int64_t)R * F2) return;
    const int o = (int)(t / F2), k = (int)(t - (int64_t)o * F2);
    const int c = (o / w) % (A + 1);
    const int64_t i = w_off + (int64_t)o * in_p + (c == A ? F2 + k : k);
    if (p != nullptr) p[i] = 0.f;
    if (m != nullptr) m[i] = 0.f;
    if (v != nullptr) v[i] = 0.f;
    if (grad != nullptr) grad[i] = 0.f;
    if (mirror != nullptr) {
        unsigned short* __restrict__ g = reinterpret_cast<unsigned short*>(mirror + (i & ~(int64_t)7)) + (i & 7);
        g[0] = 0;
        g[8] = 0;
    }
}

#undef DUEL_SCALAR_LOOP

}  // namespace isdqn
