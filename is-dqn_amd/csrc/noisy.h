// NoisyNet exploration: factorised Gaussian noise on every Dense layer (Fortunato et al., "Noisy Networks for Exploration", ICLR 2018).
// include/isdqn_hip.h, isdqn_noisy_layout holds THE definition.  Included by net_kernels.hip inside namespace isdqn, behind the learn
// step and in front of the noisy entry points: its kernels are the last but reset.h's in tests/golden/kernel_order.txt, and
// tests/test_kernel_order_host.py holds every kernel of the code object to its place there (why: docs/NOTEBOOK.md).
// Built beside the plan: no field of isdqn_net_config, no workspace region and nothing of build_plan belongs to it.  The caller owns
// sigma, its moments, the noise vectors, the composed parameters `eff` and the reduced gradient; the existing forward / loss / gradient
// code runs unchanged on `eff`.
//   noisy_sample_kernel    one launch over all noise vectors: Philox4x32-10 keyed by (seed, *noise_count, stream, layer, vector, j),
//                          Box-Muller, f(z) = sign(z) sqrt|z|.  One element per thread: a few thousand elements in all.
//   noisy_advance_kernel   one thread, behind it: *noise_count += 1 with an ordinary store (a kernel boundary orders it behind every read)
//   noisy_compose_kernel   one float4 per thread over the flat parameter buffer: eff = mu + sigma * (eout[o] * ein[i]) on Dense kernels,
//                          mu + sigma * eout[o] on Dense biases, mu elsewhere; optionally the S8 mirror of eff
//   noisy_adam_kernel      one float4 per thread over the flat buffer: Adam on mu from g, on the Dense positions of sigma from fl32(g * n)
// The three element passes find their tensor through NoisyTable, as adam_kernel does through AdamTable.  Every tensor offset and every
// Dense row length is a multiple of 8 floats, so the four elements of a thread share a tensor and a row: eout[o] is one register, ein one
// 16-byte load; the row comes from a multiply-high (FastDiv, as the conv geometry's divisions), and the table holds two entries per Dense
// layer -- six at the headline shape -- in ascending offset order, scanned linearly.  No atomics anywhere.
#pragma once

struct NoisyEntry {
    int64_t p_off, size;  // a Dense kernel [out_p][in_p] or a Dense bias [out_p] in the flat parameter buffer
    int64_t ein_off, eout_off;  // its layer's vectors in `noise` (floats)
    int in_p;  // kernel: row length; bias: 0
    FastDiv d_in;  // kernel: division by in_p (every tensor holds fewer than 2^31 elements)
};
struct NoisyTable {
    NoisyEntry e[2 * MAX_LAYERS];
    int n;
};
// vector v of the sample launch: `n` elements at `off` of `noise`, Philox counter word 1 = (stream_id << 16) | id, id = 2 l + (0 in, 1 out)
struct NoisyVec {
    int64_t off;
    int n, id, block_start, pad;
};
struct NoisyVecTable {
    NoisyVec v[2 * MAX_LAYERS];
    int n, total_blocks;
};

#include "philox.h"  // philox4x32_10, shared with augment.h

// f(z) of one standard normal from two Philox words.  u1 = (k + 1/2) 2^-24 with k = x0 >> 8 has 25 significant bits from k = 2^23 on:
// there -ln u1 is taken as -log1p(-(1 - u1)), whose argument (2^24 - k - 1/2) 2^-24 is exact in fp32; below, u1 itself is exact
__device__ __forceinline__ float noisy_value(uint32_t x0, uint32_t x1) {
    const uint32_t k = x0 >> 8;
    const float l = k < (1u << 23) ? logf(((float)k + 0.5f) * 0x1p-24f) : log1pf(-(((float)((1u << 24) - k) - 0.5f) * 0x1p-24f));
    const float u2 = (float)(x1 >> 8) * 0x1p-24f;
    const float z = sqrtf(-2.f * l) * cospif(2.f * u2);
    return copysignf(sqrtf(fabsf(z)), z);
}

constexpr int NOISY_THREADS = 256;
__global__ __launch_bounds__(NOISY_THREADS) void noisy_sample_kernel(const NoisyVecTable tab, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id,
                                                                     const int64_t* __restrict__ noise_count, float* __restrict__ noise) {
    ISDQN_EMPTY_KERNEL_RETURN
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.v[e + 1].block_start) ++e;
    const NoisyVec vec = tab.v[e];
    const int j = ((int)blockIdx.x - vec.block_start) * NOISY_THREADS + (int)threadIdx.x;
    if (j >= vec.n) return;
    ISDQN_BOUNDS_CHECK(noise_count, 8, 40);
    const uint64_t count = (uint64_t)*noise_count;
    uint32_t x0, x1;
    philox4x32_10((uint32_t)j, (stream_id << 16) | (uint32_t)vec.id, (uint32_t)count, (uint32_t)(count >> 32), seed_lo, seed_hi, x0, x1);
    noise[vec.off + j] = noisy_value(x0, x1);
}
__global__ void noisy_advance_kernel(int64_t* __restrict__ noise_count) {
    ISDQN_EMPTY_KERNEL_RETURN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ISDQN_BOUNDS_CHECK(noise_count, 8, 40);
        *noise_count = *noise_count + 1;
    }
}

// the noise factors of the four elements at offset o of the flat buffer: n[r] = eout[row] * ein[col + r] on a Dense kernel, eout[row + r]
// on a Dense bias.  false: no noisy tensor holds o
__device__ __forceinline__ bool noisy_factors(const NoisyTable& tab, const float* __restrict__ noise, int64_t o, float (&n)[4]) {
    int e = -1;
    for (int k = 0; k < tab.n; ++k)
        if (o >= tab.e[k].p_off && o < tab.e[k].p_off + tab.e[k].size) e = k;
    if (e < 0) return false;
    const NoisyEntry en = tab.e[e];
    const uint32_t i = (uint32_t)(o - en.p_off);
    if (en.in_p > 0) {
        uint32_t row, col;
        en.d_in.divmod(i, row, col);
        ISDQN_BOUNDS_CHECK(noise + en.eout_off + row, 4, 41);
        ISDQN_BOUNDS_CHECK(noise + en.ein_off + col, 16, 41);
        const float eo = noise[en.eout_off + row];
        const float4 ei = *reinterpret_cast<const float4*>(noise + en.ein_off + col);
        n[0] = eo * ei.x; n[1] = eo * ei.y; n[2] = eo * ei.z; n[3] = eo * ei.w;
    } else {
        ISDQN_BOUNDS_CHECK(noise + en.eout_off + i, 16, 41);
        const float4 eo = *reinterpret_cast<const float4*>(noise + en.eout_off + i);
        n[0] = eo.x; n[1] = eo.y; n[2] = eo.z; n[3] = eo.w;
    }
    return true;
}

// eff = mu + sigma * n in fp32, product and sum rounded separately (-ffp-contract=off); mirror != nullptr: also the S8 form of eff
__global__ __launch_bounds__(NOISY_THREADS) void noisy_compose_kernel(const NoisyTable tab, const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                      const float* __restrict__ noise, float* __restrict__ eff,
                                                                      float* __restrict__ mirror, int64_t n_params) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t o = ((int64_t)blockIdx.x * NOISY_THREADS + threadIdx.x) * 4;
    if (o >= n_params) return;
    ISDQN_BOUNDS_CHECK(mu + o, 16, 41);
    float4 p = *reinterpret_cast<const float4*>(mu + o);
    float n[4];
    if (noisy_factors(tab, noise, o, n)) {
        ISDQN_BOUNDS_CHECK(sigma + o, 16, 41);
        const float4 s = *reinterpret_cast<const float4*>(sigma + o);
        const float t0 = s.x * n[0], t1 = s.y * n[1], t2 = s.z * n[2], t3 = s.w * n[3];
        p.x = p.x + t0; p.y = p.y + t1; p.z = p.z + t2; p.w = p.w + t3;
    }
    *reinterpret_cast<float4*>(eff + o) = p;
    if (mirror != nullptr) s8_store_quad(mirror, (int)o, p.x, p.y, p.z, p.w);
}

// Adam behind the gradient-only pass on eff: g_mu = g everywhere, g_sigma = fl32(g * n) on the Dense positions; adam_kernel's element
// update with the step's bias corrections `consts` (loss_finalize_kernel wrote them when it advanced adam_count)
__global__ __launch_bounds__(NOISY_THREADS) void noisy_adam_kernel(const NoisyTable tab, const float* __restrict__ grad, const float* __restrict__ noise,
                                                                   float* __restrict__ mu, float* __restrict__ m_mu, float* __restrict__ v_mu,
                                                                   float* __restrict__ sigma, float* __restrict__ m_sigma, float* __restrict__ v_sigma,
                                                                   const float* __restrict__ consts, float lr, float b1, float b2, float eps,
                                                                   int64_t n_params) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int64_t o = ((int64_t)blockIdx.x * NOISY_THREADS + threadIdx.x) * 4;
    if (o >= n_params) return;
    ISDQN_BOUNDS_CHECK(grad + o, 16, 42);
    ISDQN_BOUNDS_CHECK(mu + o, 16, 42);
    ISDQN_BOUNDS_CHECK(m_mu + o, 16, 42);
    ISDQN_BOUNDS_CHECK(v_mu + o, 16, 42);
    float4 pm = *reinterpret_cast<const float4*>(m_mu + o);
    float4 pv = *reinterpret_cast<const float4*>(v_mu + o);
    float4 pp = *reinterpret_cast<const float4*>(mu + o);
    const float4 g = *reinterpret_cast<const float4*>(grad + o);
    const float c1 = consts[0], c2 = consts[1];
    const float inv_c1 = 1.f / c1, inv_c2 = 1.f / c2;
    const float* gp = &g.x;
    {
        float* mp = &pm.x; float* vp = &pv.x; float* xp = &pp.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) xp[r] = adam_element(mp[r], vp[r], xp[r], gp[r], b1, b2, lr, eps, inv_c1, inv_c2);
    }
    *reinterpret_cast<float4*>(m_mu + o) = pm;
    *reinterpret_cast<float4*>(v_mu + o) = pv;
    *reinterpret_cast<float4*>(mu + o) = pp;
    float n[4];
    if (!noisy_factors(tab, noise, o, n)) return;
    ISDQN_BOUNDS_CHECK(sigma + o, 16, 42);
    ISDQN_BOUNDS_CHECK(m_sigma + o, 16, 42);
    ISDQN_BOUNDS_CHECK(v_sigma + o, 16, 42);
    float4 sm = *reinterpret_cast<const float4*>(m_sigma + o);
    float4 sv = *reinterpret_cast<const float4*>(v_sigma + o);
    float4 sp = *reinterpret_cast<const float4*>(sigma + o);
    {
        float* mp = &sm.x; float* vp = &sv.x; float* xp = &sp.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) xp[r] = adam_element(mp[r], vp[r], xp[r], gp[r] * n[r], b1, b2, lr, eps, inv_c1, inv_c2);
    }
    *reinterpret_cast<float4*>(m_sigma + o) = sm;
    *reinterpret_cast<float4*>(v_sigma + o) = sv;
    *reinterpret_cast<float4*>(sigma + o) = sp;
}
