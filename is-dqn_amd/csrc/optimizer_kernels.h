// loss_finalize_kernel, and the Adam table with adam_kernel and the slab reduction grad_clip.h shares.  Included by net_kernels.hip
// inside namespace isdqn, behind head_chain.h and in front of grad_clip.h.
#pragma once
// losses[k] = mean_b td (isdqn.py:103), optional running sum (update_online_params' cumulated_losses,
// isdqn.py:62, kept on the device), head-bias gradient, Adam step counter and bias corrections.
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ loss_part,
                                                            const float* __restrict__ dbh_part, int n_blk, int B, int K,
                                                            int nha_p, float* __restrict__ losses,
                                                            float* __restrict__ loss_accum, float* __restrict__ dbh,
                                                            int* adam_count, float b1, float b2,
                                                            float* __restrict__ adam_consts) {
    ISDQN_EMPTY_KERNEL_RETURN
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    // One workgroup per 16 outputs (blocks [0, ceil(K/16)): losses, the rest: head-bias columns).  16 lanes share one
    // output: strided partial sums (eight loads in flight, added in index order), then a fixed shuffle tree.
    const int nkb = (K + 15) / 16;
    const bool is_loss = (int)blockIdx.x < nkb;
    const int col = (is_loss ? (int)blockIdx.x : (int)blockIdx.x - nkb) * 16 + grp;
    const int ncol = is_loss ? K : nha_p;
    const float* src = is_loss ? loss_part : dbh_part;
    if (!is_loss && dbh == nullptr) return;
    float s = 0.f;
    if (col < ncol)
        for (int i0 = sub; i0 < n_blk; i0 += 8 * 16) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 16;
                v[u] = i < n_blk ? src[(int64_t)i * ncol + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (col < ncol && sub == 0) {
        if (is_loss) {
            s /= (float)B;
            losses[col] = s;
            if (loss_accum != nullptr) loss_accum[col] += s;
        } else {
            dbh[col] = s;
        }
    }
    if (blockIdx.x != 0) return;
    if (adam_count != nullptr && tid == 0) {
        int t = *adam_count + 1;
        *adam_count = t;
        adam_consts[0] = (float)(1.0 - pow_int((double)b1, t));
        adam_consts[1] = (float)(1.0 - pow_int((double)b2, t));
    }
}

// Adam (optax.adam, isdqn.py:46, 85-86) over the flat parameter buffer; the gradient of every
// tensor is the sum of its slabs (split-K partials / LayerNorm-backward partials), so gradients
// are reduced here and never stored in reduced form.
struct AdamEntry {
    int64_t p_off, size, slab_stride;
    const float* g;
    int n_slabs, block_start;
    float wd;  // decoupled weight decay of the tensor (include/isdqn_hip.h, isdqn_batch_decay); 0: none
};
constexpr int ADAM_MAX_ENTRIES = 4 * MAX_LAYERS;
struct AdamTable {
    AdamEntry e[ADAM_MAX_ENTRIES];
    int n, total_blocks;
};
// The slab reduction of one float4 position, shared by adam_kernel and grad_reduce_sq_kernel (grad_clip.h) so that both form the
// reduced gradient in the same order: slab lane `sl` of 16 adds up the slabs sl, sl + 16, ... (adam_slab_lane_sum), the 16 lane sums
// go through LDS and are added in ascending lane order (adam_slab_combine).
__device__ __forceinline__ float4 adam_slab_lane_sum(const AdamEntry& en, int64_t i, int sl) {
    float4 g = float4{0.f, 0.f, 0.f, 0.f};
    int s = sl;
    // (eight slabs in flight per thread first: the first layer's weight gradient leaves one slab per image at B = 256 -- 16 dependent
    // loads per thread in batches of four were four round trips at the tail of the side queue)
#if !defined(ISDQN_ADAM_4_IN_FLIGHT)
    for (; s + 7 * 16 < en.n_slabs; s += 8 * 16) {
        float4 h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = *reinterpret_cast<const float4*>(en.g + (int64_t)(s + u * 16) * en.slab_stride + i);
#pragma unroll
        for (int u = 0; u < 8; ++u) { g.x += h[u].x; g.y += h[u].y; g.z += h[u].z; g.w += h[u].w; }
    }
#endif
    for (; s + 3 * 16 < en.n_slabs; s += 4 * 16) {
        float4 h[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) h[u] = *reinterpret_cast<const float4*>(en.g + (int64_t)(s + u * 16) * en.slab_stride + i);
#pragma unroll
        for (int u = 0; u < 4; ++u) { g.x += h[u].x; g.y += h[u].y; g.z += h[u].z; g.w += h[u].w; }
    }
    for (; s < en.n_slabs; s += 16) {
        float4 h = *reinterpret_cast<const float4*>(en.g + (int64_t)s * en.slab_stride + i);
        g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    return g;
}
__device__ __forceinline__ float4 adam_slab_combine(const float4 (*s_g)[16], int pos) {
    float4 g = s_g[0][pos];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const float4 h = s_g[k][pos];
        g.x += h.x; g.y += h.y; g.z += h.z; g.w += h.w;
    }
    return g;
}
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable tab, float* __restrict__ p, float* __restrict__ m,
                                                   float* __restrict__ v, const float* __restrict__ consts, float lr,
                                                   float b1, float b2, float eps, float* __restrict__ grad_out,
                                                   float* __restrict__ mirror, int update) {
    ISDQN_EMPTY_KERNEL_RETURN
    // A workgroup covers 16 float4 positions; 16 "slab lanes" per position split the slab reduction (up to a
    // few hundred split-K / per-image-group slabs for the conv kernels) and combine through LDS in a fixed
    // order, so the reduction is deterministic and never a long serial chain of dependent loads.
    __shared__ float4 s_g[16][16];
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].block_start) ++e;
    const AdamEntry en = tab.e[e];
    const float c1 = consts[0], c2 = consts[1];  // 1 - b1^t, 1 - b2^t (loss_finalize_kernel)
    const int pos = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t i = ((int64_t)(blockIdx.x - en.block_start) * 16 + pos) * 4;
    const bool on = i < en.size;
    float4 g = float4{0.f, 0.f, 0.f, 0.f};
    // the updating lanes request their moments and parameters now: they arrive under the slab reduction
    const int64_t o = en.p_off + i;
    float4 pm = g, pv = g, pp = g;
    if (on && sl == 0) {
        pm = *reinterpret_cast<const float4*>(m + o);
        pv = *reinterpret_cast<const float4*>(v + o);
        pp = *reinterpret_cast<const float4*>(p + o);
    }
    if (on) g = adam_slab_lane_sum(en, i, sl);
    s_g[sl][pos] = g;
    __syncthreads();
    if (sl != 0 || !on) return;
    g = adam_slab_combine(s_g, pos);
    if (grad_out != nullptr) *reinterpret_cast<float4*>(grad_out + o) = g;
    if (!update) return;  // gradient only (isdqn_net_grad_on_batch)
    float* gp = &g.x; float* mp = &pm.x; float* vp = &pv.x; float* xp = &pp.x;
    const float inv_c1 = 1.f / c1, inv_c2 = 1.f / c2;
#pragma unroll
    for (int r = 0; r < 4; ++r) gp[r] = adam_element(mp[r], vp[r], xp[r], gp[r], b1, b2, lr, eps, inv_c1, inv_c2);  // (g: the new parameters)
    if (en.wd != 0.f) {  // (wave-uniform: one tensor per workgroup)
#pragma unroll
        for (int r = 0; r < 4; ++r) gp[r] = adamw_decay(gp[r], xp[r], lr, en.wd);
    }
    pp = g;
    *reinterpret_cast<float4*>(m + o) = pm;
    *reinterpret_cast<float4*>(v + o) = pv;
    *reinterpret_cast<float4*>(p + o) = pp;
    s8_store_quad(mirror, (int)o, pp.x, pp.y, pp.z, pp.w);  // S8 mirror of the updated parameters (read by the next step's MFMA stages)
}
