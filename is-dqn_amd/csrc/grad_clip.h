// Clipping of the gradient by its global norm in front of Adam (include/isdqn_hip.h, isdqn_net_config::max_grad_norm holds THE
// definition; optax.clip_by_global_norm chained with optax.adam).
// Included by net_kernels.hip inside namespace isdqn, behind AdamTable and the slab reduction adam_kernel uses.
//   n     = sqrt(sum g^2) over every element of every entry of the step's optimizer lists, g the reduced gradient
//   scale = 1 if n < c or n == 0, else c / n
// Launches between the backward and Adam, ordered by kernel boundaries alone (no grid barrier, no atomics, no arrival counter:
// DESIGN.md section 6 measured those slower than a boundary here):
//   grad_reduce_sq_kernel       the entries with several slabs: adam_kernel's grid and adam_kernel's slab reduction (adam_slab_lane_sum /
//                               adam_slab_combine: the same bits).  Every workgroup owns 16 float4 positions of one tensor: it writes
//                               their reduced gradient back over slab 0 -- nobody else reads or writes those positions -- so that Adam
//                               reads one slab instead of all of them again, and one float64 sum of their squares to
//                               "grad_clip_partials".
//   grad_flat_sq_kernel         the entries whose one slab already is the reduced gradient (a Dense kernel that would have been fused
//                               into Adam: 4 M elements at the headline shape): one float4 per thread, 1024 elements per workgroup.
//                               adam_kernel's grid keeps 16 of 256 lanes busy at one slab -- 62 k workgroups for Dense_0, measured
//                               ~100 us per pass over it (docs/NOTEBOOK.md) -- so these entries get a grid of their own.
//   grad_clip_finalize_kernel   one workgroup: the partials of both in float64 (strided per thread, eight loads in flight, then a fixed
//                               tree through LDS), norm, scale and the two accumulators -> "grad_clip".
//   adam_flat_kernel            Adam over every entry at its slab 0, one float4 per thread, the gradient multiplied by the scale.  It
//                               forms 0 + slab 0 through adam_slab_lane_sum, as adam_kernel does at one slab: grad_out keeps its bits.
// An fp32 square is exact in float64 (24 x 24 bits), so the only roundings are those of the float64 additions and the final fp32 store.
#pragma once

// Dueling heads: the head kernel [R rows][in_p] at w_off whose structural zeros (dueling.h: columns [F2, F) of a value row, [0, F2)
// of an advantage row) leave the reduced gradient -- and with it the norm -- here.  w_off = -1: none
struct GradClipMask {
    int64_t w_off;
    int in_p, R, A, w, F2, F;
};

// the four elements at offset i of entry `en`, structural zeros of the dueling head kernel zeroed (in_p is a multiple of 8: they share a row)
__device__ __forceinline__ float4 grad_clip_live(const AdamEntry& en, const GradClipMask& dm, int64_t i, float4 g) {
    if (en.p_off != dm.w_off) return g;
    const int o = (int)(i / dm.in_p), col = (int)(i - (int64_t)o * dm.in_p);
    if (o >= dm.R) return g;
    const bool value_row = (o / dm.w) % (dm.A + 1) == dm.A;
    float* gp = &g.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = col + r;
        const bool structural = value_row ? (k >= dm.F2 && k < dm.F) : k < dm.F2;
        gp[r] = structural ? 0.f : gp[r];
    }
    return g;
}
__device__ __forceinline__ double grad_clip_sq(const float4& g) {
    return (((double)g.x * (double)g.x + (double)g.y * (double)g.y) + (double)g.z * (double)g.z) + (double)g.w * (double)g.w;
}

__global__ __launch_bounds__(256) void grad_reduce_sq_kernel(const AdamTable tab, const GradClipMask dm, double* __restrict__ partials) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ float4 s_g[16][16];
    __shared__ double s_q[16];
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].block_start) ++e;
    const AdamEntry en = tab.e[e];
    const int pos = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t i = ((int64_t)(blockIdx.x - en.block_start) * 16 + pos) * 4;
    const bool on = i < en.size;
    float4 g = float4{0.f, 0.f, 0.f, 0.f};
    if (on) {
        ISDQN_BOUNDS_CHECK(en.g + i, 16, 38);
        ISDQN_BOUNDS_CHECK(en.g + (int64_t)(en.n_slabs - 1) * en.slab_stride + i, 16, 38);
        g = adam_slab_lane_sum(en, i, sl);
    }
    s_g[sl][pos] = g;
    __syncthreads();  // (every slab load of this workgroup's positions is done: slab 0 may be overwritten below)
    if (sl == 0) {
        double q = 0.0;
        if (on) {
            g = grad_clip_live(en, dm, i, adam_slab_combine(s_g, pos));
            *reinterpret_cast<float4*>(const_cast<float*>(en.g) + i) = g;
            q = grad_clip_sq(g);
        }
        s_q[pos] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_q[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) s += s_q[k];
        partials[blockIdx.x] = s;
    }
}

// Single-slab entries: thread t of workgroup b owns the float4 at element (b * 256 + t) * 4 of its entry.  The masked head kernel is the
// only thing written back.  The workgroup's 256 float64 squares go through a fixed LDS tree
constexpr int GC_FLAT_THREADS = 256, GC_FLAT_ELEMS = 4 * GC_FLAT_THREADS;
__global__ __launch_bounds__(GC_FLAT_THREADS) void grad_flat_sq_kernel(const AdamTable tab, const GradClipMask dm, double* __restrict__ partials) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ double s_q[GC_FLAT_THREADS];
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].block_start) ++e;
    const AdamEntry en = tab.e[e];
    const int tid = threadIdx.x;
    const int64_t i = ((int64_t)(blockIdx.x - en.block_start) * GC_FLAT_THREADS + tid) * 4;
    double q = 0.0;
    if (i < en.size) {
        ISDQN_BOUNDS_CHECK(en.g + i, 16, 38);
        float4 g = adam_slab_lane_sum(en, i, 0);
        if (en.p_off == dm.w_off) {
            g = grad_clip_live(en, dm, i, g);
            *reinterpret_cast<float4*>(const_cast<float*>(en.g) + i) = g;
        }
        q = grad_clip_sq(g);
    }
    s_q[tid] = q;
    __syncthreads();
    for (int off = GC_FLAT_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) s_q[tid] += s_q[tid + off];
        __syncthreads();
    }
    if (tid == 0) partials[blockIdx.x] = s_q[0];
}

// Adam behind the norm: every entry holds its reduced gradient in slab 0 (n_slabs = 1).  adam_kernel's element update on
// fl32(g * *scale) -- "grad_clip"[1] --; grad_out keeps the unscaled gradient
__global__ __launch_bounds__(GC_FLAT_THREADS) void adam_flat_kernel(const AdamTable tab, float* __restrict__ p, float* __restrict__ m,
                                                                   float* __restrict__ v, const float* __restrict__ consts, float lr, float b1,
                                                                   float b2, float eps, float* __restrict__ grad_out, float* __restrict__ mirror,
                                                                   int update, const float* __restrict__ scale) {
    ISDQN_EMPTY_KERNEL_RETURN
    int e = 0;
    while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].block_start) ++e;
    const AdamEntry en = tab.e[e];
    const int64_t i = ((int64_t)(blockIdx.x - en.block_start) * GC_FLAT_THREADS + threadIdx.x) * 4;
    if (i >= en.size) return;
    const int64_t o = en.p_off + i;
    float4 pm = float4{0.f, 0.f, 0.f, 0.f}, pv = pm, pp = pm;
    if (update) {  // (requested in front of the gradient, as adam_kernel does)
        pm = *reinterpret_cast<const float4*>(m + o);
        pv = *reinterpret_cast<const float4*>(v + o);
        pp = *reinterpret_cast<const float4*>(p + o);
    }
    float4 g = adam_slab_lane_sum(en, i, 0);
    if (grad_out != nullptr) *reinterpret_cast<float4*>(grad_out + o) = g;
    if (!update) return;  // gradient only (isdqn_net_grad_on_batch)
    const float c1 = consts[0], c2 = consts[1], sc = *scale;
    const float inv_c1 = 1.f / c1, inv_c2 = 1.f / c2;
    float* gp = &g.x; float* mp = &pm.x; float* vp = &pv.x; float* xp = &pp.x;
#pragma unroll
    for (int r = 0; r < 4; ++r) gp[r] = adam_element(mp[r], vp[r], xp[r], gp[r] * sc, b1, b2, lr, eps, inv_c1, inv_c2);  // (g: the new parameters)
    if (en.wd != 0.f) {  // (wave-uniform: one tensor per workgroup)
#pragma unroll
        for (int r = 0; r < 4; ++r) gp[r] = adamw_decay(gp[r], xp[r], lr, en.wd);
    }
    pp = g;
    *reinterpret_cast<float4*>(m + o) = pm;
    *reinterpret_cast<float4*>(v + o) = pv;
    *reinterpret_cast<float4*>(p + o) = pp;
    s8_store_quad(mirror, (int)o, pp.x, pp.y, pp.z, pp.w);  // S8 mirror of the updated parameters, as adam_kernel leaves it
}

constexpr int GC_FIN_THREADS = 1024;
// gc: "grad_clip" [4].  `update` = 0 (a gradient-only pass): the accumulators [2], [3] stay
__global__ __launch_bounds__(GC_FIN_THREADS) void grad_clip_finalize_kernel(const double* __restrict__ partials, int n, float max_norm,
                                                                            float* __restrict__ gc, int update) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ double s_a[GC_FIN_THREADS];
    const int tid = threadIdx.x;
    double a = 0.0;
    int k = tid;
    if (tid < n) {
        ISDQN_BOUNDS_CHECK(partials + tid, 8, 39);
        ISDQN_BOUNDS_CHECK(partials + tid + (n - 1 - tid) / GC_FIN_THREADS * GC_FIN_THREADS, 8, 39);
    }
    for (; k + 7 * GC_FIN_THREADS < n; k += 8 * GC_FIN_THREADS) {
        double h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = partials[k + u * GC_FIN_THREADS];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += h[u];
    }
    for (; k < n; k += GC_FIN_THREADS) a += partials[k];
    s_a[tid] = a;
    __syncthreads();
    for (int off = GC_FIN_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) s_a[tid] += s_a[tid + off];
        __syncthreads();
    }
    if (tid != 0) return;
    const double nrm = sqrt(s_a[0]), c = (double)max_norm;
    const double scale = (nrm < c || nrm == 0.0) ? 1.0 : c / nrm;
    const float nf = (float)nrm, sf = (float)scale;
    gc[0] = nf;
    gc[1] = sf;
    if (update) {
        gc[2] += nf;
        gc[3] += sf < 1.f ? 1.f : 0.f;  // (the stored factor: what Adam's gradients were multiplied by)
    }
}
