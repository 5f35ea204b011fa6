// Normalize-and-Project on gfx950 (Lyle, Zheng, Khetarpal, Martens, van Hasselt, Pascanu, Dabney, NeurIPS 2024): after every optimizer
// update each conv and Dense kernel but the last Dense's is scaled back to the Frobenius norm it had at initialisation.  THE definition is
// include/isdqn_hip.h, isdqn_net_project_layout / _norms / _apply; the reference has no counterpart.  A translation unit of its own
// (build.PROJECT_SOURCES): the pinned code objects keep their kernels and their order.  Built beside the plan: no field of
// isdqn_net_config, no workspace region, nothing of build_plan; the entry points (net_kernels.hip, which holds the plan) fill ProjectArgs
// and call the launchers below.  Tensors, real-element predicate and chunks are pruning's (prune.h): workgroup = one chunk of PRUNE_CHUNK
// floats of one tensor, 256 threads, four 16-byte positions per thread, all four loads issued in front of the first use.
//   project_sumsq_kernel       the chunk's sum of (double)w * (double)w over its real elements (the squares are exact in float64): per
//                      thread in position order, a 6-step xor butterfly over the wave (a + b == b + a: every lane ends with the same
//                      bits), the four wave sums through LDS as (w0 + w1) + (w2 + w3).  One double per chunk to the scratch.
//   project_scale_kernel<MIRROR>  same grid.  Every workgroup adds up its tensor's chunk sums -- thread t takes chunks t, t + 256, ... in
//                      ascending order, then the same butterfly and LDS sum -- so that every workgroup of a tensor holds S_i, and with it
//                      s_i = (float)(rho_i / sqrt(S_i)), in the same bits: a function of the scratch alone, no atomic, no arrival order.
//                      Chunk 0 stores norms[i] and scales[i].  Then w * s_i: a float4 and the S8 mirror's half-group where all four
//                      lanes are real, single elements otherwise, nothing where none is or where s_i == 1.0f.
//   project_norms_kernel       one workgroup per tensor: the sum of the chunk sums in that same order, norms[i] alone.
// The kernel boundary between the two launches is the only synchronisation.  No atomics of any kind.
// ISDQN_BOUNDS site: 58 -- every load and store, the mirror's, the scratch's and the three small vectors' included -- against this
// object's own table (gemm_core.h keeps one per translation unit): isdqn_debug_project_bounds_set / _get below.
#include "project.h"

#include <string.h>

#include "gemm_core.h"  // s8_store_quad / s8_store_elem, f32x4, ISDQN_BOUNDS_CHECK and its table

namespace isdqn {

constexpr int PROJECT_THREADS = 256;
constexpr int PROJECT_WAVES = PROJECT_THREADS / 64;
constexpr int PROJECT_QUADS = PRUNE_CHUNK / 4 / PROJECT_THREADS;  // 16-byte positions per thread
static_assert(PROJECT_WAVES == 4 && PROJECT_QUADS * 4 * PROJECT_THREADS == PRUNE_CHUNK, "the LDS sum below is written for four waves");

__device__ __forceinline__ int project_tensor_of_chunk(const PruneTable& tab, int block) {
    int ti = 0;
    while (ti + 1 < tab.n && block >= tab.t[ti + 1].first_chunk) ++ti;
    return ti;
}

// bit j: float i + j of the buffer is a real element of t.  (Offsets and sizes are multiples of 8: a 16-byte position lies inside a
// tensor or outside it.)
__device__ __forceinline__ uint32_t project_real4(const PruneTensor& t, int64_t i) {
    const int64_t e64 = i - t.offset;
    if (e64 < 0 || e64 >= t.size) return 0u;
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t row, col, grp, lane;
        t.d_row.divmod((uint32_t)e64 + j, row, col);
        t.d_per.divmod(col, grp, lane);
        m |= (row < (uint32_t)t.rows_real && lane < (uint32_t)t.real_per) ? 1u << j : 0u;
    }
    return m;
}

// The chunk's 16-byte positions of thread `tid`: real[r] as project_real4, v[r] loaded wherever the position lies inside the tensor
// (padding lanes included: what they hold is never used), from the tensor's first position otherwise -- no branch around a load.
__device__ __forceinline__ void project_load(const float* p, const PruneTensor& t, int64_t i0, int tid, f32x4 (&v)[PROJECT_QUADS],
                                             uint32_t (&real)[PROJECT_QUADS]) {
#pragma unroll
    for (int r = 0; r < PROJECT_QUADS; ++r) {
        const int64_t i = i0 + 4 * (r * PROJECT_THREADS + tid);
        const bool inside = i >= t.offset && i < t.offset + t.size;
        const float* src = p + (inside ? i : t.offset);
        ISDQN_BOUNDS_CHECK(src, 16, 58);
        v[r] = *reinterpret_cast<const f32x4*>(src);
    }
#pragma unroll
    for (int r = 0; r < PROJECT_QUADS; ++r) real[r] = project_real4(t, i0 + 4 * (r * PROJECT_THREADS + tid));
}

// the sum of one value per thread, in every thread, in a fixed order
__device__ __forceinline__ double project_block_sum(double x, double* s_wave, int tid) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((tid & 63) == 0) s_wave[tid >> 6] = x;
    __syncthreads();
    const double s = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
    return s;
}

// S_i from the chunk sums of tensor t, the same bits in every workgroup that asks
__device__ __forceinline__ double project_tensor_sumsq(const double* scratch, const PruneTensor& t, double* s_wave, int tid) {
    double acc = 0.0;
    for (int c = tid; c < t.n_chunks; c += PROJECT_THREADS) {
        ISDQN_BOUNDS_CHECK(scratch + t.first_chunk + c, 8, 58);
        acc += scratch[t.first_chunk + c];
    }
    return project_block_sum(acc, s_wave, tid);
}

__global__ __launch_bounds__(PROJECT_THREADS) void project_sumsq_kernel(const ProjectArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ double s_wave[PROJECT_WAVES];
    const int tid = (int)threadIdx.x;
    const PruneTensor t = a.tab.t[project_tensor_of_chunk(a.tab, (int)blockIdx.x)];
    const int chunk = (int)blockIdx.x - t.first_chunk;
    if (chunk >= t.n_chunks) return;
    f32x4 v[PROJECT_QUADS];
    uint32_t real[PROJECT_QUADS];
    project_load(a.p, t, (t.offset & ~(int64_t)31) + (int64_t)chunk * PRUNE_CHUNK, tid, v, real);
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < PROJECT_QUADS; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = ((real[r] >> j) & 1u) ? (double)v[r][j] : 0.0;
            acc += x * x;
        }
    const double sum = project_block_sum(acc, s_wave, tid);
    if (tid == 0) {
        ISDQN_BOUNDS_CHECK(a.scratch + blockIdx.x, 8, 58);
        a.scratch[blockIdx.x] = sum;
    }
}

template <bool MIRROR>
__global__ __launch_bounds__(PROJECT_THREADS) void project_scale_kernel(const ProjectArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ double s_wave[PROJECT_WAVES];
    const int tid = (int)threadIdx.x;
    const int ti = project_tensor_of_chunk(a.tab, (int)blockIdx.x);
    const PruneTensor t = a.tab.t[ti];
    const int chunk = (int)blockIdx.x - t.first_chunk;
    if (chunk >= t.n_chunks) return;
    const int64_t i0 = (t.offset & ~(int64_t)31) + (int64_t)chunk * PRUNE_CHUNK;
    f32x4 v[PROJECT_QUADS];
    uint32_t real[PROJECT_QUADS];
    project_load(a.p, t, i0, tid, v, real);  // (in flight under the sum of the chunk sums)

    const double S = project_tensor_sumsq(a.scratch, t, s_wave, tid);
    ISDQN_BOUNDS_CHECK(a.target + ti, 8, 58);
    const double rho = a.target[ti];
    const double inf = __builtin_huge_val();
    const double norm = sqrt(S);
    const bool project = S > 0.0 && S < inf && rho > 0.0 && rho < inf;  // (a NaN fails every comparison)
    const float s = project ? (float)(rho / norm) : 1.0f;
    if (chunk == 0 && tid == 0) {
        ISDQN_BOUNDS_CHECK(a.norms + ti, 8, 58);
        ISDQN_BOUNDS_CHECK(a.scales + ti, 4, 58);
        a.norms[ti] = norm;
        a.scales[ti] = s;
    }
    if (s == 1.0f) return;  // (w * 1.0f is w: master and mirror already hold what would be stored)

    float* p = a.p;
    float* mirror = a.mirror;
#pragma unroll
    for (int r = 0; r < PROJECT_QUADS; ++r) {
        if (real[r] == 0u) continue;
        const int64_t i = i0 + 4 * (r * PROJECT_THREADS + tid);
        float* group = mirror + (i & ~(int64_t)7);  // (the 32-byte group of the mirror this position is one half of)
        const int c0 = (int)(i & 4);
        const f32x4 w = {v[r][0] * s, v[r][1] * s, v[r][2] * s, v[r][3] * s};
        if (real[r] == 15u) {
            ISDQN_BOUNDS_CHECK(p + i, 16, 58);
            *reinterpret_cast<f32x4*>(p + i) = w;
            if constexpr (MIRROR) {
                ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(group) + c0 * 2, 8, 58);
                ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(group) + c0 * 2 + 16, 8, 58);
                s8_store_quad(group, c0, w[0], w[1], w[2], w[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((real[r] >> j) & 1u) {
                    ISDQN_BOUNDS_CHECK(p + i + j, 4, 58);
                    p[i + j] = w[j];
                    if constexpr (MIRROR) {
                        ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(group) + c0 + j, 2, 58);
                        ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(group) + c0 + j + 8, 2, 58);
                        s8_store_elem(group, c0 + j, w[j]);
                    }
                }
        }
    }
}

__global__ __launch_bounds__(PROJECT_THREADS) void project_norms_kernel(const ProjectArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ double s_wave[PROJECT_WAVES];
    const int tid = (int)threadIdx.x, ti = (int)blockIdx.x;
    if (ti >= a.tab.n) return;
    const double S = project_tensor_sumsq(a.scratch, a.tab.t[ti], s_wave, tid);
    if (tid == 0) {
        ISDQN_BOUNDS_CHECK(a.norms + ti, 8, 58);
        a.norms[ti] = sqrt(S);
    }
}

static int project_check(const ProjectArgs& a, bool apply) {
    ISDQN_REQUIRE(a.p != nullptr && a.norms != nullptr && a.scratch != nullptr, ISDQN_ERR_ARG, "projection: null pointer");
    ISDQN_REQUIRE(!apply || (a.target != nullptr && a.scales != nullptr), ISDQN_ERR_ARG, "projection: null pointer");
    ISDQN_REQUIRE(((uintptr_t)a.p & 15) == 0, ISDQN_ERR_ARG, "projection: params must be 16-byte aligned");
    ISDQN_REQUIRE((((uintptr_t)a.norms | (uintptr_t)a.scratch | (uintptr_t)a.target) & 7) == 0, ISDQN_ERR_ARG,
                  "projection: target_norms, norms and scratch hold doubles and must be 8-byte aligned");
    ISDQN_REQUIRE(((uintptr_t)a.scales & 3) == 0, ISDQN_ERR_ARG, "projection: scales must be 4-byte aligned");
    ISDQN_REQUIRE(((uintptr_t)a.mirror & 31) == 0, ISDQN_ERR_ARG, "projection: the workspace's weight mirror must be 32-byte aligned");
    return ISDQN_OK;
}

static int sumsq_launch(const ProjectArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(project_sumsq_kernel, dim3((unsigned)a.tab.total_chunks), dim3(PROJECT_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_project_norms(const ProjectArgs& a, hipStream_t st) {
    if (int rc = project_check(a, false)) return rc;
    if (a.tab.total_chunks <= 0) return ISDQN_OK;
    if (int rc = sumsq_launch(a, st)) return rc;
    hipLaunchKernelGGL(project_norms_kernel, dim3((unsigned)a.tab.n), dim3(PROJECT_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_project_apply(const ProjectArgs& a, hipStream_t st) {
    if (int rc = project_check(a, true)) return rc;
    if (a.tab.total_chunks <= 0) return ISDQN_OK;
    if (int rc = sumsq_launch(a, st)) return rc;
    if (a.mirror != nullptr) hipLaunchKernelGGL(project_scale_kernel<true>, dim3((unsigned)a.tab.total_chunks), dim3(PROJECT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(project_scale_kernel<false>, dim3((unsigned)a.tab.total_chunks), dim3(PROJECT_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

}  // namespace isdqn

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build: the byte extents [lo[i], hi[i]) the projection kernels may touch, and the first access outside all
// of them (tests/test_gpu_nap_bounds.py); this object's own table, as prune_kernels.hip has one.
extern "C" int isdqn_debug_project_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_project_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif
