// Gradual magnitude pruning on gfx950 (Zhu & Gupta 2017; JaxPruner's GMP): per tensor the k smallest-magnitude real elements are marked
// in a bit mask, and the marked elements are set to +0.0 after every optimizer update.  THE definition is include/isdqn_hip.h,
// isdqn_net_prune_layout / _update / _apply; the reference has no counterpart.  A translation unit of its own (build.PRUNE_SOURCES): the
// four pinned code objects keep their kernels and their order.  Built beside the plan: no field of isdqn_net_config, no workspace region,
// nothing of build_plan; the entry points (net_kernels.hip, which holds the plan) fill PruneArgs and call the launchers below.
//   prune_select_kernel<PASS>  a radix select over the 32-bit key (0 = already pruned, else 1 + bits(|w|)), 8 bits per pass, most
//                      significant digit first, every tensor in one launch: workgroup = one chunk of PRUNE_CHUNK floats of one tensor.
//                      Every workgroup first re-derives the digits chosen so far from the finished histograms (a 256-wide scan in LDS per
//                      finished pass: no launch, no host read in between).
//                        PASS 0 .. 3  histogram of digit PASS over the real elements whose higher digits equal the prefix: counted in LDS
//                                     (1 KB, integer atomics), then added to the tensor's global histogram with integer atomics -- sums of
//                                     integers, the same in every order.
//                        PASS 4       the chunk's count of keys equal to the threshold key T: one plain store per workgroup.
//                        PASS 5       mask bits: key < T is pruned, key == T is pruned iff its rank by index among the equal keys -- the
//                                     tie counts of the chunks in front, then an index-ordered count inside the chunk (wave ballots, four
//                                     wave totals through LDS) -- is below what is left of k.  A wave owns two whole mask words per round
//                                     and changes the bits of real elements alone (atomicAnd / atomicOr: a word at the edge of a tensor may
//                                     be shared with its neighbour's workgroup; the bits are disjoint).
//                      No float atomics, no float arithmetic: the result is a pure function of (params, old mask, k).
//   prune_apply_kernel<MIRROR> the per-step pass: a lane owns one 16-byte position of [span_lo, span_hi), reads its four mask bits and
//                      stores zeros -- a float4 (and the half-group of the S8 mirror) where all four are pruned, single elements
//                      otherwise, nothing where all are kept.  No parameter is loaded.  The grid is sized by positions, capped, and strides.
// ISDQN_BOUNDS site: 52 -- every load, store and atomic, the mirror's included -- against this object's own table (gemm_core.h keeps one
// per translation unit): isdqn_debug_prune_bounds_set / _get below.
#include "prune.h"

#include <string.h>

#include <algorithm>

#include "gemm_core.h"  // s8_store_quad / s8_store_elem, ISDQN_BOUNDS_CHECK and its table

namespace isdqn {

constexpr int PRUNE_THREADS = 256;
constexpr int PRUNE_WAVES = PRUNE_THREADS / 64;
constexpr int PRUNE_ROUNDS = PRUNE_CHUNK / PRUNE_THREADS;
constexpr int PRUNE_APPLY_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups: the rest of a launch is reached by the stride

// the element at float i of the buffer, as the selection sees it
struct PruneElem {
    bool real;
    uint32_t key;
};
__device__ __forceinline__ PruneElem prune_elem(const PruneArgs& a, const PruneTensor& t, int64_t i) {
    PruneElem r{false, 0u};
    const int64_t e64 = i - t.offset;
    if (e64 < 0 || e64 >= t.size) return r;
    const uint32_t e = (uint32_t)e64;
    uint32_t row, col, grp, lane;
    t.d_row.divmod(e, row, col);
    t.d_per.divmod(col, grp, lane);
    if (row >= (uint32_t)t.rows_real || lane >= (uint32_t)t.real_per) return r;
    r.real = true;
    ISDQN_BOUNDS_CHECK(a.p + i, 4, 52);
    ISDQN_BOUNDS_CHECK(a.mask + (i >> 5), 4, 52);
    const uint32_t w = reinterpret_cast<const uint32_t*>(a.p)[i];
    const uint32_t m = a.mask[i >> 5];
    r.key = ((m >> (i & 31)) & 1u) ? 1u + (w & 0x7FFFFFFFu) : 0u;
    return r;
}

template <int PASS>
__global__ __launch_bounds__(PRUNE_THREADS) void prune_select_kernel(const PruneArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t s_sel[2];
    __shared__ uint32_t s_wave[PRUNE_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ti = 0;
    while (ti + 1 < a.tab.n && (int)blockIdx.x >= a.tab.t[ti + 1].first_chunk) ++ti;
    const PruneTensor t = a.tab.t[ti];
    const int chunk = (int)blockIdx.x - t.first_chunk;
    if (chunk >= t.n_chunks) return;
    uint32_t* hist = a.scratch + t.scratch_off;
    uint32_t* tie = hist + PRUNE_HIST_WORDS;
    const bool any = t.k > 0;  // (the same for the whole workgroup)
    if (PASS < 5 && !any) return;

    // the digits the finished passes chose, and what is left of k below them
    uint32_t prefix = 0, k_rem = (uint32_t)t.k;
    constexpr int DONE = PASS < 4 ? PASS : 4;
    if (any) {
        for (int q = 0; q < DONE; ++q) {
            ISDQN_BOUNDS_CHECK(hist + q * 256 + tid, 4, 52);
            const uint32_t c = hist[q * 256 + tid];
            s_scan[tid] = c;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const uint32_t v = tid >= d ? s_scan[tid - d] : 0u;
                __syncthreads();
                s_scan[tid] += v;
                __syncthreads();
            }
            const uint32_t incl = s_scan[tid], excl = incl - c;
            if (excl < k_rem && k_rem <= incl) {  // exactly one digit: 1 <= k_rem <= the histogram's total
                s_sel[0] = (uint32_t)tid;
                s_sel[1] = k_rem - excl;
            }
            __syncthreads();
            prefix = (prefix << 8) | s_sel[0];
            k_rem = s_sel[1];
            __syncthreads();
        }
    }

    const int64_t i0 = (t.offset & ~(int64_t)31) + (int64_t)chunk * PRUNE_CHUNK;
    if constexpr (PASS < 4) {
        s_hist[tid] = 0;
        __syncthreads();
        for (int r = 0; r < PRUNE_ROUNDS; ++r) {
            const PruneElem el = prune_elem(a, t, i0 + r * PRUNE_THREADS + tid);
            const bool match = PASS == 0 ? true : (el.key >> ((32 - 8 * PASS) & 31)) == prefix;
            if (el.real && match) atomicAdd(&s_hist[(el.key >> (24 - 8 * PASS)) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t c = s_hist[tid];
        if (c != 0) {
            ISDQN_BOUNDS_CHECK(hist + PASS * 256 + tid, 4, 52);
            atomicAdd(hist + PASS * 256 + tid, c);
        }
    } else if constexpr (PASS == 4) {
        if (tid == 0) s_sel[0] = 0;
        __syncthreads();
        uint32_t n = 0;
        for (int r = 0; r < PRUNE_ROUNDS; ++r) {
            const PruneElem el = prune_elem(a, t, i0 + r * PRUNE_THREADS + tid);
            n += (el.real && el.key == prefix) ? 1u : 0u;
        }
        if (n != 0) atomicAdd(&s_sel[0], n);
        __syncthreads();
        if (tid == 0) {
            ISDQN_BOUNDS_CHECK(tie + chunk, 4, 52);
            tie[chunk] = s_sel[0];
        }
    } else {
        // ties in the chunks in front of this one
        if (tid == 0) s_sel[0] = 0;
        __syncthreads();
        if (any) {
            uint32_t n = 0;
            for (int c = tid; c < chunk; c += PRUNE_THREADS) {
                ISDQN_BOUNDS_CHECK(tie + c, 4, 52);
                n += tie[c];
            }
            if (n != 0) atomicAdd(&s_sel[0], n);
        }
        __syncthreads();
        uint32_t run = s_sel[0];
        for (int r = 0; r < PRUNE_ROUNDS; ++r) {
            const int64_t i = i0 + r * PRUNE_THREADS + tid;
            const PruneElem el = prune_elem(a, t, i);
            const bool eq = any && el.real && el.key == prefix, lt = any && el.real && el.key < prefix;
            const unsigned long long b_eq = __ballot(eq);
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b_eq);
            __syncthreads();
            uint32_t before = run, total = 0;
#pragma unroll
            for (int w = 0; w < PRUNE_WAVES; ++w) {
                const uint32_t c = s_wave[w];
                before += w < wave ? c : 0u;
                total += c;
            }
            run += total;
            __syncthreads();
            const uint32_t rank = before + (uint32_t)__popcll(b_eq & ((1ull << lane) - 1ull));
            const bool pruned = lt || (eq && rank < k_rem);
            const unsigned long long b_real = __ballot(el.real), b_pruned = __ballot(el.real && pruned);
            if (lane == 0 || lane == 32) {
                const uint32_t rm = (uint32_t)(b_real >> lane), pm = (uint32_t)(b_pruned >> lane);
                if (rm != 0) {
                    uint32_t* word = a.mask + (i >> 5);
                    ISDQN_BOUNDS_CHECK(word, 4, 52);
                    if (pm != 0) atomicAnd(word, ~pm);
                    if ((rm & ~pm) != 0) atomicOr(word, rm & ~pm);
                }
            }
        }
    }
}

template <bool MIRROR>
__global__ __launch_bounds__(PRUNE_THREADS) void prune_apply_kernel(const PruneArgs a) {
    ISDQN_EMPTY_KERNEL_RETURN
    float* p = a.p;
    float* mirror = a.mirror;
    const int64_t q_hi = a.tab.span_hi >> 2;  // (the span's ends are multiples of 8 floats)
    const int64_t stride = (int64_t)gridDim.x * PRUNE_THREADS;
    for (int64_t q = (a.tab.span_lo >> 2) + (int64_t)blockIdx.x * PRUNE_THREADS + threadIdx.x; q < q_hi; q += stride) {
        const int64_t i = q << 2;
        ISDQN_BOUNDS_CHECK(a.mask + (i >> 5), 4, 52);
        const uint32_t kept = (a.mask[i >> 5] >> (i & 31)) & 15u;
        if (kept == 15u) continue;
        float* group = mirror + (i & ~(int64_t)7);  // (the 32-byte group of the mirror this position is one half of)
        const int c0 = (int)(i & 4);
        if (kept == 0u) {
            ISDQN_BOUNDS_CHECK(p + i, 16, 52);
            *reinterpret_cast<float4*>(p + i) = float4{0.f, 0.f, 0.f, 0.f};
            if constexpr (MIRROR) {
                ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(group) + c0 * 2, 8, 52);
                ISDQN_BOUNDS_CHECK(reinterpret_cast<char*>(group) + c0 * 2 + 16, 8, 52);
                s8_store_quad(group, c0, 0.f, 0.f, 0.f, 0.f);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((kept >> j) & 1u)) {
                    ISDQN_BOUNDS_CHECK(p + i + j, 4, 52);
                    p[i + j] = 0.f;
                    if constexpr (MIRROR) {
                        ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(group) + c0 + j, 2, 52);
                        ISDQN_BOUNDS_CHECK(reinterpret_cast<__bf16*>(group) + c0 + j + 8, 2, 52);
                        s8_store_elem(group, c0 + j, 0.f);
                    }
                }
        }
    }
}

int prune_table_finish(PruneTable& tab) {
    ISDQN_REQUIRE(tab.n >= 0 && tab.n <= PRUNE_MAX_TENSORS, ISDQN_ERR_SHAPE, "pruning: too many prunable tensors");
    int64_t chunks = 0, words = 0;
    tab.span_lo = tab.span_hi = 0;
    for (int i = 0; i < tab.n; ++i) {
        PruneTensor& t = tab.t[i];
        ISDQN_REQUIRE(t.offset >= 0 && t.offset % 8 == 0 && t.size > 0 && t.size % 8 == 0, ISDQN_ERR_SHAPE,
                      "pruning: a kernel is not laid out in groups of 8");
        ISDQN_REQUIRE(t.row_len >= 1 && t.period >= 1 && t.row_len % t.period == 0 && t.size % t.row_len == 0 && t.real_per >= 1 &&
                          t.real_per <= t.period && t.rows_real >= 1 && t.rows_real <= t.size / t.row_len,
                      ISDQN_ERR_SHAPE, "pruning: a kernel's rows do not tile its size");
        const int64_t n_real = (int64_t)t.rows_real * (t.row_len / t.period) * t.real_per;
        const int64_t first = t.offset & ~(int64_t)31;
        const int64_t n_chunks = (t.offset + t.size - first + PRUNE_CHUNK - 1) / PRUNE_CHUNK;
        ISDQN_REQUIRE(chunks + n_chunks < (1ll << 31) && n_real < (1ll << 31), ISDQN_ERR_SHAPE, "pruning: a kernel of 2^31 elements or more");
        t.n_real = (int32_t)n_real;
        t.first_chunk = (int32_t)chunks;
        t.n_chunks = (int32_t)n_chunks;
        t.pad_ = 0;
        t.scratch_off = words;
        t.d_row = FastDiv((uint32_t)t.row_len);
        t.d_per = FastDiv((uint32_t)t.period);
        chunks += n_chunks;
        words += PRUNE_HIST_WORDS + n_chunks;
        if (i == 0) tab.span_lo = t.offset;
        ISDQN_REQUIRE(t.offset >= tab.span_hi, ISDQN_ERR_SHAPE, "pruning: the kernels are not in layout order");
        tab.span_hi = t.offset + t.size;
    }
    tab.total_chunks = (int32_t)chunks;
    tab.hist_words = words;
    return ISDQN_OK;
}

static int prune_check(const PruneArgs& a) {
    ISDQN_REQUIRE(a.p != nullptr && a.mask != nullptr, ISDQN_ERR_ARG, "pruning: null pointer");
    ISDQN_REQUIRE(((uintptr_t)a.p & 15) == 0, ISDQN_ERR_ARG, "pruning: params must be 16-byte aligned");
    ISDQN_REQUIRE(((uintptr_t)a.mask & 3) == 0, ISDQN_ERR_ARG, "pruning: the mask must be 4-byte aligned");
    ISDQN_REQUIRE(((uintptr_t)a.mirror & 31) == 0, ISDQN_ERR_ARG, "pruning: the workspace's weight mirror must be 32-byte aligned");
    return ISDQN_OK;
}

static int apply_launch(const PruneArgs& a, hipStream_t st) {
    const int64_t n = (a.tab.span_hi - a.tab.span_lo) >> 2;
    if (n <= 0) return ISDQN_OK;
    const int64_t blocks = std::min<int64_t>((n + PRUNE_THREADS - 1) / PRUNE_THREADS, PRUNE_APPLY_MAX_BLOCKS);
    if (a.mirror != nullptr) hipLaunchKernelGGL(prune_apply_kernel<true>, dim3((unsigned)blocks), dim3(PRUNE_THREADS), 0, st, a);
    else hipLaunchKernelGGL(prune_apply_kernel<false>, dim3((unsigned)blocks), dim3(PRUNE_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_prune_apply(const PruneArgs& a, hipStream_t st) {
    if (int rc = prune_check(a)) return rc;
    return apply_launch(a, st);
}

template <int PASS>
static int select_launch(const PruneArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(prune_select_kernel<PASS>, dim3((unsigned)a.tab.total_chunks), dim3(PRUNE_THREADS), 0, st, a);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

int launch_prune_update(const PruneArgs& a, hipStream_t st) {
    if (int rc = prune_check(a)) return rc;
    ISDQN_REQUIRE(a.scratch != nullptr, ISDQN_ERR_ARG, "pruning: null pointer");
    ISDQN_REQUIRE(((uintptr_t)a.scratch & 3) == 0, ISDQN_ERR_ARG, "pruning: the scratch must be 4-byte aligned");
    for (int i = 0; i < a.tab.n; ++i)
        ISDQN_REQUIRE(a.tab.t[i].k >= 0 && a.tab.t[i].k <= a.tab.t[i].n_real, ISDQN_ERR_ARG,
                      "pruning: a pruned count must be in [0, the tensor's real element count]");
    if (a.tab.total_chunks <= 0) return ISDQN_OK;
    ISDQN_HIP_CHECK(hipMemsetAsync(a.scratch, 0, (size_t)a.tab.hist_words * 4, st));
    int rc;
    if ((rc = select_launch<0>(a, st))) return rc;
    if ((rc = select_launch<1>(a, st))) return rc;
    if ((rc = select_launch<2>(a, st))) return rc;
    if ((rc = select_launch<3>(a, st))) return rc;
    if ((rc = select_launch<4>(a, st))) return rc;
    if ((rc = select_launch<5>(a, st))) return rc;
    return apply_launch(a, st);
}

}  // namespace isdqn

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build: the byte extents [lo[i], hi[i]) the pruning kernels may touch, and the first access outside all of
// them (tests/test_gpu_prune_bounds.py); this object's own table, as soft_shift_kernels.hip has one.
extern "C" int isdqn_debug_prune_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_prune_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif
