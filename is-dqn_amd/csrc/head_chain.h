// head_chain_kernel with its parameters and its LDS budget.  Included by net_kernels.hip inside namespace isdqn, behind row_kernels.h
// (td_loss / td_dloss / argmax_first); launched by learn_step.h: launch_head_chain.
#pragma once
// ---------------------------------------------------------------------------------------------
// Head chain (learn path).  Everything between the last hidden activation and the gradient w.r.t. that
// layer's pre-activation is per-transition work on a few hundred floats, so one kernel does it for S
// transitions per workgroup instead of five latency-bound launches:
//   q = a W_head^T + b           (dqn.py:100-103; online rows 0..S-1 and next-state rows S..2S-1 form one
//                                  16-row MFMA tile, the waves split the contraction and reduce through LDS)
//   iterated Bellman target, squared TD loss, dL/dq   (isdqn.py:92-109, as td_kernel)
//   da = dL/dq W_head            (dL/dq has one non-zero per head and transition: K fp32 row-AXPYs, exact)
//   dz = backward of a = relu(LN(z)) over the hidden row (as ln_bwd_wide_kernel), partial (dgamma, dbeta,
//        dbias) sums per workgroup to part[wg][3][Fp]
// Workgroup 0 also advances the Adam step counter (it used to ride on loss_finalize_kernel, which now runs
// off the critical path).
// ---------------------------------------------------------------------------------------------
struct HeadChainParams {
    // hidden dense layer, finished inside this kernel for the rows a workgroup owns (dense_post_kernel's work)
    const float* slabs;     // [2B][n_slabs][Fp] split-K partial products of the hidden layer (row-interleaved)
    int n_slabs;
    int64_t slab_stride, row_pitch;  // Fp, n_slabs * Fp
    const float* hbias;     // [F] hidden bias
    float* act;             // [2B][Fp] post-activation rows (rows [0,B): states, [B,2B): next states), written here
    float* z;               // [B][Fp]  pre-LayerNorm rows of the states, written here
    const float* W;     // [O][Fp]
    const float* bias;  // [O]
    const float* gamma; // hidden LayerNorm scale / bias, or null
    const float* beta;
    int B, S, F, Fp, O, Op, K, A, oh;  // oh: online head k + oh is regressed on head k (1: iS-DQN, 0: single head)
    const int* action;
    const float* reward;
    const uint8_t* terminal;
    const float* loss_weights;  // [B] importance-sampling weights, or null (weight 1)
    const float* discount;      // [B] per-transition discounts in gamma_n's place, or null (isdqn_batch_discount::discount)
    float gamma_n, huber_delta;
    int double_q;       // isdqn_net_config::double_q: head oh + k of the next-state row selects, head k values
    Munchausen mu;      // isdqn_net_config::munchausen_*: head k of the state row gives the bonus, of the next-state row the soft value
    float* dout;        // [B][Op]  dL/dq
    float* dz;          // [B][Fp]
    float* part;        // [n_wg][3][Fp]
    float* q_values;    // [B][K]
    float* targets;     // [B][K]
    double* priorities; // [B] or null
    float* loss_part;   // [n_wg][K]
    float* dbh_part;    // [n_wg][Op]
    int* adam_count;
    float b1, b2;
    float* adam_consts;
    long long* stamps;  // profiling only (isdqn_debug_set_stamps "head_chain"): [workgroup][8] phase boundaries
};

// Transitions per workgroup (template parameter SMAX = 1, 2 or 4; HC_MAX_S in net_plan.h is the largest).  The kernel
// is instruction-issue bound (a few thousand instructions executed once per wave), and the target / data-gradient /
// LayerNorm phases scale with S, so few transitions on many workgroups win -- until every one of too many workgroups
// streams the whole head matrix from L2: S = 1 at B = 256 (20 us; S = 2: 23 us; S = 4 on 256 threads: 22 us before the
// dense_post fusion), S = 4 at B = 1024 (head_chain_plan picks about 256 workgroups).
constexpr int HC_MAX_COLS = 4;  // hidden width up to HC_THREADS * 4 (columns per thread: template parameter COLS)
// Eight waves: the kernel executes a few thousand instructions ONCE per wave, so it is bound by instruction issue and
// its dependency stalls; two waves per SIMD interleave, and each owns half the K-steps / columns.
constexpr int HC_THREADS = 512, HC_WAVES = HC_THREADS / 64;
constexpr int HC_KU = 16 / HC_WAVES;  // K-steps per wave and work item (an item covers 16 K-steps)

__host__ __device__ inline int head_chain_pitch(int Fp) { return (Fp + 31) / 32 * 32 + 8; }
static inline int head_chain_lds_bytes(int Fp, int Op, int K, int passes, int S) {
    const int PA = head_chain_pitch(Fp);
    return (passes >= 2 ? 2 : 1) * 16 * PA * 2 + (HC_WAVES * 16 * Op + 16 * Op + S * Op + Op + 4 + 2 * S * Fp) * 4 + S * K * 12 +
           HC_WAVES * 2 * S * 2 * 4 + 64;
}

template <int PASSES, int COLS, int SMAX>
__global__ __launch_bounds__(HC_THREADS) void head_chain_kernel(const HeadChainParams p) {
    ISDQN_EMPTY_KERNEL_RETURN
    extern __shared__ __attribute__((aligned(16))) char hc_smem[];
    const int PA = head_chain_pitch(p.Fp);
    constexpr int A_PLANES = PASSES >= 2 ? 2 : 1;
    __bf16* a_hi = reinterpret_cast<__bf16*>(hc_smem);
    __bf16* a_lo = a_hi + 16 * PA;
    float* qpart = reinterpret_cast<float*>(a_hi + A_PLANES * 16 * PA);  // [HC_WAVES][16][Op]
    float* s_q = qpart + HC_WAVES * 16 * p.Op;                                  // [16][Op]
    float* s_dq = s_q + 16 * p.Op;                                       // [SMAX][Op]
    float* s_d = s_dq + SMAX * p.Op;                                 // [SMAX][K]
    float* s_td = s_d + SMAX * p.K;                                  // TD loss per (transition, head): the priorities
    float* s_wtd = s_td + SMAX * p.K;                                // the same times the transition's weight: the loss partials
    float* s_red = s_wtd + SMAX * p.K;                               // [HC_WAVES][2 * SMAX][2]
    float* s_bias = s_red + HC_WAVES * 2 * SMAX * 2;                 // [Op]
    float* s_pre = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(s_bias + p.Op) + 15) & ~(uintptr_t)15);  // [2 * SMAX][Fp] hidden pre-activations, 16-B aligned

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if defined(ISDQN_DEV)
#define HC_STAMP(i)                                                                                     \
    if (p.stamps != nullptr && threadIdx.x == 0) {                                                     \
        p.stamps[(int64_t)blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memtime();              \
        if ((i) == 0) p.stamps[(int64_t)blockIdx.x * 8 + 7] = (long long)__builtin_amdgcn_s_memrealtime(); \
    }
#else
#define HC_STAMP(i)
#endif
    HC_STAMP(0);
    const int S = p.S, b0 = (int)blockIdx.x * S;
    const int Fp = p.Fp, Op = p.Op, K = p.K, A = p.A;

    if (blockIdx.x == 0 && tid == 0) {
        int t = *p.adam_count + 1;
        *p.adam_count = t;
        p.adam_consts[0] = (float)(1.0 - pow_int((double)p.b1, t));
        p.adam_consts[1] = (float)(1.0 - pow_int((double)p.b2, t));
    }

    // Global loads are requested a phase before they are needed, and nothing touches a loaded register where it is
    // requested (the data were last written from other XCDs: a first touch costs ~4000 cycles).
    // ---- operands of the later phases (raw: converted where they are used) ----
    int act[SMAX];  // action of the S transitions (selects the head rows the data gradient reads)
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        ISDQN_BOUNDS_CHECK((s < S && b0 + s < p.B) ? (const void*)(p.action + b0 + s) : zero_chunk(), 4, 20);
        act[s] = *(const ISDQN_GLOBAL int*)((s < S && b0 + s < p.B) ? (const void*)(p.action + b0 + s) : zero_chunk());
    }
    float td_r, td_w, td_g;  // reward, importance-sampling weight, discount, terminal flag of this thread's (transition, head) pair
    uint8_t td_term;
    {
        const int s = tid / K;
        const bool ok = tid < S * K && b0 + s < p.B;
        const bool okw = ok && p.loss_weights != nullptr;
        ISDQN_BOUNDS_CHECK(okw ? (const void*)(p.loss_weights + b0 + s) : zero_chunk(), 4, 29);
        td_w = *(const ISDQN_GLOBAL float*)(okw ? (const void*)(p.loss_weights + b0 + s) : zero_chunk());
        const bool okg = ok && p.discount != nullptr;
        ISDQN_BOUNDS_CHECK(okg ? (const void*)(p.discount + b0 + s) : zero_chunk(), 4, 50);
        td_g = *(const ISDQN_GLOBAL float*)(okg ? (const void*)(p.discount + b0 + s) : zero_chunk());
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.reward + b0 + s) : zero_chunk(), 4, 21);
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.terminal + b0 + s) : zero_chunk(), 1, 22);
        td_r = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.reward + b0 + s) : zero_chunk());
        td_term = *(const ISDQN_GLOBAL uint8_t*)(ok ? (const void*)(p.terminal + b0 + s) : zero_chunk());
    }
    ISDQN_BOUNDS_CHECK(tid < p.O ? (const void*)(p.bias + tid) : zero_chunk(), 4, 23);
    const float bias_v = *(const ISDQN_GLOBAL float*)(tid < p.O ? (const void*)(p.bias + tid) : zero_chunk());
    float ga[COLS], be[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
        const int c = tid + j * HC_THREADS;
        const bool ok = p.gamma != nullptr && c < p.F;
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.gamma + c) : zero_chunk(), 4, 24);
        ISDQN_BOUNDS_CHECK(ok ? (const void*)(p.beta + c) : zero_chunk(), 4, 24);
        ga[j] = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.gamma + c) : zero_chunk());
        be[j] = *(const ISDQN_GLOBAL float*)(ok ? (const void*)(p.beta + c) : zero_chunk());
    }

    // ---- the hidden dense layer is finished HERE for the 2S rows of this workgroup (dqn.py:96-99; what
    //      dense_post_kernel does in the forward-only path): split-K slabs summed in slab order, + bias, LayerNorm, ReLU.
    //      The rows go to HBM once (act: the head's weight gradient reads the state rows; z: debug / tests), to LDS as
    //      bf16 hi/lo for the head GEMM, and the pre-LayerNorm values stay in registers for the backward below.
    //      Tile rows 2S..15 are not staged: MFMA output rows depend on their own A row only, and nothing reads the q
    //      rows of those tile rows ----
    constexpr int R2 = 2 * SMAX;
    constexpr int TPR = HC_THREADS / R2;  // threads per tile row (two waves): 16-byte loads, one row per thread
    constexpr int SB = 32;                // slabs per batch = loads in flight per thread
    static_assert(TPR % 64 == 0, "a wave must not straddle two rows");
    float m1 = 0.f, m2 = 0.f;  // LayerNorm sums of this thread's row (over its columns)
    {
        const int r = tid / TPR, q = tid - r * TPR;
        const int smp = r < S ? r : r - S;
        const bool row_ok = r < 2 * S && b0 + smp < p.B;
        const int64_t grow = r < S ? (int64_t)(b0 + smp) : (int64_t)p.B + b0 + smp;
        for (int c0 = q * 4; c0 < Fp; c0 += TPR * 4) {  // (one pass up to 512 columns)
            float hb4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ISDQN_BOUNDS_CHECK(c0 + e < p.F ? (const void*)(p.hbias + c0 + e) : zero_chunk(), 4, 25);
                hb4[e] = *(const ISDQN_GLOBAL float*)(c0 + e < p.F ? (const void*)(p.hbias + c0 + e) : zero_chunk());
            }
            const ISDQN_GLOBAL f32x4* base = (const ISDQN_GLOBAL f32x4*)(row_ok ? (const void*)(p.slabs + grow * p.row_pitch + c0) : zero_chunk());
            const int64_t strd = row_ok ? p.slab_stride / 4 : 0;  // (Fp is a multiple of 8)
            f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < p.n_slabs; s0 += SB) {
                f32x4 t[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    ISDQN_BOUNDS_CHECK((const void*)(base + min(s0 + u, p.n_slabs - 1) * strd), 16, 26);
                    t[u] = base[min(s0 + u, p.n_slabs - 1) * strd];  // tail: clamped, masked in the sum
                }
#pragma unroll
                for (int u = 0; u < SB; ++u)
                    if (s0 + u < p.n_slabs) sum += t[u];  // (uniform condition; slab order)
            }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = c0 + e < p.F ? sum[e] + hb4[e] : 0.f;
                m1 += v[e];
                m2 += v[e] * v[e];
            }
            *reinterpret_cast<float4*>(s_pre + r * Fp + c0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }

    HC_STAMP(6);  // slab sums of this thread's row done
    // ---- q = a W^T work items, see below; the first batch of W fragments travels under the LayerNorm ----
    const int nkt = (PA - 8) / 32, NT = (Op + 15) / 16;
    const int nks = (nkt + 15) / 16, n_items = ((NT + 1) / 2) * nks;
    const int kg8 = (lane >> 4) * 8;
    const int arow = (lane & 15) * PA + kg8;
    auto issue_w = [&](float (&v)[2][HC_KU][8], int item) {
        const int pair = item / nks, ksb = wave + 16 * (item - pair * nks);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < HC_KU; ++u) {
                const int o = (pair * 2 + t) * 16 + (lane & 15), ks = ksb + HC_WAVES * u;
                const bool ok = item < n_items && o < p.O && ks < nkt && ks * 32 + kg8 < Fp;
                load8_aligned(ok ? p.W + (int64_t)o * Fp + ks * 32 + kg8 : zero_chunk(), v[t][u]);
            }
    };
    float wv0[2][HC_KU][8], wv1[2][HC_KU][8];
    issue_w(wv0, 0);

    float zv[SMAX][COLS];  // pre-LayerNorm values of the state rows (zero outside the row / the transition range)
    {
        for (int off = 32; off > 0; off >>= 1) {
            m1 += __shfl_xor(m1, off);
            m2 += __shfl_xor(m2, off);
        }
        if (lane == 0) {
            s_red[wave * 2] = m1;
            s_red[wave * 2 + 1] = m2;
        }
        __syncthreads();  // row sums and the pre-activation rows (s_pre) are visible
        constexpr int WPR = TPR / 64;  // waves per row
#pragma unroll
        for (int r = 0; r < R2; ++r) {
            float a1 = s_red[r * WPR * 2], a2 = s_red[r * WPR * 2 + 1];
#pragma unroll
            for (int w = 1; w < WPR; ++w) {  // fixed order
                a1 += s_red[(r * WPR + w) * 2];
                a2 += s_red[(r * WPR + w) * 2 + 1];
            }
            const float mean = a1 / (float)p.F;
            const float rstd = rsqrtf(fmaxf(a2 / (float)p.F - mean * mean, 0.f) + 1e-6f);
            const int smp = r < S ? r : r - S;
            const bool row_ok = r < 2 * S && b0 + smp < p.B;
            const int64_t grow = r < S ? (int64_t)(b0 + smp) : (int64_t)p.B + b0 + smp;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int c = tid + j * HC_THREADS;
                const float v = c < Fp ? s_pre[r * Fp + c] : 0.f;
                float y = v;
                if (p.gamma != nullptr && c < p.F) y = (v - mean) * (rstd * ga[j]) + be[j];
                y = fmaxf(y, 0.f);  // (the head chain requires a ReLU hidden layer)
                if (c >= p.F) y = 0.f;
                if (row_ok && c < Fp) {
                    s8_store_elem(p.act + grow * Fp, c, y);  // hidden activations: S8 (read back by the head weight gradient)
                    if (r < S) p.z[grow * Fp + c] = v;
                }
                if (r < 2 * S && c < PA - 8) {
                    const float ys = row_ok ? y : 0.f;
                    const __bf16 h = (__bf16)ys;
                    a_hi[r * PA + c] = h;
                    if constexpr (PASSES >= 2) a_lo[r * PA + c] = (__bf16)(ys - (float)h);
                }
                if (r < SMAX) zv[r < SMAX ? r : 0][j] = (row_ok && r < S && c < p.F) ? v : 0.f;
            }
        }
    }
    for (int i = tid; i < SMAX * Op; i += HC_THREADS) s_dq[i] = 0.f;
    if (tid < Op) s_bias[tid] = bias_v;
    for (int o = tid + HC_THREADS; o < Op; o += HC_THREADS) s_bias[o] = o < p.O ? p.bias[o] : 0.f;  // (more outputs than threads)
    __syncthreads();  // hidden rows staged
    HC_STAMP(1);  // hidden rows staged

    // ---- q = a W^T : wave w takes K-steps w, w+16, ... of every pair of 16-column tiles.  A work item is (tile pair,
    //      K-step group): its W fragments (two tiles x four K-steps) are one batch of loads, and the batch of the NEXT
    //      item is in flight while this one is multiplied ----
    {
        f32x4 acc[2];
        auto run_item = [&](float (&v)[2][HC_KU][8], int item) {
            const int pair = item / nks, ksi = item - pair * nks, ksb = wave + 16 * ksi;
            if (ksi == 0) {
                acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < HC_KU; ++u) {
                const int ks = min(ksb + HC_WAVES * u, nkt - 1);  // past the end: B is zero, A only has to be finite
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + arow + ks * 32);
                bf16x8 al;
                if constexpr (PASSES >= 2) al = *reinterpret_cast<const bf16x8*>(a_lo + arow + ks * 32);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    bf16x8 bh, bl;
                    if constexpr (PASSES >= 2) {
                        split8(v[t][u], bh, bl);
                        if constexpr (PASSES >= 3)
                            mfma_acc(acc[t], ah, bl);
                        mfma_acc(acc[t], al, bh);
                    } else {
                        round8(v[t][u], bh);
                    }
                    mfma_acc(acc[t], ah, bh);
                }
            }
            const bool last = ksi + 1 == nks;
            if (last) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int o = (pair * 2 + t) * 16 + (lane & 15);
                    if (o < Op) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) qpart[(wave * 16 + (lane >> 4) * 4 + r) * Op + o] = acc[t][r];
                    }
                }
            }
        };
        for (int item = 0; item < n_items; item += 2) {
            issue_w(wv1, item + 1);  // (past the last item: zero block)
            run_item(wv0, item);
            issue_w(wv0, item + 2);
            if (item + 1 < n_items) run_item(wv1, item + 1);
        }
    }

    // ---- data-gradient rows: head row (1 + k) * A + action of every (transition, head), four heads per batch; the
    //      first batch is requested here and travels under the target / TD phase ----
    auto issue_rows = [&](float (&w)[SMAX][4][COLS], int k0) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool on = s < S && k0 + u < K;
                const float* wr = p.W + (int64_t)(on ? (p.oh + k0 + u) * A + act[s] : 0) * Fp;
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    ISDQN_BOUNDS_CHECK(wr + (c < p.F ? c : 0), 4, 27);
                    w[s][u][j] = *(const ISDQN_GLOBAL float*)(wr + (c < p.F ? c : 0));
                }
            }
    };
    HC_STAMP(2);  // head GEMM done (this wave)
    float wr0[SMAX][4][COLS], wr1[SMAX][4][COLS];
    issue_rows(wr0, 0);
    __syncthreads();
    for (int i = tid; i < 2 * S * Op; i += HC_THREADS) {  // (tile rows 2S..15 are nobody's)
        const int o = i % Op;
        float v = qpart[i];
#pragma unroll
        for (int w = 1; w < HC_WAVES; ++w) v += qpart[w * 16 * Op + i];  // fixed order
        s_q[i] = o < p.O ? v + s_bias[o] : 0.f;
    }
    __syncthreads();

    // ---- iterated Bellman target, TD, dL/dq (isdqn.py:92-109) ----
    const float inv_b = 1.f / (float)p.B;
    if (tid < S * K) {
        const int s = tid / K, k = tid - s * K;
        const int b = b0 + s;
        float d = 0.f, td = 0.f;
        int a = 0;
        if (b < p.B) {
            a = act[0];
#pragma unroll
            for (int i = 1; i < SMAX; ++i) a = s == i ? act[i] : a;
            const float qv = s_q[s * Op + (p.oh + k) * A + a];
            const float* nq = s_q + (S + s) * Op + k * A;
            float mx = nq[0];
            if (p.double_q) {
                mx = nq[argmax_first(nq + p.oh * A, A)];
            } else {
                for (int j = 1; j < A; ++j) mx = fmaxf(mx, nq[j]);
            }
            const float gamma_n = p.discount != nullptr ? td_g : p.gamma_n;
            float tg = td_r + (1.f - (float)td_term) * gamma_n * mx;
            if (p.mu.tau > 0.f) {  // the value head's own row of the state: head k, not oh + k
                const float* sv = s_q + s * Op + k * A;
                tg = munchausen_target(td_r, 1.f - (float)td_term, gamma_n, sv[a], soft_value(sv, A, p.mu.tau), soft_value(nq, A, p.mu.tau), p.mu);
            }
            d = qv - tg;
            td = td_loss(d, p.huber_delta);
            if (p.q_values) p.q_values[(int64_t)b * K + k] = qv;
            if (p.targets) p.targets[(int64_t)b * K + k] = tg;
        }
        const float w = p.loss_weights != nullptr ? td_w : 1.f;
        const float dd = td_dloss(d, p.huber_delta) * inv_b * w;
        s_d[tid] = dd;
        s_td[tid] = td;
        s_wtd[tid] = td * w;
        s_dq[s * Op + (p.oh + k) * A + a] = dd;
    }
    __syncthreads();
    for (int i = tid; i < S * Op; i += HC_THREADS) {
        const int s = i / Op;
        if (b0 + s < p.B) p.dout[(int64_t)b0 * Op + i] = s_dq[i];
    }
    for (int c = tid; c < Op; c += HC_THREADS) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += s_dq[s * Op + c];
        p.dbh_part[(int64_t)blockIdx.x * Op + c] = sum;
    }
    if (tid < K) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += s_wtd[s * K + tid];
        p.loss_part[(int64_t)blockIdx.x * K + tid] = sum;
    }
    if (p.priorities != nullptr && tid < S && b0 + tid < p.B) {
        float sum = 0.f;
        for (int k = 0; k < K; ++k) sum += s_td[tid * K + k];
        p.priorities[b0 + tid] = sqrt((double)(sum / (float)K) + 1e-10);
    }

    HC_STAMP(3);  // targets / TD / small stores issued
    // ---- da = dL/dq W (K row-AXPYs per transition, heads in ascending order), then the LayerNorm/ReLU backward of
    //      the hidden row ----
    float da[SMAX][COLS];
#pragma unroll
    for (int s = 0; s < SMAX; ++s)
#pragma unroll
        for (int j = 0; j < COLS; ++j) da[s][j] = 0.f;
    auto axpy_rows = [&](const float (&w)[SMAX][4][COLS], int k0) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool on = s < S && k0 + u < K;
                const float dd = on ? s_d[s * K + k0 + u] : 0.f;
#pragma unroll
                for (int j = 0; j < COLS; ++j) da[s][j] += dd * w[s][u][j];
            }
    };
    for (int k0 = 0; k0 < K; k0 += 8) {  // 4 heads x S transitions x COLS columns of W rows per batch, two batches in flight
        issue_rows(wr1, k0 + 4);
        axpy_rows(wr0, k0);
        issue_rows(wr0, k0 + 8);
        if (k0 + 4 < K) axpy_rows(wr1, k0 + 4);
    }
    HC_STAMP(4);  // data-gradient rows accumulated
    float dg[COLS], db[COLS], dbias[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) dg[j] = db[j] = dbias[j] = 0.f;
    if (p.gamma != nullptr) {
        const float inv_c = 1.f / (float)p.F;
        float r1[SMAX], r2[SMAX];
        auto block_sum2 = [&]() {  // r1[s], r2[s] summed over the workgroup
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                for (int off = 32; off > 0; off >>= 1) {
                    r1[s] += __shfl_xor(r1[s], off);
                    r2[s] += __shfl_xor(r2[s], off);
                }
            __syncthreads();
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < SMAX; ++s) {
                    s_red[(wave * SMAX + s) * 2] = r1[s];
                    s_red[(wave * SMAX + s) * 2 + 1] = r2[s];
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                r1[s] = s_red[s * 2];
                r2[s] = s_red[s * 2 + 1];
#pragma unroll
                for (int w = 1; w < HC_WAVES; ++w) {  // fixed order
                    r1[s] += s_red[(w * SMAX + s) * 2];
                    r2[s] += s_red[(w * SMAX + s) * 2 + 1];
                }
            }
        };
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            r1[s] = r2[s] = 0.f;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {  // zv is zero outside the row / the transition range
                r1[s] += zv[s][j];
                r2[s] += zv[s][j] * zv[s][j];
            }
        }
        block_sum2();
        float mean[SMAX], rstd[SMAX];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            mean[s] = r1[s] * inv_c;
            rstd[s] = rsqrtf(fmaxf(r2[s] * inv_c - mean[s] * mean[s], 0.f) + 1e-6f);
            r1[s] = r2[s] = 0.f;
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const int c = tid + j * HC_THREADS;
                const bool ok = c < p.F && s < S && b0 + s < p.B;
                const float xh = (zv[s][j] - mean[s]) * rstd[s];
                const float y = xh * ga[j] + be[j];
                const float dy = (ok && y > 0.f) ? da[s][j] : 0.f;
                dg[j] += dy * xh;
                db[j] += dy;
                const float g2 = dy * ga[j];
                da[s][j] = g2;   // keep g
                zv[s][j] = ok ? xh : 0.f;  // keep xhat
                r1[s] += g2;
                r2[s] += g2 * zv[s][j];
            }
        }
        block_sum2();
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            const float m1 = r1[s] * inv_c, m2 = r2[s] * inv_c;
            if (s < S && b0 + s < p.B) {
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    if (c < Fp) {
                        const float o = c < p.F ? rstd[s] * (da[s][j] - m1 - zv[s][j] * m2) : 0.f;
                        dbias[j] += o;
                        s8_store_elem(p.dz + (int64_t)(b0 + s) * Fp, c, o);  // dz: S8
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            if (s < S && b0 + s < p.B) {
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int c = tid + j * HC_THREADS;
                    if (c < Fp) {
                        const float o = (c < p.F && zv[s][j] > 0.f) ? da[s][j] : 0.f;
                        dbias[j] += o;
                        s8_store_elem(p.dz + (int64_t)(b0 + s) * Fp, c, o);  // dz: S8
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
        const int c = tid + j * HC_THREADS;
        if (c < Fp) {
            float* pp = p.part + (int64_t)blockIdx.x * 3 * Fp;
            pp[c] = dg[j];
            pp[Fp + c] = db[j];
            pp[2 * Fp + c] = dbias[j];
        }
    }
    HC_STAMP(5);  // LayerNorm backward done, stores issued
#undef HC_STAMP
}
