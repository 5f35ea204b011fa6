// Host side of every launch: the stamps, refresh_mirror (with split_params_kernel, which keeps its place in the code object here),
// NetInput, the conv / dense / plain dispatchers, net_forward, ln_bwd, the LearnCall value of the learn / loss / gradient entry points,
// AdamList, loss_finalize / loss_and_finalize and head_expect.  Included by net_kernels.hip inside namespace isdqn, behind every kernel
// header and in front of impala.h and batchnorm.h, which are built from these dispatchers.  The templated kernels sit in the code
// object where this file first names each instantiation: reordering references here moves them (tests/test_kernel_order_host.py).
#pragma once
// =============================================================================================
// Host orchestration
// =============================================================================================
// profiling hook (not in the public header): phase stamps of the image-resident forward kernel of one layer
#if defined(ISDQN_DEV)
static long long* g_stamps = nullptr;
static int g_stamp_layer = -1;
static char g_stamp_name[32] = "";
extern "C" int isdqn_debug_set_stamps(void* buf, const char* layer_name) {
    g_stamps = (long long*)buf;
    g_stamp_layer = buf ? 0 : -1;
    snprintf(g_stamp_name, sizeof(g_stamp_name), "%s", layer_name ? layer_name : "");
    return ISDQN_OK;
}
static long long* stamps_for(const char* kernel_tag) {
    return (g_stamp_layer >= 0 && strcmp(kernel_tag, g_stamp_name) == 0) ? g_stamps : nullptr;
}
#else
static long long* stamps_for(const char*) { return nullptr; }
#endif

// fp32 master parameters -> S8 mirror (gemm_core.h): every 32-byte group of 8 values becomes 8 hi + 8 lo bf16.  The
// MFMA consumers of the weights stage the mirror by copy.  Run at the head of every entry point that takes `params`:
// the master is caller-owned memory (imports, head shifts, target copies happen outside this library).
__global__ __launch_bounds__(256) void split_params_kernel(const float* __restrict__ p, float* __restrict__ mirror, int64_t n_groups) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    float v[8];
    load8_aligned(p + g * 8, v);
    s8_store_group(mirror + g * 8, v);
}
static int refresh_mirror(const Plan& P, const float* params, float* ws, hipStream_t st) {
    const int64_t n_groups = P.n_params / 8;  // every tensor size is a multiple of 8 (padded widths)
    hipLaunchKernelGGL(split_params_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, params, ws + P.wsplit_off, n_groups);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static ConvGeom conv_geom(const Layer& l) {
    ConvGeom g;
    g.hin = l.hin; g.win = l.win; g.cin_p = l.cin_p; g.hout = l.hout; g.wout = l.wout;
    g.cout = l.cout; g.cout_p = l.cout_p; g.ksz = l.ksz; g.stride = l.stride; g.pad = l.pad;
    g.npix = l.npix; g.K = l.K;
    g.stride_sh = l.stride == 4 ? 2 : l.stride == 2 ? 1 : 0;
    g.d_npix = FastDiv(l.npix); g.d_wout = FastDiv(l.wout); g.d_cinp = FastDiv(l.cin_p);
    g.d_ksz = FastDiv(l.ksz); g.d_coutp = FastDiv(l.cout_p);
    return g;
}

// Storage of the pre-activation gradients dz of hidden layers (bit 0 of the S8 operand masks below): S8, written so
// by every producer (head chain, LayerNorm-backward epilogues and kernels); the head's dL/dq stays fp32
constexpr int DZ_S8 = 1;

struct NetInput {
    const uint8_t* frames; int64_t frame_stride; const int* frame_ids; int paired_B;  // cnn
    const float* obs; const float* obs2; int obs_split;                             // fc
    int id_pitch = 0, id_off = 0;                                                   // cnn, unpaired: see FrameSrc
};

template <int BM, int PASSES, bool U8>
static int launch_conv_fwd(const Layer& l, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                           int z_img, float* act, float* z, hipStream_t st) {
    ConvFwd<BM, PASSES, U8> p;
    p.g = conv_geom(l);
    p.W = MatSrc{wmir + l.w_off, l.K, l.cout_p, l.K, 1};
    p.in = act_in;
    p.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    p.bias = params + l.b_off;
    p.gamma = l.has_ln ? params + l.g_off : nullptr;
    p.beta = l.has_ln ? params + l.be_off : nullptr;
    p.scale = U8 ? (1.0f / 255.0f) : 1.0f;
    p.act = act; p.z = z;
    p.n_pix_total = n_img * l.npix;
    p.z_pix = z_img * l.npix;
    return launch_gemm(p, ceil_div(p.n_pix_total, 128), st);
}

// image-resident forward convolution (conv_img.h) when the input tile fits in LDS; generic engine otherwise
static int conv_fwd_img(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                        int z_img, float* act, float* z, hipStream_t st, bool* done) {
    *done = false;
    // The image-resident kernels store `act` unconditionally (only the `z` store is guarded, by z_img): a caller without an activation
    // output -- the impala Stacks pass act == nullptr for the convolutions whose output is only needed pre-activation -- must take the
    // generic engine.  (Round 3's uncommitted experiment that routed the impala convolutions here faulted on exactly that store:
    // "Memory access fault ... on address 0x9000" = null + the first image tile's offset, gpurun_out/imp1.log)
    if (act == nullptr || (z == nullptr && z_img > 0)) return ISDQN_OK;
    ConvImgParams ip;
    ip.g = conv_geom(l);
    // (two channel tiles: the kernel then alternates two accumulator sets, see conv_fwd_img_kernel)
    const int mt = l.cout_p <= 32 ? 2 : 4;
    const int passes = x3 ? (l.is_u8 ? 2 : 3) : 1;
    // pixel pitch: +8 / +16 elements so that the 16 pixels of an MFMA column tile do not share LDS banks
    // (128-byte pixel rows put them 4-5 deep on the same banks; measured model in DESIGN.md)
    ip.PP = l.is_u8 ? 0 : l.cin_p + (l.cin_p % 64 == 0 ? 16 : 8);
    int lds = conv_img_geometry(ip.g, l.is_u8, l.cin, passes >= 3 ? 2 : 1, mt, passes >= 2 ? 2 : 1, ip.R, ip.Wp,
                                ip.plane_elems, ip.PP);
    constexpr int LDS_LIMIT = 158 * 1024;  // of the 160 KB, minus the kernels' static arrays
    if (lds > LDS_LIMIT || (l.is_u8 && (l.win < 8 || l.cin > 4))) return ISDQN_OK;  // (frame ids of a stack live in 4 registers)
    if (!l.is_u8 && l.cin_p < 16) return ISDQN_OK;  // (8-channel S8 inputs -- the BatchNorm networks' first convolution -- take the generic engine)
    // A row pitch of wout (mod 8) pixels keeps the bank pattern of a fragment's pixel columns going across the end of an
    // image row (conv_img.h, PixelOrder: the short last strip of every row is where the conflicts are left); taken when it
    // costs no workgroup per CU (11-pixel rows of the stride-2 layer: 24 -> 27 columns, conflict factor 1.75 -> 1.0).
    if (!l.is_u8 && l.npix <= 128) {
        const int want = ip.Wp + (((l.wout - ip.Wp) % 8) + 8) % 8;
        const int planes = passes >= 3 ? 2 : 1;
        const int lds2 = lds + planes * ip.R * (want - ip.Wp) * ip.PP * 2;
        const int stage2 = (passes >= 2 ? 2 : 1) * (mt * 16) * 48 * 2 * 2;  // the second K group's stages (see kg2 below)
        const int old_total = lds > 80 * 1024 ? lds + stage2 : lds, new_total = lds2 > 80 * 1024 ? lds2 + stage2 : lds2;
        if (want != ip.Wp && new_total <= LDS_LIMIT && (old_total <= 80 * 1024) == (new_total <= 80 * 1024)) {
            ip.Wp = want;
            ip.plane_elems = ip.R * want * ip.PP;
            lds = lds2;
        }
    }
    ip.W = MatSrc{wmir + l.w_off, l.K, l.cout_p, l.K, 1};
    ip.in = act_in;
    ip.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    ip.bias = params + l.b_off;
    ip.gamma = l.has_ln ? params + l.g_off : nullptr;
    ip.beta = l.has_ln ? params + l.be_off : nullptr;
    ip.scale = l.is_u8 ? (1.0f / 255.0f) : 1.0f;
    ip.act = act; ip.z = z; ip.n_img = n_img; ip.z_img = z_img;
    ip.tiles_per_img = ceil_div(l.npix, 128);
    ip.d_chunk = FastDiv((uint32_t)(l.is_u8 ? ip.Wp / 8 : l.cin_p / 8));
    ip.d_Wp = FastDiv((uint32_t)ip.Wp);
    ip.d_R = FastDiv((uint32_t)ip.R);
    ip.order = PixelOrder(l.hout, l.wout, !l.is_u8 && ip.tiles_per_img == 1);
    ip.stamps = stamps_for(l.name);
    ip.ablate = 0;
    ip.Rd = 0;
#if defined(ISDQN_DEV)
    if (const char* e = getenv("ISDQN_ABLATE")) ip.ablate = atoi(e);
#endif
    *done = true;
    if (l.is_u8) {
#if !defined(ISDQN_NO_U8_PAIR)
        // one workgroup of eight waves per image, weights resident in LDS, the image staged in halves of two tiles (conv_u8_pair.h):
        //   * an even tile count (a half is two tiles; images of more than four tiles loop over their halves);
        //   * four stacked frames (the frame ids live in four registers, the resident weights are [32][256]: K = 256, eight K steps
        //     as straight-line code) and at most 32 output channels (mt == 2);
        //   * the image of a half -- the input rows of 256 consecutive pixels -- is one batch of 2 x 512 positions;
        //   * weights + that image fit the LDS (84 x 84: 34 + 41 KB, two workgroups per CU).
        // Any other geometry runs on the one-tile kernel below.  Measured at the headline size: 26.2 -> 21.2 us, the step +2 % (c2 and
        // c3).  At c5 (B = 1024, four rounds of 512 workgroups) the kernel is 86 -> 72 us but the untraced step did not resolve either
        // way in four calls (+1.6, +0.1, -0.8, +0.2 %): there is no crossover to put a batch-size threshold at, and none is here
        // (docs/NOTEBOOK.md 2026-10-20, profiles/conv0_image/).
        ip.Rd = conv_u8_pair_rows(ip.g);
        const int lds_pair = passes == 2 ? conv_u8_pair_lds<2>(ip.Rd, ip.Wp) : conv_u8_pair_lds<1>(ip.Rd, ip.Wp);
        if (mt == 2 && ip.tiles_per_img % 2 == 0 && ip.Rd * (ip.Wp / 8) <= U8P_PB * U8P_THREADS && lds_pair <= LDS_LIMIT && l.cin == 4 &&
            l.K == 256 && ip.ablate == 0)
            return passes == 2 ? launch_conv_fwd_u8_pair<2, 8>(ip, st) : launch_conv_fwd_u8_pair<1, 8>(ip, st);
#endif
        if (passes == 2) return mt == 2 ? launch_conv_fwd_img<2, 2, true>(ip, st) : launch_conv_fwd_img<4, 2, true>(ip, st);
        return mt == 2 ? launch_conv_fwd_img<2, 1, true>(ip, st) : launch_conv_fwd_img<4, 1, true>(ip, st);
    }
    // An image that leaves room for one workgroup per CU only (more than half of the 160 KB) runs with two K groups of
    // four waves, if the second pair of weight stages still fits and the accumulator exchange fits the image area.
    const int stage_bytes = (passes >= 2 ? 2 : 1) * (mt * 16) * 48 * 2 * 2;  // two stages of one K group
    static const bool no_kg = ISDQN_DEV_ENV("ISDQN_NO_KGROUPS");
    const bool kg2 = !no_kg && mt == 4 && lds > 80 * 1024 && lds + stage_bytes <= LDS_LIMIT &&
                     mt * 16 * 128 * 4 <= lds - stage_bytes && l.K >= 8 * GEMM_BK;
#if !defined(ISDQN_NO_U8_PAIR)
    // two images per workgroup, the second one prefetched into registers (conv_s8_pair.h): the one-workgroup-per-CU layer with 16 K steps
    if (passes == 3 && mt == 4 && kg2 && ip.tiles_per_img == 1 && l.K == 512 && n_img % 2 == 0 && ip.ablate == 0 && ip.stamps == nullptr &&
        ip.R * ip.Wp * (l.cin_p / 8) <= S8P_BATCH * GEMM_THREADS * 2)
        return launch_conv_fwd_s8_pair<8>(ip, st);
#endif
    if (passes == 3) return mt == 2 ? launch_conv_fwd_img<2, 3, false>(ip, st)
                          : kg2 ? launch_conv_fwd_img<4, 3, false, 2>(ip, st) : launch_conv_fwd_img<4, 3, false>(ip, st);
    return mt == 2 ? launch_conv_fwd_img<2, 1, false>(ip, st)
         : kg2 ? launch_conv_fwd_img<4, 1, false, 2>(ip, st) : launch_conv_fwd_img<4, 1, false>(ip, st);
}

static int conv_fwd(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int n_img,
                    int z_img, float* act, float* z, hipStream_t st) {
    bool done = false;
    int rc = conv_fwd_img(l, x3, params, wmir, in, act_in, n_img, z_img, act, z, st, &done);
    if (rc || done) return rc;
    const bool small = l.cout_p <= 32;
    if (l.is_u8) {
        if (x3) return small ? launch_conv_fwd<32, 2, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                             : launch_conv_fwd<64, 2, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
        return small ? launch_conv_fwd<32, 1, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                     : launch_conv_fwd<64, 1, true>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
    }
    if (x3) return small ? launch_conv_fwd<32, 3, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                         : launch_conv_fwd<64, 3, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
    return small ? launch_conv_fwd<32, 1, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st)
                 : launch_conv_fwd<64, 1, false>(l, params, wmir, in, act_in, n_img, z_img, act, z, st);
}

// number of slabs launch_plain writes for (K, splits); *steps_per_split: the K steps of each
static int effective_splits(int K, int splits, int* steps_per_split = nullptr) {
    int ksteps = ceil_div(K, GEMM_BK);
    if (splits < 1) splits = 1;
    if (splits > ksteps) splits = ksteps;
    int sps = ceil_div(ksteps, splits);
    if (steps_per_split) *steps_per_split = sps;
    return ceil_div(ksteps, sps);
}

// C[split][M][N] = A . B^T over row-major sources.  a_tr/b_tr: the operand is stored [K][rows].
template <int BM, int BN, int WM, int WN, bool ATR, bool BTR, int PASSES, bool AL, bool A2PART, bool ADAM = false, int S8M = 0>
static int launch_plain(const MatSrc& A, const float* A2, int a_split, const MatSrc& B, float* C, int ldc, int M,
                        int N, int K, int splits, int64_t slab_stride, hipStream_t st,
                        const AdamFuse* adam = nullptr) {
    PlainGemm<BM, BN, WM, WN, ATR, BTR, PASSES, AL, A2PART, ADAM, S8M> p;
    if (adam) p.adam = *adam;
    p.A = A; p.B = B; p.A2 = A2; p.a_split = a_split; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
    p.tiles_m = ceil_div(M, BM); p.tiles_n = ceil_div(N, BN);
    p.splits = effective_splits(K, splits, &p.steps_per_split);
    p.slab_stride = slab_stride;
    return launch_gemm(p, p.tiles_m * p.tiles_n * p.splits, st);
}

template <bool ATR, bool BTR, bool AL = true, bool A2PART = false, int S8M = 0>
static int plain_big(bool x3, const MatSrc& A, const float* A2, int a_split, const MatSrc& B, float* C, int ldc,
                     int M, int N, int K, int splits, int64_t slab_stride, hipStream_t st) {
    if (x3)
        return launch_plain<128, 128, 2, 2, ATR, BTR, 3, AL, A2PART, false, S8M>(A, A2, a_split, B, C, ldc, M, N, K, splits,
                                                                                 slab_stride, st);
    return launch_plain<128, 128, 2, 2, ATR, BTR, 1, AL, A2PART, false, S8M>(A, A2, a_split, B, C, ldc, M, N, K, splits,
                                                                             slab_stride, st);
}

// 128 x 64 tiles: twice the workgroups of plain_big for GEMMs whose 128 x 128 grid cannot fill 256 CUs
template <bool ATR, bool BTR, int S8M = 0>
static int plain_narrow(bool x3, const MatSrc& A, const MatSrc& B, float* C, int ldc, int M, int N, int K, int splits,
                        int64_t slab_stride, hipStream_t st) {
    if (x3) return launch_plain<128, 64, 2, 2, ATR, BTR, 3, true, false, false, S8M>(A, nullptr, 0, B, C, ldc, M, N, K, splits, slab_stride, st);
    return launch_plain<128, 64, 2, 2, ATR, BTR, 1, true, false, false, S8M>(A, nullptr, 0, B, C, ldc, M, N, K, splits, slab_stride, st);
}

// `skip_post`: leave the split-K slabs as they are (the head chain kernel finishes the layer for its own rows)
static int dense_fwd(const Layer& l, bool x3, const float* params, const float* wmir, const NetInput& in, const float* act_in, int rows,
                     int z_rows, float* slab, float* act, float* z, hipStream_t st, bool skip_post = false) {
    MatSrc A, B;
    const float* A2 = nullptr;
    int a_split = 0;
    if (l.in_unpadded_ld) {  // fc first layer: caller's [rows][obs] matrices
        A = MatSrc{in.obs, l.in_unpadded_ld, rows, l.in_f, 0};
        if (in.obs2) { A2 = in.obs2; a_split = in.obs_split; }
    } else {
        A = MatSrc{act_in, l.in_p, rows, l.in_p, 1};
    }
    B = MatSrc{wmir + l.w_off, l.in_p, l.out_f, l.in_p, 1};  // weights: S8 mirror (rows padded to in_p with zeros)
    // split-K partial products, row-interleaved: slab s of row m at slab[(m * ns + s) * out_p].  The ns partial rows of
    // one output row are one contiguous block (64 KB at the headline size) for whoever sums them; in [slab][row]
    // order they sit 1 MB apart, 32 pages per reader.
    const int ns = effective_splits(l.in_unpadded_ld ? l.in_f : l.K, l.fwd_splits);
    const int64_t slab_stride = l.out_p;
    const int ldc = ns * l.out_p;
    int rc;
    if (l.in_unpadded_ld) {
        // caller-provided observations: no alignment promise; MatSrc bounds use the true widths
        // (the observation operand bounds its own chunks to in_f; the mirror rows are read in whole aligned groups)
        rc = A2 ? plain_big<false, false, false, true, 2>(x3, A, A2, a_split, B, slab, ldc, rows, l.out_f, l.in_f,
                                                          l.fwd_splits, slab_stride, st)
                : plain_big<false, false, false, false, 2>(x3, A, nullptr, 0, B, slab, ldc, rows, l.out_f, l.in_f,
                                                           l.fwd_splits, slab_stride, st);
    } else if (l.fwd_narrow) {  // few row tiles: 128 x 64 tiles reach the workgroup count with half the split-K slabs
        rc = plain_narrow<false, false, 3>(x3, A, B, slab, ldc, rows, l.out_f, l.K, l.fwd_splits, slab_stride, st);
    } else {
        rc = plain_big<false, false, true, false, 3>(x3, A, nullptr, 0, B, slab, ldc, rows, l.out_f, l.K, l.fwd_splits, slab_stride,
                                                     st);  // activations and weights both S8
    }
    if (rc || skip_post) return rc;
    hipLaunchKernelGGL(dense_post_kernel, dim3(rows), dim3(256), 3 * l.out_p * sizeof(float), st, slab, ns, slab_stride,
                       (int64_t)ldc, rows, l.out_f, l.out_p, params + l.b_off, l.has_ln ? params + l.g_off : nullptr,
                       l.has_ln ? params + l.be_off : nullptr, l.has_relu, act, z, z_rows, l.is_head ? 0 : 1);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// (declared here, defined in impala.h / batchnorm.h: net_forward below calls them, and they are built from the dispatchers of this file)
static int impala_forward(const Plan& P, bool x3, const float* params, const float* wmir, const NetInput& in, int n_img, int z_img,
                          float* ws, hipStream_t st, int bn_mode = 0);
static int bn_forward(const Plan& P, bool x3, const float* params, const NetInput& in, int n_img, int z_img, float* ws, float* q_out, bool running,
                      hipStream_t st);

// Dueling heads: the raw rows ("head_raw" / "head_raw_target") that belong to the head-output rows `q_out` points at -- rows of the
// "q" / "logits" region or of their *_target twin (null: neither)
static float* duel_raw_rows(const Plan& P, float* ws, const float* q_out) {
    const int64_t o = q_out - ws;
    if (o >= P.out_off && o < P.out_off + (int64_t)P.N2 * P.nlog_p) return ws + P.raw_off + (o - P.out_off) / P.nlog_p * P.raw_p;
    if (P.out_t_off >= 0 && o >= P.out_t_off && o < P.out_t_off + (int64_t)P.qt_rows * P.nlog_p)
        return ws + P.raw_t_off + (o - P.out_t_off) / P.nlog_p * P.raw_p;
    return nullptr;
}
// raw rows -> the combined head-output rows every consumer reads (dueling.h)
static int duel_combine(const Plan& P, const float* raw, float* out, int n_rows, hipStream_t st) {
    const int64_t threads = (int64_t)n_rows * P.n_heads * (P.head_nb > 0 ? P.head_nb : 1);
    hipLaunchKernelGGL(duel_combine_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, st, raw, P.raw_p, out,
                       P.nlog_p, n_rows, P.n_heads, P.n_actions, P.head_nb > 0 ? P.head_nb : 1);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// forward over n_img images; hidden activations -> ws act regions, head output -> q_out [n_img][nha_p] (histogram / quantile heads:
// [n_img][nlog_p]; dueling heads: the combined rows, the head Dense's own output goes to the raw rows behind them)
static int net_forward(const Plan& P, bool x3, const float* params, const NetInput& in, int n_img, int z_img,
                       float* ws, float* q_out, hipStream_t st, int n_run = -1, int skip_post_layer = -1) {
    if (P.bn) {  // BatchNorm networks outside a learn step: the running averages (isdqn.py:130, use_running_average=True)
        ISDQN_REQUIRE(n_run < 0 && skip_post_layer < 0, ISDQN_ERR_UNSUPPORTED, "partial forward passes are not built for BatchNorm networks");
        return bn_forward(P, x3, params, in, n_img, z_img, ws, q_out, true, st);
    }
    const float* prev = nullptr;
    const float* wmir = ws + P.wsplit_off;  // refreshed by the caller (refresh_mirror) from `params`
    if (n_run < 0) n_run = P.n_layers;
    for (int i = 0; i < n_run; ++i) {
        const Layer& l = P.L[i];
        float* act = l.is_head ? q_out : ws + l.act_off;
        float* z = l.is_head ? nullptr : ws + l.z_off;
        int rc;
        if (l.is_head && P.dueling) {
            act = duel_raw_rows(P, ws, q_out);
            ISDQN_REQUIRE(act != nullptr, ISDQN_ERR_ARG, "dueling heads: the head output must go to the workspace's head rows");
        }
        if (l.kind == 2)
            rc = impala_forward(P, x3, params, wmir, in, n_img, z_img, ws, st);
        else if (l.kind == 0)
            rc = conv_fwd(l, x3, params, wmir, in, prev, n_img, z_img, act, z, st);
        else
            rc = dense_fwd(l, x3, params, wmir, in, prev, n_img, l.is_head ? 0 : z_img, ws + P.slab_off, act, z, st,
                           i == skip_post_layer);
        if (rc) return rc;
        if (l.is_head && P.dueling) {
            rc = duel_combine(P, act, q_out, n_img, st);
            if (rc) return rc;
        }
        prev = act;
    }
    return ISDQN_OK;
}

static int ln_bwd(const Layer& l, const float* params, const float* da, const float* z, int rows, float* dz,
                  float* part, int* n_blocks_out, hipStream_t st) {
    const float* gamma = l.has_ln ? params + l.g_off : nullptr;
    const float* beta = l.has_ln ? params + l.be_off : nullptr;
    const int C = l.out_f, Cp = l.out_p;
    int nb;
#define LAUNCH_SMALL(TPR)                                                                                          \
    do {                                                                                                           \
        nb = ceil_div(rows, 256 / TPR);                                                                            \
        if (nb > LN_MAX_BLOCKS) nb = LN_MAX_BLOCKS;                                                                \
        hipLaunchKernelGGL(ln_bwd_small_kernel<TPR>, dim3(nb), dim3(256), 0, st, da, z, gamma, beta, rows, C, Cp,  \
                           dz, part);                                                                              \
    } while (0)
    if (Cp <= 32) LAUNCH_SMALL(8);
    else if (Cp <= 64) LAUNCH_SMALL(16);
    else if (Cp <= 128) LAUNCH_SMALL(32);
    else if (Cp <= 256) LAUNCH_SMALL(64);
    else {
        ISDQN_REQUIRE(Cp <= 256 * LN_WIDE_MAX_COLS, ISDQN_ERR_UNSUPPORTED, "hidden dense width above 4096");
        nb = rows < LN_MAX_BLOCKS ? rows : LN_MAX_BLOCKS;
        hipLaunchKernelGGL(ln_bwd_wide_kernel, dim3(nb), dim3(256), 0, st, da, z, gamma, beta, rows, C, Cp, dz, part);
    }
#undef LAUNCH_SMALL
    ISDQN_HIP_CHECK(hipGetLastError());
    *n_blocks_out = nb;
    return ISDQN_OK;
}

template <int BM, int PASSES>
static int launch_conv_dgrad(const Layer& l, const float* wmir, const float* dz, float* da, int n_img,
                             hipStream_t st) {
    ConvDgrad<BM, PASSES> p;
    p.g = conv_geom(l);
    p.W = wmir + l.w_off;
    p.dz = dz; p.da = da; p.n_img = n_img;
    p.T = l.ksz / l.stride;
    p.Kc = p.T * p.T * l.cout_p;
    p.n_classes = l.stride * l.stride;
    int acc = 0;
    for (int c = 0; c < p.n_classes; ++c) {
        int cy = c / l.stride, cx = c % l.stride;
        int Ha = (l.hin - cy + l.stride - 1) / l.stride, Wb = (l.win - cx + l.stride - 1) / l.stride;
        p.tile_start[c] = acc;
        p.cls_d_hw[c] = FastDiv((uint32_t)(Ha * Wb));
        p.cls_d_w[c] = FastDiv((uint32_t)Wb);
        acc += ceil_div(n_img * Ha * Wb, 128);
    }
    p.tile_start[p.n_classes] = acc;
    return launch_gemm(p, acc, st);
}

template <int PASSES, bool U8>
static int launch_conv_wgrad(const Layer& l, const NetInput& in, const float* act_in, const float* dz, float* slabs,
                             int n_img, hipStream_t st) {
    ConvWgrad<PASSES, U8> p;
    p.g = conv_geom(l);
    p.n_pix = n_img * l.npix;
    p.DZ = MatSrc{dz, l.cout_p, p.n_pix, l.cout_p, 1};
    p.in = act_in;
    p.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    p.slabs = slabs;
    p.scale = U8 ? (1.0f / 255.0f) : 1.0f;
    p.tiles_n = ceil_div(l.K, 64);
    int ksteps = ceil_div(p.n_pix, GEMM_BK);
    p.steps_per_split = ceil_div(ksteps, l.gw_slabs);
    p.splits = ceil_div(ksteps, p.steps_per_split);
    return launch_gemm(p, p.tiles_n * p.splits, st);
}
// image-resident weight gradient (conv_img.h); *slabs_out = 0 when the layer does not qualify
static int conv_wgrad_img(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, float* slabs,
                          int n_img, hipStream_t st, int* slabs_out) {
    *slabs_out = 0;
    if (!l.wgi_ntw || n_img != 0 && ceil_div(n_img, l.wgi_G) > l.gw_slabs) return ISDQN_OK;
    ConvWgradImgParams wp;
    wp.g = conv_geom(l);
    const int passes = x3 ? (l.is_u8 ? 2 : 3) : 1;
    const int mt = l.cout_p <= 32 ? 2 : 4;
    int lds_unused_R, Wp, plane;
    conv_img_geometry(wp.g, l.is_u8, l.cin, 1, mt, 1, lds_unused_R, Wp, plane);
    wp.R = l.stride * (l.hout - 1) + l.ksz;  // the whole image
    wp.Wp = Wp;
    // pixel pitches: an odd multiple of 32 bytes between consecutive contraction pixels (dz rows: PA; input: stride * PPin)
    wp.PPin = l.cin_p;
    for (int pad = 0; pad <= 24; pad += 8)
        if ((l.stride * (l.cin_p + pad)) % 32 == 16) { wp.PPin = l.cin_p + pad; break; }
    wp.in_plane = l.is_u8 ? l.cin * wp.R * Wp : wp.R * Wp * wp.PPin;
    wp.PA = l.cout_p + (l.cout_p % 32 == 0 ? 16 : 8);
    wp.npix_pad = round_up(l.npix, 32);
    wp.dz_plane = wp.npix_pad * wp.PA;
    const int lds = ((passes >= 2 ? 2 : 1) * wp.dz_plane + (passes >= 3 ? 2 : 1) * wp.in_plane) * 2;
    if (lds > 150 * 1024 || (l.is_u8 && (l.win < 8 || l.cin > 4))) return ISDQN_OK;
    wp.d_chunk = FastDiv((uint32_t)(l.is_u8 ? Wp / 8 : l.cin_p / 8));
    wp.d_Wp = FastDiv((uint32_t)Wp);
    wp.d_R = FastDiv((uint32_t)wp.R);
    wp.d_dzchunk = FastDiv((uint32_t)(l.cout_p / 8));
    wp.d_npixpad = FastDiv((uint32_t)wp.npix_pad);
    wp.dz = dz; wp.in = act_in;
    wp.fs = FrameSrc{in.frames, in.frame_stride, in.frame_ids, l.cin, in.paired_B, l.hin, l.win, in.id_pitch, in.id_off};
    wp.slabs = slabs;
    wp.scale = l.is_u8 ? (1.0f / 255.0f) : 1.0f;
    wp.n_img = n_img; wp.G = l.wgi_G;
    wp.NC = 64 * l.wgi_ntw;
    wp.n_col_groups = l.K / wp.NC;
    wp.d_ncg = FastDiv((uint32_t)wp.n_col_groups);
    {
        char tag[32];
        snprintf(tag, sizeof(tag), "wgrad:%s", l.name);
        wp.stamps = stamps_for(tag);
    }
    const int groups = ceil_div(n_img, l.wgi_G);
    *slabs_out = groups;
#define WGI(MT_, NTW_, P_, U_) return launch_conv_wgrad_img<MT_, NTW_, P_, U_>(wp, groups, st)
#define WGI8(MT_, NTW_, P_, U_) return launch_conv_wgrad_img<MT_, NTW_, P_, U_, 8>(wp, groups, st)
    if (l.is_u8) {
        if (mt == 2) { if (l.wgi_ntw == 4) { if (passes == 2) WGI(2, 4, 2, true); else WGI(2, 4, 1, true); }
                       if (l.wgi_ntw == 2) { if (passes == 2) WGI(2, 2, 2, true); else WGI(2, 2, 1, true); } }
        else         { if (l.wgi_ntw == 4) { if (passes == 2) WGI(4, 4, 2, true); else WGI(4, 4, 1, true); }
                       if (l.wgi_ntw == 2) { if (passes == 2) WGI(4, 2, 2, true); else WGI(4, 2, 1, true); } }
    } else {
        if (mt == 2) { if (l.wgi_ntw == 4) { if (passes == 3) WGI(2, 4, 3, false); else WGI(2, 4, 1, false); }
                       if (l.wgi_ntw == 3) { if (passes == 3) WGI(2, 3, 3, false); else WGI(2, 3, 1, false); }
                       if (l.wgi_ntw == 2) { if (passes == 3) WGI(2, 2, 3, false); else WGI(2, 2, 1, false); } }
        else         { // full-width tiles: 32 column tiles on eight waves (25.7 -> 21 us); the 36 tiles of a 3x3x64 layer stay on four
                       // (six or eight waves re-read the dz fragments too often: 33.5 -> 37 us)
                       static const bool w4 = ISDQN_DEV_ENV("ISDQN_WGRAD_4WAVES");
                       if (l.wgi_ntw == 8 && !w4) { if (passes == 3) WGI8(4, 4, 3, false); else WGI8(4, 4, 1, false); }
                       if (l.wgi_ntw == 9) { if (passes == 3) WGI(4, 9, 3, false); else WGI(4, 9, 1, false); }
                       if (l.wgi_ntw == 8) { if (passes == 3) WGI(4, 8, 3, false); else WGI(4, 8, 1, false); }
                       if (l.wgi_ntw == 4) { if (passes == 3) WGI(4, 4, 3, false); else WGI(4, 4, 1, false); }
                       if (l.wgi_ntw == 3) { if (passes == 3) WGI(4, 3, 3, false); else WGI(4, 3, 1, false); }
                       if (l.wgi_ntw == 2) { if (passes == 3) WGI(4, 2, 3, false); else WGI(4, 2, 1, false); } }
    }
#undef WGI
#undef WGI8
    *slabs_out = 0;  // (u8 with NTW 3 is not instantiated)
    return ISDQN_OK;
}

// image-resident data gradient of conv layer `l` fused with the LayerNorm/ReLU backward of layer `below`:
// writes dz of `below` and the reduced (dgamma, dbeta, dbias) row of `below`.  *done = false: not applicable.
static void add_reduce_job(ReduceJobs& jobs, const float* part, int n_rows, int width, float* out) {
    const int i = jobs.n++;
    jobs.part[i] = part; jobs.out[i] = out; jobs.n_rows[i] = n_rows; jobs.width[i] = width;
    jobs.block_start[i + 1] = jobs.block_start[i] + ceil_div(width, 8);
}

static int conv_dgrad_img(const Layer& l, const Layer& below, bool x3, const float* params, const float* wmir, const float* dz, float* ws,
                          int n_img, hipStream_t st, bool* done, ReduceJobs* jobs) {
    *done = false;
    if (!l.dgi_tiles || below.part_rows < n_img * l.dgi_tiles) return ISDQN_OK;
    ConvDgradImgParams dp;
    dp.g = conv_geom(l);
    dp.W = wmir + l.w_off;
    dp.dz = dz;
    dp.z_in = ws + below.z_off;
    dp.gamma = below.has_ln ? params + below.g_off : nullptr;
    dp.beta = below.has_ln ? params + below.be_off : nullptr;
    dp.c_in = below.out_f;
    dp.dz_in = ws + below.dz_off;
    dp.part = ws + below.part_off;
    dp.n_img = n_img;
    dp.T = l.ksz / l.stride;
    dp.Kc = dp.T * dp.T * l.cout_p;
    // top / left zero border of the dz image: the taps of a class reach dz rows (iy + pad - py) / stride - jy, jy < T, i.e. down
    // to pad / stride - (T - 1).  (Round 1 took T - 1 rows whatever the padding; for the 3x3 / 1 layer that is one row and one
    // column too many -- a 14 x 14 instead of a 13 x 13 image, 83 KB of LDS instead of 75: ONE workgroup per CU instead of two.)
#if defined(ISDQN_DGRAD_WIDE_BORDER)
    dp.bt = dp.T - 1;
#else
    dp.bt = dp.T - 1 - l.pad / l.stride > 0 ? dp.T - 1 - l.pad / l.stride : 0;
#endif
    const int need_h = (l.hin - 1 + l.pad) / l.stride + 1, need_w = (l.win - 1 + l.pad) / l.stride + 1;
    dp.Hd = dp.bt + (l.hout > need_h ? l.hout : need_h);
    dp.Wd = dp.bt + (l.wout > need_w ? l.wout : need_w);
    // pixel pitch with (pitch bytes / 16) = 2 (mod 4): conflict-free ds_read_b128 of 16 consecutive pixels (conv_img.h)
    dp.PPd = l.cout_p + ((16 - l.cout_p % 32) + 32) % 32;
    dp.dz_plane = dp.Hd * dp.Wd * dp.PPd;
    dp.d_chunk = FastDiv((uint32_t)(l.cout_p / 8));
    dp.d_Wd = FastDiv((uint32_t)dp.Wd);
    dp.d_T = FastDiv((uint32_t)dp.T);
    {
        char tag[32];
        snprintf(tag, sizeof(tag), "dgrad:%s", l.name);
        dp.stamps = stamps_for(tag);
    }
    dp.n_classes = l.stride * l.stride;
    int acc = 0;
    for (int c = 0; c < dp.n_classes; ++c) {
        int cy = c / l.stride, cx = c % l.stride;
        int Ha = (l.hin - cy + l.stride - 1) / l.stride, Wb = (l.win - cx + l.stride - 1) / l.stride;
        dp.cls_tile_start[c] = acc;
        dp.cls_order[c] = PixelOrder(Ha, Wb, Ha * Wb <= 128);  // (a class of several tiles keeps row-major tiles)
        acc += ceil_div(Ha * Wb, l.dgi_tile_pix);
    }
    dp.cls_tile_start[dp.n_classes] = acc;
    dp.tiles_per_img = acc;
    const int mt = l.cin_p <= 32 ? 2 : 4;
    const int passes = x3 ? 3 : 1;
    const int lds = (2 * (passes >= 2 ? 2 : 1) * 32 * (mt * 16 + 16) + (passes >= 3 ? 2 : 1) * dp.dz_plane) * 2;  // TileGeom<.., true>
    if (lds > 150 * 1024) return ISDQN_OK;
    int rc;
    ISDQN_REQUIRE(acc == l.dgi_tiles, ISDQN_ERR_ARG, "data-gradient tiling differs from the plan's");
#if ISDQN_DGRAD_TILE64_BELOW > 0
    if (l.dgi_tile_pix == 64) {
        if (passes == 3) rc = mt == 2 ? launch_conv_dgrad_img<2, 3, 1>(dp, st) : launch_conv_dgrad_img<4, 3, 1>(dp, st);
        else rc = mt == 2 ? launch_conv_dgrad_img<2, 1, 1>(dp, st) : launch_conv_dgrad_img<4, 1, 1>(dp, st);
    } else
#endif
    if (passes == 3) rc = mt == 2 ? launch_conv_dgrad_img<2, 3>(dp, st) : launch_conv_dgrad_img<4, 3>(dp, st);
    else rc = mt == 2 ? launch_conv_dgrad_img<2, 1>(dp, st) : launch_conv_dgrad_img<4, 1>(dp, st);
    if (rc) return rc;
    add_reduce_job(*jobs, ws + below.part_off, n_img * dp.tiles_per_img, 3 * below.out_p, ws + below.red_off);
    *done = true;
    return ISDQN_OK;
}

static int conv_wgrad_slabs(const Layer& l, int n_img) {
    int ksteps = ceil_div(n_img * l.npix, GEMM_BK);
    int sps = ceil_div(ksteps, l.gw_slabs);
    return ceil_div(ksteps, sps);
}

// (declared here, defined in batchnorm.h: the impala torso's BatchNorm sites use them in impala.h, which batchnorm.h in turn calls)
static inline const BnSite* bn_site_of(const Plan& P, int layer);
static int bn_site_forward(const BnSite& b, const float* params, float* ws, int rows, bool running, hipStream_t st);
static int bn_site_backward(const BnSite& b, const float* params, float* ws, float* dy, int rows, bool apply, hipStream_t st);
// Which heads a loss regresses (default: the plan's iterated pairs, online head oh + k on target head k, k < K).  The analysis
// agents evaluate single-pair losses on the multi-head network: online head 1 on target head 1 (analysisdqn.py:156-183).
struct HeadSel {
    int on0 = 0, tg0 = 0, K = 0;  // (K == 0: the plan's pairs)
};

// What a learn / loss / gradient-only call asks for: every entry point of that kind fills one by field name, and the same value goes
// down to learn_or_loss, bn_learn_or_loss and impala_backward.  Plain data of the caller's pointers: nothing is allocated for it.
enum class LearnMode { Loss, Learn, GradOnly };  // forward and loss / + backward and update / + backward, grad_out alone is written
struct LearnCall {
    const isdqn_net_config* cfg = nullptr;
    LearnMode mode = LearnMode::Loss;
    float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    int32_t* adam_count = nullptr;
    const float* target_params = nullptr;  // non-null: the next states go through them (the DQN forms)
    const isdqn_batch* batch = nullptr;
    float *losses = nullptr, *loss_accum = nullptr, *q_values = nullptr, *targets = nullptr;  // q_values / targets null: their workspace regions
    double* priorities = nullptr;
    float* grad_out = nullptr;  // the reduced gradient (internal layout); a gradient-only pass needs it
    float* ws = nullptr;
    hipStream_t st = nullptr;  // the caller's stream
    HeadSel sel;
    float weight_decay = 0.f;  // AdamW (isdqn_batch_decay, read by learn_call for the calls that update; 0: plain Adam)
    int32_t decay_kinds = 0;   // bit k: tensors of isdqn_tensor_info::kind k decay
    float wd(int kind) const { return ((decay_kinds >> kind) & 1) ? weight_decay : 0.f; }  // what an optimizer entry of that kind carries
    float cql_alpha = 0.f;     // the conservative term (isdqn_batch_conservative, read by learn_call in every mode; 0: none, nothing launched)
    bool mixture = false;      // the call carries ISDQN_BATCH_MIXTURE (isdqn_batch_mixture, read by learn_call in every mode; mixture.h)
    const float* mix_alpha = nullptr;  // ... its [n_mix] device weights, checked by check_mixture (learn_step.h)
    int32_t n_mix = 0;
    bool learn() const { return mode != LearnMode::Loss; }  // a backward pass follows the loss
    bool update() const { return mode == LearnMode::Learn; }
};

// the pairs a call regresses: the plan's own, or the caller's selection held to the network's heads
static int resolve_heads(const Plan& P, HeadSel& sel) {
    if (sel.K <= 0) return sel = HeadSel{P.oh, 0, P.K}, ISDQN_OK;
    ISDQN_REQUIRE(sel.on0 >= 0 && sel.tg0 >= 0 && sel.on0 + sel.K <= P.n_heads && sel.tg0 + sel.K <= P.n_heads && sel.K <= P.K, ISDQN_ERR_ARG,
                  "head selection outside the network's heads");
    return ISDQN_OK;
}

// The optimizer kernels request p / m / v before they know whether they update: a gradient-only pass has no moments, so those
// (unused) loads read the parameters instead of a null pointer.
static void moments_of_a_gradient_only_pass(LearnCall& call) { call.adam_m = call.adam_v = call.params; }

// ---- launch helpers shared by the three learn paths (plain / LayerNorm below, BatchNorm in batchnorm.h, the torso in impala.h) ----
// `rows`: the rows the gradient flows through (B, or all 2B rows of a BatchNorm network)

// The tensors one stream's optimizer launches update, in launch order: adam_kernel once per ADAM_MAX_ENTRIES of them.
struct AdamList {
    std::vector<AdamEntry> e;
    AdamList() { e.reserve(ADAM_MAX_ENTRIES); }
    void add(int64_t p_off, int64_t size, const float* g, int n_slabs, int64_t stride, float wd) {
        e.push_back(AdamEntry{p_off, size, stride, g, n_slabs, 0, wd});
    }
    // entries [e0, e0 + ADAM_MAX_ENTRIES) as one launch's table; `per_block`: elements a workgroup of the launch covers
    AdamTable table(size_t e0, int per_block = 64) const {
        AdamTable tab;
        tab.n = 0;
        tab.total_blocks = 0;
        for (size_t k = e0; k < e.size() && k < e0 + ADAM_MAX_ENTRIES; ++k) {
            AdamEntry& t = tab.e[tab.n++];
            t = e[k];
            t.block_start = tab.total_blocks;
            tab.total_blocks += (int)((t.size + per_block - 1) / per_block);
        }
        return tab;
    }
    int launch(hipStream_t st, const Plan& P, const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, float* ws, float* grad_out,
               bool update) const {
        for (size_t e0 = 0; e0 < e.size(); e0 += ADAM_MAX_ENTRIES) {
            const AdamTable tab = table(e0);
            hipLaunchKernelGGL(adam_kernel, dim3(tab.total_blocks), dim3(256), 0, st, tab, params, adam_m, adam_v, ws + P.adam_tab_off, cfg->learning_rate,
                               cfg->adam_b1, cfg->adam_b2, cfg->adam_eps, grad_out, ws + P.wsplit_off, update ? 1 : 0);
            ISDQN_HIP_CHECK(hipGetLastError());
        }
        return ISDQN_OK;
    }
};
// a list's optimizer launches for a call (AdamList::launch keeps its own parameter list: its symbol is the parent's)
static int adam_launch(const AdamList& list, hipStream_t st, const Plan& P, const LearnCall& c) {
    return list.launch(st, P, c.cfg, c.params, c.adam_m, c.adam_v, c.ws, c.grad_out, c.update());
}

// per-head loss sums and the head-bias gradient (`width` columns) of the P.B transitions from the `n_blk` partial rows a loss kernel left
// in the workspace; `adam_count` non-null: also the step count and Adam's bias corrections
static int loss_finalize(const Plan& P, const isdqn_net_config* cfg, float* ws, int n_blk, int K, int width, float* losses, float* loss_accum,
                         bool head_bias_grad, int32_t* adam_count, hipStream_t st) {
    float* loss_part = ws + P.lpart_off;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(ceil_div(K, 16) + ceil_div(width, 16)), dim3(256), 0, st, loss_part, loss_part + (int64_t)n_blk * K, n_blk,
                       P.B, K, width, losses, loss_accum, head_bias_grad ? ws + P.dbh_off : nullptr, adam_count, cfg->adam_b1, cfg->adam_b2,
                       ws + P.adam_tab_off);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// targets, per-transition loss and dL/d(head output) of rows [0, B) from the head outputs of a finished forward (TD loss on the Q rows, or
// the HL-Gauss or the categorical projection loss on the logit rows, the quantile-regression loss on the quantile rows), then loss_finalize over the head layer's width (nlog_p: nha_p without histogram heads).
// `val_rows`: head-output rows [B][nlog_p] of the next states that supply the bootstrap value (null: rows [B, 2B) of the forward);
// `double_q`: selector head on0 + k of rows [B, 2B) of the forward -- the online parameters on the next states -- picks the action;
// Munchausen targets (cfg->munchausen_tau > 0): `state_val_rows`, head-output rows [B][nlog_p] of the states from the network that
// supplies the value (null: rows [0, B) of the forward)
// The per-transition discounts behind a batch that says it has them (include/isdqn_hip.h, isdqn_batch_discount), else null.
static inline const float* batch_discount(const isdqn_batch* batch) {
    return (batch->flags & ISDQN_BATCH_DISCOUNT) ? reinterpret_cast<const isdqn_batch_discount*>(batch)->discount : nullptr;
}
// The weight decay behind a batch that says it has one (include/isdqn_hip.h, isdqn_batch_decay), else none; unchecked (check_decay).
static inline void batch_decay(const isdqn_batch* batch, float* weight_decay, int32_t* decay_kinds) {
    const bool has = batch != nullptr && (batch->flags & ISDQN_BATCH_WEIGHT_DECAY);
    const isdqn_batch_decay* d = reinterpret_cast<const isdqn_batch_decay*>(batch);
    *weight_decay = has ? d->weight_decay : 0.f;
    *decay_kinds = has ? d->decay_kinds : 0;
}
// The conservative term's alpha behind a batch that says it has one (include/isdqn_hip.h, isdqn_batch_conservative), else 0; unchecked
// (check_conservative).
static inline float batch_conservative(const isdqn_batch* batch) {
    const bool has = batch != nullptr && (batch->flags & ISDQN_BATCH_CONSERVATIVE);
    return has ? reinterpret_cast<const isdqn_batch_conservative*>(batch)->cql_alpha : 0.f;
}
// The mixture weights behind a batch that says it has them (include/isdqn_hip.h, isdqn_batch_mixture); unchecked (check_mixture).
static inline bool batch_mixture(const isdqn_batch* batch, const float** alpha, int32_t* n_mix) {
    const bool has = batch != nullptr && (batch->flags & ISDQN_BATCH_MIXTURE);
    const isdqn_batch_mixture* m = reinterpret_cast<const isdqn_batch_mixture*>(batch);
    *alpha = has ? m->alpha : nullptr;
    *n_mix = has ? m->n_mix : 0;
    return has;
}
static int check_conservative(float cql_alpha) {
    ISDQN_REQUIRE(cql_alpha >= 0.f && cql_alpha <= 3.4028234e38f, ISDQN_ERR_ARG, "cql_alpha must be finite and >= 0");  // (NaN fails both)
    return ISDQN_OK;
}
static int check_decay(float weight_decay, int32_t decay_kinds) {
    ISDQN_REQUIRE(weight_decay >= 0.f && weight_decay <= 3.4028234e38f, ISDQN_ERR_ARG, "weight_decay must be finite and >= 0");  // (NaN fails both)
    ISDQN_REQUIRE((decay_kinds & ~ISDQN_DECAY_KINDS_ALL) == 0, ISDQN_ERR_ARG, "decay_kinds: bits 0..6 only (kinds 7 and 8 are running statistics)");
    ISDQN_REQUIRE(weight_decay == 0.f || decay_kinds != 0, ISDQN_ERR_ARG, "weight_decay > 0 needs at least one kind in decay_kinds");
    return ISDQN_OK;
}

// `c`: the call with its heads resolved and q_values / targets pointing at their destination; the step count advances in a pass with
// a backward that hands one (adam_count in a gradient-only pass: null from grad_on_batch; the noisy learn step hands its own, because
// its optimizer launch follows the pass and reads the step count's bias corrections from the same place)
static int loss_and_finalize(const Plan& P, const LearnCall& c, bool double_q = false, const float* val_rows = nullptr,
                             const float* state_val_rows = nullptr) {
    const isdqn_net_config* cfg = c.cfg;
    const isdqn_batch* batch = c.batch;
    float* ws = c.ws;
    const int B = P.B, K = c.sel.K, on0 = c.sel.on0, tg0 = c.sel.tg0;
    const bool learn = c.learn();
    const Munchausen mu{cfg->munchausen_tau, cfg->munchausen_alpha, cfg->munchausen_clip};
    if (state_val_rows == nullptr) state_val_rows = ws + P.out_off;
    const float* mun_rows = mu.tau > 0.f ? state_val_rows : nullptr;
    const float* next_rows = ws + P.out_off + (int64_t)B * P.nlog_p;
    if (val_rows == nullptr) val_rows = next_rows;
    const float* sel_rows = double_q ? next_rows : nullptr;
    const int R = P.head_nb > 0 ? rows_per_wg(K, P.head_nb) : 0;  // distributional kernels: transitions per workgroup
    const int n_blk = R ? ceil_div(B, R) : ceil_div(B, TD_ROWS);
    float* loss_part = ws + P.lpart_off;
    HeadLossArgs a{};  // (head_loss.h)
    a.out = ws + P.out_off;
    a.val = val_rows;
    a.sel = sel_rows; a.sel_pitch = P.nlog_p; a.sel_head = on0;
    a.mun = mun_rows; a.mun_pitch = P.nlog_p; a.mun_head = tg0; a.mu = mu;
    a.B = B; a.R = R; a.K = K; a.on0 = on0; a.tg0 = tg0; a.A = P.n_actions;
    a.nb = P.head_nb; a.pitch = P.nlog_p;
    a.vmin = P.hl_min; a.eta = P.head_nb > 0 ? (P.hl_max - P.hl_min) / (float)P.head_nb : 0.f; a.sigma = P.hl_sigma;
    a.huber_delta = cfg->huber_delta;
    a.action = batch->action; a.reward = batch->reward; a.terminal = batch->terminal; a.loss_weights = batch->loss_weights;
    a.discount = batch_discount(batch); a.gamma_n = cfg->gamma_n;
    a.dout = learn ? ws + P.dout_off : nullptr;
    a.q_values = c.q_values; a.targets = c.targets; a.priorities = c.priorities;
    a.loss_part = loss_part; a.dbh_part = loss_part + (int64_t)n_blk * K;
    auto launch = [&](auto kern, int threads, size_t dyn_lds) { hipLaunchKernelGGL(kern, dim3(n_blk), dim3(threads), dyn_lds, c.st, a); };
    const size_t dl_bytes = (size_t)R * K * P.head_nb * sizeof(float);  // s_dl of head_loss.h
    // NT = 64-value groups of a (head, action) a lane owns: the quantile and the categorical kernels are instantiated per count
    auto with_nt = [&](auto f) {
        switch (ceil_div(P.head_nb, 64)) {
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            case 3: f(std::integral_constant<int, 3>{}); break;
            default: f(std::integral_constant<int, 4>{}); break;
        }
    };
    if (P.qr)  // quantile heads (quantile.h): kappa = cfg->huber_delta (0: the plain pinball loss)
        with_nt([&](auto nt) {
            if (cfg->huber_delta > 0.f) launch(qr_loss_kernel<decltype(nt)::value, true>, QR_THREADS, dl_bytes);
            else launch(qr_loss_kernel<decltype(nt)::value, false>, QR_THREADS, dl_bytes);
        });
    else if (P.c51)  // categorical projection loss on the histogram heads (categorical.h)
        with_nt([&](auto nt) { launch(c51_loss_kernel<decltype(nt)::value>, C51_THREADS, dl_bytes); });
    else if (R)
        launch(hl_loss_kernel, 256, dl_bytes);
    else if (c.mixture)  // random ensemble mixture (mixture.h): K = 1, every head takes part under c.mix_alpha (mixture_kernels.hip)
    {
        if (int rc = launch_mix_td(a, n_blk, c.mix_alpha, (int)c.n_mix, c.st)) return rc;
    }
    else
        launch(td_kernel, 256, 2 * TD_ROWS * K * sizeof(float));
    ISDQN_HIP_CHECK(hipGetLastError());
    if (c.cql_alpha > 0.f) {  // the conservative term (conservative_kernels.hip), on the rows and with the row partition of the launch above
        ConservativeArgs ca{};
        ca.out = a.out; ca.dout = a.dout; ca.loss_part = a.loss_part; ca.dbh_part = a.dbh_part;
        ca.action = a.action; ca.loss_weights = a.loss_weights;
        ca.B = B; ca.rows_per_blk = R ? R : TD_ROWS; ca.n_blk = n_blk; ca.K = K; ca.on0 = on0; ca.A = P.n_actions;
        ca.nb = P.head_nb; ca.pitch = P.nlog_p; ca.quantile = P.qr ? 1 : 0;
        ca.vmin = a.vmin; ca.eta = a.eta; ca.alpha = c.cql_alpha;
        ca.dout_floats = (int64_t)P.Bb * P.nlog_p; ca.part_floats = (int64_t)P.B * (P.K + P.nlog_p);
        if (int rc = launch_conservative(ca, c.st)) return rc;
    }
    return loss_finalize(P, cfg, ws, n_blk, K, P.nlog_p, c.losses, c.loss_accum, learn, learn ? c.adam_count : nullptr, c.st);
}

// LayerNorm scale / bias and layer bias of `l` from `n_rows` partial rows of (dgamma, dbeta, dbias) at `part`
static void add_ln_bias_entries(AdamList& adam, const LearnCall& c, const Layer& l, const float* part, int n_rows, int64_t stride) {
    if (l.has_ln) {
        adam.add(l.g_off, l.out_p, part, n_rows, stride, c.wd(3));
        adam.add(l.be_off, l.out_p, part + l.out_p, n_rows, stride, c.wd(4));
    }
    if (l.b_off >= 0) adam.add(l.b_off, l.out_p, part + 2 * l.out_p, n_rows, stride, c.wd(2));  // (the impala torso has no bias of its own)
}

// generic data gradient of conv layer `l`: da [rows][hin][win][cin_p] fp32
static int conv_dgrad(const Layer& l, bool x3, const float* wmir, const float* dz, float* da, int rows, hipStream_t st) {
    const bool small = l.cin_p <= 32;
    if (x3) return small ? launch_conv_dgrad<32, 3>(l, wmir, dz, da, rows, st) : launch_conv_dgrad<64, 3>(l, wmir, dz, da, rows, st);
    return small ? launch_conv_dgrad<32, 1>(l, wmir, dz, da, rows, st) : launch_conv_dgrad<64, 1>(l, wmir, dz, da, rows, st);
}

// data gradient of dense layer `l`: da[b][in_p] = sum_o dz[b][o] * W[o][in_p]  (dz: the fp32 dL/dq of the head, S8 for a hidden layer)
// `narrow`: 128 x 64 tiles
static int dense_dgrad(const Layer& l, bool x3, const float* wmir, const float* dz, int dz_ld, float* da, int rows, bool narrow, hipStream_t st) {
    MatSrc A{dz, dz_ld, rows, l.out_p, 1};
    MatSrc Bm{wmir + l.w_off, l.in_p, l.out_f, l.in_p, 1};
    if (l.is_head)
        return narrow ? plain_narrow<false, true, 2>(x3, A, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st)
                      : plain_big<false, true, true, false, 2>(x3, A, nullptr, 0, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st);
    return narrow ? plain_narrow<false, true, DZ_S8 | 2>(x3, A, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st)
                  : plain_big<false, true, true, false, DZ_S8 | 2>(x3, A, nullptr, 0, Bm, da, l.in_p, rows, l.in_p, l.out_p, 1, 0, st);
}

// weight gradient of conv layer `l` into its slabs (image-resident kernel where the layer qualifies); *n_slabs: the slabs written
// (l.is_u8 only on the first layer of a cnn without BatchNorm, net_plan.h)
static int conv_wgrad(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, float* slabs, int rows, hipStream_t st,
                      int* n_slabs) {
    int rc = conv_wgrad_img(l, x3, in, act_in, dz, slabs, rows, st, n_slabs);
    if (rc || *n_slabs) return rc;
    *n_slabs = conv_wgrad_slabs(l, rows);
    if (l.is_u8) return x3 ? launch_conv_wgrad<2, true>(l, in, act_in, dz, slabs, rows, st) : launch_conv_wgrad<1, true>(l, in, act_in, dz, slabs, rows, st);
    return x3 ? launch_conv_wgrad<3, false>(l, in, act_in, dz, slabs, rows, st) : launch_conv_wgrad<1, false>(l, in, act_in, dz, slabs, rows, st);
}

// dense_wgrad with both operands fp32 and no alignment promise.  It runs the kernels of isdqn_selftest_gemm and is defined behind it
// (net_kernels.hip): naming their instantiation here would move them in the code object (tests/test_kernel_order_host.py)
static int dense_wgrad_fp32(const Layer& l, bool x3, const MatSrc& A, const MatSrc& Bm, float* slabs, int rows, hipStream_t st);

// weight gradient of dense layer `l` into its effective_splits(rows, l.gw_slabs) slabs:
// dW[out][in_p] = sum_b dz[b][out] * a[b][in_p], both operands stored [K = b][rows]
static int dense_wgrad(const Layer& l, bool x3, const NetInput& in, const float* act_in, const float* dz, int dz_ld, float* slabs, int rows,
                       hipStream_t st) {
    const MatSrc A{dz, dz_ld, rows, l.out_p, 1};
    const MatSrc Bm = l.in_unpadded_ld ? MatSrc{in.obs, l.in_unpadded_ld, rows, l.in_f, 0} : MatSrc{act_in, l.in_p, rows, l.in_p, 1};
    if (l.in_unpadded_ld) {  // fc first layer: caller's fp32 observations
        // (an fc network without a hidden layer: that first layer is the head, and its dz is the fp32 dL/dq, not an S8 tensor)
        if (l.is_head) return dense_wgrad_fp32(l, x3, A, Bm, slabs, rows, st);
        return plain_big<true, true, false, false, DZ_S8>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
    }
    if (l.is_head)  // dL/dq is fp32, the hidden activations are S8
        return plain_big<true, true, true, false, 2>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
    return plain_big<true, true, true, false, DZ_S8 | 2>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
}

// Histogram / quantile heads: Q rows `q` [n_rows][nha_p] <- expectations of the logit rows / means of the quantile rows `rows`
// [n_rows][nlog_p] (no-op for scalar heads).
static int head_expect_rows(const Plan& P, const float* rows, int n_rows, float* q, hipStream_t st) {
    if (P.head_nb == 0) return ISDQN_OK;
    const int64_t waves = (int64_t)n_rows * P.nha;
    if (P.qr)
        hipLaunchKernelGGL(qr_expect_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rows, n_rows, P.nha, P.head_nb, P.nlog_p,
                           P.nha_p, q);
    else
        hipLaunchKernelGGL(hl_expect_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rows, n_rows, P.nha, P.head_nb,
                           P.nlog_p, P.nha_p, P.hl_min, (P.hl_max - P.hl_min) / (float)P.head_nb, q);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}
// the rows the forward left in the "logits" region -> the "q" region
static int head_expect(const Plan& P, float* ws, int n_rows, hipStream_t st) {
    return head_expect_rows(P, ws + P.logits_off, n_rows, ws + P.q_off, st);
}
