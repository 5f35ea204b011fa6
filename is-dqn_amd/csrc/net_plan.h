// Host-side plan of the Q-network: layer geometry, internal parameter layout and workspace map.
// Mirrors slimdqn/networks/architectures/dqn.py:47-103 (cnn / fc branches) and the
// (1+K)*A head view of slimdqn/networks/isdqn.py:34-41.
#pragma once
#include <cmath>
#include <cstdlib>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"

// Image-resident conv data gradient (plan_conv_dgrad_tiles): pixels of a class per workgroup, 128 or 64.
// One four-wave workgroup per CU cannot hide its own latencies (round 4, stamps_dgrad.txt: a K step of 384 MFMA
// cycles takes 1 080), and half tiles make the conv2 data gradient of c2 7 us shorter (26.2 -> 18.9) -- but they fill
// the image and read the weight fragments twice, and in the step that CU time is taken from the kernels of the other
// queue (ab_tile64_c2.txt: the step is 3.7 % SLOWER at B = 256; at B = 32, where the chip is
// mostly empty either way, +0.2 %: noise).  Off in the product; -DISDQN_DGRAD_TILE64_BELOW=<workgroups> builds them.
#if !defined(ISDQN_DGRAD_TILE64_BELOW)
#define ISDQN_DGRAD_TILE64_BELOW 0
#endif

namespace isdqn {

constexpr int MAX_LAYERS = 12;
constexpr int LN_MAX_BLOCKS = 256;  // partial-sum slabs of the LayerNorm backward
constexpr int HC_MAX_S = 4;         // head chain kernel: most transitions per workgroup (1, 2 or 4 by batch size; online + next rows share one 16-row MFMA tile)

struct Layer {
    int kind;  // 0 conv, 1 dense
    int has_ln, has_relu, is_head;
    // conv geometry (SAME padding, dqn.py:55-69; kernel/stride fixed by the reference: 8/4, 4/2, 3/1)
    int hin, win, cin, cin_p, hout, wout, cout, cout_p, ksz, stride, pad, taps, npix;
    int is_u8;  // first conv: reads uint8 frames through the id table, K order = (plane, ky, kx)
    // dense
    int in_f, in_p;  // true / internal input width (in_p: padded to 8; after a conv torso: npix * cout_p)
    int in_unpadded_ld;  // fc first layer: the caller's obs matrix has ld = in_f
    int out_f, out_p;    // true / padded output width (conv: cout / cout_p)
    int K;               // forward contraction length (internal)
    int in_elems_p, out_elems_p;  // per-image element counts (internal)
    // parameters (float offsets into the flat buffer); -1 if absent
    int64_t w_off, b_off, g_off, be_off, w_size;
    // workspace (float offsets)
    int64_t act_off, z_off, dz_off, gw_off, part_off;
    int gw_slabs;   // split-K slabs of the weight gradient
    int fwd_splits; // dense: split-K factor of the forward GEMM
    bool fwd_narrow = false;  // dense forward on 128 x 64 tiles (S8 operands only)
    // conv: image-resident weight gradient (conv_img.h): 0 = use the generic engine
    int wgi_ntw, wgi_G, wgi_groups;
    // conv (layer >= 1): image-resident data gradient with the LayerNorm backward of the layer below fused in
    int dgi_tiles;       // workgroups per image (0 = generic engine + separate ln_bwd)
    int dgi_tile_pix;    // pixels of a class per workgroup: 128, or 64 when 128 would leave fewer than two workgroups per CU
    int64_t red_off;     // hidden layers: reduced (dgamma, dbeta, dbias) row [3][out_p]
    int part_rows;       // rows of the partial-sum region
    char name[16];
    char ln_name[16];
};

// Impala torso (architectures/dqn.py:7-36, 75-88): three Stacks.  The torso is ONE pseudo-layer (kind 2) of the layer list -- its
// output (the residual stream behind Stack_2, LayerNorm + ReLU + flatten) has the geometry of a conv layer's output, so the dense
// tail, the head chain and the fused dense data gradient treat it exactly like the cnn torso's last convolution; what is inside
// runs on the generic MFMA engine (ConvFwd / ConvDgrad / ConvWgrad problems) and a few row-wise kernels (impala.h).
constexpr int IMP_STACKS = 3, IMP_CONVS = 5;
struct ImpalaStack {
    int H, W, Hp, Wp, pool_pad;     // the first conv runs at H x W, everything behind the max-pool at Hp x Wp
    int cin, cin_p, C, C_p;
    Layer conv[IMP_CONVS];           // Conv_0 (cin -> C at H x W), Conv_1 .. Conv_4 (C -> C at Hp x Wp): geometry, parameter and slab offsets
    int64_t ln_g[2], ln_b[2];        // LayerNorm_0 / LayerNorm_1 of the two residual blocks (-1: no LayerNorm)
    // workspace (float offsets; rows of N2 images in the forward, B in the backward)
    int64_t xin_off, z0_off, arg_off, r_off[3], a1_off[2], a2_off[2], zt_off;
    int64_t dr_off, da_off, dzs_off, dz0_off, bpart_off[IMP_CONVS], lnpart_off[2];
};

// One flax.linen.BatchNorm call site (architectures/dqn.py:52-53, 59-60, 66-67, 73-74, 100-101; csrc/batchnorm.h).  The tensor it
// normalises is [rows][P][Cp] in the internal layout.  `spatial` (BatchNorm(axis=(1, 2)) on an image tensor): one statistic per pixel
// position p over the batch AND the C channels; otherwise (2-D input) one per internal column p * Cp + c over the batch.
struct BnSite {
    int layer;    // hidden layer whose post-ReLU activation it normalises (-1: the network input x / 255; -2 - (2 s + b): residual
                  // block b of impala Stack s, behind its ReLU -- dqn.py:29-30)
    int spatial;
    int P, C, Cp; // positions, channels, padded channels
    int G, G_p;   // statistic groups (spatial: P; feature: P * Cp internal columns), padded to 8
    int64_t scale_off, bias_off, mean_off, var_off;  // parameter buffer (floats): scale / bias are optimised, mean / var are the running averages
    int64_t in_off, out_off, bmean_off, bvar_off, s1_off, s2_off;  // workspace (floats): S8 input / output rows, batch statistics, backward sums
    char name[32];  // Flax module path ("BatchNorm_3", "Stack_1/BatchNorm_0")
};

struct Plan {
    ImpalaStack imp[IMP_STACKS];
    int n_layers;
    Layer L[MAX_LAYERS];
    int B, N2;
    int bn;   // cfg->batch_norm
    int Bb;   // rows the backward runs over: B (the next-state half has a zero cotangent, isdqn.py:99) -- N2 with BatchNorm, whose
              // batch statistics carry the gradient into the next-state rows
    int n_bn;
    BnSite bns[MAX_LAYERS + 1 + 2 * IMP_STACKS];
    int64_t x0_off;  // BatchNorm, cnn: the network input frames / 255 as S8 [N2][h * w][8]; fc: concat(state, next_state) fp32 [N2][obs]
    int n_heads, n_actions, nha, nha_p;
    // head layer width: nha Q-values, or nha * head_nb outputs with per-action blocks of head_nb values: the logits of the HL-Gauss
    // histogram loss (cfg->n_bins > 0) or the quantile values of QR-DQN (cfg->n_quantiles > 0; `qr` says which loss runs); `c51`:
    // the histogram heads train on the C51 categorical projection loss (cfg->categorical) instead of HL-Gauss
    int nlog, nlog_p, head_nb;
    bool qr, c51;
    float hl_min, hl_max, hl_sigma;
    // K regressed heads; head k + oh (online rows) is regressed on head k (next-state rows).  iS-DQN: n_heads = 1 + K,
    // oh = 1 (isdqn.py:96-98).  A single head (n_heads = 1) is TF-DQN: K = 1, oh = 0 -- the head is regressed on its own
    // stop-gradient target (tfdqn.py:68-80).
    int K, oh;
    int64_t n_params;
    // workspace (float offsets unless noted)
    int64_t q_off, logits_off, out_off, dout_off, da_off, slab_off, qv_off, tg_off, dbh_off, adam_tab_off, lpart_off;
    // Double Q-learning (cfg->double_q), forms with separate target parameters: head output of the target network on the B next
    // states (q_target: Q rows [B][nha_p]; histogram heads: logits_target [B][nlog_p], q_target their expectations).  -1 without
    // Munchausen targets (cfg->munchausen_tau > 0) with separate target parameters: the same regions hold the target network's head
    // output on all 2B rows, states first (qt_rows = 2B; B with double_q; 0 without either option)
    int double_q, qt_rows;
    bool munchausen;
    int64_t qt_off, logits_t_off, out_t_off;
    // Dueling heads (cfg->dueling; csrc/dueling.h): the head Dense writes raw rows of raw_p = (n_heads * (A + 1) * w padded to 8)
    // values into "head_raw" / "head_raw_target", duel_combine_kernel turns them into the rows at out_off / out_t_off; the loss
    // kernels' dout / dbh go through duel_backward_kernel into "dout_raw" / "dbh_raw", where the head's backward starts.  -1 without
    int dueling, raw, raw_p, duel_f, duel_f2;  // duel_f: width of the last hidden Dense, duel_f2: its half (the value stream)
    int64_t raw_off, raw_t_off, dout_raw_off, dbh_raw_off;
    // Global-norm gradient clipping (cfg->max_grad_norm > 0; csrc/grad_clip.h): "grad_clip_partials" holds one float64 sum of squares
    // per workgroup of grad_reduce_sq_kernel / grad_flat_sq_kernel (gc_part_cap of them: every tensor rounded up to whole workgroups of 64),
    // "grad_clip" the four floats of include/isdqn_hip.h.  -1 without
    bool grad_clip;
    int64_t gc_part_off, gc_off, gc_part_cap;
    int64_t wsplit_off;  // S8 mirror of the parameter buffer (same offsets as the fp32 master; weights only are read from it)
    int64_t slab_floats, da_floats;
    int64_t ws_bytes;
    std::vector<std::pair<std::string, std::pair<int64_t, int64_t>>> regions;  // name -> (byte offset, byte size)
};

static inline void same_padding(int size, int k, int s, int& out, int& lo) {
    out = (size + s - 1) / s;
    int total = (out - 1) * s + k - size;
    if (total < 0) total = 0;
    lo = total / 2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// build_plan, phase by phase.  Every phase is a free function of the configuration and of what the phases before it left in the
// plan; the order of the checks -- which refusal answers when two are violated -- is part of the interface
// (tests/test_plan_snapshot_host.py holds messages, codes, their order and every field to a recorded snapshot).
// ---------------------------------------------------------------------------------------------------------------------------------

// Phase 1: what the configuration alone decides.
static inline int check_options(const isdqn_net_config* cfg) {
    ISDQN_REQUIRE(cfg != nullptr, ISDQN_ERR_ARG, "null config");
    ISDQN_REQUIRE(cfg->arch == ISDQN_ARCH_CNN || cfg->arch == ISDQN_ARCH_FC || cfg->arch == ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED,
                  "architecture_type must be cnn, impala or fc");
    ISDQN_REQUIRE(cfg->n_features >= (cfg->arch == ISDQN_ARCH_FC ? 0 : 3) && cfg->n_features <= ISDQN_MAX_FEATURES,
                  ISDQN_ERR_ARG, "bad n_features");
    ISDQN_REQUIRE(cfg->n_actions >= 1 && cfg->n_heads >= 1, ISDQN_ERR_ARG, "need n_actions >= 1 and n_heads >= 1");
    ISDQN_REQUIRE(cfg->batch_size >= 1 && cfg->batch_size <= 4096, ISDQN_ERR_ARG, "batch_size must be in [1, 4096]");
    ISDQN_REQUIRE(cfg->precision == ISDQN_PRECISION_BF16X3 || cfg->precision == ISDQN_PRECISION_BF16, ISDQN_ERR_ARG,
                  "bad precision");
    ISDQN_REQUIRE(cfg->huber_delta >= 0.f, ISDQN_ERR_ARG, "huber_delta must be >= 0 (0 = squared error)");
    ISDQN_REQUIRE(cfg->max_grad_norm >= 0.f, ISDQN_ERR_ARG, "max_grad_norm must be >= 0 (0 = off, inf = measure only)");  // (NaN fails too)
    ISDQN_REQUIRE(cfg->batch_norm == 0 || cfg->batch_norm == 1, ISDQN_ERR_ARG, "batch_norm must be 0 or 1");
    ISDQN_REQUIRE(cfg->double_q == 0 || cfg->double_q == 1, ISDQN_ERR_ARG, "double_q must be 0 or 1");
    ISDQN_REQUIRE(std::isfinite(cfg->munchausen_tau) && cfg->munchausen_tau >= 0.f, ISDQN_ERR_ARG, "munchausen_tau must be finite and >= 0 (0 = off)");
    if (cfg->munchausen_tau > 0.f) {
        ISDQN_REQUIRE(cfg->munchausen_alpha >= 0.f && cfg->munchausen_alpha <= 1.f, ISDQN_ERR_ARG, "munchausen_alpha must be in [0, 1]");
        ISDQN_REQUIRE(std::isfinite(cfg->munchausen_clip) && cfg->munchausen_clip <= 0.f, ISDQN_ERR_ARG, "munchausen_clip must be finite and <= 0");
        ISDQN_REQUIRE(cfg->double_q == 0, ISDQN_ERR_ARG, "double_q and munchausen_tau > 0 exclude each other (the soft value has no argmax to decouple)");
    }
    ISDQN_REQUIRE(cfg->n_quantiles == 0 || (cfg->n_quantiles >= 2 && cfg->n_quantiles <= 256), ISDQN_ERR_ARG,
                  "n_quantiles must be 0 (off) or in [2, 256]");
    if (cfg->n_quantiles > 0) {  // (huber_delta > 0 is allowed here: it is kappa)
        ISDQN_REQUIRE(cfg->n_bins == 0, ISDQN_ERR_ARG, "n_quantiles > 0 and the histogram loss (n_bins > 0) exclude each other");
        ISDQN_REQUIRE(cfg->munchausen_tau == 0.f, ISDQN_ERR_UNSUPPORTED,
                      "n_quantiles > 0: Munchausen targets (munchausen_tau > 0) are not built for quantile heads");
        ISDQN_REQUIRE(cfg->batch_norm == 0, ISDQN_ERR_UNSUPPORTED, "n_quantiles > 0: quantile heads are not built for BatchNorm networks");
    }
    ISDQN_REQUIRE(cfg->n_bins == 0 || (cfg->n_bins >= 2 && cfg->n_bins <= 256), ISDQN_ERR_ARG, "n_bins must be 0 (off) or in [2, 256]");
    ISDQN_REQUIRE(cfg->categorical == 0 || cfg->categorical == 1, ISDQN_ERR_ARG, "categorical must be 0 or 1");
    if (cfg->categorical == 1) {  // (huber_delta, batch_norm and the size limits: refused below, as the histogram heads refuse them)
        ISDQN_REQUIRE(cfg->n_quantiles == 0, ISDQN_ERR_ARG, "categorical = 1 and n_quantiles > 0 exclude each other");
        ISDQN_REQUIRE(cfg->n_bins > 0, ISDQN_ERR_ARG, "categorical = 1 needs the histogram heads (n_bins > 0)");
        ISDQN_REQUIRE(cfg->munchausen_tau == 0.f, ISDQN_ERR_UNSUPPORTED,
                      "categorical = 1: Munchausen targets (munchausen_tau > 0) are not built for the categorical loss");
    }
    if (cfg->n_bins > 0) {
        ISDQN_REQUIRE(cfg->hl_max > cfg->hl_min, ISDQN_ERR_ARG, "histogram loss: hl_max must be > hl_min");
        ISDQN_REQUIRE(cfg->categorical == 1 || cfg->hl_sigma > 0.f, ISDQN_ERR_ARG, "histogram loss: hl_sigma must be > 0");
        ISDQN_REQUIRE(cfg->huber_delta == 0.f, ISDQN_ERR_ARG, "huber_delta and the histogram loss (n_bins > 0) exclude each other");
        ISDQN_REQUIRE(cfg->batch_norm == 0, ISDQN_ERR_UNSUPPORTED, "the histogram loss is not built for BatchNorm networks");
    }
    return ISDQN_OK;
}

// Phase 2: batch rows, head geometry and the limits that depend on it.  Runs in front of every torso check.
static inline int plan_heads(const isdqn_net_config* cfg, Plan& P) {
    P.B = cfg->batch_size;
    P.N2 = 2 * P.B;
    P.bn = cfg->batch_norm;
    P.Bb = P.bn ? P.N2 : P.B;
    P.x0_off = -1;
    P.n_heads = cfg->n_heads;
    P.K = cfg->n_heads >= 2 ? cfg->n_heads - 1 : 1;
    P.oh = cfg->n_heads >= 2 ? 1 : 0;
    P.n_actions = cfg->n_actions;
    P.nha = cfg->n_heads * cfg->n_actions;
    P.nha_p = round_up(P.nha, 8);
    P.qr = cfg->n_quantiles > 0;
    P.c51 = cfg->categorical == 1;
    P.head_nb = P.qr ? cfg->n_quantiles : cfg->n_bins;
    P.hl_min = cfg->hl_min; P.hl_max = cfg->hl_max; P.hl_sigma = cfg->hl_sigma;
    P.nlog = P.head_nb > 0 ? P.nha * P.head_nb : P.nha;
    P.nlog_p = round_up(P.nlog, 8);
    ISDQN_REQUIRE(P.qr || P.head_nb == 0 || P.K <= 64, ISDQN_ERR_UNSUPPORTED, "the histogram loss is built for at most 64 regressed heads");
    ISDQN_REQUIRE(!P.qr || P.K <= 64, ISDQN_ERR_UNSUPPORTED, "n_quantiles > 0: the quantile loss is built for at most 64 regressed heads");
    // (dense_post_kernel stages a whole head row, bias and LayerNorm rows in 64 KB of LDS: 3 * 5456 floats)
    ISDQN_REQUIRE(P.qr || P.head_nb == 0 || P.nlog <= 5456, ISDQN_ERR_UNSUPPORTED, "histogram heads: n_heads * n_actions * n_bins must be <= 5456");
    ISDQN_REQUIRE(!P.qr || P.nlog <= 5456, ISDQN_ERR_UNSUPPORTED, "quantile heads: n_heads * n_actions * n_quantiles must be <= 5456");
    ISDQN_REQUIRE(cfg->dueling == 0 || cfg->dueling == 1, ISDQN_ERR_ARG, "dueling must be 0 or 1");
    P.dueling = cfg->dueling;
    P.raw = P.dueling ? cfg->n_heads * (cfg->n_actions + 1) * (P.head_nb > 0 ? P.head_nb : 1) : 0;
    P.raw_p = round_up(P.raw, 8);
    if (P.dueling) {
        ISDQN_REQUIRE(cfg->batch_norm == 0, ISDQN_ERR_UNSUPPORTED, "dueling heads are not built for BatchNorm networks");
        ISDQN_REQUIRE(cfg->arch != ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED, "dueling heads are not built for the impala torso");
        ISDQN_REQUIRE(P.K <= 64, ISDQN_ERR_UNSUPPORTED, "dueling heads are built for at most 64 regressed heads");
        ISDQN_REQUIRE(P.head_nb == 0 || P.raw <= 5456, ISDQN_ERR_UNSUPPORTED,
                      "dueling histogram / quantile heads: n_heads * (n_actions + 1) * width must be <= 5456");
        ISDQN_REQUIRE(cfg->n_features > (cfg->arch == ISDQN_ARCH_FC ? 0 : 3), ISDQN_ERR_ARG, "dueling heads need a hidden Dense in front of the head");
        P.duel_f = cfg->features[cfg->n_features - 1];
        ISDQN_REQUIRE(P.duel_f >= 2 && P.duel_f % 2 == 0, ISDQN_ERR_ARG, "dueling heads: the last hidden Dense must have an even width");
        P.duel_f2 = P.duel_f / 2;
    }
    P.grad_clip = cfg->max_grad_norm > 0.f;
    if (P.grad_clip) {  // (their learn paths -- bn_learn_or_loss, impala_backward -- run optimizer launches of their own)
        ISDQN_REQUIRE(cfg->batch_norm == 0, ISDQN_ERR_UNSUPPORTED, "gradient clipping is not built for BatchNorm networks");
        ISDQN_REQUIRE(cfg->arch != ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED, "gradient clipping is not built for the impala torso");
    }
    P.double_q = cfg->double_q;
    P.munchausen = cfg->munchausen_tau > 0.f;
    P.qt_rows = P.munchausen ? P.N2 : P.double_q ? P.B : 0;
    return ISDQN_OK;
}

// Phase 3: torso and dense tail, layer by layer in Flax's order.  The only state the layers share: where the next parameter tensor
// goes and how many modules of each class Flax has named so far.
struct ParamCursor {
    int64_t poff = 0;
    int n_conv = 0, n_dense = 0, n_ln = 0;
    int n_bn_top = 0;  // (Flax counts BatchNorm modules per parent: the Stacks' own ones are "Stack_s/BatchNorm_b")
};
// what the first Dense reads: true / internal width and per-image element count
struct DenseInput { int f, p, elems_p; };

static inline void place_kernel_bias(ParamCursor& cur, Layer& l) {
    l.w_off = cur.poff; cur.poff += l.w_size;
    l.b_off = cur.poff; cur.poff += l.out_p;
}
// LayerNorm scale and bias of `width` floats each (-1 without)
static inline void place_layer_norm(ParamCursor& cur, bool has_ln, int width, int64_t& g_off, int64_t& be_off) {
    g_off = be_off = -1;
    if (!has_ln) return;
    g_off = cur.poff; cur.poff += width;
    be_off = cur.poff; cur.poff += width;
}
// a layer's own LayerNorm, a module of the network's top level: "LayerNorm_n"
static inline void place_named_layer_norm(ParamCursor& cur, Layer& l) {
    place_layer_norm(cur, l.has_ln, l.out_p, l.g_off, l.be_off);
    if (l.has_ln) snprintf(l.ln_name, sizeof(l.ln_name), "LayerNorm_%d", cur.n_ln++);
}

// BatchNorm_i in call order (Flax auto-names per class): scale and bias join the optimised parameters here, the running
// averages are placed behind all of them (place_batch_stats)
static inline void add_bn(Plan& P, ParamCursor& cur, int layer, int spatial, int Pn, int C, int Cp, const char* name = nullptr) {
    BnSite& b = P.bns[P.n_bn++];
    b.layer = layer; b.spatial = spatial; b.P = Pn; b.C = C; b.Cp = Cp;
    b.G = spatial ? Pn : Pn * Cp;
    b.G_p = round_up(b.G, 8);
    b.scale_off = cur.poff; cur.poff += b.G_p;
    b.bias_off = cur.poff; cur.poff += b.G_p;
    if (name) snprintf(b.name, sizeof(b.name), "%s", name);
    else snprintf(b.name, sizeof(b.name), "BatchNorm_%d", cur.n_bn_top++);
}
static inline void place_batch_stats(Plan& P, ParamCursor& cur) {  // batch_stats (running mean / var): behind every optimised tensor
    for (int s = 0; s < P.n_bn; ++s) {
        P.bns[s].mean_off = cur.poff; cur.poff += P.bns[s].G_p;
        P.bns[s].var_off = cur.poff; cur.poff += P.bns[s].G_p;
    }
    P.n_params = cur.poff;
}

// Geometry of a SAME convolution (cin -> cout channels at h x w, k x k taps): everything of the Layer that follows from the shape.
// Returns the left padding along w; the callers refuse one that differs from l.pad.
static inline int conv_geometry(Layer& l, int h, int w, int cin, int cin_p, int cout, int k, int stride, bool is_u8) {
    l.kind = 0;
    l.is_u8 = is_u8;
    l.hin = h; l.win = w; l.cin = cin; l.cin_p = cin_p;
    l.ksz = k; l.stride = stride; l.taps = k * k;
    int pad_w;
    same_padding(h, k, stride, l.hout, l.pad);
    same_padding(w, k, stride, l.wout, pad_w);
    l.cout = cout;
    l.cout_p = round_up(cout, 8);
    l.npix = l.hout * l.wout;
    l.out_f = l.cout; l.out_p = l.cout_p;
    l.K = is_u8 ? cin * 64 : l.taps * cin_p;
    l.in_elems_p = h * w * cin_p;
    l.out_elems_p = l.npix * l.cout_p;
    l.w_size = (int64_t)l.cout_p * l.K;
    return pad_w;
}

static inline int plan_cnn_torso(const isdqn_net_config* cfg, Plan& P, ParamCursor& cur, DenseInput& in) {
    static const int KS[3] = {8, 4, 3}, ST[3] = {4, 2, 1};  // kernel / stride fixed by the reference (dqn.py:55-69)
    ISDQN_REQUIRE(cfg->obs_h >= 8 && cfg->obs_w >= 8 && cfg->obs_c >= 1 && cfg->obs_c <= 16, ISDQN_ERR_ARG,
                  "bad observation shape");
    int h = cfg->obs_h, w = cfg->obs_w, c = cfg->obs_c, c_p = cfg->obs_c;
    if (P.bn) {  // dqn.py:52-53: the first convolution reads BatchNorm(x / 255): S8 rows of 8-padded channels, generic K order
        ISDQN_REQUIRE(cfg->obs_c <= 8, ISDQN_ERR_UNSUPPORTED, "BatchNorm: at most 8 stacked frames");
        c_p = 8;
        add_bn(P, cur, -1, 1, h * w, c, c_p);
    }
    for (int i = 0; i < 3; ++i) {
        Layer& l = P.L[P.n_layers++];
        l.has_ln = cfg->layer_norm ? 1 : 0;
        l.has_relu = 1;
        const int pad_w = conv_geometry(l, h, w, c, c_p, cfg->features[i], KS[i], ST[i], i == 0 && !P.bn);
        ISDQN_REQUIRE(pad_w == l.pad, ISDQN_ERR_UNSUPPORTED, "non-square padding is not supported");
        ISDQN_REQUIRE(l.cout >= 1 && l.cout <= 64, ISDQN_ERR_UNSUPPORTED,
                      "conv widths above 64 channels are not supported by the fused LayerNorm epilogue");
        snprintf(l.name, sizeof(l.name), "Conv_%d", cur.n_conv++);
        place_kernel_bias(cur, l);
        place_named_layer_norm(cur, l);
        // dqn.py:59-60, 66-67: BatchNorm(axis=(1, 2)) behind the first two ReLUs; :72-74: behind the flatten (a 2-D tensor: per feature)
        if (P.bn) add_bn(P, cur, i, i < 2 ? 1 : 0, l.npix, l.cout, l.cout_p);
        h = l.hout; w = l.wout; c = l.cout; c_p = l.cout_p;
    }
    in = {h * w * c, h * w * c_p, h * w * c_p};
    return ISDQN_OK;
}

// one 3 x 3 convolution of a Stack: no LayerNorm or ReLU of its own (the Stack's row-wise kernels run them)
static inline void plan_impala_conv(ParamCursor& cur, Layer& l, int h, int w, int cin, int cin_p, int cout, int index) {
    conv_geometry(l, h, w, cin, cin_p, cout, 3, 1, false);
    snprintf(l.name, sizeof(l.name), "Conv_%d", index);
    place_kernel_bias(cur, l);
    l.g_off = l.be_off = -1;
}

static inline int plan_impala_torso(const isdqn_net_config* cfg, Plan& P, ParamCursor& cur, DenseInput& in) {
    ISDQN_REQUIRE(cfg->obs_h >= 8 && cfg->obs_w >= 8 && cfg->obs_c >= 1 && cfg->obs_c <= 8, ISDQN_ERR_ARG, "bad observation shape");
    int h = cfg->obs_h, w = cfg->obs_w, c = cfg->obs_c, c_p = 8;
    if (P.bn) add_bn(P, cur, -1, 1, h * w, c, c_p);  // dqn.py:78-79
    for (int s = 0; s < IMP_STACKS; ++s) {
        ImpalaStack& S = P.imp[s];
        S.H = h; S.W = w; S.cin = c; S.cin_p = c_p;
        S.C = cfg->features[s];
        ISDQN_REQUIRE(S.C >= 1 && S.C <= 64, ISDQN_ERR_UNSUPPORTED, "impala stack widths above 64 channels are not supported");
        S.C_p = round_up(S.C, 8);
        int pw;
        same_padding(h, 3, 2, S.Hp, S.pool_pad);
        same_padding(w, 3, 2, S.Wp, pw);
        ISDQN_REQUIRE(pw == S.pool_pad, ISDQN_ERR_UNSUPPORTED, "non-square observations are not supported by the impala torso");
        // parameters in Flax's order inside a Stack: Conv_0, then per block LayerNorm_b, Conv_{1+2b}, Conv_{2+2b} (dqn.py:17-34)
        plan_impala_conv(cur, S.conv[0], h, w, c, c_p, S.C, 0);
        for (int b = 0; b < 2; ++b) {
            place_layer_norm(cur, cfg->layer_norm != 0, S.C_p, S.ln_g[b], S.ln_b[b]);
            if (P.bn) {  // dqn.py:29-30: BatchNorm(axis=(1, 2)) behind the block's ReLU
                char nm[32];
                snprintf(nm, sizeof(nm), "Stack_%d/BatchNorm_%d", s, b);
                add_bn(P, cur, -2 - (2 * s + b), 1, S.Hp * S.Wp, S.C, S.C_p, nm);
            }
            for (int k = 1 + 2 * b; k <= 2 + 2 * b; ++k) plan_impala_conv(cur, S.conv[k], S.Hp, S.Wp, S.C, S.C_p, S.C, k);
        }
        h = S.Hp; w = S.Wp; c = S.C; c_p = S.C_p;
    }
    // the torso as one pseudo-layer: output geometry of a conv layer, the LayerNorm behind the last Stack as its LayerNorm
    Layer& l = P.L[P.n_layers++];
    l.kind = 2;
    l.has_ln = cfg->layer_norm ? 1 : 0;
    l.has_relu = 1;
    l.hin = cfg->obs_h; l.win = cfg->obs_w; l.cin = cfg->obs_c; l.cin_p = 8;
    l.hout = h; l.wout = w; l.cout = c; l.cout_p = c_p; l.npix = h * w;
    l.out_f = c; l.out_p = c_p;
    l.in_elems_p = cfg->obs_h * cfg->obs_w * 8;
    l.out_elems_p = l.npix * c_p;
    l.w_size = 0; l.w_off = -1; l.b_off = -1;
    snprintf(l.name, sizeof(l.name), "Impala");
    place_named_layer_norm(cur, l);
    if (P.bn) add_bn(P, cur, P.n_layers - 1, 0, l.npix, l.cout, l.cout_p);  // dqn.py:86-88: per feature behind the flatten
    in = {h * w * c, h * w * c_p, h * w * c_p};
    return ISDQN_OK;
}

static inline int plan_fc_input(const isdqn_net_config* cfg, DenseInput& in) {
    ISDQN_REQUIRE(cfg->obs_c >= 1, ISDQN_ERR_ARG, "bad observation dim");
    in = {cfg->obs_c, round_up(cfg->obs_c, 8), round_up(cfg->obs_c, 8)};
    return ISDQN_OK;
}

// the hidden Dense layers and the head
static inline int plan_dense_tail(const isdqn_net_config* cfg, Plan& P, ParamCursor& cur, DenseInput in) {
    const int first_dense = cfg->arch == ISDQN_ARCH_FC ? 0 : 3;
    for (int i = first_dense; i <= cfg->n_features; ++i) {
        ISDQN_REQUIRE(P.n_layers < MAX_LAYERS, ISDQN_ERR_ARG, "too many layers");
        Layer& l = P.L[P.n_layers++];
        l.kind = 1;
        l.is_head = (i == cfg->n_features);
        l.has_ln = (!l.is_head && cfg->layer_norm) ? 1 : 0;
        l.has_relu = l.is_head ? 0 : 1;
        l.in_f = in.f; l.in_p = in.p;
        l.in_unpadded_ld = (cfg->arch == ISDQN_ARCH_FC && i == 0) ? in.f : 0;
        l.out_f = l.is_head ? (P.dueling ? P.raw : P.nlog) : cfg->features[i];
        // what the row-wise kernels behind a Dense run: ln_bwd_wide_kernel holds 16 columns per thread (256 * LN_WIDE_MAX_COLS,
        // row_kernels.h), dense_post_kernel stages a head row with its bias and LayerNorm rows in 64 KB of LDS (3 * 5456 floats)
        ISDQN_REQUIRE(l.out_f >= 1 && l.out_f <= (l.is_head ? 5456 : 4096), ISDQN_ERR_ARG, "bad dense width");
        l.out_p = round_up(l.out_f, 8);
        l.K = l.in_p;
        l.in_elems_p = in.elems_p;
        l.out_elems_p = l.out_p;
        l.w_size = (int64_t)l.out_p * l.in_p;
        snprintf(l.name, sizeof(l.name), "Dense_%d", cur.n_dense++);
        place_kernel_bias(cur, l);
        place_named_layer_norm(cur, l);
        if (P.bn && !l.is_head) add_bn(P, cur, P.n_layers - 1, 0, 1, l.out_f, l.out_p);  // dqn.py:100-101
        in = {l.out_f, l.out_p, l.out_p};
    }
    return ISDQN_OK;
}

// Phase 4: the tiling decisions of the forward and backward pass -- pure functions of a layer and of B / Bb / N2.

// conv weight gradient on the generic engine: split the contraction (online pixels) over about 256 workgroups
static inline int conv_wgrad_split(const Layer& l, int Bb) {
    int tiles_n = ceil_div(l.K, 64);
    int ksteps = ceil_div(Bb * l.npix, 32);
    int s = 256 / tiles_n;
    if (s < 1) s = 1;
    if (s > ksteps) s = ksteps;
    return s;
}

// conv (layer >= 1): image-resident data gradient, dgi_tiles workgroups per image (0: generic engine + separate ln_bwd)
static inline void plan_conv_dgrad_tiles(Layer& l, int Bb) {
    if (l.ksz % l.stride != 0 || l.cout_p > 64 || l.cin_p > 64) return;
    auto tiles_of = [&](int tile_pix) {
        int tiles = 0;
        for (int c = 0; c < l.stride * l.stride; ++c) {
            int cy = c / l.stride, cx = c % l.stride;
            int Ha = (l.hin - cy + l.stride - 1) / l.stride, Wb = (l.win - cx + l.stride - 1) / l.stride;
            tiles += ceil_div(Ha * Wb, tile_pix);
        }
        return tiles;
    };
    l.dgi_tile_pix = Bb * tiles_of(128) < ISDQN_DGRAD_TILE64_BELOW ? 64 : 128;  // (the switch and its measurement: top of this file)
    l.dgi_tiles = tiles_of(l.dgi_tile_pix);
}

// conv: image-resident weight gradient (conv_img.h): column groups of 64*NTW k' columns x groups of G images ~ 256 workgroups.
// May raise gw_slabs: one slab per group of images.
static inline void plan_conv_wgrad_image(Layer& l, int Bb) {
    if (l.K % 64 != 0 || !(l.is_u8 || l.cin_p % 16 == 0)) return;
    int ntw = (l.K % 256 == 0) ? 4 : (l.K % 192 == 0) ? 3 : (l.K % 128 == 0) ? 2 : 0;
    if (l.K == 512) ntw = 2;
    // 64 output channels and K <= 576: one workgroup owns every k' column (8 or 9 column tiles per
    // wave), so each image pair is staged into LDS exactly once instead of once per column group
    const bool wide = l.cout_p == 64 && !l.is_u8 && (l.K == 512 || l.K == 576);
    if (wide) ntw = l.K / 64;
    if (!ntw) return;
    int ncg = l.K / (64 * ntw);
    int G = (Bb * ncg + 255) / 256;
    // two images per workgroup at the headline batch (measured best, 1: 2681, 2: 2806 steps/s: 128 workgroups share
    // the CUs with the data-gradient chain); larger batches keep at least one workgroup per CU instead of 128
    // workgroups of 8 images (c5: conv2 / conv1 weight gradients 74 / 66 us on half the chip)
    if (wide) G = (Bb + 127) / 128;
#if !defined(ISDQN_WGRAD_G128)
    if (wide && G > 2) G = std::max(2, (Bb + 255) / 256);
#endif
    if (G < 1) G = 1;
    l.wgi_ntw = ntw;
    l.wgi_G = G;
    l.wgi_groups = ceil_div(Bb, G);
    if (l.wgi_groups > l.gw_slabs) l.gw_slabs = l.wgi_groups;
}

// dense: split-K slabs of the weight gradient (batch rows) and of the forward GEMM; returns the floats of forward slabs it needs
static inline int64_t plan_dense_tiling(Layer& l, int Bb, int N2) {
    int tiles = ceil_div(l.out_p, 128) * ceil_div(l.in_p, 128);
    int ksteps = ceil_div(Bb, 32);
    int s = tiles >= 128 ? 1 : 256 / tiles;
    if (s > ksteps) s = ksteps;
    if (s < 1) s = 1;
    l.gw_slabs = s;
    // forward split-K slabs
    // ~512 workgroups (two per CU hide each other's operand latency).  A GEMM of few 128 x 128 tiles gets there with
    // 128 x 64 tiles and half the split-K slabs: same time at the headline size, 32 MB less slab traffic per step.
    int ft = ceil_div(N2, 128) * ceil_div(l.out_p, 128);
    l.fwd_narrow = ft <= 64 && !l.in_unpadded_ld && l.out_p % 64 == 0;
    if (l.fwd_narrow) ft = ceil_div(N2, 128) * ceil_div(l.out_p, 64);
    int fs = ft >= 256 ? 1 : 512 / ft;
    int fk = ceil_div(l.K, 32);
#if defined(ISDQN_DEV)
    if (const char* e = getenv("ISDQN_FWD_SPLITS")) fs = atoi(e);  // development: split-K factor of the forward GEMM
#endif
    if (fs > fk) fs = fk;
    if (fs < 1) fs = 1;
    l.fwd_splits = fs;
    return (int64_t)fs * N2 * l.out_p;
}

// rows of a hidden layer's partial-sum region ("part/"): the most any kernel that reduces into it emits
static inline int part_rows_of(const Plan& P, int i) {
    const Layer& l = P.L[i];
    int rows = LN_MAX_BLOCKS;
    if (l.kind == 1 && P.B > rows) rows = P.B;  // head chain: one row per workgroup, as few as one transition each
    if (i + 1 < P.n_layers && P.L[i + 1].dgi_tiles > 0 && P.B * P.L[i + 1].dgi_tiles > rows) rows = P.B * P.L[i + 1].dgi_tiles;
    // conv layer under the first dense layer: the fused dense data-gradient + LN backward emits one partial
    // row per (64-sample tile, pixel)
    if (l.kind != 1 && i + 1 < P.n_layers && P.L[i + 1].kind == 1 && l.cout_p == 64 && ceil_div(P.B, 64) * l.npix > rows)
        rows = ceil_div(P.B, 64) * l.npix;
    return rows;
}

static inline void plan_tiling(const isdqn_net_config* cfg, Plan& P) {
    for (int i = 0; i < P.n_layers; ++i) {
        Layer& l = P.L[i];
        // (BatchNorm: the first convolution's data gradient is needed too -- the input BatchNorm's scale / bias gradient)
        if (i > 0 || (P.bn && l.kind == 0)) P.da_floats = std::max(P.da_floats, (int64_t)P.Bb * l.in_elems_p);
        if (l.kind == 0) {
            if (i > 0) plan_conv_dgrad_tiles(l, P.Bb);
            l.gw_slabs = conv_wgrad_split(l, P.Bb);
            plan_conv_wgrad_image(l, P.Bb);
        } else if (l.kind == 1) {
            P.slab_floats = std::max(P.slab_floats, plan_dense_tiling(l, P.Bb, P.N2));
        }
    }
    for (int i = 0; i < P.n_layers; ++i)  // (behind the loop above: a layer's rows depend on the tiling of the layer that consumes it)
        if (!P.L[i].is_head) P.L[i].part_rows = part_rows_of(P, i);
    if (cfg->arch == ISDQN_ARCH_IMPALA)
        for (int s = 0; s < IMP_STACKS; ++s)
            for (int k = 0; k < IMP_CONVS; ++k) P.imp[s].conv[k].gw_slabs = conv_wgrad_split(P.imp[s].conv[k], P.Bb);
}

// Phase 5: the workspace map.  Placement only, and the order is the layout: every offset depends on it.
struct RegionCursor {
    Plan& P;
    int64_t off = 0;  // floats
    int64_t operator()(const std::string& name, int64_t floats) {
        int64_t o = off;
        floats = (floats + 63) / 64 * 64;  // 256-B granules
        P.regions.push_back({name, {o * 4, floats * 4}});
        off += floats;
        return o;
    }
};

// per layer: act, z, dz, red, gw; then every hidden layer's partial sums
static inline void place_layer_regions(Plan& P, RegionCursor& region) {
    for (int i = 0; i < P.n_layers; ++i) {
        Layer& l = P.L[i];
        l.act_off = l.z_off = l.dz_off = l.part_off = -1;
        if (!l.is_head) {
            l.act_off = region(std::string("act/") + l.name, (int64_t)P.N2 * l.out_elems_p);
            l.z_off = region(std::string("z/") + l.name, (int64_t)P.Bb * l.out_elems_p);
            l.dz_off = region(std::string("dz/") + l.name, (int64_t)P.Bb * l.out_elems_p);
            l.red_off = region(std::string("red/") + l.name, 3 * (int64_t)l.out_p);
        }
        l.gw_off = region(std::string("gw/") + l.name, (int64_t)l.gw_slabs * l.w_size);
    }
    for (int i = 0; i < P.n_layers; ++i) {
        Layer& l = P.L[i];
        if (!l.is_head) l.part_off = region(std::string("part/") + l.name, (int64_t)l.part_rows * 3 * l.out_p);
    }
}

static inline void place_impala_regions(Plan& P, RegionCursor& region) {
    for (int s = 0; s < IMP_STACKS; ++s) {
        ImpalaStack& S = P.imp[s];
        const std::string pre = "imp/s" + std::to_string(s) + "/";
        const int64_t big = (int64_t)S.H * S.W, small = (int64_t)S.Hp * S.Wp;
        S.xin_off = region(pre + "xin", P.N2 * big * S.cin_p);
        S.z0_off = region(pre + "z0", P.N2 * big * S.C_p);
        S.arg_off = region(pre + "argmax", (P.N2 * small * S.C_p + 3) / 4);
        for (int k = 0; k < 3; ++k) S.r_off[k] = region(pre + "r" + std::to_string(k), P.N2 * small * S.C_p);
        for (int b = 0; b < 2; ++b) {
            S.a1_off[b] = region(pre + "a1_" + std::to_string(b), P.N2 * small * S.C_p);
            S.a2_off[b] = region(pre + "a2_" + std::to_string(b), P.N2 * small * S.C_p);
            S.lnpart_off[b] = region(pre + "lnpart" + std::to_string(b), (int64_t)LN_MAX_BLOCKS * 2 * S.C_p);
        }
        S.zt_off = region(pre + "zt", P.N2 * small * S.C_p);
        S.dr_off = region(pre + "dr", P.Bb * small * S.C_p);
        S.da_off = region(pre + "da", P.Bb * std::max(big * S.cin_p, small * S.C_p));
        S.dzs_off = region(pre + "dzs", P.Bb * big * S.C_p);
        S.dz0_off = region(pre + "dz0", P.Bb * big * S.C_p);
        for (int k = 0; k < IMP_CONVS; ++k) {
            Layer& c = S.conv[k];
            S.bpart_off[k] = region(pre + "bpart" + std::to_string(k), (int64_t)LN_MAX_BLOCKS * S.C_p);
            c.gw_off = region(pre + "gw" + std::to_string(k), (int64_t)c.gw_slabs * c.w_size);
        }
    }
}

static inline void place_bn_regions(Plan& P, RegionCursor& region) {
    for (int s = 0; s < P.n_bn; ++s) {
        BnSite& b = P.bns[s];
        const std::string pre = std::string("bn/") + b.name + "/";
        const int64_t width = (int64_t)b.P * b.Cp;
        if (b.layer == -1) {
            P.x0_off = region("bn/x0", (int64_t)P.N2 * width);
            b.in_off = P.x0_off;
        } else if (b.layer <= -2) {  // impala block: the S8 output of its [LayerNorm +] ReLU
            const int sb = -2 - b.layer;
            b.in_off = P.imp[sb / 2].a1_off[sb % 2];
        } else {
            b.in_off = P.L[b.layer].act_off;
        }
        b.out_off = region(pre + "out", (int64_t)P.N2 * width);
        b.bmean_off = region(pre + "mean", b.G_p);
        b.bvar_off = region(pre + "var", b.G_p);
        b.s1_off = region(pre + "dbias", b.G_p);
        b.s2_off = region(pre + "dscale", b.G_p);
    }
}

static inline void plan_workspace(const isdqn_net_config* cfg, Plan& P) {
    RegionCursor region{P};
    place_layer_regions(P, region);
    if (cfg->arch == ISDQN_ARCH_IMPALA) place_impala_regions(P, region);
    place_bn_regions(P, region);
    if (P.bn && cfg->arch == ISDQN_ARCH_FC)  // concat(state, next_state) as one matrix (the first layer's weight gradient contracts over all 2B rows)
        P.x0_off = region("bn/x0", (int64_t)P.N2 * P.L[0].in_f);
    P.q_off = region("q", (int64_t)P.N2 * P.nha_p);
    // the head layer's output rows [2B][nlog_p]: the Q-values themselves, or the histogram logits / quantile values (the "q" rows then
    // hold their expectations / means, written by hl_expect_kernel / qr_expect_kernel for forward / best_action(s))
    P.logits_off = P.head_nb > 0 ? region("logits", (int64_t)P.N2 * P.nlog_p) : -1;
    P.out_off = P.head_nb > 0 ? P.logits_off : P.q_off;
    P.dout_off = region("dout", (int64_t)P.Bb * P.nlog_p);
    P.da_off = region("da", P.da_floats);
    P.slab_off = region("slab", P.slab_floats);
    P.qv_off = region("q_values", (int64_t)P.B * P.K);
    P.tg_off = region("targets", (int64_t)P.B * P.K);
    P.dbh_off = region("dbh", P.nlog_p);
    P.adam_tab_off = region("adam_consts", 64);
    P.lpart_off = region("loss_partials", (int64_t)P.B * (P.K + P.nlog_p));
    P.wsplit_off = region("wsplit", P.n_params);
    // (appended: a configuration without the option keeps every offset and the total it had.  The plan does not know whether the
    // caller will pass target parameters, so the regions exist with the option whatever the form: only the *_target entry points
    // and grad_on_batch with target_params read them, iS-DQN / TF-DQN learn steps leave them untouched)
    P.qt_off = P.qt_rows ? region("q_target", (int64_t)P.qt_rows * P.nha_p) : -1;
    P.logits_t_off = (P.qt_rows && P.head_nb > 0) ? region("logits_target", (int64_t)P.qt_rows * P.nlog_p) : -1;
    P.out_t_off = P.head_nb > 0 ? P.logits_t_off : P.qt_off;
    // (dueling heads: appended behind everything else, so that an off configuration keeps every offset and the total it had)
    P.raw_off = P.dueling ? region("head_raw", (int64_t)P.N2 * P.raw_p) : -1;
    P.raw_t_off = (P.dueling && P.qt_rows) ? region("head_raw_target", (int64_t)P.qt_rows * P.raw_p) : -1;
    P.dout_raw_off = P.dueling ? region("dout_raw", (int64_t)P.B * P.raw_p) : -1;
    P.dbh_raw_off = P.dueling ? region("dbh_raw", P.raw_p) : -1;
    // (gradient clipping: likewise appended.  A workgroup of the reduction covers 64 elements of one tensor; a layer has at most four
    // tensors -- kernel, bias, LayerNorm scale and bias -- each of which may end in a partly filled workgroup)
    P.gc_part_cap = P.grad_clip ? (P.n_params + 63) / 64 + 4 * (int64_t)P.n_layers : 0;
    P.gc_part_off = P.grad_clip ? region("grad_clip_partials", 2 * P.gc_part_cap) : -1;
    P.gc_off = P.grad_clip ? region("grad_clip", 4) : -1;
    P.ws_bytes = region.off * 4;
}

// The plan of a configuration: a pure function of *cfg.  P starts value-initialised, so a field the configuration does not use
// holds 0 (-1 where its comment promises -1); on a refusal P is unspecified.
static inline int build_plan(const isdqn_net_config* cfg, Plan& P) {
    P = Plan{};
    int rc = check_options(cfg);
    if (rc) return rc;
    rc = plan_heads(cfg, P);
    if (rc) return rc;
    ParamCursor cur;
    DenseInput in{};
    rc = cfg->arch == ISDQN_ARCH_CNN ? plan_cnn_torso(cfg, P, cur, in)
         : cfg->arch == ISDQN_ARCH_IMPALA ? plan_impala_torso(cfg, P, cur, in)
                                          : plan_fc_input(cfg, in);
    if (rc) return rc;
    rc = plan_dense_tail(cfg, P, cur, in);
    if (rc) return rc;
    place_batch_stats(P, cur);
    plan_tiling(cfg, P);
    plan_workspace(cfg, P);
    return ISDQN_OK;
}

// The plan of a configuration never changes: cache the last few (a training process uses one or two
// configurations; building the plan allocates strings/vectors, which showed up in the per-step host time).
static inline const Plan* cached_plan(const isdqn_net_config* cfg, int* rc_out) {
    struct Slot { isdqn_net_config cfg; Plan plan; bool used = false; };
    static thread_local Slot slots[4];
    static thread_local int next = 0;
    *rc_out = ISDQN_OK;
    if (cfg == nullptr) { *rc_out = ISDQN_ERR_ARG; set_last_error("null config"); return nullptr; }
    for (auto& s : slots)
        if (s.used && memcmp(&s.cfg, cfg, sizeof(*cfg)) == 0) return &s.plan;
    Slot& s = slots[next];
    next = (next + 1) % 4;
    s.used = false;
    int rc = build_plan(cfg, s.plan);
    if (rc) { *rc_out = rc; return nullptr; }
    memcpy(&s.cfg, cfg, sizeof(*cfg));
    s.used = true;
    return &s.plan;
}

// Every tensor of the parameter buffer in the order of the layer list, then the BatchNorm sites: visit(const isdqn_tensor_info&).
// ndim is the length of `flax_shape`; the rest of the two arrays stays 0.
static inline isdqn_tensor_info tensor_info(const char* mod, const char* leaf, int64_t off, int64_t size, int kind, int layer,
                                            std::initializer_list<int> flax_shape, std::initializer_list<int> dims) {
    isdqn_tensor_info t;
    memset(&t, 0, sizeof(t));
    snprintf(t.name, sizeof(t.name), "%s/%s", mod, leaf);
    t.offset = off; t.size = size; t.kind = kind; t.layer = layer; t.ndim = (int)flax_shape.size();
    std::copy(flax_shape.begin(), flax_shape.end(), t.flax_shape);
    std::copy(dims.begin(), dims.end(), t.dims);
    return t;
}

template <class Visit>
static inline void for_each_param_tensor(const Plan& P, Visit&& visit) {
    auto layer_norm = [&](const char* mod, int64_t g_off, int64_t be_off, int width, int width_p, int layer) {
        visit(tensor_info(mod, "scale", g_off, width_p, 3, layer, {width}, {width_p}));
        visit(tensor_info(mod, "bias", be_off, width_p, 4, layer, {width}, {width_p}));
    };
    for (int i = 0; i < P.n_layers; ++i) {
        const Layer& l = P.L[i];
        if (l.kind == 2) {  // impala torso: Stack_s / {Conv_k, LayerNorm_b} (Flax nests the Stack's modules: "Stack_0/Conv_1/kernel")
            for (int s = 0; s < IMP_STACKS; ++s) {
                const ImpalaStack& S = P.imp[s];
                char mod[40];
                for (int k = 0; k < IMP_CONVS; ++k) {
                    const Layer& c = S.conv[k];
                    if (k >= 1 && (k & 1) && S.ln_g[(k - 1) / 2] >= 0) {  // LayerNorm_b sits in front of Conv_{1+2b}
                        const int b = (k - 1) / 2;
                        snprintf(mod, sizeof(mod), "Stack_%d/LayerNorm_%d", s, b);
                        layer_norm(mod, S.ln_g[b], S.ln_b[b], S.C, S.C_p, i);
                    }
                    snprintf(mod, sizeof(mod), "Stack_%d/%s", s, c.name);
                    visit(tensor_info(mod, "kernel", c.w_off, c.w_size, 0, i, {3, 3, c.cin, c.cout}, {c.cout_p, c.taps, c.cin_p}));
                    visit(tensor_info(mod, "bias", c.b_off, c.out_p, 2, i, {c.cout}, {c.out_p}));
                }
            }
        } else {
            if (l.kind == 0)
                visit(tensor_info(l.name, "kernel", l.w_off, l.w_size, 0, i, {l.ksz, l.ksz, l.cin, l.cout},
                                  {l.cout_p, l.is_u8 ? l.cin : l.taps, l.is_u8 ? 64 : l.cin_p}));
            else
                visit(tensor_info(l.name, "kernel", l.w_off, l.w_size, 1, i, {l.in_f, l.out_f}, {l.out_p, l.in_p}));
            visit(tensor_info(l.name, "bias", l.b_off, l.out_p, 2, i, {l.out_f}, {l.out_p}));
        }
        if (l.has_ln) layer_norm(l.ln_name, l.g_off, l.be_off, l.out_f, l.out_p, i);
    }
    for (int s = 0; s < P.n_bn; ++s) {  // BatchNorm_s: scale / bias ("params"), mean / var ("batch_stats")
        const BnSite& b = P.bns[s];
        int H, W;
        if (b.layer == -1) { H = P.L[0].hin; W = P.L[0].win; }
        else if (b.layer <= -2) { H = P.imp[(-2 - b.layer) / 2].Hp; W = P.imp[(-2 - b.layer) / 2].Wp; }
        else { H = P.L[b.layer].hout; W = P.L[b.layer].wout; }
        const int64_t offs[4] = {b.scale_off, b.bias_off, b.mean_off, b.var_off};
        static const char* const leaves[4] = {"scale", "bias", "mean", "var"};
        for (int k = 0; k < 4; ++k) {
            if (b.spatial) visit(tensor_info(b.name, leaves[k], offs[k], b.G_p, 5 + k, b.layer, {H, W}, {b.G, b.P, b.C, b.Cp}));
            else visit(tensor_info(b.name, leaves[k], offs[k], b.G_p, 5 + k, b.layer, {b.P * b.C}, {b.G, b.P, b.C, b.Cp}));
        }
    }
}

}  // namespace isdqn
