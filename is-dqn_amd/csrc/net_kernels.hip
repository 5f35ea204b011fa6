// iS-DQN Q-network on gfx950: forward over the 1+K shared heads, iterated Bellman target, squared TD
// loss, backward and Adam.  Reference: slimdqn/networks/architectures/dqn.py:47-103 and
// slimdqn/networks/isdqn.py:82-135.  Contractions run on the MFMA tile engine (gemm_core.h,
// net_problems.h); the row-wise kernels (row_kernels.h) are the HBM-bound remainder.
// One translation unit, split by concern: this file holds the include list -- its order is the order of the kernels in the code
// object, held to tests/golden/kernel_order.txt by tests/test_kernel_order_host.py -- and the C ABI.
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>
#include <atomic>

#include "conv_img.h"
#include "conv_u8_pair.h"
#include "conv_s8_pair.h"
#include "head_loss.h"
#include "conservative.h"
#include "soft_shift.h"
#include "prune.h"
#include "project.h"
#include "mixture.h"
#include "munchausen.h"
#include "hl_gauss.h"
#include "quantile.h"
#include "categorical.h"
#include "redo.h"
#include "dueling.h"
#include "net_plan.h"
#include "net_problems.h"

namespace isdqn {

#include "row_kernels.h"
#include "head_chain.h"
#include "optimizer_kernels.h"
#include "grad_clip.h"  // (inside namespace isdqn, behind the Adam table and the slab reduction it shares)
#include "aux_kernels.h"
#include "net_launch.h"
#include "impala.h"
#include "batchnorm.h"

}  // namespace isdqn

using namespace isdqn;

#if defined(ISDQN_BOUNDS)
// Bounds-checked development build (gemm_core.h: ISDQN_BOUNDS_CHECK): register the byte extents of every tensor the caller hands to
// the library -- [lo[i], hi[i]) -- and clear the record; read back the first load that fell outside all of them (synchronises).
extern "C" int isdqn_debug_bounds_set(const uint64_t* lo, const uint64_t* hi, int32_t n) {
    ISDQN_REQUIRE(n >= 0 && n <= 64, ISDQN_ERR_ARG, "at most 64 regions");
    isdqn::BoundsTable t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; ++i) { t.lo[i] = lo[i]; t.hi[i] = hi[i]; }
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(isdqn::isdqn_bounds), &t, sizeof(t)));
    return ISDQN_OK;
}
extern "C" int isdqn_debug_bounds_get(int32_t* bad, int32_t* site, uint64_t* addr) {
    isdqn::BoundsTable t;
    ISDQN_HIP_CHECK(hipDeviceSynchronize());
    ISDQN_HIP_CHECK(hipMemcpyFromSymbol(&t, HIP_SYMBOL(isdqn::isdqn_bounds), sizeof(t)));
    *bad = t.bad; *site = t.bad_site; *addr = t.bad_addr;
    return ISDQN_OK;
}
#endif

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" int isdqn_net_param_layout(const isdqn_net_config* cfg, int64_t* n_param_floats, isdqn_tensor_info* infos,
                                      int32_t max_infos, int32_t* n_infos) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    if (n_param_floats) *n_param_floats = P.n_params;
    int n = 0;
    for_each_param_tensor(P, [&](const isdqn_tensor_info& t) {
        if (infos && n < max_infos) memcpy(&infos[n], &t, sizeof(t));
        ++n;
    });
    if (n_infos) *n_infos = n;
    return ISDQN_OK;
}

extern "C" int isdqn_net_workspace_bytes(const isdqn_net_config* cfg, int64_t* bytes) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(bytes != nullptr, ISDQN_ERR_ARG, "null pointer");
    *bytes = P.ws_bytes;
    return ISDQN_OK;
}

extern "C" int isdqn_net_workspace_region(const isdqn_net_config* cfg, const char* name, int64_t* offset_bytes,
                                          int64_t* size_bytes) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(name != nullptr, ISDQN_ERR_ARG, "null name");
    for (auto& r : P.regions)
        if (r.first == name) {
            if (offset_bytes) *offset_bytes = r.second.first;
            if (size_bytes) *size_bytes = r.second.second;
            return ISDQN_OK;
        }
    set_last_error("unknown workspace region '%s'", name);
    return ISDQN_ERR_ARG;
}

static int check_input(const isdqn_net_config* cfg, const uint8_t* frames, int64_t frame_stride,
                       const int32_t* frame_ids, const float* obs) {
    if (cfg->arch != ISDQN_ARCH_FC) {
        ISDQN_REQUIRE(frames && frame_ids, ISDQN_ERR_ARG, "cnn / impala need frames and frame_ids");
        ISDQN_REQUIRE(frame_stride >= (int64_t)cfg->obs_h * cfg->obs_w, ISDQN_ERR_SHAPE, "frame_stride < h*w");
    } else {
        ISDQN_REQUIRE(obs != nullptr, ISDQN_ERR_ARG, "fc needs obs");
    }
    return ISDQN_OK;
}

// What the entry points that run a forward over the caller's observations share (forward, best_action(s), analysis, redo)
struct Inference {
    const Plan* plan = nullptr;
    NetInput in{};
    float* ws = nullptr;
    hipStream_t st = nullptr;
    bool x3 = false;
    // the plan, the entry point's own refusals (`own_checks(plan)`, in its own order and words), then the observations
    template <class Checks>
    int begin(const isdqn_net_config* cfg, const uint8_t* frames, int64_t frame_stride, const int32_t* frame_ids, const float* obs,
              void* workspace, void* stream, Checks own_checks) {
        int rc;
        plan = cached_plan(cfg, &rc);
        if (!plan) return rc;
        if ((rc = own_checks(*plan))) return rc;
        if ((rc = check_input(cfg, frames, frame_stride, frame_ids, obs))) return rc;
        in = NetInput{frames, frame_stride, frame_ids, 0, obs, nullptr, 0};
        ws = (float*)workspace;
        st = (hipStream_t)stream;
        x3 = cfg->precision == ISDQN_PRECISION_BF16X3;
        return ISDQN_OK;
    }
    // the mirror of `params` (`refresh`: unless the caller vouches for it), then the first `n_run` layers (-1: all) over `n_rows` rows
    int forward(const float* params, int n_rows, float* q_out, bool refresh = true, int n_run = -1) const {
        if (refresh)
            if (int rc = refresh_mirror(*plan, params, ws, st)) return rc;
        return net_forward(*plan, x3, params, in, n_rows, 0, ws, q_out, st, n_run);
    }
};

extern "C" int isdqn_net_forward(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                 int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                                 float* q_out, void* workspace, void* stream) {
    Inference c;
    int rc = c.begin(cfg, frames, frame_stride, frame_ids, obs, workspace, stream, [&](const Plan& P) -> int {
        ISDQN_REQUIRE(params && q_out && workspace, ISDQN_ERR_ARG, "null pointer");
        ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2*batch_size]");
        return ISDQN_OK;
    });
    if (rc) return rc;
    const Plan& P = *c.plan;
    float* ws = c.ws;
    hipStream_t st = c.st;
    rc = c.forward(params, n_rows, ws + P.out_off);
    if (rc) return rc;
    rc = head_expect(P, ws, n_rows, st);
    if (rc) return rc;
    // q_out is the unpadded (n_rows, nha) view
    ISDQN_HIP_CHECK(hipMemcpy2DAsync(q_out, (size_t)P.nha * 4, ws + P.q_off, (size_t)P.nha_p * 4, (size_t)P.nha * 4,
                                     n_rows, hipMemcpyDeviceToDevice, st));
    return ISDQN_OK;
}

#include "learn_step.h"  // (host code only, and outside namespace isdqn, where it always stood: BackwardSchedule's symbols keep their names)

// what every learn / loss / gradient entry point is handed, as its LearnCall; each fills the rest by field name
static LearnCall learn_call(const isdqn_net_config* cfg, LearnMode mode, const float* params, const isdqn_batch* batch, float* losses, float* q_values,
                            float* targets, void* workspace, void* stream) {
    LearnCall c;
    c.cfg = cfg; c.mode = mode; c.params = const_cast<float*>(params); c.batch = batch;
    c.losses = losses; c.q_values = q_values; c.targets = targets; c.ws = (float*)workspace; c.st = (hipStream_t)stream;
    // (the loss-only and the gradient-only calls update nothing: a decay behind their batch is not read)
    if (mode == LearnMode::Learn) batch_decay(batch, &c.weight_decay, &c.decay_kinds);
    c.cql_alpha = batch_conservative(batch);  // (a loss term: every mode takes it)
    c.mixture = batch_mixture(batch, &c.mix_alpha, &c.n_mix);  // (and so is the mixture)
    return c;
}

extern "C" int isdqn_net_learn_on_batch(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v,
                                        int32_t* adam_count, const isdqn_batch* batch, float* losses,
                                        float* losses_accum, float* q_values, float* targets, double* priorities,
                                        void* workspace, void* stream) {
    LearnCall c = learn_call(cfg, LearnMode::Learn, params, batch, losses, q_values, targets, workspace, stream);
    c.adam_m = adam_m; c.adam_v = adam_v; c.adam_count = adam_count; c.loss_accum = losses_accum; c.priorities = priorities;
    return learn_or_loss(c);
}

// Test hook (not in the public header): learn_on_batch that also writes the reduced gradient (internal layout).
extern "C" int isdqn_net_learn_on_batch_debug(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v,
                                              int32_t* adam_count, const isdqn_batch* batch, float* losses,
                                              float* losses_accum, float* q_values, float* targets, double* priorities,
                                              void* workspace, void* stream, float* grad_out) {
    LearnCall c = learn_call(cfg, LearnMode::Learn, params, batch, losses, q_values, targets, workspace, stream);
    c.adam_m = adam_m; c.adam_v = adam_v; c.adam_count = adam_count; c.loss_accum = losses_accum; c.priorities = priorities;
    c.grad_out = grad_out;
    return learn_or_loss(c);
}

extern "C" int isdqn_net_loss_on_batch(const isdqn_net_config* cfg, const float* params, const isdqn_batch* batch,
                                       float* losses, float* q_values, float* targets, void* workspace, void* stream) {
    return learn_or_loss(learn_call(cfg, LearnMode::Loss, params, batch, losses, q_values, targets, workspace, stream));
}

// Gradient of a TD loss without an update (the diagnostics of AnalysisDQN, analysisdqn.py:156-219): `n_pairs` > 0 regresses
// online heads online_head + k on target heads target_head + k (k < n_pairs) instead of the plan's iterated pairs;
// `target_params` != NULL takes the next states through those parameters (the target-based loss).
extern "C" int isdqn_net_grad_on_batch(const isdqn_net_config* cfg, const float* params, const float* target_params,
                                       const isdqn_batch* batch, int32_t online_head, int32_t target_head, int32_t n_pairs,
                                       float* grad_out, float* losses, float* q_values, float* targets, void* workspace,
                                       void* stream) {
    ISDQN_REQUIRE(grad_out != nullptr, ISDQN_ERR_ARG, "null grad_out");
    LearnCall c = learn_call(cfg, LearnMode::GradOnly, params, batch, losses, q_values, targets, workspace, stream);
    c.target_params = target_params; c.grad_out = grad_out;
    if (n_pairs > 0) c.sel = HeadSel{online_head, target_head, n_pairs};
    return learn_or_loss(c);
}

extern "C" int isdqn_net_refresh_mirror(const isdqn_net_config* cfg, const float* params, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(params != nullptr && workspace != nullptr, ISDQN_ERR_ARG, "null pointer");
    return refresh_mirror(*Pp, params, (float*)workspace, (hipStream_t)stream);
}

extern "C" int isdqn_net_bn_commit_running(const isdqn_net_config* cfg, float* params, const void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(params != nullptr && workspace != nullptr, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(Pp->bn, ISDQN_ERR_ARG, "not a BatchNorm network");
    return bn_commit_running(*Pp, params, (const float*)workspace, (hipStream_t)stream);
}

// DQN.learn_on_batch / loss_on_batch (dqn.py:59-83): separate target parameters for the next states.
extern "C" int isdqn_net_learn_on_batch_target(const isdqn_net_config* cfg, float* params, const float* target_params,
                                               float* adam_m, float* adam_v, int32_t* adam_count, const isdqn_batch* batch,
                                               float* losses, float* losses_accum, float* q_values, float* targets,
                                               double* priorities, void* workspace, void* stream) {
    ISDQN_REQUIRE(target_params != nullptr, ISDQN_ERR_ARG, "null target_params");
    LearnCall c = learn_call(cfg, LearnMode::Learn, params, batch, losses, q_values, targets, workspace, stream);
    c.target_params = target_params;
    c.adam_m = adam_m; c.adam_v = adam_v; c.adam_count = adam_count; c.loss_accum = losses_accum; c.priorities = priorities;
    return learn_or_loss(c);
}

extern "C" int isdqn_net_loss_on_batch_target(const isdqn_net_config* cfg, const float* params, const float* target_params,
                                              const isdqn_batch* batch, float* losses, float* q_values, float* targets,
                                              void* workspace, void* stream) {
    ISDQN_REQUIRE(target_params != nullptr, ISDQN_ERR_ARG, "null target_params");
    LearnCall c = learn_call(cfg, LearnMode::Loss, params, batch, losses, q_values, targets, workspace, stream);
    c.target_params = target_params;
    return learn_or_loss(c);
}

extern "C" int isdqn_net_shift_params(const isdqn_net_config* cfg, float* params, void* stream) {
    Plan P{};
    int rc = build_plan(cfg, P);
    if (rc) return rc;
    ISDQN_REQUIRE(params != nullptr, ISDQN_ERR_ARG, "null pointer");
    const Layer& l = P.L[P.n_layers - 1];
    hipLaunchKernelGGL(shift_kernel, dim3(ceil_div(l.in_p + 1, 256)), dim3(256), 0, (hipStream_t)stream,
                       params + l.w_off, params + l.b_off, P.dueling ? P.raw : P.nlog,
                       (P.n_actions + (P.dueling ? 1 : 0)) * (P.head_nb > 0 ? P.head_nb : 1), l.in_p);  // (dueling: the value rows move with their head)
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_net_best_action(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                     int64_t frame_stride, const int32_t* frame_ids, const float* obs,
                                     int32_t idx_network, int32_t* out_action, void* workspace, void* stream) {
    Inference c;
    int rc = c.begin(cfg, frames, frame_stride, frame_ids, obs, workspace, stream, [&](const Plan& P) -> int {
        ISDQN_REQUIRE(params && out_action && workspace, ISDQN_ERR_ARG, "null pointer");
        ISDQN_REQUIRE(idx_network >= 0 && idx_network < P.K, ISDQN_ERR_ARG, "idx_network out of range");
        return ISDQN_OK;
    });
    if (rc) return rc;
    const Plan& P = *c.plan;
    float* ws = c.ws;
    hipStream_t st = c.st;
    rc = c.forward(params, 1, ws + P.out_off);
    if (rc) return rc;
    rc = head_expect(P, ws, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(64), 0, st, ws + P.q_off, P.n_actions, P.oh + idx_network, out_action);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// best_action for n observations in one forward (vectorised environments: n host envs, one launch chain), with the
// "weight mirror is current" promise of ISDQN_BATCH_MIRROR_CURRENT as a flag.
extern "C" int isdqn_net_best_actions(const isdqn_net_config* cfg, const float* params, const uint8_t* frames,
                                      int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                                      const int32_t* idx_networks, int32_t* out_actions, int32_t flags, void* workspace,
                                      void* stream) {
    Inference c;
    int rc = c.begin(cfg, frames, frame_stride, frame_ids, obs, workspace, stream, [&](const Plan& P) -> int {
        ISDQN_REQUIRE(params && (idx_networks || (flags & ISDQN_ACT_MEAN_HEADS)) && out_actions && workspace, ISDQN_ERR_ARG, "null pointer");
        ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
        return ISDQN_OK;
    });
    if (rc) return rc;
    const Plan& P = *c.plan;
    float* ws = c.ws;
    hipStream_t st = c.st;
    rc = c.forward(params, n_rows, ws + P.out_off, /*refresh=*/!(flags & ISDQN_BATCH_MIRROR_CURRENT));
    if (rc) return rc;
    rc = head_expect(P, ws, n_rows, st);
    if (rc) return rc;
    if (flags & ISDQN_ACT_MEAN_HEADS)  // the head average's greedy action (mixture.h): every head, idx_networks is not read
        return launch_argmax_mean(ws + P.q_off, n_rows, P.nha_p, P.n_actions, P.n_heads, out_actions, st);
    else
        hipLaunchKernelGGL(argmax_rows_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, st, ws + P.q_off, n_rows, P.nha_p, P.n_actions,
                           P.oh, P.K, idx_networks, out_actions);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// eval_srank_and_dead_neurons' device part (experiments/base/srank_and_dead_neurons.py:8-22): the torso on n_rows observations.
extern "C" int isdqn_net_analysis_layout(const isdqn_net_config* cfg, int32_t* n_hidden, int64_t* sizes, int32_t max_sizes) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(n_hidden != nullptr, ISDQN_ERR_ARG, "null pointer");
    int n = 0;
    auto put = [&](int64_t v) {
        if (sizes != nullptr && n < max_sizes) sizes[n] = v;
        ++n;
    };
    if (P.L[0].kind == 2)  // impala: the two ReLU outputs of each residual block of each Stack (analysis_architecture.py:27-40)
        for (int s = 0; s < IMP_STACKS; ++s)
            for (int k = 0; k < 4; ++k) put((int64_t)P.imp[s].Hp * P.imp[s].Wp * P.imp[s].C);
    for (int i = 0; i < P.n_layers - 1; ++i) {
        const Layer& l = P.L[i];
        put(l.kind != 1 ? (int64_t)l.npix * l.cout : (int64_t)l.out_f);
    }
    *n_hidden = n;
    return ISDQN_OK;
}

extern "C" int isdqn_net_analysis(const isdqn_net_config* cfg, const float* params, const uint8_t* frames, int64_t frame_stride,
                                  const int32_t* frame_ids, const float* obs, int32_t n_rows, float* features_out,
                                  float* scores_out, void* workspace, void* stream) {
    Inference c;
    int rc = c.begin(cfg, frames, frame_stride, frame_ids, obs, workspace, stream, [&](const Plan& P) -> int {
        ISDQN_REQUIRE(params && features_out && scores_out && workspace, ISDQN_ERR_ARG, "null pointer");
        ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
        ISDQN_REQUIRE(P.n_layers >= 2, ISDQN_ERR_SHAPE, "no hidden layer");
        return ISDQN_OK;
    });
    if (rc) return rc;
    const Plan& P = *c.plan;
    float* ws = c.ws;
    hipStream_t st = c.st;
    // BatchNorm networks: as the reference applies AnalysisNet (srank_and_dead_neurons.py:17: mutable batch_stats, use_running_average
    // left False) -- the batch statistics of the analysed rows; the whole network runs (its head output is not used)
    if (P.bn) {
        rc = refresh_mirror(P, params, ws, st);
        if (rc) return rc;
        rc = bn_forward(P, c.x3, params, c.in, n_rows, 0, ws, ws + P.q_off, /*running=*/false, st);
    } else {
        rc = c.forward(params, n_rows, ws + P.q_off, /*refresh=*/true, P.n_layers - 1);
    }
    if (rc) return rc;
    int64_t off = 0;
    auto rowsum = [&](const float* act_s8, int elems_p, int cpp, int c, int64_t width, float* feat) -> int {
        hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(elems_p, 256)), dim3(256), 0, st, act_s8, n_rows, elems_p, cpp, c, scores_out + off, feat,
                           feat ? (int)width : 0);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += width;
        return ISDQN_OK;
    };
    if (P.L[0].kind == 2)
        for (int s = 0; s < IMP_STACKS; ++s) {
            const ImpalaStack& S = P.imp[s];
            const int elems_p = S.Hp * S.Wp * S.C_p;
            for (int b = 0; b < 2; ++b) {  // relu([LN](r)) in front of the block's BatchNorm, relu(conv) behind its first convolution
                if ((rc = rowsum(ws + S.a1_off[b], elems_p, S.C_p, S.C, (int64_t)S.Hp * S.Wp * S.C, nullptr))) return rc;
                if ((rc = rowsum(ws + S.a2_off[b], elems_p, S.C_p, S.C, (int64_t)S.Hp * S.Wp * S.C, nullptr))) return rc;
            }
        }
    for (int i = 0; i < P.n_layers - 1; ++i) {
        const Layer& l = P.L[i];
        const int cpp = l.kind != 1 ? l.cout_p : l.out_p, c = l.kind != 1 ? l.cout : l.out_f;
        const bool last = i == P.n_layers - 2;
        const int64_t width = l.kind != 1 ? (int64_t)l.npix * l.cout : (int64_t)l.out_f;
        // the sums are those of the ReLU output (in front of a BatchNorm); the feature matrix leaves the network behind the last
        // BatchNorm (analysis_architecture.py:115-122): a second pass over that site's output, sums discarded into the head's q rows
        if ((rc = rowsum(ws + l.act_off, l.out_elems_p, cpp, c, width, (last && !P.bn) ? features_out : nullptr))) return rc;
        if (last && P.bn) {
            const BnSite* b = bn_site_of(P, i);
            hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(l.out_elems_p, 256)), dim3(256), 0, st, (const float*)(ws + b->out_off), n_rows,
                               l.out_elems_p, cpp, c, ws + P.slab_off, features_out, (int)width);
            ISDQN_HIP_CHECK(hipGetLastError());
        }
    }
    return ISDQN_OK;
}

// ReDo (Sokar et al. 2023; csrc/redo.h): the recyclable layers are the hidden ones, in network order.
static int redo_supported(const isdqn_net_config* cfg, const Plan& P) {
    ISDQN_REQUIRE(cfg->arch != ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED,
                  "ReDo is not built for the impala torso: its residual adds make a neuron's outgoing weights ambiguous");
    ISDQN_REQUIRE(!P.bn, ISDQN_ERR_UNSUPPORTED, "ReDo is not built for BatchNorm networks: per-position statistics sit between the layers");
    ISDQN_REQUIRE(P.n_layers >= 2, ISDQN_ERR_SHAPE, "no hidden layer");
    return ISDQN_OK;
}

extern "C" int isdqn_net_redo_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* n_neurons, int32_t max_layers) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    if ((rc = redo_supported(cfg, P))) return rc;
    ISDQN_REQUIRE(n_layers != nullptr, ISDQN_ERR_ARG, "null pointer");
    for (int i = 0; i < P.n_layers - 1 && n_neurons != nullptr && i < max_layers; ++i) n_neurons[i] = P.L[i].out_f;
    *n_layers = P.n_layers - 1;
    return ISDQN_OK;
}

extern "C" int isdqn_net_redo(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, const float* fresh_params,
                              const uint8_t* frames, int64_t frame_stride, const int32_t* frame_ids, const float* obs, int32_t n_rows,
                              float tau, float* scores_out, int32_t* mask_out, int32_t* n_recycled_out, void* workspace, void* stream) {
    Inference c;
    int rc = c.begin(cfg, frames, frame_stride, frame_ids, obs, workspace, stream, [&](const Plan& P) -> int {
        if (int rc2 = redo_supported(cfg, P)) return rc2;
        ISDQN_REQUIRE(params && fresh_params && scores_out && mask_out && n_recycled_out && workspace, ISDQN_ERR_ARG, "null pointer");
        ISDQN_REQUIRE((adam_m == nullptr) == (adam_v == nullptr), ISDQN_ERR_ARG, "adam_m and adam_v must be both null or both given");
        ISDQN_REQUIRE(std::isfinite(tau) && tau >= 0.f, ISDQN_ERR_ARG, "tau must be finite and >= 0");
        ISDQN_REQUIRE(n_rows >= 1 && n_rows <= P.N2, ISDQN_ERR_SHAPE, "n_rows must be in [1, 2 * batch_size] (workspace rows)");
        return ISDQN_OK;
    });
    if (rc) return rc;
    const Plan& P = *c.plan;
    float* ws = c.ws;
    hipStream_t st = c.st;
    const int n_hidden = P.n_layers - 1;
    rc = c.forward(params, n_rows, ws + P.q_off, /*refresh=*/true, n_hidden);
    if (rc) return rc;
    // score: per-position sums over the rows into scratch (the data-gradient region: the forward does not touch it, and it holds a
    // batch of the widest input any layer above the first reads, so one image of any hidden layer's output), then one workgroup
    float* possum = ws + P.da_off;
    int64_t off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        const int npix = l.kind == 0 ? l.npix : 1;
        ISDQN_REQUIRE((int64_t)npix * l.out_f <= P.da_floats && l.out_f <= REDO_MAX_WIDTH, ISDQN_ERR_UNSUPPORTED, "ReDo: hidden layer too wide");
        hipLaunchKernelGGL(act_rowsum_kernel, dim3(ceil_div(l.out_elems_p, 256)), dim3(256), 0, st, (const float*)(ws + l.act_off), n_rows,
                           l.out_elems_p, l.out_p, l.out_f, possum, (float*)nullptr, 0);
        ISDQN_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(redo_score_kernel, dim3(1), dim3(256), 0, st, (const float*)possum, npix, l.out_f, (float)((int64_t)n_rows * npix), tau,
                           scores_out + off, mask_out + off, n_recycled_out + i);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    // recycle: every incoming side first, then every outgoing side -- where a dormant neuron reads a dormant neuron the weight is 0
    off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        hipLaunchKernelGGL(redo_incoming_kernel, dim3(ceil_div(l.K, 1024), l.out_f), dim3(256), 0, st, params, adam_m, adam_v, fresh_params,
                           (const int*)(mask_out + off), l.w_off, l.K, l.b_off, l.g_off, l.be_off);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    off = 0;
    for (int i = 0; i < n_hidden; ++i) {
        const Layer& l = P.L[i];
        const Layer& nx = P.L[i + 1];
        hipLaunchKernelGGL(redo_outgoing_kernel, dim3(ceil_div(nx.K / 8, 256), nx.out_p), dim3(256), 0, st, params, adam_m, adam_v,
                           (const int*)(mask_out + off), l.out_f, l.out_p, nx.w_off, nx.K);
        ISDQN_HIP_CHECK(hipGetLastError());
        off += l.out_f;
    }
    return refresh_mirror(P, params, ws, st);
}

// ---- noisy Dense layers (noisy.h; include/isdqn_hip.h, isdqn_noisy_layout) ----
namespace isdqn {
#include "noisy.h"  // (behind the learn step: tests/test_kernel_order_host.py holds every kernel to its place)
}  // namespace isdqn
// the plan behind its own checks, then the three refusals of the noisy entry points in their documented order
static const Plan* noisy_plan(const isdqn_net_config* cfg, int* rc) {
    const Plan* Pp = cached_plan(cfg, rc);
    if (!Pp) return nullptr;
    auto refuse = [&](const char* msg) -> const Plan* {
        set_last_error("%s", msg);
        *rc = ISDQN_ERR_UNSUPPORTED;
        return nullptr;
    };
    if (cfg->batch_norm) return refuse("noisy layers are not built for BatchNorm networks: running statistics would be committed into the composed parameters");
    if (cfg->arch == ISDQN_ARCH_IMPALA) return refuse("noisy layers are not built for the impala torso");
    if (cfg->max_grad_norm > 0.f)
        return refuse("noisy layers with max_grad_norm > 0 are a follow-up: the global norm must cover the gradient of sigma too");
    return Pp;
}
// noise layout: per noisy layer ein[in_p] then eout[out_p], the layers concatenated in network order
static int64_t noisy_tables(const Plan& P, NoisyTable* tab, NoisyVecTable* vecs) {
    int64_t off = 0;
    int l_noisy = 0;
    if (tab) tab->n = 0;
    if (vecs) { vecs->n = 0; vecs->total_blocks = 0; }
    for (int i = 0; i < P.n_layers; ++i) {
        const Layer& l = P.L[i];
        if (l.kind != 1) continue;
        const int64_t ein = off, eout = off + l.in_p;
        if (tab) {
            tab->e[tab->n++] = NoisyEntry{l.w_off, l.w_size, ein, eout, l.in_p, FastDiv((uint32_t)l.in_p)};
            tab->e[tab->n++] = NoisyEntry{l.b_off, (int64_t)l.out_p, ein, eout, 0, FastDiv()};
        }
        if (vecs) {
            const int widths[2] = {l.in_p, l.out_p};
            const int64_t offs[2] = {ein, eout};
            for (int v = 0; v < 2; ++v) {
                vecs->v[vecs->n++] = NoisyVec{offs[v], widths[v], 2 * l_noisy + v, vecs->total_blocks, 0};
                vecs->total_blocks += ceil_div(widths[v], NOISY_THREADS);
            }
        }
        off += l.in_p + l.out_p;
        ++l_noisy;
    }
    return off;
}

extern "C" int isdqn_noisy_layout(const isdqn_net_config* cfg, int32_t* n_layers, int64_t* offsets, int32_t* in_widths, int32_t* out_widths,
                                  int32_t max_layers, int64_t* n_noise_floats) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    NoisyVecTable vecs;  // (two vectors per noisy layer: ein, then eout)
    const int64_t total = noisy_tables(*Pp, nullptr, &vecs);
    const int n = vecs.n / 2;
    if (n_layers) *n_layers = n;
    if (n_noise_floats) *n_noise_floats = total;
    if (!offsets && !in_widths && !out_widths) return ISDQN_OK;  // a query of the count and the total
    // (the arrays must hold every layer: nothing is truncated silently)
    ISDQN_REQUIRE(max_layers >= n, ISDQN_ERR_ARG, "isdqn_noisy_layout: max_layers is smaller than the number of noisy layers (returned in *n_layers)");
    for (int k = 0; k < n; ++k) {
        if (offsets) offsets[k] = vecs.v[2 * k].off;
        if (in_widths) in_widths[k] = vecs.v[2 * k].n;
        if (out_widths) out_widths[k] = vecs.v[2 * k + 1].n;
    }
    return ISDQN_OK;
}

extern "C" int isdqn_noisy_sample(const isdqn_net_config* cfg, uint64_t seed, int32_t stream_id, int64_t* noise_count, float* noise, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(noise_count != nullptr && noise != nullptr, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(stream_id == 0 || stream_id == 1, ISDQN_ERR_ARG, "stream_id must be 0 (online) or 1 (target)");
    NoisyVecTable vecs;
    noisy_tables(*Pp, nullptr, &vecs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noisy_sample_kernel, dim3(vecs.total_blocks), dim3(NOISY_THREADS), 0, st, vecs, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)stream_id, (const int64_t*)noise_count, noise);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(noisy_advance_kernel, dim3(1), dim3(64), 0, st, noise_count);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

static int noisy_compose(const Plan& P, const NoisyTable& tab, const float* mu, const float* sigma, const float* noise, float* eff, float* ws,
                         hipStream_t st) {
    const int64_t quads = P.n_params / 4;  // (every tensor size is a multiple of 8)
    hipLaunchKernelGGL(noisy_compose_kernel, dim3((unsigned)((quads + NOISY_THREADS - 1) / NOISY_THREADS)), dim3(NOISY_THREADS), 0, st, tab, mu, sigma,
                       noise, eff, ws ? ws + P.wsplit_off : nullptr, P.n_params);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_noisy_compose(const isdqn_net_config* cfg, const float* mu, const float* sigma, const float* noise, float* eff,
                                   void* workspace, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(mu && sigma && noise && eff, ISDQN_ERR_ARG, "null pointer");
    NoisyTable tab;
    noisy_tables(*Pp, &tab, nullptr);
    return noisy_compose(*Pp, tab, mu, sigma, noise, eff, (float*)workspace, (hipStream_t)stream);
}

extern "C" int isdqn_noisy_learn_on_batch(const isdqn_net_config* cfg, float* mu, float* sigma, float* m_mu, float* v_mu, float* m_sigma,
                                          float* v_sigma, int32_t* adam_count, const float* noise, float* eff, const float* eff_target,
                                          float* grad, const isdqn_batch* batch, float* losses, float* losses_accum, float* q_values,
                                          float* targets, double* priorities, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = noisy_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(mu && sigma && m_mu && v_mu && m_sigma && v_sigma && adam_count && noise && eff && grad && batch && workspace, ISDQN_ERR_ARG,
                  "null pointer");
    {  // AdamW: noisy_adam_kernel walks the flat buffer and does not know the conv tensors' kinds
        float weight_decay;
        int32_t decay_kinds;
        batch_decay(batch, &weight_decay, &decay_kinds);
        if ((rc = check_decay(weight_decay, decay_kinds))) return rc;
        ISDQN_REQUIRE(weight_decay == 0.f, ISDQN_ERR_UNSUPPORTED, "weight decay under NoisyNet exploration is not built");
    }
    if ((rc = check_conservative(batch_conservative(batch)))) return rc;  // (in front of the first launch)
    ISDQN_REQUIRE(!(batch->flags & ISDQN_BATCH_MIXTURE), ISDQN_ERR_UNSUPPORTED, "the mixture under NoisyNet exploration is not built");
    NoisyTable tab;
    noisy_tables(P, &tab, nullptr);
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    rc = noisy_compose(P, tab, mu, sigma, noise, eff, ws, st);
    if (rc) return rc;
    // the full two-stream gradient pass on eff: its optimizer launches write the reduced gradient (masked under dueling) and update
    // nothing; loss_finalize_kernel advances adam_count and leaves the bias corrections in the workspace, as in a plain learn step
    isdqn_batch_discount b{*batch, batch_discount(batch)};  // (the copy keeps the discounts that may follow the caller's batch)
    b.batch.flags |= ISDQN_BATCH_MIRROR_CURRENT;  // (compose wrote the mirror of eff; the *_target form rebuilds both mirrors itself)
    b.batch.flags &= ~(ISDQN_BATCH_WEIGHT_DECAY | ISDQN_BATCH_CONSERVATIVE);  // (the copy ends at the discounts)
    LearnCall c = learn_call(cfg, LearnMode::GradOnly, eff, &b.batch, losses, q_values, targets, workspace, stream);
    c.cql_alpha = batch_conservative(batch);  // (the conservative term behind the caller's batch)
    c.target_params = eff_target; c.adam_count = adam_count; c.loss_accum = losses_accum; c.priorities = priorities; c.grad_out = grad;
    rc = learn_or_loss(c);
    if (rc) return rc;
    const int64_t quads = P.n_params / 4;
    hipLaunchKernelGGL(noisy_adam_kernel, dim3((unsigned)((quads + NOISY_THREADS - 1) / NOISY_THREADS)), dim3(NOISY_THREADS), 0, st, tab, (const float*)grad,
                       noise, mu, m_mu, v_mu, sigma, m_sigma, v_sigma, (const float*)(ws + P.adam_tab_off), cfg->learning_rate, cfg->adam_b1, cfg->adam_b2,
                       cfg->adam_eps, P.n_params);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// ---- periodic resets and EMA targets (reset.h; include/isdqn_hip.h, isdqn_net_reset / isdqn_net_ema) ----
namespace isdqn {
#include "reset.h"  // (new kernels go last: tests/test_kernel_order_host.py)
}  // namespace isdqn

extern "C" int isdqn_net_reset_layout(const isdqn_net_config* cfg, int32_t* n_layers, int32_t* first_dense_layer) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    int first = Pp->n_layers;
    for (int i = Pp->n_layers - 1; i >= 0; --i)
        if (Pp->L[i].kind == 1) first = i;
    if (n_layers) *n_layers = Pp->n_layers;
    if (first_dense_layer) *first_dense_layer = first;
    return ISDQN_OK;
}

extern "C" int isdqn_net_reset(const isdqn_net_config* cfg, float* params, float* adam_m, float* adam_v, int32_t* adam_count,
                               const float* fresh_params, int32_t split_layer, float shrink_lower, float perturb_lower, float shrink_upper,
                               float perturb_upper, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params && fresh_params, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE((adam_m == nullptr) == (adam_v == nullptr), ISDQN_ERR_ARG, "adam_m and adam_v must be both null or both given");
    const float fac[4] = {shrink_lower, perturb_lower, shrink_upper, perturb_upper};
    for (float f : fac) ISDQN_REQUIRE(std::isfinite(f) && f >= 0.f, ISDQN_ERR_ARG, "every shrink / perturb factor must be finite and >= 0");
    ISDQN_REQUIRE(split_layer >= 0 && split_layer <= P.n_layers, ISDQN_ERR_ARG, "split_layer must be in [0, n_layers]");
    {
        const uintptr_t a = (uintptr_t)params, b = (uintptr_t)fresh_params, bytes = (uintptr_t)P.n_params * 4;
        ISDQN_REQUIRE(a + bytes <= b || b + bytes <= a, ISDQN_ERR_ARG, "fresh_params overlaps params");
    }
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = (((uintptr_t)params | (uintptr_t)fresh_params | (uintptr_t)adam_m | (uintptr_t)adam_v) & 15) == 0;
    const bool touch[2] = {!(shrink_lower == 1.f && perturb_lower == 0.f), !(shrink_upper == 1.f && perturb_upper == 0.f)};
    ResetTable tab;
    tab.s[0] = shrink_lower; tab.q[0] = perturb_lower; tab.s[1] = shrink_upper; tab.q[1] = perturb_upper;
    tab.n = 0;
    tab.total_blocks = 0;
    int launch_rc = ISDQN_OK;
    auto flush = [&]() {
        if (tab.n == 0 || launch_rc) return;
        hipLaunchKernelGGL(reset_kernel, dim3(std::min(tab.total_blocks, RESET_MAX_BLOCKS)), dim3(RESET_THREADS), 0, st, tab, params, adam_m, adam_v,
                           fresh_params);
        if (hipGetLastError() != hipSuccess) {
            set_last_error("isdqn_net_reset: kernel launch failed");
            launch_rc = ISDQN_ERR_HIP;
        }
        tab.n = 0;
        tab.total_blocks = 0;
    };
    for_each_param_tensor(P, [&](const isdqn_tensor_info& t) {
        const int upper = t.layer >= split_layer ? 1 : 0;
        if (!touch[upper] || t.size <= 0) return;
        // one launch per tensor would do for a tensor of 2^31 * RESET_BLOCK_ELEMS elements; the plan's tensors hold fewer than 2^31
        const int vec = (aligned && t.offset % 4 == 0 && t.size % 4 == 0) ? 2 : 0;
        const int blocks = (int)((t.size + RESET_BLOCK_ELEMS - 1) / RESET_BLOCK_ELEMS);
        if (tab.n == RESET_MAX_ENTRIES) flush();
        tab.e[tab.n++] = ResetEntry{t.offset, t.size, tab.total_blocks, upper | vec};
        tab.total_blocks += blocks;
    });
    flush();
    if (launch_rc) return launch_rc;
    if (adam_count != nullptr) {
        hipLaunchKernelGGL(reset_count_kernel, dim3(1), dim3(64), 0, st, adam_count);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (workspace != nullptr) return refresh_mirror(P, params, (float*)workspace, st);
    return ISDQN_OK;
}

extern "C" int isdqn_net_ema(const isdqn_net_config* cfg, float* target, const float* online, float tau, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    ISDQN_REQUIRE(target && online, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(tau >= 0.f && tau <= 1.f, ISDQN_ERR_ARG, "tau must be in [0, 1]");  // (NaN fails both comparisons)
    ISDQN_REQUIRE(target != online, ISDQN_ERR_ARG, "target and online are the same buffer");
    if (tau == 0.f) return ISDQN_OK;
    const int64_t n = Pp->n_params;
    hipStream_t st = (hipStream_t)stream;
    if (tau == 1.f) {  // the bits of `online`, a NaN target and the sign of a zero included
        ISDQN_HIP_CHECK(hipMemcpyAsync(target, online, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        return ISDQN_OK;
    }
    const bool aligned = (((uintptr_t)target | (uintptr_t)online) & 15) == 0;
    const int64_t n4 = aligned ? n / 4 : 0;
    const int64_t work = std::max<int64_t>(n4, n - 4 * n4);
    const int64_t blocks = std::min<int64_t>((work + RESET_THREADS - 1) / RESET_THREADS, RESET_MAX_BLOCKS);
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(RESET_THREADS), 0, st, target, online, 1.0f - tau, tau, n4, n);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

extern "C" int isdqn_selftest_gemm(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K,
                                   int32_t a_tr, int32_t b_tr, int32_t precision, int32_t split_k, void* stream) {
    ISDQN_REQUIRE(A && B && C, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(M > 0 && N > 0 && K > 0, ISDQN_ERR_SHAPE, "bad shape");
    const bool x3 = precision == ISDQN_PRECISION_BF16X3;
    hipStream_t st = (hipStream_t)stream;
    // ROW operand: [rows][K] ; TR operand: [K][rows].  No alignment promises (self-test shapes are arbitrary).
    MatSrc a = a_tr ? MatSrc{A, M, K, M, 0} : MatSrc{A, K, M, K, 0};
    MatSrc b = b_tr ? MatSrc{B, N, K, N, 0} : MatSrc{B, K, N, K, 0};
    const int64_t slab = (int64_t)M * N;
    if (!a_tr && !b_tr) return plain_big<false, false, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    if (!a_tr && b_tr) return plain_big<false, true, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    if (a_tr && !b_tr) return plain_big<true, false, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
    return plain_big<true, true, false>(x3, a, nullptr, 0, b, C, N, M, N, K, split_k, slab, st);
}

namespace isdqn {
// (declared in net_launch.h in front of dense_wgrad)
static int dense_wgrad_fp32(const Layer& l, bool x3, const MatSrc& A, const MatSrc& Bm, float* slabs, int rows, hipStream_t st) {
    return plain_big<true, true, false>(x3, A, nullptr, 0, Bm, slabs, l.in_p, l.out_p, l.in_p, rows, l.gw_slabs, l.w_size, st);
}
}  // namespace isdqn

// ---- soft head shift (include/isdqn_hip.h, isdqn_net_soft_shift): host code here, the kernel in soft_shift_kernels.hip ----

extern "C" int isdqn_net_soft_shift(const isdqn_net_config* cfg, float* params, float tau, void* workspace, void* stream) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(params != nullptr, ISDQN_ERR_ARG, "null pointer");
    ISDQN_REQUIRE(tau >= 0.f && tau <= 1.f, ISDQN_ERR_ARG, "tau must be in [0, 1]");  // (NaN fails both comparisons)
    ISDQN_REQUIRE(P.n_heads >= 2, ISDQN_ERR_ARG, "a soft head shift needs n_heads >= 2: a single head has no upper neighbour");
    ISDQN_REQUIRE(((uintptr_t)params & 15) == 0, ISDQN_ERR_ARG, "soft head shift: params must be 16-byte aligned");
    if (tau == 0.f) return ISDQN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (tau == 1.f) {  // the hard shift's bits, a NaN and the sign of a zero included
        if ((rc = isdqn_net_shift_params(cfg, params, stream))) return rc;
        if (workspace != nullptr) return refresh_mirror(P, params, (float*)workspace, st);
        return ISDQN_OK;
    }
    const Layer& l = P.L[P.n_layers - 1];
    SoftShiftArgs a;
    a.p = params;
    a.mirror = workspace != nullptr ? (float*)workspace + P.wsplit_off : nullptr;
    a.w_off = l.w_off; a.b_off = l.b_off; a.in_p = l.in_p;
    a.R = (P.n_actions + (P.dueling ? 1 : 0)) * (P.head_nb > 0 ? P.head_nb : 1);  // the block isdqn_net_shift_params moves
    a.K = P.n_heads - 1;
    a.omt = 1.0f - tau; a.tau = tau;
    // every position the grid touches lies inside the last Dense (the launcher checks what the 16-byte lanes and the mirror's groups need)
    ISDQN_REQUIRE((int64_t)P.n_heads * a.R == (P.dueling ? P.raw : P.nlog) && (int64_t)P.n_heads * a.R <= l.out_p, ISDQN_ERR_SHAPE,
                  "soft head shift: the head blocks do not tile the last Dense");
    ISDQN_REQUIRE(l.w_off + (int64_t)l.out_p * l.in_p <= P.n_params && l.b_off + (int64_t)l.out_p <= P.n_params, ISDQN_ERR_SHAPE,
                  "soft head shift: the last Dense lies outside the parameter buffer");
    return launch_soft_shift(a, st);
}

// ---- gradual magnitude pruning (include/isdqn_hip.h, isdqn_net_prune_*): host code here, the kernels in prune_kernels.hip ----

// the prunable tensors of a plan in layout order: every conv and Dense kernel but the last Dense's.  info_index (may be null): where
// each of them sits in isdqn_net_param_layout's table
static int prune_table(const isdqn_net_config* cfg, const Plan** plan_out, PruneTable& tab, int32_t* info_index) {
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(cfg->arch != ISDQN_ARCH_IMPALA, ISDQN_ERR_UNSUPPORTED, "pruning is not built for the impala torso");
    ISDQN_REQUIRE(!P.bn, ISDQN_ERR_UNSUPPORTED, "pruning is not built for batch_norm");
    memset(&tab, 0, sizeof(tab));
    for (int i = 0; i + 1 < P.n_layers; ++i) {
        const Layer& l = P.L[i];
        ISDQN_REQUIRE(tab.n < PRUNE_MAX_TENSORS && l.w_size < (1ll << 31), ISDQN_ERR_SHAPE, "pruning: too many or too large kernels");
        PruneTensor& t = tab.t[tab.n];
        t.offset = l.w_off;
        t.size = (int32_t)l.w_size;
        t.rows_real = l.out_f;
        if (l.kind == 0) {
            t.row_len = l.K;
            t.period = l.is_u8 ? l.K : l.cin_p;  // Conv_0's [plane][ky][kx] rows have no padded lane
            t.real_per = l.is_u8 ? l.K : l.cin;
        } else {
            const bool torso = i > 0 && P.L[i - 1].kind == 0;  // columns [pixel][c padded to 8]
            t.row_len = l.in_p;
            t.period = torso ? P.L[i - 1].cout_p : l.in_p;
            t.real_per = torso ? P.L[i - 1].cout : l.in_f;
        }
        ISDQN_REQUIRE(l.w_off >= 0 && l.w_off + l.w_size <= P.n_params, ISDQN_ERR_SHAPE, "pruning: a kernel lies outside the parameter buffer");
        if (info_index) {  // (for_each_param_tensor: kernel, bias and the LayerNorm pair of every layer in front)
            int n = 0;
            for (int j = 0; j < i; ++j) n += 2 + (P.L[j].has_ln ? 2 : 0);
            info_index[tab.n] = n;
        }
        ++tab.n;
    }
    if ((rc = prune_table_finish(tab))) return rc;
    *plan_out = Pp;
    return ISDQN_OK;
}

extern "C" int isdqn_net_prune_layout(const isdqn_net_config* cfg, int32_t* n_tensors, int64_t* infos, int32_t max_infos, int64_t* mask_words,
                                      int64_t* scratch_bytes) {
    const Plan* Pp;
    PruneTable tab;
    int32_t index[PRUNE_MAX_TENSORS];
    if (int rc = prune_table(cfg, &Pp, tab, index)) return rc;
    if (n_tensors) *n_tensors = tab.n;
    for (int i = 0; infos && i < tab.n && i < max_infos; ++i) {
        infos[4 * i + 0] = index[i];
        infos[4 * i + 1] = tab.t[i].offset;
        infos[4 * i + 2] = tab.t[i].size;
        infos[4 * i + 3] = tab.t[i].n_real;
    }
    if (mask_words) *mask_words = (Pp->n_params + 31) / 32;
    if (scratch_bytes) *scratch_bytes = tab.hist_words * 4;
    return ISDQN_OK;
}

extern "C" int isdqn_net_prune_update(const isdqn_net_config* cfg, float* params, const int32_t* n_pruned, uint32_t* mask, void* scratch,
                                      void* workspace, void* stream) {
    const Plan* Pp;
    PruneArgs a;
    if (int rc = prune_table(cfg, &Pp, a.tab, nullptr)) return rc;
    ISDQN_REQUIRE(params && n_pruned && mask && scratch, ISDQN_ERR_ARG, "null pointer");
    for (int i = 0; i < a.tab.n; ++i) a.tab.t[i].k = n_pruned[i];
    a.p = params;
    a.mirror = workspace != nullptr ? (float*)workspace + Pp->wsplit_off : nullptr;
    a.mask = mask;
    a.scratch = (uint32_t*)scratch;
    return launch_prune_update(a, (hipStream_t)stream);
}

extern "C" int isdqn_net_prune_apply(const isdqn_net_config* cfg, float* params, const uint32_t* mask, void* workspace, void* stream) {
    const Plan* Pp;
    PruneArgs a;
    if (int rc = prune_table(cfg, &Pp, a.tab, nullptr)) return rc;
    ISDQN_REQUIRE(params && mask, ISDQN_ERR_ARG, "null pointer");
    a.p = params;
    a.mirror = workspace != nullptr ? (float*)workspace + Pp->wsplit_off : nullptr;
    a.mask = const_cast<uint32_t*>(mask);
    a.scratch = nullptr;
    return launch_prune_apply(a, (hipStream_t)stream);
}

// ---- Normalize-and-Project (include/isdqn_hip.h, isdqn_net_project_*): host code here, the kernels in project_kernels.hip.  The
// projected tensors are the prunable ones: prune_table above, with its refusals ----

extern "C" int isdqn_net_project_layout(const isdqn_net_config* cfg, int32_t* n_tensors, int64_t* infos, int32_t max_infos,
                                        int64_t* scratch_bytes) {
    const Plan* Pp;
    PruneTable tab;
    int32_t index[PRUNE_MAX_TENSORS];
    if (int rc = prune_table(cfg, &Pp, tab, index)) return rc;
    if (n_tensors) *n_tensors = tab.n;
    for (int i = 0; infos && i < tab.n && i < max_infos; ++i) {
        infos[4 * i + 0] = index[i];
        infos[4 * i + 1] = tab.t[i].offset;
        infos[4 * i + 2] = tab.t[i].size;
        infos[4 * i + 3] = tab.t[i].n_real;
    }
    if (scratch_bytes) *scratch_bytes = project_scratch_bytes(tab);
    return ISDQN_OK;
}

extern "C" int isdqn_net_project_norms(const isdqn_net_config* cfg, const float* params, double* norms, void* scratch, void* stream) {
    const Plan* Pp;
    ProjectArgs a;
    if (int rc = prune_table(cfg, &Pp, a.tab, nullptr)) return rc;
    ISDQN_REQUIRE(params && norms && scratch, ISDQN_ERR_ARG, "null pointer");
    a.p = const_cast<float*>(params);
    a.mirror = nullptr;
    a.target = nullptr;
    a.norms = norms;
    a.scales = nullptr;
    a.scratch = (double*)scratch;
    return launch_project_norms(a, (hipStream_t)stream);
}

extern "C" int isdqn_net_project_apply(const isdqn_net_config* cfg, float* params, const double* target_norms, double* norms, float* scales,
                                       void* scratch, void* workspace, void* stream) {
    const Plan* Pp;
    ProjectArgs a;
    if (int rc = prune_table(cfg, &Pp, a.tab, nullptr)) return rc;
    ISDQN_REQUIRE(params && target_norms && norms && scales && scratch, ISDQN_ERR_ARG, "null pointer");
    a.p = params;
    a.mirror = workspace != nullptr ? (float*)workspace + Pp->wsplit_off : nullptr;
    a.target = target_norms;
    a.norms = norms;
    a.scales = scales;
    a.scratch = (double*)scratch;
    return launch_project_apply(a, (hipStream_t)stream);
}

// ---- random ensemble mixture (mixture.h, mixture_kernels.hip; include/isdqn_hip.h, isdqn_mixture_draw / isdqn_batch_mixture) ----
extern "C" int isdqn_mixture_draw(int32_t n_heads, uint64_t seed, int64_t* draw_count, float* alpha, void* stream) {
    ISDQN_REQUIRE(n_heads >= 1 && n_heads <= MIX_MAX_HEADS, ISDQN_ERR_ARG, "isdqn_mixture_draw: n_heads must be in [1, 1024]");
    ISDQN_REQUIRE(draw_count != nullptr && alpha != nullptr, ISDQN_ERR_ARG, "null pointer");
    return launch_mixture_draw((int)n_heads, seed, draw_count, alpha, (hipStream_t)stream);
}
