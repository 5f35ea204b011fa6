// The learn step of a network without BatchNorm, phase by phase: SideStream, LearnCtx, head_chain_plan, learn_forward, learn_loss,
// WgradJob / BackwardSchedule, learn_backward, clipped_adam, learn_optimizer, and learn_or_loss, which every learn / loss / gradient
// entry point calls with its LearnCall (net_launch.h).  Included by net_kernels.hip behind batchnorm.h and check_input, outside
// namespace isdqn (where this code always stood: the weak symbols of BackwardSchedule's members keep their names).  Host code only; it names head_chain_kernel's and the fused-Adam GEMM's instantiations first (tests/test_kernel_order_host.py).
#pragma once
// Side stream for the weight gradients.  The backward's critical path is dgrad -> LayerNorm-backward -> dgrad ...;
// every weight gradient only needs its layer's dz and is needed again by Adam at the very end, so they run on a
// second HIP stream and share the CUs with the data-gradient chain (both sides are partly latency bound and
// their workgroups co-reside).  One stream + event pool per device, created on first use, never destroyed.
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2 * MAX_LAYERS + 4];
    int n_ev = 0;
    std::atomic<unsigned> next{0};  // several agents / host threads of one process may share a device's pool
    std::atomic<int> state{0};      // 0 = not created, 1 = being created, 2 = ready, -1 = unavailable
};
static SideStream* side_stream() {
    static SideStream per_dev[ISDQN_MAX_DEVICES];
    if (ISDQN_DEV_ENV("ISDQN_SINGLE_STREAM")) return nullptr;
    SideStream& s = per_dev[current_device_slot()];
    int st = s.state.load(std::memory_order_acquire);
    if (st == 2) return &s;
    if (st == -1) return nullptr;
    int expected = 0;
    if (s.state.compare_exchange_strong(expected, 1)) {
        bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
        s.n_ev = 2 * MAX_LAYERS + 4;
        for (int i = 0; ok && i < s.n_ev; ++i) ok = hipEventCreateWithFlags(&s.ev[i], hipEventDisableTiming) == hipSuccess;
        s.state.store(ok ? 2 : -1, std::memory_order_release);
        return ok ? &s : nullptr;
    }
    while ((st = s.state.load(std::memory_order_acquire)) == 1) {}  // another thread is creating it
    return st == 2 ? &s : nullptr;
}
static hipEvent_t next_event(SideStream* ss) { return ss->ev[ss->next.fetch_add(1, std::memory_order_relaxed) % (unsigned)ss->n_ev]; }
// make `waiter` wait for everything enqueued so far on `signaller`
static int chain(SideStream* ss, hipStream_t signaller, hipStream_t waiter) {
    hipEvent_t e = next_event(ss);
    ISDQN_HIP_CHECK(hipEventRecord(e, signaller));
    ISDQN_HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
    return ISDQN_OK;
}

// What a learn / loss / gradient-only call on a network without BatchNorm fixes before its first launch (learn_or_loss).
struct LearnCtx : LearnCall {  // (the call as learn_or_loss hands it on: heads resolved, q_values / targets at their destination)
    const Plan& P;
    const bool x3;
    const int B, K;  // K: the pairs the call regresses (sel.K)
    const NetInput in;
    LearnCtx(const LearnCall& call, const Plan& plan)
        : LearnCall(call), P(plan), x3(call.cfg->precision == ISDQN_PRECISION_BF16X3), B(plan.B), K(call.sel.K),
          in{call.batch->frames, call.batch->frame_stride, call.batch->frame_ids, plan.B, call.batch->state, call.batch->next_state, plan.B} {}
    SideStream* ss = nullptr;   // learn steps: the weight-gradient stream (nullptr: everything runs on the caller's stream)
    hipStream_t wst = nullptr;  // stream of the weight gradients: ss->stream, or st
    bool double_q = false;      // Double Q-learning targets (cfg->double_q, unless selector and value are the same head of the same rows)
    bool munchausen = false;    // Munchausen targets (cfg->munchausen_tau > 0); excludes double_q (build_plan)
    int hc_S = 0, hc_wg = 0;    // head chain (head_chain_plan): transitions per workgroup, workgroups; 0 = generic loss and head backward
    const float* wmir() const { return ws + P.wsplit_off; }
    const Layer& hid() const { return P.L[P.n_layers >= 2 ? P.n_layers - 2 : 0]; }
    const Layer& head() const { return P.L[P.n_layers - 1]; }
};

// head chain eligibility (learn steps on the plan's own heads): last hidden layer dense + ReLU, widths within the kernel's limits
static void head_chain_plan(LearnCtx& c, bool plan_heads) {
    const Plan& P = c.P;
    const Layer& hid = c.hid();
    static const bool hc_disabled = ISDQN_DEV_ENV("ISDQN_NO_HEAD_CHAIN");
    // (histogram and quantile heads take the generic backward: head GEMMs at the logit width; the head chain is built for scalar heads)
    // (dueling heads too: the chain multiplies by the head kernel itself and knows no combine)
    if (P.dueling) return;
    // (the conservative term too: its dL/dq is dense over the actions, the chain exploits one non-zero per row and pair)
    if (c.cql_alpha > 0.f) return;
    // (the mixture too: H non-zeros per row of dL/dq, and a loss kernel of its own)
    if (c.mixture) return;
    if (!(c.update() && plan_heads && !hc_disabled && c.target_params == nullptr && P.head_nb == 0 && P.n_layers >= 2 && hid.kind == 1 &&
          !hid.is_head && hid.has_relu && hid.out_p <= HC_THREADS * HC_MAX_COLS && hid.out_p % 8 == 0))
        return;
    // transitions per workgroup: the per-transition phases scale with S (the kernel is instruction-issue bound) while
    // every workgroup streams the whole head matrix from L2, so S follows the batch: about 256 workgroups
    const int S = c.B >= 1024 ? 4 : c.B >= 512 ? 2 : 1;
    const int n_wg = ceil_div(c.B, S);
    if (n_wg <= hid.part_rows && S * c.K <= HC_THREADS && head_chain_lds_bytes(hid.out_p, P.nha_p, c.K, c.x3 ? 3 : 1, S) <= 150 * 1024) {
        c.hc_S = S;
        c.hc_wg = n_wg;
    }
}

static int learn_forward(const LearnCtx& c) {
    const Plan& P = c.P;
    const isdqn_batch* batch = c.batch;
    float* ws = c.ws;
    const int B = c.B;
    int rc;
    if (c.target_params != nullptr) {
        // Separate target parameters: a forward of the target parameters, then one of the online parameters, over the same workspace.
        // One row per form: the target forward's input, rows and head-output rows; the rows head_expect_rows turns into "q_target"
        // (histogram / quantile heads; 0: none); the online forward's input and rows.  Its z rows are the B states in every form.
        struct Form {
            NetInput t_in; int t_rows; float* t_out; int expect_rows;
            NetInput on_in; int on_rows;
        };
        const int stack = c.cfg->arch != ISDQN_ARCH_FC ? c.cfg->obs_c : 0;
        const NetInput nx{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->next_state, nullptr, 0, 2 * stack, stack};
        const NetInput on{batch->frames, batch->frame_stride, batch->frame_ids, 0, batch->state, nullptr, 0, 2 * stack, 0};
        const Form f =
            // Munchausen DQN: the target parameters value the states too, so they run over concat(state, next_state) (2B rows of head
            // output -> "q_target" / "logits_target", states first); then the online parameters over the B states, as the DQN form below
            c.munchausen ? Form{c.in, P.N2, ws + P.out_t_off, P.N2, on, B}
            // Double DQN: the target parameters value the B next states (head output -> "q_target" / "logits_target"), then ONE forward
            // of the online parameters over concat(state, next_state) as the iS-DQN path runs it: its next-state rows select
            : c.double_q ? Form{nx, B, ws + P.out_t_off, B, c.in, P.N2}
            // DQN (dqn.py:74-88): the next states go through the TARGET parameters, the states through the online ones: two
            // forwards of B images each over the same workspace, q rows [B, 2B) first, then rows [0, B) (+ z of every layer)
                         : Form{nx, B, ws + P.out_off + (int64_t)B * P.nlog_p, 0, on, B};
        rc = refresh_mirror(P, c.target_params, ws, c.st);
        if (rc) return rc;
        rc = net_forward(P, c.x3, c.target_params, f.t_in, f.t_rows, 0, ws, f.t_out, c.st);
        if (rc) return rc;
        if (f.expect_rows > 0 && P.head_nb > 0) {
            rc = head_expect_rows(P, ws + P.logits_t_off, f.expect_rows, ws + P.qt_off, c.st);
            if (rc) return rc;
        }
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
        return net_forward(P, c.x3, c.params, f.on_in, f.on_rows, B, ws, ws + P.out_off, c.st);
    }
    // The optimizer writes the updated parameters in both forms, so a learn step leaves the mirror current; a caller
    // that chains learn steps on one workspace with nothing else writing `params` in between says so
    // (ISDQN_BATCH_MIRROR_CURRENT: the captured multi-step graphs) and the refresh is skipped.
    if (!(batch->flags & ISDQN_BATCH_MIRROR_CURRENT)) {
        rc = refresh_mirror(P, c.params, ws, c.st);
        if (rc) return rc;
    }
    // forward on concat(state, next_state) (isdqn.py:95); the head chain takes over at the last hidden layer's split-K slabs
    return net_forward(P, c.x3, c.params, c.in, P.N2, B, ws, ws + P.out_off, c.st, c.hc_S ? P.n_layers - 1 : -1, c.hc_S ? P.n_layers - 2 : -1);
}

static int launch_head_chain(const LearnCtx& c) {
    const Plan& P = c.P;
    const Layer &hid = c.hid(), &head = c.head();
    float* ws = c.ws;
    HeadChainParams hp;
    hp.act = ws + hid.act_off; hp.z = ws + hid.z_off;
    hp.slabs = ws + P.slab_off;
    hp.n_slabs = effective_splits(hid.in_unpadded_ld ? hid.in_f : hid.K, hid.fwd_splits);
    hp.slab_stride = hid.out_p;
    hp.row_pitch = (int64_t)hp.n_slabs * hid.out_p;
    hp.hbias = c.params + hid.b_off;
    hp.W = c.params + head.w_off; hp.bias = c.params + head.b_off;
    hp.gamma = hid.has_ln ? c.params + hid.g_off : nullptr;
    hp.beta = hid.has_ln ? c.params + hid.be_off : nullptr;
    hp.B = c.B; hp.S = c.hc_S; hp.F = hid.out_f; hp.Fp = hid.out_p; hp.O = P.nha; hp.Op = P.nha_p; hp.K = c.K; hp.oh = P.oh;
    hp.A = P.n_actions;
    hp.action = c.batch->action; hp.reward = c.batch->reward; hp.terminal = c.batch->terminal;
    hp.loss_weights = c.batch->loss_weights; hp.discount = batch_discount(c.batch);
    hp.gamma_n = c.cfg->gamma_n; hp.huber_delta = c.cfg->huber_delta;
    hp.double_q = c.double_q ? 1 : 0;
    hp.mu = Munchausen{c.cfg->munchausen_tau, c.cfg->munchausen_alpha, c.cfg->munchausen_clip};
    hp.dout = ws + P.dout_off; hp.dz = ws + hid.dz_off; hp.part = ws + hid.part_off;
    hp.q_values = c.q_values; hp.targets = c.targets; hp.priorities = c.priorities;
    hp.loss_part = ws + P.lpart_off; hp.dbh_part = hp.loss_part + (int64_t)c.hc_wg * c.K;
    hp.adam_count = c.adam_count; hp.b1 = c.cfg->adam_b1; hp.b2 = c.cfg->adam_b2; hp.adam_consts = ws + P.adam_tab_off;
    hp.stamps = stamps_for("head_chain");
    const int lds = head_chain_lds_bytes(hid.out_p, P.nha_p, c.K, c.x3 ? 3 : 1, c.hc_S);
    const int cols = ceil_div(hid.out_p, HC_THREADS) <= 1 ? 1 : ceil_div(hid.out_p, HC_THREADS) <= 2 ? 2 : 4;
    auto launch_hc = [&](auto kern, int slot) -> int {
        static LdsConfigured configured[18];
        if (int rc2 = ensure_dynamic_lds(kern, lds, configured[slot])) return rc2;
        ISDQN_REPORT_OCCUPANCY(kern, HC_THREADS, lds, c.hc_wg);
        hipLaunchKernelGGL(kern, dim3(c.hc_wg), dim3(HC_THREADS), lds, c.st, hp);
        ISDQN_HIP_CHECK(hipGetLastError());
        return ISDQN_OK;
    };
    auto by_cols = [&](auto passes_c, auto s_c, int base) -> int {
        constexpr int PS = decltype(passes_c)::value, SS = decltype(s_c)::value;
        return cols == 1 ? launch_hc(&head_chain_kernel<PS, 1, SS>, base) : cols == 2 ? launch_hc(&head_chain_kernel<PS, 2, SS>, base + 1)
                                                                        : launch_hc(&head_chain_kernel<PS, 4, SS>, base + 2);
    };
    auto by_s = [&](auto passes_c, int base) -> int {
        return c.hc_S == 1 ? by_cols(passes_c, std::integral_constant<int, 1>{}, base)
             : c.hc_S == 2 ? by_cols(passes_c, std::integral_constant<int, 2>{}, base + 3)
                           : by_cols(passes_c, std::integral_constant<int, 4>{}, base + 6);
    };
    return c.x3 ? by_s(std::integral_constant<int, 3>{}, 0) : by_s(std::integral_constant<int, 1>{}, 9);
}

// The two small kernels that only need the head chain's outputs: the loss / head-bias sums of its per-workgroup partials, and the
// head's weight gradient (dL/dq fp32, hidden activations S8)
static int head_chain_sums(const LearnCtx& c, hipStream_t s) {
    return loss_finalize(c.P, c.cfg, c.ws, c.hc_wg, c.K, c.P.nha_p, c.losses, c.loss_accum, true, nullptr, s);
}
static int head_chain_tail(const LearnCtx& c, hipStream_t s) {
    if (int rc = head_chain_sums(c, s)) return rc;
    const Layer& head = c.head();
    return dense_wgrad(head, c.x3, c.in, c.ws + c.hid().act_off, c.ws + c.P.dout_off, c.P.nlog_p, c.ws + head.gw_off, c.B, s);
}

// targets, loss, dL/dq: q_values / targets / priorities / per-head loss partials are final behind it
static int learn_loss(const LearnCtx& c) {
    // the target network's own head output ("q_target" / "logits_target": next states; Munchausen: states, then next states)
    const bool tnet = (c.double_q || c.munchausen) && c.target_params != nullptr;
    if (!c.hc_S) {
        int rc = loss_and_finalize(c.P, c, c.double_q, tnet ? c.ws + c.P.out_t_off + (c.munchausen ? (int64_t)c.B * c.P.nlog_p : 0) : nullptr,
                                   (tnet && c.munchausen) ? c.ws + c.P.out_t_off : nullptr);
        if (rc || !(c.learn() && c.P.dueling)) return rc;
        // dueling heads: dL/d(combined rows) and the reduced head-bias gradient -> the raw head's (dueling.h), where the backward starts
        const Plan& P = c.P;
        const int w = P.head_nb > 0 ? P.head_nb : 1;
        const int64_t threads = (int64_t)(c.B + 1) * P.n_heads * w;
        hipLaunchKernelGGL(duel_backward_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, c.st,
                           (const float*)(c.ws + P.dout_off), P.nlog_p, c.ws + P.dout_raw_off, P.raw_p, (const float*)(c.ws + P.dbh_off),
                           c.ws + P.dbh_raw_off, c.B, P.n_heads, P.n_actions, w);
        ISDQN_HIP_CHECK(hipGetLastError());
        return ISDQN_OK;
    }
    if (int rc = launch_head_chain(c)) return rc;
    // with a weight-gradient stream the sums leave the critical path: BackwardSchedule enqueues head_chain_tail() there
    return c.ss ? ISDQN_OK : head_chain_sums(c, c.st);
}

// One layer's weight gradient as the schedule sees it (plain data: a deferred one waits in BackwardSchedule)
struct WgradJob {
    int layer = -1;  // -1: none
    hipStream_t stream = nullptr;
    hipEvent_t wait = nullptr;  // deferred: the fork recorded on the caller's stream behind the layer's data gradient
    const float* dz = nullptr;  // gradient w.r.t. the layer's pre-activation output
    int dz_ld = 0;
};

// dense weight gradient straight into Adam: one workgroup holds the whole contraction
// (a gradient-only pass runs the same kernel with the stores of p / m / v switched off)
static int dense_wgrad_fused_adam(const LearnCtx& c, const Layer& l, const float* act_in, const WgradJob& j) {
    const MatSrc A{j.dz, j.dz_ld, c.B, l.out_p, 1};
    const MatSrc Bm{act_in, l.in_p, c.B, l.in_p, 1};
    AdamFuse af{c.params + l.w_off, c.adam_m + l.w_off, c.adam_v + l.w_off, c.ws + c.P.adam_tab_off,
                c.cfg->learning_rate, c.cfg->adam_b1, c.cfg->adam_b2, c.cfg->adam_eps,
                c.grad_out ? c.grad_out + l.w_off : nullptr, c.ws + c.P.wsplit_off + l.w_off, c.update() ? 1 : 0, c.wd(1)};
    // 64x64 tiles: the contraction is only B deep, the kernel lives off streaming p/m/v through the Adam
    // epilogue, and 128x128 tiles would leave 100 workgroups for 256 CUs
    // (operands: dz of a hidden layer -- or the fp32 dL/dq of the head -- and the S8 activations below it)
    if (l.is_head)
        return c.x3 ? launch_plain<64, 64, 2, 2, true, true, 3, true, false, true, 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1, 0,
                                                                                      j.stream, &af)
                    : launch_plain<64, 64, 2, 2, true, true, 1, true, false, true, 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1, 0,
                                                                                      j.stream, &af);
    return c.x3 ? launch_plain<64, 64, 2, 2, true, true, 3, true, false, true, DZ_S8 | 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1,
                                                                                          0, j.stream, &af)
                : launch_plain<64, 64, 2, 2, true, true, 1, true, false, true, DZ_S8 | 2>(A, nullptr, 0, Bm, nullptr, l.in_p, l.out_p, l.in_p, c.B, 1,
                                                                                          0, j.stream, &af);
}

// weight gradient -> slabs and an entry in the optimizer list of its stream, or straight into Adam
// `adam`: [0] caller's stream, [1] weight-gradient stream
static int weight_gradient(const LearnCtx& c, const WgradJob& j, AdamList* adam) {
    const Layer& l = c.P.L[j.layer];
    float* ws = c.ws;
    const float* act_in = j.layer > 0 ? ws + c.P.L[j.layer - 1].act_off : nullptr;
    int w_slabs, rc;
    if (l.is_head && c.hc_S && c.ss) {  // enqueued by head_chain_tail()
        w_slabs = effective_splits(c.B, l.gw_slabs);
    } else if (l.kind == 0) {
        rc = conv_wgrad(l, c.x3, c.in, act_in, j.dz, ws + l.gw_off, c.B, j.stream, &w_slabs);
        if (rc) return rc;
    } else {
        w_slabs = effective_splits(c.B, l.gw_slabs);
        // (gradient clipping: no parameter may move before the norm of the whole gradient is known -- the one slab goes to "gw/")
        if (w_slabs == 1 && !l.in_unpadded_ld && !c.P.grad_clip) return dense_wgrad_fused_adam(c, l, act_in, j);
        rc = dense_wgrad(l, c.x3, c.in, act_in, j.dz, j.dz_ld, ws + l.gw_off, c.B, j.stream);
        if (rc) return rc;
    }
    adam[c.ss && j.stream == c.wst ? 1 : 0].add(l.w_off, l.w_size, ws + l.gw_off, w_slabs, l.w_size, c.wd(l.kind == 0 ? 0 : 1));
    return ISDQN_OK;
}

#if !defined(ISDQN_FORK_LATE_MAX_B)
#define ISDQN_FORK_LATE_MAX_B 768
#endif
// The side-stream policy of one learn step's backward pass: which stream a weight gradient runs on, where the caller's stream
// forks, and in which order the kernels behind a fork are created.  Without a side stream (c.ss == nullptr) nothing forks and
// every kernel is enqueued in line on the caller's stream.
//
//  * Streams.  Weight gradients of the middle layers go to the side stream.  Every fork costs the main stream an event record
//    (a ~6 us bubble), so the head's tiny weight gradient and the first layer's (nothing is left to overlap with) stay on the
//    main stream, and a dense layer (its Adam may be fused: an in-place update) forks once, AFTER its data gradient: dz is final
//    and the data gradient, which reads W, is enqueued, so the update on the side stream cannot overtake it.
//  * Tail swap.  With at least three layers the last two weight gradients swap streams: layer 1's follows its data gradient on
//    the caller's stream, layer 0's (which only needs that data gradient's output) runs beside it.
//  * Head chain.  Its loss / head-bias sums and the head's weight gradient (head_chain_tail) leave the critical path: they are
//    enqueued on the side stream behind the first fork the backward pass makes anyway (no fork is spent on these two small
//    kernels alone), or in line when no layer forked.
//  * The caller's event (batch->priorities_ready: q_values / targets / priorities are final behind the loss) is likewise
//    recorded at the first point that forks the caller's stream anyway, else at the end of the backward (no side stream: at once).
//  * Which queue the replayed graph gives a kernel: a node's FIRST-created successor stays on its queue, the others move to
//    another one and start ~12 us late.  Round 4's order (fork_late; c2 +1.2 %, c3 +7.5 %;
//    -DISDQN_FORK_LATE_MAX_B=0 keeps round 3's):
//      - the data-gradient chain is created first behind every fork, so it stays on the capturing queue all the way: a layer
//        that forks after its data gradient records the fork there, but its side-stream kernels are created (`deferred`, flush)
//        only after the NEXT layer's data gradient has been enqueued on the caller's stream;
//      - the two head kernels become successors of the HEAD CHAIN on the side stream (head_event) -- created behind the dense
//        data gradient, which therefore stays the head chain's first successor -- and run under the dense data gradient; the new
//        queue's late start is hidden there, and it is what lets the first convolution data gradient become resident before the
//        fused-Adam GEMM's 968 workgroups ask for the CUs.
//    Large batches keep round 3's order: at B = 1024 every kernel is several rounds of workgroups, which queue gets the CUs first
//    no longer matters and the new order measured 0.6 % slower (profiles/round4/ab_fork_c5.txt; ab_thresholds.txt: +2.0 % at
//    B = 32, +1.7 % at 128, +1.5 % at 512, +2.0 % at 768).
//  * Two optimizer lists: tensors whose gradient is produced on the side stream are updated there, the others on the caller's
//    stream, so the step ends with two short Adam launches side by side instead of join -> reduce -> one Adam.  The side
//    stream may update its own tensors only when every reader of the weights is behind it (adam_on_side): with the tail swap
//    its last kernel (layer 0's weight gradient) waited for the last data gradient of the caller's stream.
struct BackwardSchedule {
    const LearnCtx& c;
    AdamList* const adam;  // [0] caller's stream, [1] side stream
    const bool tail_swap, fork_late;
    bool prio_pending, head_pending;  // priorities_ready / head_chain_tail() still to be enqueued
    hipEvent_t head_event = nullptr;  // fork_late: the head chain's end on the caller's stream
    bool forked = false, layer0_chained = false;
    WgradJob deferred;  // the side-stream work of the layer above, held back until this layer's data gradient is enqueued

    BackwardSchedule(const LearnCtx& ctx, AdamList* lists)
        : c(ctx), adam(lists), tail_swap(ctx.ss && ctx.P.n_layers >= 3 && !ctx.P.L[1].is_head),
          fork_late(ctx.ss != nullptr && ctx.P.L[0].kind != 2 && ctx.B <= ISDQN_FORK_LATE_MAX_B),
          prio_pending(ctx.batch->priorities_ready != nullptr), head_pending(ctx.hc_S && ctx.ss) {}

    bool wgrad_on_side(int i) const { return c.ss && !c.P.L[i].is_head && (tail_swap ? i != 1 : i > 0); }
    // (the head's weight gradient behind a head chain: head_chain_tail() on the side stream)
    hipStream_t wgrad_stream(int i) const { return wgrad_on_side(i) || (c.P.L[i].is_head && c.hc_S) ? c.wst : c.st; }
    bool forks_after_dgrad(int i) const { return wgrad_on_side(i) && c.P.L[i].kind == 1 && i > 0; }
    // dz of the layer is final on the main stream (layer 0 with the tail swap: chain_layer0() already forked)
    bool forks_before_dgrad(int i) const { return wgrad_on_side(i) && !forks_after_dgrad(i) && !(i == 0 && layer0_chained); }
    // (gradient clipping: never -- both streams join in front of the norm, learn_optimizer)
    bool adam_on_side() const { return c.ss && forked && tail_swap && !c.P.grad_clip; }

    int signal_priorities() {
        if (prio_pending) {
            prio_pending = false;
            ISDQN_HIP_CHECK(hipEventRecord((hipEvent_t)c.batch->priorities_ready, c.st));
        }
        return ISDQN_OK;
    }
    int run_head_tail(hipStream_t s) {
        if (!head_pending) return ISDQN_OK;
        head_pending = false;
        return head_chain_tail(c, s);
    }
    // behind the loss, in front of the first layer
    int begin() {
        if (!c.ss)
            if (int rc = signal_priorities()) return rc;
        if (fork_late && head_pending) {
            head_event = next_event(c.ss);
            ISDQN_HIP_CHECK(hipEventRecord(head_event, c.st));
        }
        return ISDQN_OK;
    }
    // fork in front of a layer's data gradient
    int fork(hipStream_t side) {
        if (int rc = chain(c.ss, c.st, side)) return rc;
        if (int rc = signal_priorities()) return rc;
        forked = true;
        // (held-back side work of the layer above enqueues the two head kernels itself, behind this layer's data gradient)
        return deferred.layer < 0 ? run_head_tail(side) : ISDQN_OK;
    }
    // fork behind a layer's data gradient; *defer: the job's kernels wait (as `deferred`) for the next layer's data gradient
    int fork_after_dgrad(WgradJob& job, bool* defer) {
        if (!fork_late) {
            if (int rc = chain(c.ss, c.st, job.stream)) return rc;
            if (int rc = signal_priorities()) return rc;
            forked = true;
            return run_head_tail(job.stream);
        }
        if (head_event != nullptr && head_pending) {  // (the dense data gradient is enqueued: the head chain keeps it as first successor)
            ISDQN_HIP_CHECK(hipStreamWaitEvent(job.stream, head_event, 0));
            if (int rc = run_head_tail(job.stream)) return rc;
        }
        job.wait = next_event(c.ss);
        ISDQN_HIP_CHECK(hipEventRecord(job.wait, c.st));
        *defer = true;
        forked = true;
        return signal_priorities();
    }
    // tail swap, behind layer 1's fused data gradient: layer 0's dz is final, its weight gradient may start beside layer 1's
    int chain_layer0() {
        if (int rc = chain(c.ss, c.st, c.wst)) return rc;
        forked = layer0_chained = true;
        return run_head_tail(c.wst);
    }
    // the held-back side-stream work, now that the data gradient it yields to is enqueued
    int flush() {
        if (deferred.layer < 0) return ISDQN_OK;
        const WgradJob j = deferred;
        deferred.layer = -1;
        ISDQN_HIP_CHECK(hipStreamWaitEvent(j.stream, j.wait, 0));
        if (int rc = run_head_tail(j.stream)) return rc;
        return weight_gradient(c, j, adam);
    }
    // behind the last layer
    int finish() {
        if (int rc = flush()) return rc;
        if (int rc = run_head_tail(c.st)) return rc;  // no layer forked: keep the two kernels in line
        return signal_priorities();
    }
};

// first dense layer over a 64-channel conv output: data gradient + LN/ReLU backward of the layer below in one kernel
static bool dense_dgrad_ln_applies(const Layer& l, const Layer& below, int B) {
    return l.kind == 1 && below.kind != 1 && below.cout_p == 64 && !l.in_unpadded_ld && below.part_rows >= ceil_div(B, 128) * below.npix;
}
static int dense_dgrad_ln(const LearnCtx& c, const Layer& l, const Layer& below, const float* dz, int dz_ld, ReduceJobs* red) {
    float* ws = c.ws;
    const int B = c.B;
    auto launch = [&](auto prob) {
        prob.A = MatSrc{dz, dz_ld, B, l.out_p, 1};
        prob.B = MatSrc{c.wmir() + l.w_off, l.in_p, l.out_f, l.in_p, 1};
        prob.z = ws + below.z_off;
        prob.gamma = below.has_ln ? c.params + below.g_off : nullptr;
        prob.beta = below.has_ln ? c.params + below.be_off : nullptr;
        prob.dz_out = ws + below.dz_off;
        prob.part = ws + below.part_off;
        prob.ldc = l.in_p; prob.M = B; prob.N = l.in_p; prob.K = l.out_p; prob.c_in = below.out_f;
        prob.tiles_m = ceil_div(B, decltype(prob)::BM); prob.tiles_n = l.in_p / 64;
        return launch_gemm(prob, prob.tiles_m * prob.tiles_n, c.st);
    };
    // 128-row tiles (8 accumulators per wave).  64-row tiles fill the chip better (196 workgroups, -3 us)
    // but are a four-accumulator kernel, and those are not run-to-run stable on gfx950
    // at most one workgroup per CU (242 at the headline size): two K groups of four waves (gemm_core.h)
    static const bool no_kg = ISDQN_DEV_ENV("ISDQN_NO_KGROUPS");
    const bool kg2 = !no_kg && ceil_div(B, 128) * (l.in_p / 64) <= 256 && l.out_p % 64 == 0;
    int rc;
    // ISDQN_DGRAD64 (development): 64-row tiles, one K group
#if defined(ISDQN_DGRAD64)
    (void)kg2;
    rc = c.x3 ? launch(DenseDgradLN<3, 64>{}) : launch(DenseDgradLN<1, 64>{});
    constexpr int DG_BM = 64;
#else
    if (kg2) rc = c.x3 ? launch(DenseDgradLN<3, 128, 2>{}) : launch(DenseDgradLN<1, 128, 2>{});
    else rc = c.x3 ? launch(DenseDgradLN<3, 128>{}) : launch(DenseDgradLN<1, 128>{});
    constexpr int DG_BM = 128;
#endif
    if (rc) return rc;
    add_reduce_job(*red, ws + below.part_off, ceil_div(B, DG_BM) * (l.in_p / 64), 3 * below.out_p, ws + below.red_off);
    return ISDQN_OK;
}

// data gradient of layer i > 0 for the layer below.  *dz_fused: a fused kernel also ran the LN/ReLU backward of the layer below (its dz
// is written, the partial rows of its parameter gradients are a job in `red`); otherwise da (w.r.t. that layer's activation) is in ws+da_off
static int data_gradient(const LearnCtx& c, int i, const float* dz, int dz_ld, bool* dz_fused, ReduceJobs* red) {
    const Layer &l = c.P.L[i], &below = c.P.L[i - 1];
    float* da = c.ws + c.P.da_off;
    *dz_fused = false;
    if (l.is_head && c.hc_S) return ISDQN_OK;  // dz of the hidden layer came from the head chain
    if (l.kind == 0) {
        int rc = conv_dgrad_img(l, below, c.x3, c.params, c.wmir(), dz, c.ws, c.B, c.st, dz_fused, red);
        if (rc || *dz_fused) return rc;
        return conv_dgrad(l, c.x3, c.wmir(), dz, da, c.B, c.st);
    }
    if (dense_dgrad_ln_applies(l, below, c.B)) {
        *dz_fused = true;
        return dense_dgrad_ln(c, l, below, dz, dz_ld, red);
    }
    const bool narrow = ceil_div(c.B, 128) * ceil_div(l.in_p, 128) < 200;
    return dense_dgrad(l, c.x3, c.wmir(), dz, dz_ld, da, c.B, narrow, c.st);
}

// backward (online rows only: the next-state half has a zero cotangent, isdqn.py:99), top layer first.  Per layer: parameter-gradient
// entries -> maybe fork -> data gradient for the layer below -> what the layer above deferred -> fork after the data gradient, or
// defer -> weight gradient
static int learn_backward(const LearnCtx& c, BackwardSchedule& sched, AdamList* adam, ReduceJobs* red) {
    const Plan& P = c.P;
    float* ws = c.ws;
    const int B = c.B;
    int rc;
    // gradient w.r.t. the current layer's pre-activation output (dueling heads: of the raw head, "dout_raw" / "dbh_raw")
    const float* dz_cur = ws + (P.dueling ? P.dout_raw_off : P.dout_off);
    int dz_ld = P.dueling ? P.raw_p : P.nlog_p;
    bool dz_fused = false;  // dz of layer i was already produced by the fused data gradient of layer i+1
    for (int i = P.n_layers - 1; i >= 0; --i) {
        const Layer& l = P.L[i];
        if (l.is_head) {
            adam[c.hc_S && c.ss ? 1 : 0].add(l.b_off, l.out_p, ws + (P.dueling ? P.dbh_raw_off : P.dbh_off), 1, 0, c.wd(2));  // loss_finalize_kernel's stream
        } else {
            dz_cur = ws + l.dz_off;
            dz_ld = l.out_p;
            if (c.hc_S && i == P.n_layers - 2) {  // dz and the partial sums came from the head chain
                add_ln_bias_entries(adam[0], c, l, ws + l.part_off, c.hc_wg, 3 * (int64_t)l.out_p);
            } else if (dz_fused) {  // (reduce_rows_kernel, in front of Adam)
                add_ln_bias_entries(adam[0], c, l, ws + l.red_off, 1, 0);
            } else {
                // da (w.r.t. this layer's activation) was left in ws+da_off by layer i+1's data-gradient
                int nb = 0;
                rc = ln_bwd(l, c.params, ws + P.da_off, ws + l.z_off, l.kind != 1 ? B * l.npix : B, ws + l.dz_off, ws + l.part_off, &nb, c.st);
                if (rc) return rc;
                add_ln_bias_entries(adam[0], c, l, ws + l.part_off, nb, 3 * (int64_t)l.out_p);
            }
        }
        if (l.kind == 2) {  // the impala torso: its own backward (generic engine + row-wise kernels) and optimizer launches, on the caller's stream
            rc = impala_backward(P, c, B);
            if (rc) return rc;
            continue;
        }
        WgradJob job;
        job.layer = i; job.stream = sched.wgrad_stream(i); job.dz = dz_cur; job.dz_ld = dz_ld;
        if (sched.forks_before_dgrad(i)) {
            rc = sched.fork(job.stream);
            if (rc) return rc;
        }
        // data gradient for the layer below first: it reads this layer's weights, which the fused-Adam
        // weight-gradient epilogue below updates in place
        dz_fused = false;
        if (i > 0) {
            rc = data_gradient(c, i, dz_cur, dz_ld, &dz_fused, red);
            if (rc) return rc;
        }
        rc = sched.flush();
        if (rc) return rc;
        bool defer = false;
        if (sched.forks_after_dgrad(i)) {
            rc = sched.fork_after_dgrad(job, &defer);
            if (rc) return rc;
        }
        if (sched.tail_swap && i == 1 && dz_fused) {
            rc = sched.chain_layer0();
            if (rc) return rc;
        }
        if (defer) {
            sched.deferred = job;
        } else {
            rc = weight_gradient(c, job, adam);
            if (rc) return rc;
        }
    }
    return sched.finish();
}

// Gradient clipping (cfg->max_grad_norm > 0; grad_clip.h), on the caller's stream behind the join of both streams and behind
// reduce_rows_kernel.  The entries of both lists in two tables: those with several slabs -> grad_reduce_sq_kernel (the reduced
// gradient over slab 0, one float64 sum of squares per workgroup), those whose one slab IS the reduced gradient (the Dense kernels
// that would have been fused into Adam, the reduced rows, the head bias) -> grad_flat_sq_kernel, 1024 elements per workgroup; the
// dueling head's structural zeros leave the gradient in whichever of the two holds the head kernel.  Then grad_clip_finalize_kernel
// (norm, scale, accumulators -> "grad_clip") and one adam_flat_kernel over every entry at its slab 0, multiplied by the scale.  A
// gradient-only pass runs all of them: the Adam launch is what writes grad_out
static int clipped_adam(const LearnCtx& c, const AdamList* adam) {
    const Plan& P = c.P;
    AdamList multi, single, all;
    for (int k = 0; k < 2; ++k)
        for (const AdamEntry& t : adam[k].e) {
            (t.n_slabs > 1 ? multi : single).e.push_back(t);
            all.add(t.p_off, t.size, t.g, 1, 0, t.wd);
        }
    ISDQN_REQUIRE(all.e.size() <= (size_t)ADAM_MAX_ENTRIES, ISDQN_ERR_UNSUPPORTED, "gradient clipping: more tensors than one optimizer table holds");
    const AdamTable tab_m = multi.table(0), tab_s = single.table(0, GC_FLAT_ELEMS), tab_a = all.table(0, GC_FLAT_ELEMS);
    const int n_part = tab_m.total_blocks + tab_s.total_blocks;
    ISDQN_REQUIRE(n_part <= P.gc_part_cap, ISDQN_ERR_SHAPE, "gradient clipping: more workgroups than the partials region holds");
    GradClipMask dm{-1, 0, 0, 0, 0, 0, 0};
    if (P.dueling) dm = GradClipMask{c.head().w_off, c.head().in_p, P.raw, P.n_actions, P.head_nb > 0 ? P.head_nb : 1, P.duel_f2, P.duel_f};
    double* partials = reinterpret_cast<double*>(c.ws + P.gc_part_off);
    float* gc = c.ws + P.gc_off;
    if (tab_m.total_blocks > 0) {
        hipLaunchKernelGGL(grad_reduce_sq_kernel, dim3(tab_m.total_blocks), dim3(256), 0, c.st, tab_m, dm, partials);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (tab_s.total_blocks > 0) {
        hipLaunchKernelGGL(grad_flat_sq_kernel, dim3(tab_s.total_blocks), dim3(GC_FLAT_THREADS), 0, c.st, tab_s, dm, partials + tab_m.total_blocks);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(GC_FIN_THREADS), 0, c.st, (const double*)partials, n_part, c.cfg->max_grad_norm, gc,
                       c.update() ? 1 : 0);
    ISDQN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(adam_flat_kernel, dim3(tab_a.total_blocks), dim3(GC_FLAT_THREADS), 0, c.st, tab_a, c.params, c.adam_m, c.adam_v,
                       (const float*)(c.ws + P.adam_tab_off), c.cfg->learning_rate, c.cfg->adam_b1, c.cfg->adam_b2, c.cfg->adam_eps, c.grad_out,
                       c.ws + P.wsplit_off, c.update() ? 1 : 0, (const float*)(gc + 1));
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// the partial-row reductions the fused data gradients left, and the optimizer launches of both streams; the call is complete on
// the caller's stream behind it (and the next call may touch the workspace)
static int learn_optimizer(const LearnCtx& c, const BackwardSchedule& sched, const AdamList* adam, const ReduceJobs& red) {
    auto run_adam = [&](const AdamList& list, hipStream_t s) { return adam_launch(list, s, c.P, c); };
    int rc;
    if (sched.adam_on_side()) {
        rc = run_adam(adam[1], c.wst);
        if (rc) return rc;
    } else if (c.ss) {  // all weight gradients done before Adam
        rc = chain(c.ss, c.wst, c.st);
        if (rc) return rc;
    }
    if (red.n > 0) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(red.block_start[red.n]), dim3(256), 0, c.st, red);
        ISDQN_HIP_CHECK(hipGetLastError());
    }
    if (c.P.grad_clip) {  // (adam_on_side() is false: the side stream was joined above, every gradient of the step is final here)
        rc = clipped_adam(c, adam);
    } else {
        rc = run_adam(adam[0], c.st);
        if (rc) return rc;
        rc = sched.adam_on_side() ? chain(c.ss, c.wst, c.st) : run_adam(adam[1], c.st);
    }
    if (rc || !c.P.dueling) return rc;
    // dueling heads: behind the head's Adam the structural zeros of the head kernel are written again (Adam is per element: this equals
    // a masked gradient exactly).  What orders the launch: without a head chain BackwardSchedule keeps the head's weight gradient --
    // fused into Adam, or reduced by run_adam(adam[0]) above -- and its bias entry on the caller's stream, and whatever the side stream
    // updates is joined into the caller's stream by chain(c.ss, c.wst, c.st), in front of Adam or in the line above; so every optimizer
    // launch of the step is behind this point on c.st.  A schedule that moves the head's update to the side stream has to keep that
    // join in front of this launch.  A gradient-only pass masks grad_out alone
    const Plan& P = c.P;
    const Layer& head = c.head();
    const int64_t threads = (int64_t)P.raw * P.duel_f2;
    float* const none = nullptr;
    hipLaunchKernelGGL(duel_mask_kernel, dim3((unsigned)((threads + DUEL_THREADS - 1) / DUEL_THREADS)), dim3(DUEL_THREADS), 0, c.st,
                       c.update() ? c.params : none, c.update() ? c.adam_m : none, c.update() ? c.adam_v : none, c.update() ? c.ws + P.wsplit_off : none,
                       c.grad_out, head.w_off, head.in_p, P.raw, P.n_actions, P.head_nb > 0 ? P.head_nb : 1, P.duel_f2);
    ISDQN_HIP_CHECK(hipGetLastError());
    return ISDQN_OK;
}

// What a call that carries ISDQN_BATCH_MIXTURE must be (include/isdqn_hip.h, isdqn_batch_mixture: the refusals, in this order)
static int check_mixture(const Plan& P, const LearnCall& call) {
    const isdqn_net_config* cfg = call.cfg;
    ISDQN_REQUIRE(call.mix_alpha != nullptr, ISDQN_ERR_ARG, "isdqn_batch_mixture: null alpha");
    ISDQN_REQUIRE(call.n_mix == cfg->n_heads, ISDQN_ERR_ARG, "isdqn_batch_mixture: n_mix must equal cfg->n_heads");
    ISDQN_REQUIRE(cfg->n_heads <= MIX_MAX_HEADS, ISDQN_ERR_UNSUPPORTED, "the mixture is built for at most 1024 heads");
    ISDQN_REQUIRE(cfg->n_bins == 0, ISDQN_ERR_UNSUPPORTED, "the mixture on histogram heads is not built (scalar heads only)");
    ISDQN_REQUIRE(cfg->n_quantiles == 0, ISDQN_ERR_UNSUPPORTED, "the mixture on quantile heads is not built (scalar heads only)");
    ISDQN_REQUIRE(!(cfg->munchausen_tau > 0.f), ISDQN_ERR_UNSUPPORTED, "the mixture with Munchausen targets is not built");
    ISDQN_REQUIRE(!P.bn, ISDQN_ERR_UNSUPPORTED, "the mixture on BatchNorm networks is not built");
    ISDQN_REQUIRE(!(call.cql_alpha > 0.f), ISDQN_ERR_UNSUPPORTED, "a conservative term on the mixture is a follow-up");
    ISDQN_REQUIRE(call.sel.K <= 0, ISDQN_ERR_UNSUPPORTED, "the mixture regresses all heads: isdqn_net_grad_on_batch with n_pairs > 0 is refused");
    return ISDQN_OK;
}

// (`call`: by value -- the moments of a gradient-only pass, the resolved heads and the destinations of q_values / targets are filled in here)
static int learn_or_loss(LearnCall call) {
    const isdqn_net_config* cfg = call.cfg;
    const isdqn_batch* batch = call.batch;
    const bool learn = call.learn();
    int rc;
    const Plan* Pp = cached_plan(cfg, &rc);
    if (!Pp) return rc;
    const Plan& P = *Pp;
    ISDQN_REQUIRE(call.params && batch && call.losses && call.ws, ISDQN_ERR_ARG, "null pointer");
    if ((rc = check_decay(call.weight_decay, call.decay_kinds))) return rc;
    if ((rc = check_conservative(call.cql_alpha))) return rc;
    ISDQN_REQUIRE(batch->B == P.B, ISDQN_ERR_SHAPE, "batch->B != cfg->batch_size");
    ISDQN_REQUIRE(batch->action && batch->reward && batch->terminal, ISDQN_ERR_ARG, "null batch field");
    rc = check_input(cfg, batch->frames, batch->frame_stride, batch->frame_ids, batch->state);
    if (rc) return rc;
    if (cfg->arch == ISDQN_ARCH_FC) ISDQN_REQUIRE(batch->next_state != nullptr, ISDQN_ERR_ARG, "fc needs next_state");
    if (call.mode == LearnMode::Learn) ISDQN_REQUIRE(call.adam_m && call.adam_v && call.adam_count, ISDQN_ERR_ARG, "null optimizer state");
    if (call.mode == LearnMode::GradOnly) {
        ISDQN_REQUIRE(call.grad_out != nullptr, ISDQN_ERR_ARG, "a gradient-only pass needs grad_out");
        moments_of_a_gradient_only_pass(call);
    }
    if (P.bn) {  // BatchNorm: the layer-by-layer form over all 2B rows (batchnorm.h)
        ISDQN_REQUIRE(call.target_params == nullptr || call.mode == LearnMode::GradOnly, ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: separate target parameters only in gradient-only passes (the reference's DQN cannot run with "
                      "batch_norm, dqn.py:86)");
        ISDQN_REQUIRE(call.target_params == nullptr || cfg->double_q == 0, ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: double_q with separate target parameters is not defined (no statistics for an online forward "
                      "of the next states)");
        ISDQN_REQUIRE(call.target_params == nullptr || !P.munchausen, ISDQN_ERR_UNSUPPORTED,
                      "BatchNorm networks: Munchausen targets with separate target parameters are not defined (no statistics for a target "
                      "forward of the states)");
    }
    if (call.mixture) {  // (in front of the first launch: a refused call launches nothing)
        if ((rc = check_mixture(P, call))) return rc;
        call.sel = HeadSel{0, 0, 1};  // one regressed "pair": the mixture of all heads on the mixture of all heads
    }
    const bool plan_heads = call.sel.K <= 0;
    rc = resolve_heads(P, call.sel);
    if (rc) return rc;
    if (call.q_values == nullptr) call.q_values = call.ws + P.qv_off;
    if (call.targets == nullptr) call.targets = call.ws + P.tg_off;
    if (P.bn) return bn_learn_or_loss(P, call);
    LearnCtx c(call, P);
    // (same head of the same rows selecting and valuing -- TF-DQN -- is the max form: Q[argmax Q] == max Q)
    c.double_q = cfg->double_q != 0 && !(call.target_params == nullptr && call.sel.on0 == call.sel.tg0);
    c.munchausen = P.munchausen;
    head_chain_plan(c, plan_heads);
    c.ss = learn ? side_stream() : nullptr;
    c.wst = c.ss ? c.ss->stream : c.st;

    rc = learn_forward(c);
    if (rc) return rc;
    rc = learn_loss(c);
    if (rc) return rc;
    if (!learn) {
        if (batch->priorities_ready != nullptr) ISDQN_HIP_CHECK(hipEventRecord((hipEvent_t)batch->priorities_ready, c.st));
        return ISDQN_OK;
    }
    AdamList adam[2];  // [0] caller's stream, [1] weight-gradient stream
    ReduceJobs red;    // partial-row reductions left by the fused data gradients (one launch before Adam)
    red.n = 0;
    red.block_start[0] = 0;
    BackwardSchedule sched(c, adam);
    rc = sched.begin();
    if (rc) return rc;
    rc = learn_backward(c, sched, adam, &red);
    if (rc) return rc;
    return learn_optimizer(c, sched, adam, red);
}
