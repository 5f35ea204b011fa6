"""GPU parity of the BatchNorm variants (slimdqn/networks/architectures/dqn.py:52-53, 59-60, 66-67, 73-74, 100-101; learn step
isdqn.py:82-103 with batch_norm=True) against the CPU oracle (oracle/network.py: parity unpinned, like the rest of the network
numerics -- the reference holds no numbers and flax is not installed), through the C ABI (csrc/batchnorm.h).

What is compared: the acting forward on the running averages; q-values / targets / per-head losses of the training-mode pass on
concat(state, next_state) within 1e-3; every leaf's first-step gradient (BatchNorm scale / bias included: they carry the part of the
gradient that reaches the next-state rows); the running averages a learn step leaves; parameters after Adam; three chained steps.
Below them, stage by stage on the run's own operands (bf16x3 and bf16):
test_batchnorm_stages_match_a_model_of_each_kernel_on_its_own_operands."""
import numpy as np
import pytest
import torch

from oracle.replay_buffer import ReplayElement
from tests.gpu_helpers import device_batch, make_frame_batch, make_pair

pytestmark = pytest.mark.gpu

CNN = [
    # obs, feats, K, A, B, layer_norm
    pytest.param(((84, 84, 4), (7, 9, 11, 13), 3, 5, 6, True), id="tiny-ln"),
    pytest.param(((84, 84, 4), (16, 20, 12, 24), 2, 3, 5, False), id="tiny-noln"),
    pytest.param(((84, 84, 4), (32, 64, 64, 512), 9, 9, 8, True), id="headline-arch-B8"),
    pytest.param(((44, 44, 2), (8, 16, 8, 32), 2, 4, 9, True), id="44x44x2-B9-ragged"),
]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _check_step(oracle, eng, batch, ref, n_steps=3, grad_tol=3e-3, later_loss_tol=1e-3, trajectory=True):
    """``trajectory=False`` (the impala torso: max-pool winners and ReLU masks of 2B small images -- a few decisions differ between two
    fp32-class forwards, and Adam moves an entry whose gradient changes sign by a full lr either way): the first step's update is
    checked against Adam applied to the path's OWN gradient instead of against the oracle's parameters, later losses loosely."""
    K = oracle.n_bellman_iterations
    # ---- training-mode pass: q-values, targets, losses (batch statistics of the 2B rows) ----
    o_q, o_t, o_td = oracle.loss_terms(oracle.params, ref)
    o_loss = o_td.mean(0).detach().numpy()
    stats_before = eng.export_batch_stats()
    losses = eng.loss_on_batch(batch).cpu().numpy()
    assert np.abs(eng.q_values.cpu().numpy() - o_q.detach().numpy()).max() < 1e-3
    assert np.abs(eng.targets.cpu().numpy() - o_t.detach().numpy()).max() < 1e-3
    assert np.abs(losses - o_loss).max() < 1e-3 * max(1.0, np.abs(o_loss).max())
    after_loss = eng.export_batch_stats()
    for m in stats_before:  # loss_on_batch leaves the running averages alone
        for n in stats_before[m]:
            np.testing.assert_array_equal(after_loss[m][n], stats_before[m][n])

    grad = torch.zeros_like(eng.params)
    p, st = oracle.params, oracle.optimizer_state
    for step in range(n_steps):
        o_grads, _ = oracle.grads(p, ref)
        p, st, o_losses = oracle.learn_on_batch(p, st, ref)
        p0 = eng.params.clone()
        losses = eng.learn_on_batch(batch, grad_out=grad).cpu().numpy()
        assert np.abs(losses - o_losses).max() < (1e-3 if step == 0 else later_loss_tol) * max(1.0, np.abs(o_losses).max()), f"step {step}"
        if step == 0:
            g = eng.internal_to_flax_grads(grad)
            for mod in o_grads:
                for leaf in o_grads[mod]:
                    e = _rel(g[mod][leaf], o_grads[mod][leaf].numpy())
                    assert e < grad_tol, f"grad {mod}/{leaf}: rel err {e}"
            num = sum(float(np.sum((np.asarray(g[m][n], np.float64) - o_grads[m][n].numpy()) ** 2)) for m in o_grads for n in o_grads[m])
            den = sum(float(np.sum(o_grads[m][n].numpy().astype(np.float64) ** 2)) for m in o_grads for n in o_grads[m])
            assert num <= (3 * grad_tol) ** 2 * den, f"whole gradient, Euclidean: {(num / den) ** 0.5}"
            if not trajectory:  # optax.adam's first step on the path's own gradient: p -= lr * g / (|g| + eps), optimised tensors only
                want = p0 - eng.cfg.learning_rate * grad / (grad.abs() + eng.cfg.adam_eps)
                sel = torch.zeros_like(grad, dtype=torch.bool)
                for info in eng.infos:
                    if info.kind < 7:
                        sel[info.offset : info.offset + info.size] = True
                assert float((eng.params - want)[sel].abs().max()) < 2e-6
            pri = eng.priorities.cpu().numpy()
            exp = np.sqrt(o_td.detach().numpy().mean(1) + 1e-10)
            assert np.abs(pri - exp).max() < 1e-2 * max(1.0, exp.max())
        got_stats = eng.export_batch_stats()
        for m, l in oracle.batch_stats.items():  # ra = 0.99 ra + 0.01 batch (isdqn.py:87-88)
            for n, t in l.items():
                d = np.abs(got_stats[m][n] - t.numpy()).max()
                # (after the first update the two parameter sets differ by Adam's normalised steps: activations, and with
                # them the batch statistics, drift by ~1e-3)
                assert d < (2e-5 if step == 0 else max(2e-4, 0.1 * later_loss_tol)) * max(1.0, float(t.abs().max())), f"step {step}: running {n} of {m}: {d}"
    assert int(eng.adam_count.item()) == n_steps
    if not trajectory:
        return
    got = eng.export_flax()
    for mod in p:
        for leaf in p[mod]:
            d = np.abs(got[mod][leaf] - p[mod][leaf].numpy()).max()
            # three Adam steps of lr = 1e-3: an element whose gradient is ~0 can take its normalised steps with the other sign
            assert d < 3e-3, f"param {mod}/{leaf}: {d}"
    assert int(eng.adam_count.item()) == n_steps


@pytest.mark.parametrize("cfg", CNN)
def test_cnn_batchnorm_matches_the_oracle(cfg):
    obs, feats, K, A, B, ln = cfg
    oracle, eng, _ = make_pair(feats, K, A, B, obs=obs, layer_norm=ln, seed=3, batch_norm=True)
    h, w, stack = obs
    frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=11, h=h, w=w, stack=stack)
    batch = device_batch(eng, frames, ids, action, reward, terminal)

    # ---- acting forward: the running averages (isdqn.py:130) ----
    both = torch.cat((torch.tensor(ref.state), torch.tensor(ref.next_state)))
    q_run = oracle.apply(oracle.params, both, use_running_average=True).detach().numpy()
    flat_ids = np.concatenate([ids[:, :stack], ids[:, stack:]], 0).copy()
    q = eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1], frame_ids=torch.from_numpy(flat_ids).cuda(), n_rows=2 * B)
    q = q.cpu().numpy().reshape(2 * B, 1 + K, A)
    assert np.abs(q - q_run).max() < 1e-3 * max(1.0, np.abs(q_run).max()), f"acting forward max err {np.abs(q - q_run).max()}"
    # one row alone gives the same values as inside the batch: nothing of the acting path depends on the other rows
    q1 = eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1], frame_ids=torch.from_numpy(flat_ids[3:4].copy()).cuda(), n_rows=1)
    assert np.abs(q1.cpu().numpy().reshape(1 + K, A) - q[3]).max() < 1e-5

    _check_step(oracle, eng, batch, ref)


IMPALA = [
    pytest.param(((84, 84, 4), (8, 16, 8, 32), 2, 3, 8, True), id="84x84x4-ln-B8"),
    pytest.param(((36, 36, 2), (16, 8, 16, 24), 3, 4, 9, False), id="36x36x2-noln-B9"),
]


@pytest.mark.parametrize("cfg", IMPALA)
def test_impala_batchnorm_matches_the_oracle(cfg):
    """The impala torso with BatchNorm (dqn.py:29-30, 78-79, 86-88): a site on x / 255, one behind the ReLU of each of the six residual
    blocks ("Stack_s/BatchNorm_b"), one per feature behind the flatten, one behind Dense_0."""
    obs, feats, K, A, B, ln = cfg
    # (float64 oracle: per-feature statistics over 16-18 rows divide by small deviations, fp32 noise on the oracle's side would
    # eat a good part of the 1e-3 bar.  The gradient bound is direct -- no pinned ReLU / max-pool decisions as in
    # tests/test_gpu_impala.py, whose independent-oracle bound is 15 % Euclidean for the same reason -- hence 5e-2 of each leaf's
    # largest entry and 15 % of the whole vector; measured: <= 1.6e-2 per leaf)
    oracle, eng, params = make_pair(feats, K, A, B, arch="impala", obs=obs, layer_norm=ln, seed=6, batch_norm=True, dtype=torch.float64)
    assert "Stack_2/BatchNorm_1" in params and eng.export_batch_stats()["Stack_0/BatchNorm_0"]["var"].shape == params["Stack_0/BatchNorm_0"]["scale"].shape
    h, w, stack = obs
    frames, ids, action, reward, terminal, ref = make_frame_batch(B, A, seed=13, h=h, w=w, stack=stack)
    batch = device_batch(eng, frames, ids, action, reward, terminal)
    both = torch.cat((torch.tensor(ref.state), torch.tensor(ref.next_state)))
    q_run = oracle.apply(oracle.params, both, use_running_average=True).detach().numpy()
    flat_ids = np.concatenate([ids[:, :stack], ids[:, stack:]], 0).copy()
    q = eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1], frame_ids=torch.from_numpy(flat_ids).cuda(), n_rows=2 * B)
    q = q.cpu().numpy().reshape(2 * B, 1 + K, A)
    assert np.abs(q - q_run).max() < 1e-3 * max(1.0, np.abs(q_run).max()), f"acting forward max err {np.abs(q - q_run).max()}"
    _check_step(oracle, eng, batch, ref, n_steps=2, grad_tol=5e-2, later_loss_tol=5e-2, trajectory=False)


FC = [
    pytest.param((8, (100, 100), 1, 4, 32, True), id="lunar-lander-100x100-ln"),
    pytest.param((6, (24, 40, 16), 3, 3, 10, False), id="three-hidden-noln-B10"),
]


@pytest.mark.parametrize("cfg", FC)
def test_fc_batchnorm_matches_the_oracle(cfg):
    d, feats, K, A, B, ln = cfg
    oracle, eng, _ = make_pair(feats, K, A, B, arch="fc", obs=(d,), layer_norm=ln, seed=5, adam_eps=1e-8, batch_norm=True)
    rng = np.random.default_rng(7)
    st, nx = rng.normal(size=(B, d)).astype(np.float32), rng.normal(size=(B, d)).astype(np.float32)
    action = rng.integers(0, A, B).astype(np.int32)
    reward = rng.normal(size=B).astype(np.float32)
    terminal = (rng.random(B) < 0.3).astype(np.uint8)
    ref = ReplayElement(state=st, action=action.astype(np.int64), reward=reward.astype(np.float64), next_state=nx,
                        is_terminal=terminal.astype(np.int64))
    dev = lambda a: torch.from_numpy(a).cuda()
    batch = eng.make_batch(state=dev(st), next_state=dev(nx), action=dev(action), reward=dev(reward), terminal=dev(terminal))
    q_run = oracle.apply(oracle.params, torch.tensor(st), use_running_average=True).detach().numpy()
    q = eng.forward(obs=dev(st), n_rows=B).cpu().numpy().reshape(B, 1 + K, A)
    assert np.abs(q - q_run).max() < 1e-3 * max(1.0, np.abs(q_run).max())
    _check_step(oracle, eng, batch, ref)


def test_batchnorm_learn_steps_are_bitwise_repeatable():
    feats, K, A, B = (16, 32, 32, 64), 3, 4, 16
    outs = []
    for _ in range(2):
        _, eng, _ = make_pair(feats, K, A, B, seed=9, batch_norm=True)
        frames, ids, action, reward, terminal, _ref = make_frame_batch(B, A, seed=4)
        batch = device_batch(eng, frames, ids, action, reward, terminal)
        for _s in range(3):
            eng.learn_on_batch(batch)
        outs.append((eng.params.cpu().numpy().copy(), eng.adam_v.cpu().numpy().copy(), eng.losses.cpu().numpy().copy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_unbuilt_batchnorm_combinations_raise():
    _, eng, _ = make_pair((7, 9, 11, 13), 2, 3, 4, seed=1, batch_norm=True)
    frames, ids, action, reward, terminal, _ref = make_frame_batch(4, 3, seed=2)
    batch = device_batch(eng, frames, ids, action, reward, terminal)
    with pytest.raises(Exception):  # the DQN form (separate target parameters) does not exist with BatchNorm -- in the reference either
        eng.learn_on_batch_target(batch, eng.params.clone())
    with pytest.raises(Exception):
        eng.loss_on_batch_target(batch, eng.params.clone())
    # (the gradient-only pass takes separate target parameters: the analysis agents, tests/test_gpu_analysis_agents.py)


def test_agent_with_batchnorm_trains_acts_and_exports_like_the_oracle_agent():
    """iSDQN(batch_norm=True) end to end on the device replay (captured one-step graph included): per-step losses against the
    oracle agent fed from the oracle replay with the same seed, the greedy action from the running averages, and the model pickle
    layout {"params", "batch_stats"}."""
    from oracle.isdqn import iSDQN as Oracle
    from oracle.replay_buffer import ReplayBuffer as ORB, TransitionElement as OT
    from oracle.samplers import UniformSamplingDistribution as OU
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    K, A, B, feats = 2, 4, 8, [8, 16, 16, 32]
    agent = iSDQN(0, (84, 84, 4), A, K, feats, True, True, "cnn", 1e-3, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=B)
    model = agent.get_model()["params"]
    assert set(model) == {"params", "batch_stats"} and model["batch_stats"]["BatchNorm_0"]["var"].shape == (84, 84)
    assert model["params"]["BatchNorm_3"]["scale"].shape == (11 * 11 * 16,) and model["params"]["Conv_0"]["kernel"].shape == (8, 8, 4, 8)
    oracle = Oracle(0, (84, 84, 4), A, K, feats, True, True, "cnn", 1e-3, 0.99, 1, 1, 6, adam_eps=1.5e-4, params=model["params"])
    rb = ReplayBuffer(UniformSamplingDistribution(1), B, 64)
    orb = ORB(OU(1), B, 64)
    rng = np.random.default_rng(0)
    for t in range(30):
        obs = rng.integers(0, 256, (84, 84), dtype=np.uint8)
        a, r, term = int(rng.integers(0, A)), float(rng.choice([-1.0, 0.0, 1.0])), bool(t % 13 == 12)
        rb.add(TransitionElement(obs, a, r, term, term))
        orb.add(OT(obs, a, r, term, term))
    per_step = []
    for step in range(1, 5):
        agent.update_online_params(step, rb)
        oracle.update_online_params(step, orb)
        per_step.append((agent._engine.losses.cpu().numpy().astype(np.float64), oracle.cumulated_losses.copy()))
    # per-step losses: the first step starts from identical parameters (1e-3); afterwards the two trajectories take Adam's
    # normalised steps apart and 16-row batch statistics amplify that (a few per cent after four steps at lr = 1e-3)
    prev = np.zeros(K)
    for i, (got, cum) in enumerate(per_step):
        exp = cum - prev
        prev = cum
        tol = 1e-3 if i == 0 else 5e-2
        assert np.abs(got - exp).max() < tol * max(1.0, np.abs(exp).max()), (i, got, exp)
    acc = agent._engine.losses_accum.cpu().numpy()
    np.testing.assert_allclose(acc, np.sum([g for g, _ in per_step], axis=0), rtol=1e-5)  # the device accumulator (isdqn.py:62)
    stats = agent.get_model()["params"]["batch_stats"]
    for m, l in oracle.batch_stats.items():
        for n, t in l.items():
            assert np.abs(stats[m][n] - t.numpy()).max() < 5e-3 * max(1.0, float(t.abs().max())), (m, n)  # (four drifting steps, see above)
    # acting (isdqn.py:127-135, use_running_average=True) on the ORACLE's trained model, handed over as the reference's pytree
    # {"params", "batch_stats"}: no trajectory drift between the two sides, so the 1e-3 bar applies
    state = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
    o_model = oracle.get_model()["params"]
    q_all = oracle.apply(oracle.params, torch.tensor(state)[None], use_running_average=True)[0].detach().numpy()
    q_a = agent.q_values(o_model, state)
    assert np.abs(q_a - q_all).max() < 1e-3 * max(1.0, np.abs(q_all).max())
    for head in range(K):
        top2 = np.sort(q_all[1 + head])[-2:]
        if top2[1] - top2[0] > 2e-3:  # (a near tie may legitimately resolve differently within the parity tolerance)
            assert agent.best_action(o_model, state, key=head) == oracle.best_action(oracle.params, state, head)
    # and on the agent's own parameters the greedy action is the argmax of its own q row
    q_own = agent.q_values(agent.params, state)
    for head in range(K):
        assert agent.best_action(agent.params, state, key=head) == int(np.argmax(q_own[1 + head]))


def test_tfdqn_with_batchnorm_matches_the_oracle():
    """TFDQN(batch_norm=True) (tfdqn.py:56-80): one shared-parameter head regressed on its own stop-gradient target, training-mode
    BatchNorm over concat(state, next_state); a learn step's loss, running averages and parameters against the oracle's."""
    from oracle.dqn import TFDQN as Oracle
    from slimdqn.networks.tfdqn import TFDQN

    A, B, feats = 4, 8, [8, 16, 16, 32]
    agent = TFDQN(0, (84, 84, 4), A, feats, True, True, "cnn", 1e-3, 0.99, 1, 1, 6, adam_eps=1.5e-4, batch_size=B)
    model = agent.get_model()["params"]
    assert set(model) == {"params", "batch_stats"}
    oracle = Oracle(0, (84, 84, 4), A, feats, True, True, "cnn", 1e-3, 0.99, 1, 1, 6, adam_eps=1.5e-4, params=model["params"])
    _frames, _ids, _a, _r, _t, ref = make_frame_batch(B, A, seed=21)
    o_loss = float(oracle.loss_on_batch(oracle.params, ref)[0])
    oracle.params, oracle.optimizer_state, o_loss2 = oracle.learn_on_batch(oracle.params, oracle.optimizer_state, ref)
    _, _, loss = agent.learn_on_batch(agent.params, agent.optimizer_state, ref)
    got = float(loss.cpu().numpy().reshape(-1)[0])
    assert abs(got - o_loss) < 1e-3 * max(1.0, abs(o_loss)) and abs(o_loss - o_loss2) < 1e-12
    after = agent.get_model()["params"]
    for m, l in oracle.batch_stats.items():
        for n, t in l.items():
            assert np.abs(after["batch_stats"][m][n] - t.numpy()).max() < 2e-5 * max(1.0, float(t.abs().max())), (m, n)
    exp = oracle.get_model()["params"]["params"]
    for m in exp:
        for n in exp[m]:
            assert np.abs(after["params"][m][n] - exp[m][n]).max() < 2.001e-3, (m, n)  # one Adam step of lr = 1e-3


@pytest.mark.parametrize("algo, arch", [("isdqn", "cnn"), ("tfdqn", "cnn"), ("isdqn", "impala")])
def test_entry_points_with_the_batch_norm_flag(tmp_path, algo, arch):
    """`-bn` through the reference's entry points (experiments/atari/isdqn.py, tfdqn.py; launch_job/atari/launch.sh BATCH_NORM=1):
    training runs, the vectorised acting path reads the running averages, and the saved model carries both Flax collections."""
    import json
    import pickle

    from experiments.atari import isdqn as e_isdqn, tfdqn as e_tfdqn

    run = {"isdqn": e_isdqn.run, "tfdqn": e_tfdqn.run}[algo]
    name = f"bn{algo}{arch}_Synthetic"
    argv = ["-en", name, "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-rbc", "200", "-bs", "8", "-n", "1", "-horizon", "40", "-at", arch,
            "-ne", "2", "-ntspe", "48", "-utd", "4", "-nis", "16", "-ed", "100", "-ln", "-bn", "-tuf", "16", "-env", "synthetic", "-nenvs", "2"]
    if algo == "isdqn":
        argv += ["-nbi", "2"]
    run(argv, root=str(tmp_path))
    out = tmp_path / "atari" / "exp_output" / name
    assert json.load(open(out / "parameters.json"))[algo]["batch_norm"] is True  # (an agent parameter: parser_argument.py:27-36)
    model = pickle.load(open(out / algo / "models" / "1", "rb"))["params"]
    assert set(model) == {"params", "batch_stats"}
    stats = model["batch_stats"]
    top = stats["BatchNorm_0"]
    assert top["mean"].shape == (84, 84) and float(np.abs(top["mean"]).max()) > 0.0  # moved off Flax's initial (0, 1) by the learn steps
    if arch == "impala":
        assert stats["Stack_2"]["BatchNorm_1"]["var"].shape == (11, 11) and model["params"]["Stack_0"]["BatchNorm_0"]["scale"].shape == (42, 42)
    else:
        assert model["params"]["BatchNorm_3"]["scale"].shape == (11 * 11 * 8,) and stats["BatchNorm_4"]["var"].shape == (16,)


# ---------------------------------------------------------------------------------------------------------------------------------
# Stage by stage: every kernel of csrc/batchnorm.h and every contraction between them against a float64 model of that ONE stage on
# the HIP run's own input tensor of the stage (tests/helpers/batchnorm_stages.py, tests/helpers/bf16_model.py).
def _bn_stage_runs():
    from tests.helpers.batchnorm_stages import CASES

    both = ("cnn-84x84x4-B40", "fc-d6-B37")
    return [pytest.param(c, p, id=f"{c}-{p}") for c in CASES for p in (("bf16x3", "bf16") if c in both else
                                                                         ("bf16",) if c == "cnn-headline-B8" else ("bf16x3",))]


@pytest.mark.parametrize("case,precision", _bn_stage_runs())
def test_batchnorm_stages_match_a_model_of_each_kernel_on_its_own_operands(case, precision):
    """loss_on_batch, learn_on_batch(grad_out=g), then forward on the running averages; every stored tensor against ONE stage
    recomputed in float64 from the run's own input of that stage.  `passes` = 3 (bf16x3) / 1 (bf16).  Bounds are derived
    (batchnorm_stages.py: ROUNDING * depth * 2^-24 * magnitudes, depth from the kernel's own summation order; bf16_model.py:
    c 2^-24 S), not fitted.  Every row and element of every tensor named here is asserted.

    Cases (batchnorm_stages.CASES): cnn-84x84x4-B40 -- N = 80, the spatial lane loop's second iteration, partly filled;
    cnn-52x60x2-B33-noln -- N = 66, C < Cp at the input site (2 frames of 8 channels), a spatial site (20 / 24) and the flatten site (12 / 16), non-square P;
    cnn-headline-B8 in bf16 -- the 64-channel routes and a 512-wide feature site; fc-d6-B37 -- N = 74 (nine full row slices and a
    partial one), width 304 (two workgroups, the second partly on), one head regressed on its own target (TF-DQN: built directly,
    make_pair always adds a target head).

    Forward, all 2B rows, in network order:
      bn/x0                == split_words(frames_to_x) (cnn) / concat(state, next_state) (fc)                    bit for bit
      bn/<site>/mean, var  ~  bn_stats(own input, S8 hi + lo)                                                    d_mean, d_var
      bn/<site>/out (S8)   ~  bn_apply(own input, own mean / var, parameters); padded channels 0; well-formed S8 words
      z/<layer>            ~  conv / dense(passes, own bn/<site>/out planes, split(W)) + bias   bound(S + |b|, chain_depth);
                              control: the other pass count 4x further away in the 2-norm and outside the bound on half of the
                              elements.  Conv_0 here is the generic engine on an 8-channel S8 input (K = 512): its only test.
      act/<layer> (S8)     ~  ln_relu_fwd(own z);   q ~ the head on the last site's out;   q_values == own q, targets ~ Bellman
      after loss_on_batch the whole parameter buffer (running averages included) is unchanged bit for bit.
    Backward, all 2B rows (dout rows [B, 2B) are filled with 1.0 before the step: the workspace is zero only once):
      dout                 rows [B, 2B) exactly 0; rows [0, B): 2 td / B at (online head + k, a_b), every other column exactly 0
      da (cnn, as left)    ~  conv_dgrad(own dz/Conv_0): the data gradient into the first convolution's input
      bn/BatchNorm_0/dbias, dscale (cnn)  ~  s1, s2 of bn_backward(own bn/x0, own da)                            d_s1, d_s2
      every other site: da recomputed from own dz/<layer above> (or dout) and split(W) at `passes` with its bound E_da;
        dbias, dscale      ~  s1, s2 of bn_backward(own act, da), bounds with E_da carried in
        dz/<layer> (S8)    ~  ln_relu_bwd(own z, own ReLU mask, dx), dx from da and the run's OWN s1 / s2, E_da carried through
        fc: region da, as left, ~ dx of BatchNorm_0
      BatchNorm scale / bias leaves of g == the dscale / dbias regions bit for bit (one slab)
      kernel leaves ~ conv_wgrad / wgrad(passes, own operands) over the 2B rows, bias leaves ~ sum dz  (bf16 model's bounds)
      running averages after the step ~ running(before, own batch mean / var) within 2 ulp
    Acting: forward() of all 2B rows and of row 3 alone, on the updated parameters and their running averages.  On q only, against
    the chain of the same stage functions with every bound carried through the next (bn_apply's E_x, exact_layer, ln_relu_fwd's
    E_z): a worst case in every layer, so loose (reported as bound / max |q|).  And stage by stage on what forward() leaves in the
    workspace: bn/x0, every bn/<site>/out from its own input and the running averages, every act/<layer> through the model of its
    contraction (z is not stored by forward), q from the last site's out, with the pass-count control.

    The impala torso's BatchNorm sites (the input site on bn/x0, "Stack_s/BatchNorm_b" on imp/s{s}/a1_{b}, the feature site on
    act/Impala: the same six kernels) are held the same way in tests/test_gpu_impala_backward.py, forward, backward, running averages
    and acting.  Not covered here: the LayerNorm scale / bias leaves (tests/test_gpu_dense_routes.py, and the impala blocks' in
    tests/test_gpu_impala_backward.py).

    Measured on the MI355X, max over the 6 runs (max |d| / bound; against 2^-24 S where S is the whole bound, with c):
      mean 0.139, var 0.118                      bn/<site>/out 0.971 (S8 storage's worst case 2^-17 |y| dominates)
      z 0.105; 4.04 against c = 18 .. 150        act 0.71 with LayerNorm, 0.997 without (relu is exact: S8 storage is all that is left)
      q 0.068; 1.23 against c = 18 .. 48         targets 0.32, dout 0.34
      dbias 0.054, dscale 0.041                  dz 0.78 (noln: S8 storage), 0.43 with LayerNorm
      da as left 0.101; 3.07 against c <= 148    kernel leaves 0.185; 3.33 against c = 18 .. 276, bias leaves 0.45
      running mean / var 0.000 of 2 ulp (bit-equal to the fp32 expression on every element)
      acting, own operands: out 0.970, act 0.52, q 0.070; 1.26 against c.  Acting, chain as a whole: 0.002 -- its composed bound
      is 0.036 .. 0.84 of max |q| (bf16x3: fc, noln cnn), 372 x with LayerNorm (row variances over 8 channels) and 4.8 .. 8.5e5 x in
      bf16: a worst case in every layer says nothing there, which is why the acting forward is also checked stage by stage.
    Other pass count outside the bound, smallest share: z 82 % (headline Conv_2 in bf16), q 99 %.
    Mutations (scratch copies of csrc/batchnorm.h, one library each; new runs failing / end-to-end tests of this file failing):
      spatial divisor N * Cp               4 cnn runs (BatchNorm_0/mean, all 7056 elements) / cnn 4, impala 2, tfdqn
      spatial lane loop stops after n < 64 B40 x 2, B33 (BatchNorm_0/mean, every element)   / none: no other test has N > 64
      feature kernel sums 7 of 8 slices    all 6                                            / cnn 4, impala 2, fc 2, tfdqn
      inv_m without the C factor           4 cnn runs (dz/Conv_1)                           / cnn 4, impala 2
      bn_bwd_apply reads the running var   all 6 (dz/Dense_0, dz/Dense_1)                   / cnn 4, impala 2, fc 2
      bn_running_kernel with momentum 0.9  all 6 (running mean)                             / all 9 oracle tests
      bn_zero_kernel skipped               all 6 (next-state rows of dL/dq)                 / none: a fresh workspace is zero"""
    from slimdqn._engine import QNetEngine
    from tests.helpers import batchnorm_stages as BS
    from tests.helpers import bf16_model as M
    from tests.helpers import impala_stages as IS
    from tests.test_gpu_bf16_model import _conv_wgrad_chain, _dense_wgrad_slabs, _fwd_splits

    inp = BS.case_inputs(case)
    cfg = inp["cfg"]
    arch, obs, feats, K, A, B, ln, n_heads = (cfg[k] for k in ("arch", "obs", "feats", "K", "A", "B", "ln", "n_heads"))
    passes, other = (3, 1) if precision == "bf16x3" else (1, 3)
    N2, nha, oh = 2 * B, n_heads * A, 1 if n_heads >= 2 else 0
    nha_p = -(-nha // 8) * 8
    if n_heads == 1 + K:
        _, eng, params = make_pair(feats, K, A, B, arch=arch, obs=obs, layer_norm=ln, seed=BS.PARAM_SEED, batch_norm=True, precision=precision)
        for m in params:  # the host test holds THESE inputs to account (tests/test_batchnorm_stages_host.py)
            for n in params[m]:
                np.testing.assert_array_equal(params[m][n], inp["params"][m][n])
    else:
        eng = QNetEngine(obs, A, n_heads, list(feats), arch, ln, B, gamma_n=0.99, learning_rate=1e-3, adam_eps=1.5e-4, precision=precision,
                         batch_norm=True)
        eng.import_flax(inp["params"], batch_stats=inp["stats"])
    got_stats = eng.export_batch_stats()
    for m in inp["stats"]:
        for n in inp["stats"][m]:
            np.testing.assert_array_equal(got_stats[m][n], inp["stats"][m][n])
    dev = eng.params.device
    d_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if arch == "cnn":
        h, w, stack = obs
        frames, ids = inp["frames"], inp["ids"]
        batch = device_batch(eng, frames, ids, inp["action"], inp["reward"], inp["terminal"])
    else:
        obs_all = np.concatenate([inp["state"], inp["next_state"]])
        batch = eng.make_batch(state=d_(inp["state"]), next_state=d_(inp["next_state"]), action=d_(inp["action"]), reward=d_(inp["reward"]),
                               terminal=d_(inp["terminal"]))
    layers, sites = BS.layers(cfg), BS.site_layout(cfg)
    site_of = {s["layer"]: s for s in sites}
    offs = {i.name.decode(): int(i.offset) for i in eng.infos}

    p_before = eng.params.clone()
    eng.loss_on_batch(batch)
    torch.cuda.synchronize()
    assert torch.equal(eng.params.view(torch.int32), p_before.view(torch.int32)), "loss_on_batch changed the parameter buffer"
    eng.region("dout")[B * nha_p : N2 * nha_p] = 1.0  # whatever an earlier step left there: bn_zero_kernel has to clear it
    g = torch.zeros_like(eng.params)
    eng.learn_on_batch(batch, grad_out=g)
    torch.cuda.synchronize()
    hip_g = eng.internal_to_flax_grads(g)
    p0 = inp["params"]

    usage, report = {}, []

    def check(row, got, want, bnd, S=None, alt=None, elementwise=True, label=None):
        used, ratio, frac = M.check(got, want, bnd, S, alt, elementwise_control=elementwise, label=label or row)
        u = usage.setdefault(row, [0.0, 0.0, 1.0])
        u[0], u[1] = max(u[0], used), max(u[1], ratio or 0.0)
        u[2] = min(u[2], frac) if frac is not None else u[2]
        report.append(f"{label or row}: max |d| / bound = {used:.3f}" + (f", max |d| / 2^-24 S = {ratio:.2f}" if ratio is not None else "")
                      + (f", other passes outside: {frac:.0%}" if frac is not None else ""))

    vec = lambda mod, leaf: torch.from_numpy(np.asarray(p0[mod][leaf], np.float64)).to(dev)
    wsplit = lambda mod: M.split(torch.from_numpy(np.asarray(p0[mod]["kernel"])).to(dev))
    group = lambda s, leaf, src: src[offs[f"{s['name']}/{leaf}"] : offs[f"{s['name']}/{leaf}"] + s["G"]]  # internal groups of a site tensor
    reg = lambda s, name: eng.region(s["prefix"] + name)[: s["G"]]

    def s8(name, rows, pitch):
        hi, lo = M.s8_planes(eng.region(name), rows, pitch)
        assert int(M.s8_malformed(hi, lo).sum()) == 0, f"{name}: elements that are not a nearest-even split"
        return hi, lo

    def site_planes(s, which):
        """(hi, lo) [N2][P][Cp] of a site's S8 input ("src") or output ("out")"""
        name = s["src"] if which == "src" else s["prefix"] + "out"
        return tuple(t.reshape(N2, s["P"], s["Cp"]) for t in s8(name, N2, s["P"] * s["Cp"]))

    def true_planes(s, planes):
        """a site's planes as the next layer reads them: true channels, [N2][P * C]"""
        return tuple(t[:, :, : s["C"]].reshape(N2, -1) for t in planes)

    def site_forward(s):
        x = sum(site_planes(s, "src"))
        mean, var, d_mean, d_var = BS.bn_stats(x, s["spatial"], s["C"])
        own_mean, own_var = reg(s, "mean").double(), reg(s, "var").double()
        check("mean", own_mean, mean, d_mean, label=f"{s['name']}/mean")
        check("var", own_var, var, d_var, label=f"{s['name']}/var")
        y, E = BS.bn_apply(x, own_mean, own_var, group(s, "scale", p_before).double(), group(s, "bias", p_before).double(), s["spatial"], s["C"])
        out = site_planes(s, "out")
        for t in out:
            assert float(t[..., s["C"]:].abs().max() if s["C"] < s["Cp"] else 0.0) == 0.0, f"{s['name']}/out: padded channels are not 0"
        check("out", sum(out), y, E, label=f"{s['name']}/out")
        return out

    # ---------------------------------------------------------------- forward
    if arch == "cnn":
        x0 = IS.frames_to_x(d_(frames), IS.paired_ids(ids, stack), h, w, stack)
        assert torch.equal(eng.region("bn/x0")[: N2 * h * w * 8].view(torch.int32), M.split_words(x0)), "bn/x0 is not the S8 split of uint8 / 255"
        cur = site_forward(site_of[-1])
    else:
        x_fc = d_(obs_all)
        assert torch.equal(eng.region("bn/x0")[: N2 * obs[0]].view(torch.int32), x_fc.reshape(-1).view(torch.int32)), "bn/x0 is not concat(state, next_state)"
        cur = None

    def contraction(i, l, xin, mod, p, src=None):
        """(value + bias, S + |bias|, c) of layer l (None: the head) on input planes xin at p passes; src: the parameters (default: before the step)"""
        src = src or p0
        wt = M.split(torch.from_numpy(np.asarray(src[mod]["kernel"])).to(dev))
        b = torch.from_numpy(np.asarray(src[mod]["bias"], np.float64)).to(dev)
        if l is not None and l["kind"] == 0:
            v, S = M.conv(p, xin, wt, l["s"])
            c = M.chain_depth(l["K"])
        else:
            v, S = M.dense(p, xin, wt)
            in_p = l["in_p"] if l is not None else layers[-1]["cp"]
            out_p = l["cp"] if l is not None else nha_p
            c = M.chain_depth(in_p, slabs=_fwd_splits(N2, out_p, in_p, arch == "fc" and i == 0))
        return v + b, S + b.abs(), c

    def layer_input(i, l, below_out):
        if l is not None and l["kind"] == 0:
            return tuple(t.reshape(N2, l["hin"], l["win"], l["cin_p"])[..., : l["cin"]] for t in below_out)
        if i == 0:
            return M.split(x_fc)
        return true_planes(site_of[i - 1], below_out)

    inputs = {}
    for i, l in enumerate(layers):
        xin = inputs[i] = layer_input(i, l, cur)
        want, S, c = contraction(i, l, xin, l["name"], passes)
        alt, _, _ = contraction(i, l, xin, l["name"], other)
        shape = (N2, l["npix"], l["c"])
        z = eng.region(f"z/{l['name']}")[: N2 * l["npix"] * l["cp"]].reshape(N2, l["npix"], l["cp"])[:, :, : l["c"]].double()
        check("z", z, want.reshape(shape), M.bound(S, c).reshape(shape), S.reshape(shape), alt.reshape(shape), label=f"z/{l['name']} (c = {c})")
        gamma, beta = (vec(l["ln"], k) if l["ln"] else None for k in ("scale", "bias"))
        a, E = M.ln_relu_fwd(z, gamma, beta, torch.zeros_like(z), has_ln=l["ln"] is not None)
        act = sum(s8(f"act/{l['name']}", N2, l["npix"] * l["cp"])).reshape(N2, l["npix"], l["cp"])
        assert float(act[..., l["c"]:].abs().max() if l["c"] < l["cp"] else 0.0) == 0.0, f"act/{l['name']}: padded channels are not 0"
        check("act", act[:, :, : l["c"]], a, E, label=f"act/{l['name']}")
        cur = site_forward(site_of[i])
    head = f"Dense_{sum(l['kind'] == 1 for l in layers)}"
    xin = inputs[len(layers)] = layer_input(len(layers), None, cur)
    want, S, c = contraction(len(layers), None, xin, head, passes)
    alt, _, _ = contraction(len(layers), None, xin, head, other)
    q = eng.region("q")[: N2 * nha_p].reshape(N2, nha_p)[:, :nha]
    check("q", q.double(), want, M.bound(S, c), S, alt, label=f"q (c = {c})")
    a_idx = d_(inp["action"].astype(np.int64))
    cols = (torch.arange(K, device=dev)[None, :] + oh) * A + a_idx[:, None]
    assert torch.equal(eng.q_values, q[:B].gather(1, cols)), "q_values are not the taken actions' q"
    r64, t64 = d_(inp["reward"].astype(np.float64)), d_(inp["terminal"].astype(np.float64))
    tg = M.bellman_targets(q[B:].double(), r64, t64, 0.99, K, A)
    check("targets", eng.targets.double(), tg, M.ROUNDING * 3 * M.U * (r64.abs()[:, None] + tg.abs()) + M.FLOOR)

    # ---------------------------------------------------------------- backward
    dout = eng.region("dout")[: N2 * nha_p].reshape(N2, nha_p)
    assert float(dout[B:].abs().max()) == 0.0, "next-state rows of dL/dq are not zero"
    td = eng.q_values.double() - eng.targets.double()
    want = torch.zeros(B, nha_p, dtype=torch.float64, device=dev).scatter_(1, cols, 2.0 * td / B)
    check("dout", dout[:B].double(), want, M.ROUNDING * 3 * M.U * want.abs() + (want != 0) * M.FLOOR)
    hit = torch.zeros(B, nha_p, dtype=torch.bool, device=dev).scatter_(1, cols, torch.ones_like(cols, dtype=torch.bool))
    assert torch.equal(dout[:B] != 0, hit), "dL/dq: not exactly one non-zero per transition and regressed head"

    dq = M.split(dout[:, :nha])
    wt = wsplit(head)
    da, S = M.dense(passes, dq, tuple(t.T for t in wt))
    E_da = M.bound(S, M.chain_depth(nha_p, epilogue=3))
    dz_planes = {}
    for i in range(len(layers) - 1, -1, -1):
        l, s = layers[i], site_of[i]
        pad = lambda t: BS._pad_channels(t.reshape(N2, s["P"], s["C"]), s["Cp"])
        x = sum(site_planes(s, "src"))
        mean, var, scale = reg(s, "mean").double(), reg(s, "var").double(), group(s, "scale", p_before).double()
        dy, E_dy = pad(da), pad(E_da)
        s1, d_s1, s2, d_s2, _, _ = BS.bn_backward(x, dy, mean, var, scale, s["spatial"], s["C"], E_dy=E_dy)
        own_s1, own_s2 = reg(s, "dbias").double(), reg(s, "dscale").double()
        check("dbias", own_s1, s1, d_s1, label=f"{s['name']}/dbias")
        check("dscale", own_s2, s2, d_s2, label=f"{s['name']}/dscale")
        _, _, _, _, dx, d_dx = BS.bn_backward(x, dy, mean, var, scale, s["spatial"], s["C"], E_dy=E_dy, s1=own_s1, s2=own_s2)
        if arch == "fc" and i == 0:  # nothing is written over BatchNorm_0's in-place backward
            own = eng.region("da")[: N2 * s["Cp"]].reshape(N2, 1, s["Cp"]).double()
            check("da as left", own, dx, d_dx, label="da (fc: dx of BatchNorm_0)")
        z = eng.region(f"z/{l['name']}")[: N2 * l["npix"] * l["cp"]].reshape(N2, l["npix"], l["cp"])[:, :, : l["c"]].double()
        act = sum(M.s8_planes(eng.region(f"act/{l['name']}"), N2, l["npix"] * l["cp"])).reshape(N2, l["npix"], l["cp"])[:, :, : l["c"]]
        gamma = vec(l["ln"], "scale") if l["ln"] else None
        dzm, E = M.ln_relu_bwd(z, gamma, (act > 0).double(), dx[:, :, : l["c"]], d_dx[:, :, : l["c"]], has_ln=l["ln"] is not None)
        dzp = tuple(t.reshape(N2, l["npix"], l["cp"]) for t in s8(f"dz/{l['name']}", N2, l["npix"] * l["cp"]))
        for t in dzp:
            assert float(t[..., l["c"]:].abs().max() if l["c"] < l["cp"] else 0.0) == 0.0, f"dz/{l['name']}: padded channels are not 0"
        dzp = dz_planes[i] = tuple(t[:, :, : l["c"]] for t in dzp)
        check("dz", sum(dzp), dzm, E, label=f"dz/{l['name']}")
        wt = wsplit(l["name"])
        if l["kind"] == 0:
            da, S = M.conv_dgrad(passes, dzp, wt, (l["hin"], l["win"]), l["s"])
            E_da = M.bound(S, M.chain_depth(l["k"] ** 2 * l["cp"], epilogue=4))
        elif i > 0:
            da, S = M.dense(passes, tuple(t.reshape(N2, -1) for t in dzp), tuple(t.T for t in wt))
            E_da = M.bound(S, M.chain_depth(l["cp"], epilogue=3))
    if arch == "cnn":  # the input site: `da` still holds Conv_0's data gradient (bn_site_backward(..., apply = false))
        s = site_of[-1]
        own_da = eng.region("da")[: N2 * s["P"] * 8].reshape(N2, s["P"], 8).double()
        pad = lambda t: BS._pad_channels(t.reshape(N2, s["P"], s["C"]), 8)
        check("da as left", own_da, pad(da), pad(E_da), pad(S), label="da (cnn: data gradient into Conv_0's input)")
        x = sum(site_planes(s, "src"))
        s1, d_s1, s2, d_s2, _, _ = BS.bn_backward(x, own_da, reg(s, "mean").double(), reg(s, "var").double(), group(s, "scale", p_before).double(),
                                                  True, s["C"])
        check("dbias", reg(s, "dbias").double(), s1, d_s1, label=f"{s['name']}/dbias (own da)")
        check("dscale", reg(s, "dscale").double(), s2, d_s2, label=f"{s['name']}/dscale (own da)")

    # ---------------------------------------------------------------- leaves of g, running averages
    for s in sites:
        for leaf, name in (("scale", "dscale"), ("bias", "dbias")):
            assert torch.equal(group(s, leaf, g).view(torch.int32), reg(s, name).view(torch.int32)), f"{s['name']}/{leaf} of g is not the {name} region"
        for leaf, name in (("mean", "mean"), ("var", "var")):
            want, ulp2 = BS.running(group(s, leaf, p_before).cpu().numpy(), reg(s, name).cpu().numpy())
            got = group(s, leaf, eng.params).cpu().numpy().astype(np.float64)
            check(f"running {leaf}", torch.from_numpy(got), torch.from_numpy(want.astype(np.float64)), torch.from_numpy(ulp2), label=f"{s['name']} running {leaf}")
    for i in range(len(layers) + 1):
        l = layers[i] if i < len(layers) else None
        mod = l["name"] if l is not None else head
        dz = dz_planes[i] if l is not None else dq
        xin = inputs[i]
        if l is not None and l["kind"] == 0:
            want, S = M.conv_wgrad(passes, xin, dz, l["k"], l["s"])
            steps, slabs = _conv_wgrad_chain(N2, dict(l, name=l["name"] + " (S8 input)"))
            c = M.ROUNDING * (M.MFMA_TREE + steps + slabs + 2)
        else:
            want, S = M.wgrad(passes, xin, tuple(t.reshape(N2, -1) for t in dz))
            in_p = l["in_p"] if l is not None else layers[-1]["cp"]
            c = M.chain_depth(N2, slabs=_dense_wgrad_slabs(N2, in_p, l["cp"] if l is not None else nha_p))
        gk = torch.from_numpy(np.asarray(hip_g[mod]["kernel"], np.float64)).to(dev)
        check("kernel leaves", gk, want, M.bound(S, c), S, label=f"{mod}/kernel (c = {c})")
        dzv = (dz[0] + dz[1]).reshape(-1, dz[0].shape[-1])
        bS = dzv.abs().sum(0)
        gb = torch.from_numpy(np.asarray(hip_g[mod]["bias"], np.float64)).to(dev)
        check("bias leaves", gb, dzv.sum(0), M.bound(bS, M.chain_depth(0, slabs=dzv.shape[0], epilogue=4)) + M.S8_STORE * bS, label=f"{mod}/bias")

    # ---------------------------------------------------------------- acting: the running averages of the updated parameters
    p1, after = eng.export_flax(), eng.params.clone()
    k64 = lambda mod, leaf: torch.from_numpy(np.asarray(p1[mod][leaf], np.float64)).to(dev)

    def site_running(s, x, E_x):
        return BS.bn_apply(x, *(group(s, k, after).double() for k in ("mean", "var", "scale", "bias")), s["spatial"], s["C"], E_x=E_x)

    if arch == "cnn":
        flat_ids = np.concatenate([ids[:, :stack], ids[:, stack:]], 0).copy()
        fwd = lambda rows: eng.forward(frames=batch._keep[0], frame_stride=frames.shape[1], frame_ids=d_(flat_ids[rows].copy()), n_rows=len(flat_ids[rows]))
        x = sum(M.split(x0)).reshape(N2, h * w, 8)
        y, E = site_running(site_of[-1], x, torch.zeros_like(x))
    else:
        fwd = lambda rows: eng.forward(obs=d_(obs_all[rows].copy()), n_rows=len(obs_all[rows]))
        y, E = None, None

    def acting_stages(q_got, rows):
        """the acting forward's own tensors, as it left them in the workspace, one stage at a time: bn/<site>/out from its own input and
        the running averages, act/<layer> through the model of its contraction on own bn/<site>/out (z is not stored: E_z goes through
        ln_relu_fwd, as for the next-state rows in test_gpu_bf16_model.py), q on the last site's out"""
        n = len(range(N2)[rows])
        cur_ = None
        if arch == "cnn":
            assert torch.equal(eng.region("bn/x0")[: n * h * w * 8].view(torch.int32), M.split_words(x0[rows])), "acting: bn/x0"
        for i, l in enumerate(layers + [None]):
            sb = site_of.get(i - 1)
            if sb is not None:
                pitch = sb["P"] * sb["Cp"]
                x = sum(M.s8_planes(eng.region(sb["src"]), n, pitch)).reshape(n, sb["P"], sb["Cp"])
                y_, E_ = site_running(sb, x, None)
                hi, lo = M.s8_planes(eng.region(sb["prefix"] + "out"), n, pitch)
                assert int(M.s8_malformed(hi, lo).sum()) == 0, f"acting {sb['name']}/out: not a nearest-even split"
                cur_ = tuple(t.reshape(n, sb["P"], sb["Cp"]) for t in (hi, lo))
                check("acting out", sum(cur_), y_, E_, label=f"acting ({n} rows) {sb['name']}/out")
                if l is not None and l["kind"] == 0:
                    xin_ = tuple(t.reshape(n, l["hin"], l["win"], l["cin_p"])[..., : l["cin"]] for t in cur_)
                else:
                    xin_ = tuple(t[:, :, : sb["C"]].reshape(n, -1) for t in cur_)
            else:
                xin_ = M.split(x_fc[rows])
            mod = l["name"] if l is not None else head
            want_, S_, c_ = contraction(i, l, xin_, mod, passes, p1)
            alt_, _, _ = contraction(i, l, xin_, mod, other, p1)
            if l is None:
                check("acting q (own operands)", q_got, want_, M.bound(S_, c_), S_, alt_, label=f"acting ({n} rows) q on own operands")
                return
            shape_ = (n, l["npix"], l["c"])
            gamma, beta = (k64(l["ln"], k) if l["ln"] else None for k in ("scale", "bias"))
            a_, Ea_ = M.ln_relu_fwd(want_.reshape(shape_), gamma, beta, M.bound(S_, c_).reshape(shape_), has_ln=l["ln"] is not None)
            altA, _ = M.ln_relu_fwd(alt_.reshape(shape_), gamma, beta, M.bound(S_, c_).reshape(shape_), has_ln=l["ln"] is not None)
            hi, lo = M.s8_planes(eng.region(f"act/{l['name']}"), n, l["npix"] * l["cp"])
            assert int(M.s8_malformed(hi, lo).sum()) == 0, f"acting act/{l['name']}: not a nearest-even split"
            got_ = (hi + lo).reshape(n, l["npix"], l["cp"])
            assert float(got_[..., l["c"]:].abs().max() if l["c"] < l["cp"] else 0.0) == 0.0, f"acting act/{l['name']}: padded channels are not 0"
            check("acting act", got_[:, :, : l["c"]], a_, Ea_, None, altA, elementwise=False, label=f"acting ({n} rows) act/{l['name']}")

    q_all = fwd(slice(0, N2)).double()
    torch.cuda.synchronize()
    acting_stages(q_all, slice(0, N2))
    q_one = fwd(slice(3, 4)).double()
    torch.cuda.synchronize()
    acting_stages(q_one, slice(3, 4))
    # the chain as a whole, on q only: every stage's bound carried through the next (worst case in every layer: loose, reported below)
    for i, l in enumerate(layers + [None]):
        mod = l["name"] if l is not None else head
        W, b = k64(mod, "kernel"), k64(mod, "bias")
        if l is not None and l["kind"] == 0:
            cut = lambda t: t.reshape(N2, l["hin"], l["win"], l["cin_p"])[..., : l["cin"]]
            op = lambda a_, w_, s_=l["s"]: M.conv(1, (a_, None), (w_, None), s_)[0]
            z, Ez, _ = BS.exact_layer(op, cut(y), cut(E), W, passes, M.chain_depth(l["K"]))
        else:
            if y is None:
                xi, Ei = x_fc.double(), torch.zeros_like(x_fc, dtype=torch.float64)
            else:
                sb = site_of[i - 1]
                xi, Ei = (t[:, :, : sb["C"]].reshape(N2, -1) for t in (y, E))
            in_p = l["in_p"] if l is not None else layers[-1]["cp"]
            c = M.chain_depth(in_p, slabs=_fwd_splits(N2, l["cp"] if l is not None else nha_p, in_p, arch == "fc" and i == 0))
            z, Ez, _ = BS.exact_layer(torch.matmul, xi, Ei, W, passes, c)
        z, Ez = z + b, Ez + M.ROUNDING * M.U * b.abs()
        if l is None:
            break
        gamma, beta = (k64(l["ln"], k) if l["ln"] else None for k in ("scale", "bias"))
        shape = (N2, l["npix"], l["c"])
        a, Ea = M.ln_relu_fwd(z.reshape(shape), gamma, beta, Ez.reshape(shape), has_ln=l["ln"] is not None)
        y, E = site_running(site_of[i], BS._pad_channels(a, l["cp"]), BS._pad_channels(Ea, l["cp"]))
    check("acting q", q_all, z, Ez, label="forward(2B rows) on the running averages")
    check("acting q", q_one, z[3:4], Ez[3:4], label="forward(row 3 alone)")
    report.append(f"acting q: bound / max |q| = {float(Ez.max() / z.abs().max()):.2e}")

    print()
    for line in report:
        print("  " + line)
    for row, (used, ratio, frac) in usage.items():
        print(f"  USAGE {case}-{precision} {row}: max |d| / bound = {used:.3f}, max |d| / 2^-24 S = {ratio:.2f}, other passes outside >= {frac:.0%}")
