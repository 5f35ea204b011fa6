"""Host side of ReDo (Sokar et al. 2023; include/isdqn_hip.h, isdqn_net_redo), no GPU: the CPU reference of tests/helpers/redo.py on
networks small enough to write the expected buffers by hand, the -redo / -redot flags and their refusals, and the seeds of the fresh
parameters.  The device side is tests/test_gpu_redo.py."""
import json
import os

import numpy as np
import pytest

from tests.helpers import redo as hr


def test_recycle_on_a_hand_written_two_layer_fc_net():
    """obs 2 -> Dense_0 (3 neurons) -> Dense_1 (2 outputs), neuron 1 dormant.  Internal layout: both kernels are [8][8] (rows =
    outputs, padded to 8), the vectors 8 floats.  Expected, written out: row 1 of Dense_0 and bias 1 come from the fresh buffer with
    all 8 lanes of the row; column 1 of Dense_1 is 0 in all 8 rows; the moments are 0 exactly there; nothing else moves."""
    lay = hr.HostLayout((2,), 2, 1, (3,), "fc", False)
    assert [i.name.decode() for i in lay.infos] == ["Dense_0/kernel", "Dense_0/bias", "Dense_1/kernel", "Dense_1/bias"]
    assert lay.n_param_floats == 64 + 8 + 64 + 8
    tree = {"Dense_0": {"kernel": np.array([[1, 2, 3], [4, 5, 6]], np.float32), "bias": np.array([0.5, -1000.0, 0.25], np.float32)},
            "Dense_1": {"kernel": np.array([[7, 8], [9, 10], [11, 12]], np.float32), "bias": np.array([1.5, 2.5], np.float32)}}
    new = {"Dense_0": {"kernel": -np.array([[10, 20, 30], [40, 50, 60]], np.float32), "bias": np.array([70, 80, 90], np.float32)},
           "Dense_1": {"kernel": np.full((3, 2), 99, np.float32), "bias": np.full(2, 99, np.float32)}}
    p, fresh = hr.to_flat(lay, tree), hr.to_flat(lay, new)
    w0 = p[:64].reshape(8, 8)
    assert np.array_equal(w0[:3, :2], tree["Dense_0"]["kernel"].T) and w0[3:].sum() == 0 and w0[:, 2:].sum() == 0
    m = np.arange(1, 145, dtype=np.float32)   # non-zero everywhere, padding lanes included
    v = m + 1000
    layers = hr.hidden_layers(lay)
    assert [(l.module, l.n_neurons, l.ln_module) for l in layers] == [("Dense_0", 3, None)]
    p2, m2, v2 = hr.recycle(lay, p, m, v, fresh, [np.array([False, True, False])])

    exp_p, written = p.copy(), np.zeros(144, bool)
    exp_p[8:16] = [-20, -50, 0, 0, 0, 0, 0, 0]  # Dense_0 row 1 <- fresh (8 lanes: the padded input lanes too)
    written[8:16] = True
    exp_p[64 + 1] = 80                           # its bias
    written[64 + 1] = True
    for row in range(8):                         # column 1 of Dense_1, the padded rows too
        exp_p[72 + row * 8 + 1] = 0
        written[72 + row * 8 + 1] = True
    assert np.array_equal(p2, exp_p)
    assert np.array_equal(m2, np.where(written, 0, m)) and np.array_equal(v2, np.where(written, 0, v))
    assert written.sum() == 8 + 1 + 8
    # the inputs are not modified, and an empty mask changes nothing
    assert p[9] == 5 and m[9] == 10
    for a, b in zip(hr.recycle(lay, p, m, v, fresh, [np.zeros(3, bool)]), (p, m, v)):
        assert np.array_equal(a, b)


def test_recycle_with_layer_norm_and_a_dormant_pair_ends_in_zero():
    """Two hidden layers with LayerNorm, neuron 0 of Dense_0 and neuron 1 of Dense_1 dormant: LayerNorm scale / bias of the neuron are
    reset with it, and the weight from the one dormant neuron into the other ends up 0 (outgoing zeros are written last)."""
    lay = hr.HostLayout((2,), 2, 1, (2, 2), "fc", True)
    rng = np.random.default_rng(0)
    shapes = {i.name.decode(): tuple(i.flax_shape[: i.ndim]) for i in lay.infos}
    def tree(lo):
        out = {}
        for name, shape in shapes.items():
            mod, leaf = name.rsplit("/", 1)
            out.setdefault(mod, {})[leaf] = rng.uniform(lo, lo + 1, shape).astype(np.float32)
        return out
    p, fresh = hr.to_flat(lay, tree(1.0)), hr.to_flat(lay, tree(5.0))
    m = np.ones_like(p)
    p2, m2, v2 = hr.recycle(lay, p, m, m, fresh, [np.array([True, False]), np.array([False, True])])
    at = {i.name.decode(): i for i in lay.infos}
    view = lambda buf, name: buf[at[name].offset : at[name].offset + at[name].size].reshape(int(at[name].dims[0]), -1)
    assert np.array_equal(view(p2, "Dense_0/kernel")[0], view(fresh, "Dense_0/kernel")[0])
    for name in ("Dense_0/bias", "LayerNorm_0/scale", "LayerNorm_0/bias"):
        assert view(p2, name)[0] == view(fresh, name)[0] and view(p2, name)[1] == view(p, name)[1] and view(m2, name)[0] == 0 and view(m2, name)[1] == 1
    d1 = view(p2, "Dense_1/kernel")
    assert d1[1, 0] == 0 and d1[1, 1] == view(fresh, "Dense_1/kernel")[1, 1] and d1[0, 0] == 0 and d1[0, 1] == view(p, "Dense_1/kernel")[0, 1]
    assert view(p2, "LayerNorm_1/scale")[1] == view(fresh, "LayerNorm_1/scale")[1]
    assert np.array_equal(view(p2, "Dense_2/kernel")[:, 1], np.zeros(8)) and np.array_equal(view(p2, "Dense_2/kernel")[:, 0], view(p, "Dense_2/kernel")[:, 0])
    assert np.array_equal(m2, v2)


def test_outgoing_columns_of_the_cnn_layouts():
    """Where the next layer reads neuron c, in the internal layout: [tap][c_pad] behind a convolution (12 channels pad to 16) and
    p * c_pad + c in the first Dense behind the torso."""
    lay = hr.HostLayout((84, 84, 4), 5, 4, (8, 12, 16, 24), "cnn", True)
    layers = hr.hidden_layers(lay)
    assert [(l.module, l.n_neurons, l.ln_module) for l in layers] == [("Conv_0", 8, "LayerNorm_0"), ("Conv_1", 12, "LayerNorm_1"),
                                                                      ("Conv_2", 16, "LayerNorm_2"), ("Dense_0", 24, "LayerNorm_3")]
    assert np.array_equal(np.flatnonzero(hr._outgoing_columns(lay, layers[0], 3)), np.arange(16) * 8 + 3)      # Conv_1: 4 x 4 taps of 8 lanes
    assert np.array_equal(np.flatnonzero(hr._outgoing_columns(lay, layers[1], 11)), np.arange(9) * 16 + 11)    # Conv_2: 3 x 3 taps of 16 lanes
    assert np.array_equal(np.flatnonzero(hr._outgoing_columns(lay, layers[2], 15)), np.arange(121) * 16 + 15)  # Dense_0: 11 x 11 positions
    assert np.array_equal(np.flatnonzero(hr._outgoing_columns(lay, layers[3], 23)), [23])                      # the last Dense
    # Conv_0 keeps its [out][plane][ky * 8 + kx] form: a neuron's incoming weights are still one row of the leading axis
    assert tuple(layers[0].kernel.dims[:3]) == (8, 4, 64)


def test_dormant_masks_and_margins():
    a = [np.array([0.0, 1.0, 3.0]), np.zeros(4)]
    masks = hr.dormant_masks(a, 0.0)
    assert masks[0].tolist() == [True, False, False] and masks[1].tolist() == [True] * 4  # a layer that is zero everywhere
    assert hr.dormant_masks(a, 0.75)[0].tolist() == [True, True, False]                   # mean 4 / 3: a <= 1
    assert np.allclose(hr.threshold_margins(a, 0.1)[0], [0.1, 0.65, 2.15]) and np.isinf(hr.threshold_margins(a, 0.1)[1]).all()


BASE = ["-en", "redo_Synthetic", "-s", "1", "-dw", "-f", "8", "8", "8", "16", "-at", "cnn", "-tuf", "16"]


def test_flags_parse_and_stay_out_of_parameters_json(tmp_path):
    from experiments.base.utils import prepare_logs

    p = prepare_logs("atari", "isdqn", BASE, root=str(tmp_path))
    assert p["redo_frequency"] == 0 and p["redo_tau"] == 0.1
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        p = prepare_logs("atari", algo, BASE + ["-redo", "32", "-redot", "0.025"], root=str(tmp_path))
        assert p["redo_frequency"] == 32 and p["redo_tau"] == 0.025
    for algo in ("isdqn", "dqn", "tfdqn"):
        p = prepare_logs("lunar_lander", algo, ["-en", "redo", "-s", "1", "-dw", "--redo_frequency", "400", "--redo_tau", "0"], root=str(tmp_path))
        assert p["redo_frequency"] == 400 and p["redo_tau"] == 0.0
    stored = json.load(open(tmp_path / "atari" / "exp_output" / "redo_Synthetic" / "parameters.json"))
    assert not any("redo" in k for section in stored.values() for k in section)


@pytest.mark.parametrize("extra,message", [
    (["-redo", "24"], "REDO_FREQUENCY_REFUSED"),        # not a multiple of -tuf 16
    (["-redo", "8"], "REDO_FREQUENCY_REFUSED"),
    (["-redo", "-16"], "REDO_FREQUENCY_REFUSED"),
    (["-redo", "16", "-redot", "-0.1"], "redo_tau"),
    (["-redo", "16", "-redot", "nan"], "redo_tau"),
    (["-redo", "16", "-bn"], "REDO_BATCH_NORM_REFUSED"),
    (["-redo", "16", "-at", "impala"], "REDO_IMPALA_REFUSED"),
])
def test_refusals_come_before_anything_is_written(tmp_path, extra, message):
    from experiments.base import parser_argument
    from experiments.base.utils import prepare_logs
    from slimdqn import _engine

    text = getattr(parser_argument, message, None) or getattr(_engine, message, None) or message
    with pytest.raises(ValueError) as e:
        prepare_logs("atari", "isdqn", BASE + extra, root=str(tmp_path))
    assert text in str(e.value)
    assert not os.path.exists(tmp_path / "atari")
    # the same options without -redo are accepted: the two flags mean nothing then
    rest = [a for i, a in enumerate(extra) if a != "-redo" and (i == 0 or extra[i - 1] != "-redo")]
    prepare_logs("atari", "isdqn", BASE + rest, root=str(tmp_path))


def test_check_redo_of_the_agents():
    from slimdqn._engine import REDO_BATCH_NORM_REFUSED, REDO_IMPALA_REFUSED, check_redo

    check_redo("cnn", False)
    check_redo("fc", False)
    with pytest.raises(ValueError, match="impala") as e:
        check_redo("impala", False)
    assert str(e.value) == REDO_IMPALA_REFUSED
    with pytest.raises(ValueError) as e:
        check_redo("cnn", True)
    assert str(e.value) == REDO_BATCH_NORM_REFUSED


def test_recycle_seeds_are_distinct_deterministic_and_never_the_init_seed():
    from slimdqn.networks._agent import recycle_seed

    seeds = [recycle_seed(s, k) for s in (0, 1, 7) for k in range(50)]
    assert len(set(seeds)) == len(seeds) and not set(seeds) & {0, 1, 7}
    assert seeds == [recycle_seed(s, k) for s in (0, 1, 7) for k in range(50)]
    # a child of the agent's seed in the SeedSequence tree: its stream is not the init stream of any small seed
    first = lambda s: np.random.default_rng(s).uniform(size=4).tolist()
    inits = [first(s) for s in range(64)]
    assert all(first(recycle_seed(s, k)) not in inits for s in (0, 1, 7) for k in range(4))


def test_fresh_parameters_follow_the_initialisation():
    """QNetEngine.fresh_params(seed) uploads the tree init_params(seed) uploads (one function builds it); different seeds give
    different kernels, the same seed the same bits; biases 0 and LayerNorm scales 1 whatever the seed."""
    from slimdqn._engine import QNetEngine
    from slimdqn.networks._agent import recycle_seed

    for arch, obs, feats in (("cnn", (84, 84, 4), (8, 12, 16, 24)), ("fc", (11,), (40, 24))):
        lay = hr.HostLayout(obs, 5, 4, feats, arch, True)
        a, b, c = (hr.to_flat(lay, QNetEngine._init_tree(lay, s)) for s in (3, 3, recycle_seed(3, 0)))
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        d = hr.to_flat(lay, QNetEngine._init_tree(lay, recycle_seed(3, 1)))
        for info in lay.infos:
            x, y, z = (f[info.offset : info.offset + info.size] for f in (a, c, d))
            if info.kind in (0, 1):
                assert not np.array_equal(x, y) and not np.array_equal(y, z)
            else:
                assert np.array_equal(x, y) and set(np.unique(x)) <= {0.0, 1.0}


def test_the_c_abi_refuses_without_touching_a_device():
    """Argument checks of isdqn_net_redo that come before any launch: each refusal of the header with its code."""
    import ctypes

    from slimdqn import _hip

    lay = hr.HostLayout((11,), 5, 4, (40, 24), "fc", True)
    lib, cfg = lay.lib, lay.cfg
    n, widths = ctypes.c_int32(), (ctypes.c_int32 * 8)()
    assert lib.isdqn_net_redo_layout(ctypes.byref(cfg), ctypes.byref(n), widths, 8) == 0 and [widths[i] for i in range(n.value)] == [40, 24]
    assert lib.isdqn_net_redo_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0) == 0 and n.value == 2
    cnn = hr.HostLayout((84, 84, 4), 5, 4, (8, 12, 16, 24), "cnn", False)
    assert lib.isdqn_net_redo_layout(ctypes.byref(cnn.cfg), ctypes.byref(n), widths, 8) == 0 and [widths[i] for i in range(n.value)] == [8, 12, 16, 24]
    one = 4096  # stands for a non-null pointer: every call below is refused before anything is read or launched

    def call(cfg=cfg, params=one, m=one, v=one, fresh=one, obs=one, n_rows=50, tau=0.1, scores=one, mask=one, count=one, ws=one):
        return lib.isdqn_net_redo(ctypes.byref(cfg), params, m, v, fresh, None, 0, None, obs, n_rows, tau, scores, mask, count, ws, None)

    for null in ("params", "fresh", "scores", "mask", "count", "ws"):
        assert call(**{null: None}) == _hip.ERR_ARG, null
    assert call(m=None) == _hip.ERR_ARG and call(v=None) == _hip.ERR_ARG
    assert "both" in _hip.last_error()
    for tau in (-0.1, float("nan"), float("inf")):
        assert call(tau=tau) == _hip.ERR_ARG
    for n_rows in (0, -1, 65):
        assert call(n_rows=n_rows) == _hip.ERR_SHAPE
    assert call(obs=None) == _hip.ERR_ARG
    imp = hr.HostLayout((84, 84, 4), 5, 4, (8, 16, 16, 24), "impala", True)
    assert call(cfg=imp.cfg) == _hip.ERR_UNSUPPORTED and "impala" in _hip.last_error()
    assert lib.isdqn_net_redo_layout(ctypes.byref(imp.cfg), ctypes.byref(n), widths, 8) == _hip.ERR_UNSUPPORTED
    cfg.batch_norm = 1
    try:
        assert call() == _hip.ERR_UNSUPPORTED and "BatchNorm" in _hip.last_error()
    finally:
        cfg.batch_norm = 0
