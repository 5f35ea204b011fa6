"""Host-side checks of the random-shift augmentation (include/isdqn_hip.h, isdqn_replay_augment_shift) on the numpy model of
tests/helpers/augment.py: the gather against an independent formulation (np.pad + crop), the identity at pad 0, the uniformity of the
specified draw, the counter arithmetic of one S*B-row launch against S launches, the wrong readings against the property test the GPU
file uses, and the flags / refusals of the Python layers.  No GPU."""
import argparse
import inspect
import os

import numpy as np
import pytest

from tests.helpers import augment as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0123456789AB


def test_every_shift_equals_replicate_pad_and_crop():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (7, 5), dtype=np.uint8)
    n = 0
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            assert np.array_equal(am.shift_frame(img, dy, dx), am.shift_by_pad_and_crop(img, dy, dx, 4)), (dy, dx)
            n += 1
    assert n == 81
    # a pad larger than the frame: the clamp handles it
    small = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    for dy, dx in ((-6, 6), (6, -6), (5, 0), (0, -5)):
        assert np.array_equal(am.shift_frame(small, dy, dx), am.shift_by_pad_and_crop(small, dy, dx, 6))


def _case(h, w, stack, n_rows, stride=None, n_frames=None, seed=1):
    rng = np.random.default_rng(seed)
    stride = h * w if stride is None else stride
    n_frames = n_frames or 3 * n_rows * stack
    frames = rng.integers(0, 256, (n_frames, stride), dtype=np.uint8)
    ids = rng.integers(0, n_frames, (n_rows, 2 * stack)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.2] = -1
    return frames, ids


def test_pad_zero_is_the_identity_copy_and_minus_one_stays():
    h, w, stack = 7, 5, 3
    frames, ids = _case(h, w, stack, 6, stride=h * w + 3)
    before = np.full((6 * 2 * stack, h * w + 3), 0xA5, np.uint8)
    pool, out_ids, count = am.augment(frames, h, w, stack, ids, 6, 0, SEED, 11, pool=before)
    assert count == 12
    for r in range(6):
        for k in range(2 * stack):
            f = r * 2 * stack + k
            if ids[r, k] < 0:
                assert out_ids[r, k] == -1 and (pool[f] == 0xA5).all()  # not written
            else:
                assert out_ids[r, k] == f and np.array_equal(pool[f, : h * w], frames[ids[r, k], : h * w])
                assert (pool[f, h * w :] == 0xA5).all()  # the bytes between h*w and the stride keep what they held


def test_the_draw_is_uniform_and_the_halves_draw_independently():
    """8,192 rows x 2 halves at pad 4 under the committed seed: each of the 9 values of dx and of dy within 6 binomial standard
    deviations of 16,384 / 9 (sqrt(16384 * (1/9) * (8/9)) = 40.2: +-241 around 1,820); state and next-state shifts of a row differ in at
    least 95 % of the rows (expected 80 / 81).  A condition on the specified mapping: if this seed fails, the mapping is wrong."""
    dy, dx = am.draws(8192, 8192, 4, SEED, 0)
    assert dy.min() == -4 and dy.max() == 4 and dx.min() == -4 and dx.max() == 4
    for d in (dy, dx):
        counts = np.bincount((d + 4).reshape(-1), minlength=9)
        assert counts.sum() == 16384 and len(counts) == 9
        assert np.abs(counts - 16384 / 9).max() <= 241, counts
    differ = ((dy[:, 0] != dy[:, 1]) | (dx[:, 0] != dx[:, 1])).mean()
    assert differ >= 0.95, differ
    # dx and dy of one draw are different words of the block
    assert (dy != dx).mean() > 0.8
    # pad 0: no shift at all; the range follows the pad
    z = am.draws(64, 64, 0, SEED, 3)
    assert not z[0].any() and not z[1].any()
    for pad in (1, 6, 127):
        y, x = am.draws(4096, 4096, pad, SEED, 0)
        assert y.min() >= -pad and y.max() <= pad and x.min() >= -pad and x.max() <= pad


def test_the_counter_words_are_what_the_header_says():
    from tests.helpers.noisy import philox4x32_10

    pad, count, B = 4, (1 << 32) + 5, 3  # a count whose high word is not zero
    dy, dx = am.draws(2 * B, B, pad, SEED, count)
    for r in range(2 * B):
        t, b = count + r // B, r % B
        for half in (0, 1):
            x = philox4x32_10([b, 0x80000000 | half, t & 0xFFFFFFFF, t >> 32], [SEED & 0xFFFFFFFF, SEED >> 32])
            assert dx[r, half] == ((int(x[0][0]) * 9) >> 32) - 4 and dy[r, half] == ((int(x[1][0]) * 9) >> 32) - 4
    # bit 31 of counter word 1 is what separates these draws from the noisy layers' ((stream_id << 16) | vector id < 2^31)
    a = philox4x32_10([0, 0x80000000, 5, 0], [1, 2])
    b = philox4x32_10([0, 0, 5, 0], [1, 2])
    assert int(a[0][0]) != int(b[0][0])


def test_one_launch_over_s_times_b_rows_is_s_launches_over_b_rows():
    h, w, stack, S, B = 6, 5, 2, 4, 3
    frames, ids = _case(h, w, stack, S * B)
    pool, out_ids, count = am.augment(frames, h, w, stack, ids, B, 4, SEED, 7)
    assert count == 7 + S
    c = 7
    for s in range(S):
        p, o, c2 = am.augment(frames, h, w, stack, ids[s * B : (s + 1) * B], B, 4, SEED, c)
        assert c2 == c + 1
        c = c2
        s2 = 2 * stack
        assert np.array_equal(p, pool[s * B * s2 : (s + 1) * B * s2])
        want = out_ids[s * B : (s + 1) * B]
        assert np.array_equal(np.where(o >= 0, o + s * B * s2, -1), want)  # the same frames, counted from the big pool's base
    assert c == count
    # the same count gives the same draws, the next count others
    again = am.augment(frames, h, w, stack, ids, B, 4, SEED, 7)[0]
    other = am.augment(frames, h, w, stack, ids, B, 4, SEED, 8)[0]
    assert np.array_equal(again, pool) and not np.array_equal(other, pool)
    # rows_per_step must divide the rows
    with pytest.raises(AssertionError):
        am.augment(frames, h, w, stack, ids, 5, 4, SEED, 0)


def test_the_property_test_passes_the_model_and_catches_every_wrong_reading():
    frames, ids, h, w, stack, pad = am.ramp_case()
    dy, dx = am.draws(ids.shape[0], ids.shape[0], pad, SEED, 2)
    pool, out_ids, _ = am.augment(frames, h, w, stack, ids, ids.shape[0], pad, SEED, 2)
    assert am.check_ramp_properties(pool, out_ids, ids, h, w, stack, pad, dy, dx) == []
    assert am.check_ramp_properties(pool, out_ids, ids, h, w, stack, pad) == []  # from the output alone
    for variant in am.VARIANTS[1:]:
        bad, bad_ids, _ = am.augment(frames, h, w, stack, ids, ids.shape[0], pad, SEED, 2, variant=variant)
        fails = am.check_ramp_properties(bad, bad_ids, ids, h, w, stack, pad, dy, dx)
        assert fails, f"the property test let the wrong reading '{variant}' through"
    # the two readings that need no expectation are caught from the output alone
    for variant in ("per_frame", "same_halves", "zero_pad"):
        bad, bad_ids, _ = am.augment(frames, h, w, stack, ids, ids.shape[0], pad, SEED, 2, variant=variant)
        assert am.check_ramp_properties(bad, bad_ids, ids, h, w, stack, pad), variant


def test_read_shift_reads_every_shift_back():
    h, w, pad = 11, 13, 4
    src = am.ramp_frames(9, h, w)[8].reshape(h, w)
    for dy in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            assert am.read_shift(am.shift_frame(src, dy, dx), 8, h, w, pad) == (dy, dx)


# ---------------------------------------------------------------------------------------------- flags, refusals, keywords
def _parse(argv, algo="isdqn"):
    from experiments.base import parser_argument as pa

    parser = argparse.ArgumentParser()
    pa.add_base_arguments(parser)
    getattr(pa, f"add_{algo}_arguments")(parser)
    pa.add_engine_arguments(parser)
    return vars(parser.parse_args(["-en", "x_Game", "-s", "1"] + argv))


def test_the_flags_their_defaults_and_augment_kwargs():
    from experiments.base import parser_argument as pa

    p = _parse([])
    assert p["augment"] is False and p["augment_pad"] == 4
    assert pa.augment_kwargs(p) == {}
    assert pa.augment_kwargs(_parse(["-augp", "6"])) == {}  # -augp means nothing without -aug
    for algo in ("isdqn", "dqn", "tfdqn", "analysisdqn", "analysistfdqn"):
        assert pa.augment_kwargs(_parse(["-aug"], algo=algo)) == dict(augment_pad=4)
    assert pa.augment_kwargs(_parse(["--augment", "--augment_pad", "2"])) == dict(augment_pad=2)
    # the README's DER-style line parses
    der = _parse(["-aug", "-augp", "4", "-noisy", "-duel", "-dq", "-per", "-n", "10", "-utd", "2", "-f", "32", "64", "64", "512"])
    assert der["augment"] and der["noisy_nets"] and der["dueling"] and der["double_q"] and der["prioritized"]


def test_check_augment_refuses_fc_and_pads_out_of_range():
    from slimdqn import _engine

    check = _engine.check_augment
    for arch in ("cnn", "impala", "fc"):
        check(0, arch)  # off goes with everything
    for pad in (1, 4, 127):
        check(pad, "cnn")
        check(pad, "impala")
        with pytest.raises(ValueError) as e:
            check(pad, "fc")
        assert str(e.value) == _engine.AUGMENT_FC_REFUSED
    for pad in (-1, 128, 2.5, True):
        with pytest.raises(ValueError) as e:
            check(pad, "cnn")
        assert str(e.value) == _engine.AUGMENT_PAD_REFUSED


@pytest.mark.parametrize("env,algo,extra,words", [("lunar_lander", "dqn", ["-aug"], "image frames"), ("lunar_lander", "isdqn", ["-aug", "-augp", "2"], "image frames"),
                                                  ("lunar_lander", "tfdqn", ["-aug"], "image frames"), ("atari", "isdqn", ["-aug", "-augp", "200"], "augment_pad"),
                                                  ("atari", "dqn", ["-aug", "-at", "fc", "-f", "16", "16"], "image frames")])
def test_aug_on_what_it_is_not_built_for_is_refused_before_anything_is_written(tmp_path, env, algo, extra, words):
    from experiments.base.utils import prepare_logs

    with pytest.raises(ValueError) as e:
        prepare_logs(env, algo, ["-en", "g_Game", "-dw", "-s", "1"] + extra, root=str(tmp_path))
    assert words in str(e.value)
    assert not (tmp_path / env).exists()  # before the output directory is created


def test_aug_goes_with_every_image_torso_and_stays_out_of_parameters_json(tmp_path):
    import json

    from experiments.base.utils import prepare_logs

    for i, extra in enumerate((["-at", "cnn"], ["-at", "impala", "-f", "8", "8", "8", "16"], ["-at", "cnn", "-bn"], ["-at", "cnn", "-f", "8", "8", "8", "16", "-noisy", "-duel", "-dq"])):
        p = prepare_logs("atari", "isdqn", ["-en", f"t{i}_Game", "-dw", "-s", "1", "-aug"] + extra, root=str(tmp_path))
        assert p["augment"] and p["augment_pad"] == 4
    on = json.load(open(tmp_path / "atari" / "exp_output" / "t0_Game" / "parameters.json"))
    prepare_logs("atari", "isdqn", ["-en", "plain_Game", "-dw", "-s", "1", "-at", "cnn"], root=str(tmp_path))
    plain = json.load(open(tmp_path / "atari" / "exp_output" / "plain_Game" / "parameters.json"))
    assert not any("augment" in k for k in list(on["isdqn"]) + list(on["shared_parameters"]))
    assert set(on["isdqn"]) == set(plain["isdqn"]) and set(on["shared_parameters"]) == set(plain["shared_parameters"])


def test_entry_points_pass_the_keyword_to_their_agents():
    base = os.path.join(ROOT, "is-dqn_amd", "experiments")
    for rel in ("atari/isdqn.py", "atari/dqn.py", "atari/analysisdqn.py", "atari/tfdqn.py", "atari/analysistfdqn.py"):
        assert "**augment_kwargs(p)" in open(os.path.join(base, rel)).read(), rel


def test_agents_take_the_keyword_and_refuse_before_an_engine_is_built():
    from slimdqn import _engine
    from slimdqn._graph import GraphedUpdate
    from slimdqn.networks._agent import augment_seed, recycle_seed
    from slimdqn.networks.analysisdqn import AnalysisDQN
    from slimdqn.networks.analysistfdqn import AnalysisTFDQN
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.isdqn import iSDQN
    from slimdqn.networks.tfdqn import TFDQN

    for f in (DQN.__init__, iSDQN.__init__, TFDQN.__init__):
        assert inspect.signature(f).parameters["augment_pad"].default == 0
    assert inspect.signature(GraphedUpdate.__init__).parameters["augment"].default is None
    feats = [16, 16]
    makes = (lambda **kw: iSDQN(0, (8,), 4, 2, feats, True, False, "fc", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw),
             lambda **kw: AnalysisDQN(0, (8,), 4, 2, feats, True, False, "fc", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw),
             lambda **kw: DQN(0, (8,), 4, feats, True, "fc", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw),
             lambda **kw: TFDQN(0, (8,), 4, feats, True, False, "fc", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw),
             lambda **kw: AnalysisTFDQN(0, (8,), 4, feats, True, False, "fc", 1e-3, 0.99, 1, 1, 4, batch_size=4, **kw))
    for make in makes:  # raised before an engine is built (no GPU here: building one would raise something else)
        with pytest.raises(ValueError) as e:
            make(augment_pad=4)
        assert str(e.value) == _engine.AUGMENT_FC_REFUSED
        with pytest.raises(ValueError) as e:
            make(augment_pad=-1)
        assert str(e.value) == _engine.AUGMENT_PAD_REFUSED
    # the seed of the draws: a child of the agent's seed, 64 bits, neither the seed nor a recycle seed
    s = augment_seed(3)
    assert 0 <= s < 1 << 64 and s != 3 and s == augment_seed(3) and s != augment_seed(4)
    assert s != recycle_seed(3, 0) & ((1 << 64) - 1)


def test_replay_buffer_augment_refuses_vector_observations():
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    rb = ReplayBuffer(UniformSamplingDistribution(0), 4, 16, stack_size=1, device="cpu")
    rb._allocate((8,), floating=True)
    with pytest.raises(ValueError):
        rb.augment(None, 4, 1, None)
