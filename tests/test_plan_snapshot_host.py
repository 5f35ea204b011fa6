"""The host-side plan of the Q-network (csrc/net_plan.h) against tests/golden/plan_snapshot.txt, without a GPU.  The plan is a pure
function of isdqn_net_config, and everything else in the library trusts it blindly: a wrong offset or slab count fails no other CPU
test.  The snapshot was recorded (oracle/make_golden_plan.py) from the single 490-line builder before it was split into phases; it is
never regenerated from the code it is compared with -- where the two disagree, the code is wrong.

(a) tests/helpers/plan_dump.cpp, compiled against the tree as a host program, over the grid of tests/helpers/plan_grid.py: return
    code, refusal message and every plan field the configuration defines;
(b) the built library through ctypes: isdqn_net_param_layout, isdqn_net_workspace_bytes and isdqn_net_workspace_region of every
    region name, for the accepted configurations of the valid grid;
(c) the dumper built with -ftrivial-auto-var-init=zero and =pattern prints the same: no printed field is read before it is set.
    In the --all mode too, which prints every field of every array element: a plan starts value-initialised."""
import os

import pytest

from tests.helpers import plan_grid as pg

CSRC = os.path.join(pg.ROOT, "is-dqn_amd", "csrc")
UNREACHABLE = {"too many layers"}  # ISDQN_MAX_FEATURES = 8 gives at most 3 + 6 layers, MAX_LAYERS is 12


@pytest.fixture(scope="module")
def dumpers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan_dump")
    flags = {"plain": [], "zero": ["-ftrivial-auto-var-init=zero"], "pattern": ["-ftrivial-auto-var-init=pattern"]}
    procs = {k: pg.compile_dumper(CSRC, str(tmp / k), f) for k, f in flags.items()}
    assert all(p.wait() == 0 for p in procs.values())
    return {k: str(tmp / k) for k in flags}


@pytest.fixture(scope="module")
def lib():
    import importlib.util

    spec = importlib.util.spec_from_file_location("isdqn_build", os.path.join(pg.ROOT, "is-dqn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from slimdqn import _hip

    return _hip.lib()


@pytest.fixture(scope="module")
def golden():
    text = open(pg.GOLDEN).read()
    plan, rest = text.split("[plan]\n")[1].split("[messages]\n")
    messages, rest = rest.split("[refusals]\n")
    rows, full = rest.split("[full]\n")
    blocks = {}
    for block in full.split("== ")[1:]:
        name, body = block.split("\n", 1)
        blocks[name] = tuple(body.split("-- abi\n"))
    return dict(plan=[l.split("\t") for l in plan.splitlines()], refusals=pg.read_refusals(messages.splitlines(), rows.splitlines()), full=blocks)


@pytest.fixture(scope="module")
def valid(dumpers):
    cfgs = pg.valid_grid()
    return cfgs, pg.run_dumper(dumpers["plain"], cfgs)


HASH_ONLY = "the snapshot holds its SHA-256 only: dump this configuration from the recorded commit and from the tree to see the field"


def first_difference(got, want):
    """The first struct line and field (a `field=value` token or a region) in which two dumps differ."""
    g, w = got.splitlines(), want.splitlines()
    for a, b in zip(g, w):
        if a != b:
            ta, tb = a.split(" "), b.split(" ")
            for x, y in zip(ta, tb):
                if x != y:
                    return f"{tb[0]}: got '{x}', the snapshot holds '{y}'"
            return f"{tb[0]}: got {len(ta)} tokens, the snapshot holds {len(tb)}"
    return f"got {len(g)} lines, the snapshot holds {len(w)}"


def test_the_grid_holds_what_it_must():
    valid = pg.valid_grid()
    assert {c["arch"] for c in valid} == {pg.CNN, pg.FC, pg.IMPALA}
    assert {c["batch_size"] for c in valid} >= {1, 31, 32, 48, 256, 257, 4096}
    assert {(c["n_heads"], c["n_actions"]) for c in valid} >= {(h, a) for h in (1, 2, 10) for a in (1, 3, 18)}
    for arch in (pg.CNN, pg.IMPALA):
        mine = [c for c in valid if c["arch"] == arch]
        assert {(c["obs_h"], c["obs_w"], c["obs_c"]) for c in mine} == {(84, 84, 4), (8, 8, 1), (64, 64, 3), (100, 100, 4)}
        assert {c["features"] for c in mine} == set(pg.FEATS) and {(c["layer_norm"], c["batch_norm"]) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    fc = [c for c in valid if c["arch"] == pg.FC]
    assert {c["obs_c"] for c in fc} == {8, 9, 1} and {c["features"] for c in fc} == {(), (64,), (100, 200)}
    for opt in pg.OPTIONS.values():  # every option alone and the advertised combinations, on every arch
        assert {c["arch"] for c in valid if all(c[k] == v for k, v in opt.items())} == {pg.CNN, pg.FC, pg.IMPALA}
    assert len(valid) + len(pg.refusal_grid()) < 5000  # a few thousand lines: the test takes seconds


def test_plan_of_every_valid_configuration_is_the_snapshot(valid, golden):
    cfgs, dumped = valid
    assert [pg.describe(c) for c in cfgs] == [g[0] for g in golden["plan"]], "the grid is not the one the snapshot was recorded from"
    for (rc, body), (name, want_rc, want, *_) in zip(dumped, golden["plan"]):
        got = body.strip() if rc else pg.sha(body)
        assert (rc, got) == (int(want_rc), want), f"{name}: rc {rc} '{got}', the snapshot holds rc {want_rc} '{want}'" + ("" if rc else f" ({HASH_ONLY})")


def test_every_refusal_and_which_of_two_answers_first_is_the_snapshot(dumpers, golden):
    sweep = pg.refusal_sweep()
    for (tag, a, b, _), (rc, body) in zip(sweep, pg.run_dumper(dumpers["plain"], [c for _, _, _, c in sweep])):
        got = (rc, body.strip() if rc else pg.sha(body))
        assert got == golden["refusals"][(tag, a, b)], f"{tag} base, mutation {a}{' over ' + b if b else ''}: got {got}, the snapshot holds {golden['refusals'][(tag, a, b)]}"


def test_full_dumps_are_the_snapshot_field_by_field(dumpers, golden):
    full = pg.full_text_grid()
    assert [pg.describe(c) for c in full] == list(golden["full"])
    for c, (rc, body) in zip(full, pg.run_dumper(dumpers["plain"], full)):
        want = golden["full"][pg.describe(c)][0]
        assert rc == 0 and body == want, f"{pg.describe(c)}: {first_difference(body, want)}"


def test_every_reachable_refusal_of_the_builder_is_in_the_snapshot(golden):
    seen = {g[2] for g in golden["plan"] if int(g[1]) != 0} | {m for rc, m in golden["refusals"].values() if rc != 0}
    msgs = pg.builder_messages(CSRC)
    assert len(msgs) >= 50 and UNREACHABLE <= set(msgs)
    assert set(msgs) - seen == UNREACHABLE


def test_c_abi_layout_entry_points_are_the_snapshot(lib, valid, golden):
    cfgs, dumped = valid
    for c, (rc, body), g in zip(cfgs, dumped, golden["plan"]):
        if rc == 0:
            assert pg.sha(pg.abi_text(lib, c, pg.region_names(body))) == g[3], f"{g[0]} ({HASH_ONLY})"
    for c in pg.full_text_grid():
        want_plan, want = golden["full"][pg.describe(c)]
        got = pg.abi_text(lib, c, pg.region_names(want_plan))
        assert got == want, f"{pg.describe(c)}: {first_difference(got, want)}"


@pytest.mark.parametrize("all_fields", [False, True], ids=["defined", "all"])
def test_no_printed_field_is_read_before_it_is_set(dumpers, all_fields):
    cfgs = pg.valid_grid() + pg.refusal_grid() + pg.full_text_grid()
    zero, pattern = (pg.run_dumper(dumpers[k], cfgs, all_fields) for k in ("zero", "pattern"))
    for c, z, p in zip(cfgs, zero, pattern):
        assert z == p, f"{pg.describe(c)}: {first_difference(p[1], z[1])}"
    if not all_fields:
        assert zero == pg.run_dumper(dumpers["plain"], cfgs)
