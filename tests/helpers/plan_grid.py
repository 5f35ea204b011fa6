"""The configurations of the plan snapshot (tests/golden/plan_snapshot.txt) and everything its two users share:
oracle/make_golden_plan.py records the snapshot, tests/test_plan_snapshot_host.py holds the tree to it.

A configuration is a dict of the fields of isdqn_net_config (floats as C hex float strings, so nothing is ever rounded; `features` a
tuple), or None for the null pointer.  `line` writes it as tests/helpers/plan_dump.cpp reads it, `describe` as the snapshot names it."""
import ctypes
import hashlib
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DUMPER = os.path.join(ROOT, "tests", "helpers", "plan_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_snapshot.txt")

INT_A = ["arch", "obs_h", "obs_w", "obs_c", "n_features"]
INT_B = ["n_actions", "n_heads", "dueling", "layer_norm", "batch_size", "precision"]
FLOAT_A = ["gamma_n", "learning_rate", "adam_b1", "adam_b2", "adam_eps", "max_grad_norm", "huber_delta", "munchausen_tau", "munchausen_alpha",
           "munchausen_clip"]
INT_C = ["batch_norm", "categorical", "n_bins", "n_quantiles"]
FLOAT_B = ["hl_min", "hl_max", "hl_sigma"]
CNN, FC, IMPALA = 0, 1, 2

# every float a dyadic number with a short hex form; the plan reads max_grad_norm, huber_delta, the Munchausen and the hl_* fields only
BASE = dict(arch=CNN, obs_h=84, obs_w=84, obs_c=4, features=(32, 64, 64, 512), n_actions=9, n_heads=4, dueling=0, layer_norm=1, batch_size=32,
            precision=0, gamma_n="0x1.fap-1", learning_rate="0x1p-14", adam_b1="0x1.cp-1", adam_b2="0x1.ffp-1", adam_eps="0x1p-26",
            max_grad_norm="0", huber_delta="0", munchausen_tau="0", munchausen_alpha="0x1.cp-1", munchausen_clip="-0x1p+0", batch_norm=0,
            categorical=0, n_bins=0, n_quantiles=0, hl_min="-0x1.4p+3", hl_max="0x1.4p+3", hl_sigma="0x1.8p-1", double_q=0)
BASE_FC = dict(BASE, arch=FC, obs_h=1, obs_w=1, obs_c=8, features=(100, 200))
BASE_IMPALA = dict(BASE, arch=IMPALA)
TAU = "0x1p-5"


def line(cfg):
    """The text line of a configuration dict (`features` a tuple; `n_features` defaults to its length)."""
    if cfg is None:
        return "null"
    feats = tuple(cfg["features"]) + (0,) * (8 - len(cfg["features"]))
    c = dict(cfg, n_features=cfg.get("n_features", len(cfg["features"])))
    return " ".join(str(v) for v in [c[k] for k in INT_A] + list(feats) + [c[k] for k in INT_B + FLOAT_A + INT_C + FLOAT_B] + [c["double_q"]])


def describe(cfg):
    """A configuration as the snapshot names it: its arch's base and every field that differs from it."""
    if cfg is None:
        return "null"
    arch = {CNN: "cnn", FC: "fc", IMPALA: "impala"}.get(cfg["arch"], f"arch={cfg['arch']}")
    base = {"fc": BASE_FC, "impala": BASE_IMPALA}.get(arch, BASE)
    c = dict(cfg, n_features=cfg.get("n_features", len(cfg["features"])))
    b = dict(base, n_features=len(base["features"]), arch=c["arch"])
    return " ".join([arch] + [f"{k}={','.join(map(str, c[k])) if k == 'features' else c[k]}" for k in sorted(b) if c[k] != b[k]])


def net_config(text):
    """The ctypes isdqn_net_config of a line."""
    from slimdqn import _hip

    tok = text.split()
    c = _hip.NetConfig()
    names = INT_A + [None] * 8 + INT_B + FLOAT_A + INT_C + FLOAT_B + ["double_q"]
    assert len(tok) == len(names) == len(_hip.NetConfig._fields_) + 7
    for i, (name, t) in enumerate(zip(names, tok)):
        if name is None:
            c.features[i - len(INT_A)] = int(t)
        elif name in FLOAT_A or name in FLOAT_B:
            setattr(c, name, float.fromhex(t))
        else:
            setattr(c, name, int(t))
    return c


# ------------------------------------------------------------------ the valid part
OPTIONS = {
    "plain": {},
    "hl2": dict(n_bins=2), "hl51": dict(n_bins=51), "hl256": dict(n_bins=256),
    "c51": dict(n_bins=51, categorical=1), "c51_sigma0": dict(n_bins=51, categorical=1, hl_sigma="0"),
    "qr2": dict(n_quantiles=2), "qr51": dict(n_quantiles=51), "qr256": dict(n_quantiles=256),
    "duel": dict(dueling=1), "dq": dict(double_q=1), "munchausen": dict(munchausen_tau=TAU),
    "gc10": dict(max_grad_norm="0x1.4p+3"), "gcinf": dict(max_grad_norm="inf"), "huber": dict(huber_delta="0x1p+0"),
    "qr_huber": dict(n_quantiles=51, huber_delta="0x1p+0"), "hl_dq": dict(n_bins=51, double_q=1), "hl_munchausen": dict(n_bins=51, munchausen_tau=TAU),
    "duel_dq_hl_cat": dict(dueling=1, double_q=1, n_bins=51, categorical=1),
    "duel_qr_gc": dict(dueling=1, n_quantiles=51, max_grad_norm="0x1.4p+3"),
}
BATCHES = [1, 31, 32, 48, 256, 257, 4096]
OBS = [(84, 84, 4), (8, 8, 1), (64, 64, 3), (100, 100, 4)]
FEATS = [(32, 64, 64, 512), (32, 64, 64), (32, 64, 64, 1024), (16, 32, 32, 256), (5, 7, 9, 100), (64, 64, 64, 512, 512)]
FC_OBS = [8, 9, 1]
FC_FEATS = [(), (64,), (100, 200)]
HEADS = [(h, a) for h in (1, 2, 10) for a in (1, 3, 18)]


def valid_grid():
    """Geometry: arch x observation x widths x batch size crossed in full -- what the tiling decisions are functions of -- with
    layer_norm, batch_norm and the head shape riding along in rotation.  Options: every option x arch x three head shapes in rotation,
    at two batch sizes in rotation.  Not every line is accepted -- an option the impala torso refuses, 256 bins on 180 outputs -- and
    the snapshot records those refusals like everything else."""
    out, n = [], 0
    for arch in (CNN, IMPALA):
        for (h, w, c), feats, B in itertools.product(OBS, FEATS, BATCHES):
            heads, actions = HEADS[n % len(HEADS)]
            out.append(dict(BASE, arch=arch, obs_h=h, obs_w=w, obs_c=c, features=feats, batch_size=B, layer_norm=n % 2, batch_norm=(n // 2) % 2,
                            n_heads=heads, n_actions=actions))
            n += 1
    for c, feats, B in itertools.product(FC_OBS, FC_FEATS, BATCHES):
        heads, actions = HEADS[n % len(HEADS)]
        out.append(dict(BASE_FC, obs_c=c, features=feats, batch_size=B, layer_norm=n % 2, batch_norm=(n // 2) % 2, n_heads=heads, n_actions=actions))
        n += 1
    for base in (BASE, BASE_IMPALA, BASE_FC):
        for opt, k in itertools.product(OPTIONS.values(), range(3)):
            heads, actions = HEADS[n % len(HEADS)]
            out.append(dict(base, n_heads=heads, n_actions=actions, batch_size=(32, 257)[(n // 3) % 2], **opt))
            n += 1
    return out


def full_text_grid():
    """The configurations whose whole dump the snapshot keeps as text: every arch plain, cnn and fc with BatchNorm, and on the cnn
    base the histogram heads, Munchausen targets and the two advertised combinations (between them every option region)."""
    out = [BASE, BASE_IMPALA, BASE_FC, dict(BASE, batch_norm=1), dict(BASE_FC, batch_norm=1)]
    return out + [dict(BASE, **OPTIONS[name]) for name in ("hl51", "munchausen", "duel_dq_hl_cat", "duel_qr_gc")]


# ------------------------------------------------------------------ the refusals: one mutation per ISDQN_REQUIRE of the builder
HL = dict(n_bins=51)
MUTATIONS = {  # in the order of the checks in csrc/net_plan.h; None: the null pointer
    "null": None,
    "arch": dict(arch=3),
    "n_features_9": dict(n_features=9),
    "n_features_2": dict(n_features=2),  # (fc: accepted)
    "n_actions_0": dict(n_actions=0),
    "n_heads_0": dict(n_heads=0),
    "batch_0": dict(batch_size=0),
    "batch_4097": dict(batch_size=4097),
    "precision": dict(precision=2),
    "huber_neg": dict(huber_delta="-0x1p+0"),
    "gc_neg": dict(max_grad_norm="-0x1p+0"),
    "gc_nan": dict(max_grad_norm="nan"),
    "bn_2": dict(batch_norm=2),
    "dq_2": dict(double_q=2),
    "tau_neg": dict(munchausen_tau="-0x1p-5"),
    "tau_inf": dict(munchausen_tau="inf"),
    "alpha": dict(munchausen_tau=TAU, munchausen_alpha="0x1.8p+0"),
    "clip": dict(munchausen_tau=TAU, munchausen_clip="0x1p-1"),
    "tau_dq": dict(munchausen_tau=TAU, double_q=1),
    "nq_1": dict(n_quantiles=1),
    "nq_257": dict(n_quantiles=257),
    "nq_bins": dict(n_quantiles=51, n_bins=51),
    "nq_tau": dict(n_quantiles=51, munchausen_tau=TAU),
    "nq_bn": dict(n_quantiles=51, batch_norm=1),
    "bins_1": dict(n_bins=1),
    "bins_257": dict(n_bins=257),
    "cat_2": dict(categorical=2),
    "cat_nq": dict(categorical=1, n_quantiles=51),
    "cat_nobins": dict(categorical=1),
    "cat_tau": dict(categorical=1, n_bins=51, munchausen_tau=TAU),
    "hl_range": dict(HL, hl_max="-0x1.4p+3"),
    "hl_sigma": dict(HL, hl_sigma="0"),
    "hl_huber": dict(HL, huber_delta="0x1p+0"),
    "hl_bn": dict(HL, batch_norm=1),
    "hl_k65": dict(n_bins=2, n_heads=66, n_actions=2),
    "qr_k65": dict(n_quantiles=2, n_heads=66, n_actions=2),
    "hl_5457": dict(n_bins=107, n_heads=1, n_actions=51),
    "qr_5457": dict(n_quantiles=107, n_heads=1, n_actions=51),
    "duel_2": dict(dueling=2),
    "duel_bn": dict(dueling=1, batch_norm=1),
    "duel_impala": dict(dueling=1, arch=IMPALA, obs_h=84, obs_w=84, obs_c=4, features=(32, 64, 64, 512)),
    "duel_k65": dict(dueling=1, n_heads=66, n_actions=2),
    "duel_raw": dict(dueling=1, n_bins=51, n_heads=10, n_actions=10),  # 5100 logits fit, 5610 raw outputs do not
    "duel_no_hidden": dict(dueling=1, n_features=3),  # (fc: 3 > 0 hidden layers, another check answers)
    "duel_no_hidden_fc": dict(dueling=1, n_features=0),  # (cnn: bad n_features answers first)
    "duel_odd": dict(dueling=1, features=(32, 64, 64, 511), n_features=4),
    "gc_bn": dict(max_grad_norm="inf", batch_norm=1),
    "gc_impala": dict(max_grad_norm="0x1.4p+3", arch=IMPALA, obs_h=84, obs_w=84, obs_c=4, features=(32, 64, 64, 512)),
    "obs_h_7": dict(obs_h=7),
    "obs_c_17": dict(obs_c=17),
    "obs_c_0": dict(obs_c=0),
    "bn_obs_c_9": dict(batch_norm=1, obs_c=9),
    "obs_w_86": dict(obs_w=86),
    "conv_65": dict(features=(65, 64, 64, 512), n_features=4),
    "conv_0": dict(features=(32, 64, 0, 512), n_features=4),
    "impala_obs_c_9": dict(arch=IMPALA, obs_h=84, obs_w=84, obs_c=9, features=(32, 64, 64, 512)),
    "impala_65": dict(arch=IMPALA, obs_h=84, obs_w=84, obs_c=4, features=(32, 65, 64, 512)),
    "impala_obs_w_85": dict(arch=IMPALA, obs_h=84, obs_w=85, obs_c=4, features=(32, 64, 64, 512)),
    "dense_0": dict(features=(32, 64, 64, 0), n_features=4),
    "dense_8193": dict(features=(32, 64, 64, 8193), n_features=4),
    "head_8200": dict(n_heads=100, n_actions=82),
}
# the fc base pairs only the mutations that leave it an fc network or move it whole to another arch
FC_SKIP = {"n_features_2", "duel_no_hidden", "obs_h_7", "obs_c_17", "bn_obs_c_9", "obs_w_86", "conv_65", "conv_0"}


def _mutate(base, *names):
    cfg = dict(base)
    for n in names:
        if MUTATIONS[n] is None:
            return None
        cfg.update(MUTATIONS[n])
    if "n_features" not in cfg:
        cfg["n_features"] = len(cfg["features"])
    return cfg


def refusal_sweep():
    """[(base name, mutation a, mutation b or None, configuration)]: on both bases every single mutation and every pair of mutations
    (the second applied over the first): the pairs pin which check answers first when two are violated."""
    out = [("cnn", "null", None, None)]
    for tag, base, skip in (("cnn", BASE, set()), ("fc", BASE_FC, FC_SKIP)):
        names = [n for n in MUTATIONS if n not in skip and MUTATIONS[n] is not None]
        for i, a in enumerate(names):
            out.append((tag, a, None, _mutate(base, a)))
            out += [(tag, a, b, _mutate(base, a, b)) for b in names[i + 1:]]
    return out


def refusal_grid():
    return [c for _, _, _, c in refusal_sweep()]


def write_refusals(results):
    """The two refusal sections of the snapshot from [(rc, message or SHA-256 of the dump)] in the order of refusal_sweep(): a table
    of the distinct (rc, message) in order of first appearance, then one row per (base, a): the table index of `a` alone and of
    (a, b) for every later mutation b, in the order of MUTATIONS; an accepted configuration is written =<SHA-256>."""
    ids, rows = {}, {}
    for (tag, a, b, _), (rc, text) in zip(refusal_sweep(), results):
        token = "=" + text if rc == 0 else str(ids.setdefault((rc, text), len(ids) + 1))
        rows.setdefault((tag, a), []).append(token)
    return (["[messages]"] + [f"{i}\t{rc}\t{m}" for (rc, m), i in ids.items()] +
            ["[refusals]"] + [f"{tag} {a}\t{' '.join(t)}" for (tag, a), t in rows.items()])


def read_refusals(messages, rows):
    """{(base, a, b): (rc, message or SHA-256)} of the two sections write_refusals wrote."""
    table = {i: (int(rc), m) for i, rc, m in (l.split("\t") for l in messages)}
    tokens = {tuple(k.split()): t.split() for k, t in (l.split("\t") for l in rows)}
    out = {}
    for tag, a, b, _ in refusal_sweep():
        t = tokens[(tag, a)].pop(0)
        out[(tag, a, b)] = (0, t[1:]) if t.startswith("=") else table[t]
    assert not any(tokens.values())
    return out


def builder_messages(csrc):
    """Every refusal message of the builder in `csrc`/net_plan.h: the string literal(s) that close each ISDQN_REQUIRE."""
    import re

    text = open(os.path.join(csrc, "net_plan.h")).read()
    msgs = []
    for m in re.finditer(r"ISDQN_REQUIRE\(", text):
        stmt = text[m.end():text.index(");", m.end())]
        msgs.append("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', stmt)))
    return msgs


# ------------------------------------------------------------------ the dumper
def compile_dumper(csrc, exe, flags=()):
    """Popen of the host compile of plan_dump.cpp against the headers in `csrc` (no device code: -x c++)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the compiler is-dqn_amd/build.py uses
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")  # -x c++ drops hipcc's own -I
    return subprocess.Popen([hipcc, "-x", "c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include, "-I", csrc, *flags,
                             DUMPER, "-o", exe])


def run_dumper(exe, cfgs, all_fields=False):
    """[(rc, body text)] of the configuration dicts `cfgs` through the dumper."""
    lines = [line(c) for c in cfgs]
    text = subprocess.run([exe] + (["--all"] if all_fields else []), input="\n".join(lines) + "\n", capture_output=True, encoding="utf-8", errors="replace",
                          check=True).stdout
    out = []
    for block in text.split("== ")[1:]:
        cfg, rc, body = block.split("\n", 2)
        assert cfg == lines[len(out)]
        out.append((int(rc.split()[1]), body))
    assert len(out) == len(lines)
    return out


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def region_names(body):
    return [t.split("=")[0] for l in body.splitlines() if l.startswith("regions") for t in l.split()[1:]]


# ------------------------------------------------------------------ the C ABI of the built library
def abi_text(lib, config, regions):
    """isdqn_net_param_layout (every field of every isdqn_tensor_info), isdqn_net_workspace_bytes and isdqn_net_workspace_region of
    every name in `regions`, as text."""
    from slimdqn import _hip

    cfg = net_config(line(config))
    n, cnt = ctypes.c_int64(), ctypes.c_int32()
    rc = lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt))
    out = [f"layout rc {rc} n_params {n.value} tensors {cnt.value}"]
    infos = (_hip.TensorInfo * cnt.value)()
    rc = lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt))
    out.append(f"layout rc {rc} n_params {n.value} tensors {cnt.value}")
    for t in infos:
        out.append(f"tensor {t.name.decode()} {t.offset} {t.size} {t.kind} {t.layer} {t.ndim} {list(t.flax_shape)} {list(t.dims)}")
    b = ctypes.c_int64()
    rc = lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(b))
    out.append(f"workspace rc {rc} bytes {b.value}")
    found = []
    for name in regions:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        rc = lib.isdqn_net_workspace_region(ctypes.byref(cfg), name.encode(), ctypes.byref(off), ctypes.byref(size))
        found.append(f"{name}={rc}:{off.value}+{size.value}")
    return "\n".join(out + ["regions " + " ".join(found)]) + "\n"


# ------------------------------------------------------------------ the snapshot file
def snapshot(dump, lib):
    """The text of the snapshot: `dump(cfgs)` runs the dumper, `lib` is the loaded library.
    [plan]: valid_grid(), one line each: configuration (describe), rc, then the refusal's message, or the SHA-256 of the dump and the
    SHA-256 of abi_text.  [messages], [refusals]: refusal_sweep() (write_refusals).  [full]: full_text_grid(), dump and abi_text whole."""
    valid, full = valid_grid(), full_text_grid()
    out = ["[plan]"]
    for c, (rc, body) in zip(valid, dump(valid)):
        out.append(f"{describe(c)}\t{rc}\t" + (body.strip() if rc else f"{sha(body)}\t{sha(abi_text(lib, c, region_names(body)))}"))
    out += write_refusals([(rc, body.strip() if rc else sha(body)) for rc, body in dump(refusal_grid())])
    out.append("[full]")
    for c, (rc, body) in zip(full, dump(full)):
        assert rc == 0, describe(c)
        out.append(f"== {describe(c)}\n{body}-- abi\n{abi_text(lib, c, region_names(body))}".rstrip("\n"))
    return "\n".join(out) + "\n"
