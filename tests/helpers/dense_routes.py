"""Which kernel every Dense layer of the tail runs on, restated on the host, and the cases of tests/test_gpu_dense_routes.py.

Two halves, as tests/helpers/conv_routes.py.  The plan-level half (conv_routes.layers, fwd_splits, dense_wgrad_slabs, fwd_narrow,
part_rows: csrc/net_plan.h) is held to the real code by tests/test_dense_routes_host.py through tests/helpers/plan_dump.cpp.  The
launch-level half (routes: csrc/learn_step.h, csrc/net_launch.h) has no host entry point: it is written from the source, every rule
with its file and line, and tests/test_dense_routes_host.py pins its result for every case and precision as a literal table, so that
a moved threshold fails a test instead of moving a case onto another kernel.

Pure Python: no GPU, no torch."""
from tests.helpers import conv_routes as R

_ceil, _round_up = R._ceil, R._round_up
layers, fwd_splits, dense_wgrad_slabs = R.layers, R.fwd_splits, R.dense_wgrad_slabs

LN_MAX_BLOCKS = 256  # net_plan.h:28
LN_WIDE_MAX_COLS = 16  # row_kernels.h:213
HIDDEN_MAX = 256 * LN_WIDE_MAX_COLS  # net_plan.h plan_dense_tail: the widest hidden Dense the plan accepts
HEAD_MAX = 5456  # net_plan.h plan_dense_tail / plan_heads: the widest head row (dense_post_kernel: 3 rows in 64 KB of LDS)
HC_THREADS, HC_MAX_COLS, HC_WAVES = 512, 4, 8  # head_chain.h:57-60


# ------------------------------------------------------------------ the selection code, restated (net_plan.h, learn_step.h)
def _dense_dgrad_ln(cfg, layers):
    """The fused data gradient + LayerNorm backward under the first dense layer of a cnn: None when it is not taken
    (net_kernels.hip:2186-2187), else its K groups (2: DenseDgradLN<P, 128, 2>, 1: DenseDgradLN<P, 128>; :2206, :2213-2214).
    part_rows of the conv layer below: net_plan.h:389-390, 463-464."""
    if cfg["arch"] != "cnn":
        return None
    B, below, d0 = cfg["B"], layers[2], layers[3]
    part_rows = max(256, _ceil(B, 64) * below["npix"]) if below["cp"] == 64 else 256
    if below["cp"] != 64 or part_rows < _ceil(B, 128) * below["npix"]:
        return None
    return 2 if _ceil(B, 128) * (d0["in_p"] // 64) <= 256 and d0["cp"] % 64 == 0 else 1


def _head_chain(cfg, hid_p, nha_p, K, passes):
    """(S, COLS) the learn step's head chain runs with, or None when it is skipped: net_kernels.hip:1929-1941 (eligibility, S),
    :471-475 (head_chain_lds_bytes), :2012-2015 (COLS).  part_rows: net_plan.h:389-390."""
    B = cfg["B"]
    if hid_p > 512 * 4 or hid_p % 8:
        return None
    S = 4 if B >= 1024 else 2 if B >= 512 else 1
    part_rows = max(256, B)
    pitch = _ceil(hid_p, 32) * 32 + 8
    lds = (2 if passes >= 2 else 1) * 16 * pitch * 2 + (8 * 16 * nha_p + 16 * nha_p + S * nha_p + nha_p + 4 + 2 * S * hid_p) * 4 + S * K * 8 + 8 * 2 * S * 2 * 4 + 64
    if _ceil(B, S) > part_rows or S * K > 512 or lds > 150 * 1024:
        return None
    cols = _ceil(hid_p, 512)
    return S, (1 if cols == 1 else 2 if cols == 2 else 4)


# (the two functions above stood in tests/test_gpu_bf16_model.py, which imports them back; their file and line references are those
# of the single source file they were written from.  Today: learn_step.h:63-86 head_chain_plan, :165 COLS, :405-407 and :427
# DenseDgradLN, head_chain.h:63-68 the LDS bytes -- which now count S * K * 12 bytes of per-pair state where _head_chain counts
# S * K * 8.  head_chain_lds_bytes below is today's formula; tests/test_dense_routes_host.py holds every case to the same decision
# under both.)
def head_chain_lds_bytes(hid_p, nha_p, K, passes, S):
    """head_chain.h:63-68"""
    pitch = _ceil(hid_p, 32) * 32 + 8
    return ((2 if passes >= 2 else 1) * 16 * pitch * 2 + (HC_WAVES * 16 * nha_p + 16 * nha_p + S * nha_p + nha_p + 4 + 2 * S * hid_p) * 4
            + S * K * 12 + HC_WAVES * 2 * S * 2 * 4 + 64)


def effective_splits(K, splits):
    """(slabs written, K steps of each) of a split-K GEMM: net_launch.h:199-206"""
    ksteps = _ceil(K, 32)
    splits = max(1, min(splits, ksteps))
    sps = _ceil(ksteps, splits)
    return _ceil(ksteps, sps), sps


def dense_layers(cfg):
    """The Dense layers of the plan in order, the head last, as dicts: name, i (plan index), c / cp (true / padded width), in_f / in_p,
    unpadded (the fc first layer reads the caller's rows), head, ln; and the hidden layers of conv_routes.layers in front of them."""
    hidden, head_in_p = layers(cfg)
    nha = (1 + cfg["K"]) * cfg["A"]
    out = []
    in_f = cfg.get("obs", R.FC_OBS)[0] if cfg["arch"] == "fc" else None
    for i, L in enumerate(hidden):
        if L["kind"] == 1:
            out.append(dict(L, i=i, in_f=in_f if in_f is not None else L["in_p"], unpadded=cfg["arch"] == "fc" and i == 0, head=False))
            in_f = L["c"]
        else:
            in_f = L["npix"] * L["c"]
    n_dense = len(out)
    out.append(dict(name=f"Dense_{n_dense}", kind=1, ln=None, c=nha, cp=_round_up(nha, 8), npix=1, K=head_in_p, in_p=head_in_p, i=len(hidden),
                    in_f=in_f if in_f is not None else head_in_p, unpadded=cfg["arch"] == "fc" and not hidden, head=True))
    return hidden, out


def part_rows(cfg, hidden, i):
    """rows of the partial-sum region of hidden layer i: net_plan.h:512-522 part_rows_of (dense layers; a convolution under the first
    Dense: conv_routes.plan_fields)"""
    L, B = hidden[i], cfg["B"]
    if L["kind"] == 1:
        return max(LN_MAX_BLOCKS, B)
    return R.plan_fields(cfg, B)[i]["part_rows"]


def routes(cfg, precision, update=True):
    """Per Dense layer, the head last: dict(name, fwd, head, dgrad, ln, wgrad).  `update`: a learn step; False: a gradient-only pass
    (grad_on_batch), which never takes the head chain (learn_step.h:75 c.update()).
      fwd:   dict(kernel="unpadded" | "plain_narrow" | "plain_big", splits (the plan's factor), slabs (what dense_post_kernel or the
             head chain sums), passes (column passes of dense_post_kernel), post ("dense_post" or "chain": who finishes the row in a
             learn step; forward-only calls always run dense_post_kernel))
      head:  (the head only) dict(kernel="chain", S, cols) or dict(kernel="generic")
      dgrad: the data gradient this layer runs for the layer below: None (the lowest layer; the head under the chain),
             dict(kernel="DenseDgradLN", kg) or dict(kernel="narrow" | "big")
      ln:    (hidden layers) the LayerNorm / ReLU backward that writes this layer's dz: dict(kernel="chain" | "small" | "wide", tpr,
             rows (the most rows summed into one partial row), parts (partial rows), by ("adam": adam_kernel sums them))
      wgrad: dict(kernel="fused-adam") or dict(kernel="slabs", slabs, steps)"""
    x3 = precision == "bf16x3"
    B, K = cfg["B"], cfg["K"]
    hidden, dense = dense_layers(cfg)
    head = dense[-1]
    # learn_step.h:63-86 head_chain_plan (scalar heads, the plan's own pairs, an update step): the last hidden layer is a Dense
    hc = None
    if update and hidden and hidden[-1]["kind"] == 1:  # :75 c.update() && n_layers >= 2 && hid.kind == 1
        hc = _head_chain(cfg, head["in_p"], head["cp"], K, 3 if x3 else 1)
    out = []
    for d, L in enumerate(dense):
        r = dict(name=L["name"])
        # forward: net_plan.h:497-507, net_launch.h:256-272
        N2 = 2 * B
        ft = _ceil(N2, 128) * _ceil(L["cp"], 128)
        narrow = ft <= 64 and not L["unpadded"] and L["cp"] % 64 == 0
        fs = fwd_splits(N2, L["cp"], L["in_p"], L["unpadded"])
        ns, _ = effective_splits(L["in_f"] if L["unpadded"] else L["in_p"], fs)  # net_launch.h:256
        chain_here = hc is not None and d == len(dense) - 2  # learn_step.h:135: the chain finishes the last hidden layer's rows
        r["fwd"] = dict(kernel="unpadded" if L["unpadded"] else "plain_narrow" if narrow else "plain_big", splits=fs, slabs=ns,
                        passes=_ceil(L["cp"], 512), post="chain" if chain_here else "dense_post")  # row_kernels.h:38 (512 columns a pass)
        if L["head"]:
            r["head"] = dict(kernel="chain", S=hc[0], cols=hc[1]) if hc else dict(kernel="generic")
        # data gradient for the layer below: learn_step.h:446-462
        if L["i"] == 0 or (L["head"] and hc):  # :450
            r["dgrad"] = None
        else:
            below = hidden[L["i"] - 1]
            kg = _dense_dgrad_ln(cfg, hidden) if below["kind"] != 1 else None  # :405-407 (the first Dense of a cnn)
            if kg:
                r["dgrad"] = dict(kernel="DenseDgradLN", kg=kg, ksteps=_ceil(L["cp"], 32))  # :419 K = out_p
            else:
                r["dgrad"] = dict(kernel="narrow" if _ceil(B, 128) * _ceil(L["in_p"], 128) < 200 else "big")  # :460
        # LayerNorm / ReLU backward of a hidden Dense: learn_step.h:483-493, net_launch.h:342-368
        if not L["head"]:
            if chain_here:  # :483-484: one partial row per workgroup of S transitions
                r["ln"] = dict(kernel="chain", tpr=0, rows=hc[0], parts=_ceil(B, hc[0]), by="adam")
            else:
                cp = L["cp"]
                tpr = 8 if cp <= 32 else 16 if cp <= 64 else 32 if cp <= 128 else 64 if cp <= 256 else 0  # net_launch.h:355-358
                if tpr:
                    rpb = 256 // tpr  # row_kernels.h:121
                    nb = min(_ceil(B, rpb), LN_MAX_BLOCKS)  # net_launch.h:350-351
                    r["ln"] = dict(kernel="small", tpr=tpr, rows=rpb * _ceil(_ceil(B, rpb), nb), parts=nb, by="adam")
                else:
                    assert cp <= HIDDEN_MAX, "ln_bwd refuses the width (net_launch.h:360)"
                    nb = min(B, LN_MAX_BLOCKS)  # :361
                    r["ln"] = dict(kernel="wide", tpr=0, cols=_ceil(cp, 256), rows=_ceil(B, nb), parts=nb, by="adam")
        # weight gradient: learn_step.h:254-271 (no gradient clipping in these cases)
        slabs, steps = effective_splits(B, dense_wgrad_slabs(B, L["in_p"], L["cp"]))  # :260, :265
        if L["head"] and hc:  # :259, :195: head_chain_tail on the weight-gradient stream, always into slabs
            r["wgrad"] = dict(kernel="slabs", slabs=slabs, steps=steps)
        elif slabs == 1 and not L["unpadded"]:  # :267
            r["wgrad"] = dict(kernel="fused-adam", slabs=1, steps=steps)
        else:
            r["wgrad"] = dict(kernel="slabs", slabs=slabs, steps=steps)
        out.append(r)
    return out


def plan_fields(cfg):
    """Per Dense layer, the head last, the plan's own decisions as plan_dump prints them: fwd_narrow, fwd_splits, gw_slabs, part_rows
    (hidden layers), in_p, out_p, in_unpadded_ld."""
    hidden, dense = dense_layers(cfg)
    B = cfg["B"]
    out = []
    for L in dense:
        N2 = 2 * B
        ft = _ceil(N2, 128) * _ceil(L["cp"], 128)
        f = dict(fwd_narrow=int(ft <= 64 and not L["unpadded"] and L["cp"] % 64 == 0), fwd_splits=fwd_splits(N2, L["cp"], L["in_p"], L["unpadded"]),
                 gw_slabs=dense_wgrad_slabs(B, L["in_p"], L["cp"]), in_p=L["in_p"], out_p=L["cp"], out_f=L["c"],
                 in_unpadded_ld=L["in_f"] if L["unpadded"] else 0)
        if not L["head"]:
            f["part_rows"] = part_rows(cfg, hidden, L["i"])
        out.append(f)
    return out


def fmt(r):
    """A layer's routes as the literal table of tests/test_dense_routes_host.py writes them: (fwd, head or ln, dgrad, wgrad)."""
    f = r["fwd"]
    fwd = f"{f['kernel']} x{f['splits']} slabs={f['slabs']} passes={f['passes']} {f['post']}"
    if "head" in r:
        h = r["head"]
        mid = f"chain<S={h['S']},COLS={h['cols']}>" if h["kernel"] == "chain" else "generic-head"
    else:
        n = r["ln"]
        kern = {"chain": "chain", "small": f"small<{n['tpr']}>", "wide": f"wide cols={n.get('cols')}"}[n["kernel"]]
        mid = f"{kern} rows={n['rows']} parts={n['parts']} by={n['by']}"
    d = r["dgrad"]
    dg = "none" if d is None else f"DenseDgradLN kg={d['kg']} ksteps={d['ksteps']}" if d["kernel"] == "DenseDgradLN" else d["kernel"]
    w = r["wgrad"]
    wg = "fused-adam" if w["kernel"] == "fused-adam" else f"slabs={w['slabs']}x{w['steps']}"
    return fwd, mid, dg, wg


def conv2_ln(cfg):
    """The LayerNorm backward of the convolution under the first Dense of a cnn that takes DenseDgradLN: dict(kernel="fused", rows,
    parts, by="reduce_rows") -- one partial row per (128-sample tile, 64-column tile) (learn_step.h:420, :440: each sums up to
    128 samples of the 64 / cp pixels its columns cover), summed by reduce_rows_kernel in front of Adam (:485-486, :587-590)."""
    hidden, dense = dense_layers(cfg)
    d0 = dense[0]
    below = hidden[d0["i"] - 1]
    return dict(kernel="fused", rows=min(cfg["B"], 128) * (64 // below["cp"]), parts=_ceil(cfg["B"], 128) * (d0["in_p"] // 64), by="reduce_rows")


# ------------------------------------------------------------------ the cases
LADDER = (21, 64, 128, 200, 264, 520, 72)
CASES = {
    "fc-ladder": dict(arch="fc", obs=(11,), feats=LADDER, K=2, A=3, B=37, ln=True),
    "fc-ladder-relu": dict(arch="fc", obs=(11,), feats=LADDER, K=2, A=3, B=5, ln=False),
    "fc-rows": dict(arch="fc", obs=(8,), feats=(200, 120, 16), K=1, A=2, B=2100, ln=True),
    "fc-2048": dict(arch="fc", obs=(8,), feats=(16, 2048), K=2, A=3, B=9, ln=True),
    "fc-4096": dict(arch="fc", obs=(8,), feats=(8, 4096), K=1, A=2, B=3, ln=True),
    "fc-dgrad-big": dict(arch="fc", obs=(8,), feats=(1024, 40), K=1, A=2, B=3200, ln=True),
    "cnn-2dense": dict(arch="cnn", obs=(40, 40, 2), feats=(16, 32, 64, 104, 200), K=3, A=3, B=7, ln=True),
    "fc-headonly": dict(arch="fc", obs=(9,), feats=(), K=2, A=3, B=5, ln=False),
}
PRECISIONS = {"fc-ladder": ("bf16x3", "bf16"), "fc-ladder-relu": ("bf16x3",), "fc-rows": ("bf16x3",), "fc-2048": ("bf16x3", "bf16"),
              "fc-4096": ("bf16x3",), "fc-dgrad-big": ("bf16",), "cnn-2dense": ("bf16x3", "bf16"), "fc-headonly": ("bf16x3",)}
RUNS = [(c, p) for c in CASES for p in PRECISIONS[c]]
HOST_ONLY = {"fc-dgrad-big-3072": dict(CASES["fc-dgrad-big"], B=3072)}  # the narrow side of the data gradient's switch, in the host table only
