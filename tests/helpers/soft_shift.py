"""numpy float32 restatement of the definition of include/isdqn_hip.h, isdqn_net_soft_shift -- the soft head shift of iS-DQN -- on the
flat parameter vector of the internal layout, driven by the tensor table of isdqn_net_param_layout, and the wrong variants the tests must
be able to tell from it (the pattern of tests/helpers/reset.py: each wrong variant is first shown to differ from the definition on the
test's own inputs, so that a device result that equals the definition cannot equal a variant).

    new[k] = fl32( fl32(omt * old[k]) + fl32(tau * old[k+1]) ),  omt = fl32(1 - tau),  k = 0 .. K-1

Every product and the sum are ONE float32 numpy operation on float32 operands: what __fmul_rn / __fadd_rn compute.  A QNetEngine or a
tests.helpers.redo.HostLayout can be passed as ``lay``."""
import numpy as np

F32 = np.float32


def head_geometry(lay):
    """(w_off, b_off, in_p, out_p, R, K) of the last Dense: its kernel is [out_p][in_p] at w_off, its bias [out_p] at b_off; the first
    (1 + K) * R rows are the head blocks, R = (n_actions + dueling) * max(n_bins, n_quantiles, 1), the rows behind them padding."""
    last = max(int(i.layer) for i in lay.infos)
    kernel = next(i for i in lay.infos if int(i.layer) == last and int(i.kind) == 1)
    bias = next(i for i in lay.infos if int(i.layer) == last and int(i.kind) == 2)
    in_p = int(kernel.dims[1])
    out_p = int(kernel.size) // in_p
    assert out_p * in_p == int(kernel.size) and int(bias.size) == out_p
    cfg = lay.cfg
    R = (int(cfg.n_actions) + (1 if int(cfg.dueling) else 0)) * max(int(cfg.n_bins), int(cfg.n_quantiles), 1)
    K = int(cfg.n_heads) - 1
    assert (1 + K) * R <= out_p
    return int(kernel.offset), int(bias.offset), in_p, out_p, R, K


def blend(omt, tau, lo, up, fma=False):
    """fl32(fl32(omt * lo) + fl32(tau * up)); ``fma``: the WRONG variant fl32(omt * lo + fl32(tau * up)) with the first product
    unrounded, what a contracted v_fma_f32 gives (float64 holds the product of two float32 exactly)."""
    omt, tau = F32(omt), F32(tau)
    with np.errstate(invalid="ignore", over="ignore"):
        if fma:
            return (np.float64(omt) * lo.astype(np.float64) + (tau * up).astype(F32).astype(np.float64)).astype(F32)
        return ((omt * lo).astype(F32) + (tau * up).astype(F32)).astype(F32)


def head_views(lay, flat):
    """(weights [1 + K][R][in_p], biases [1 + K][R]) as views of the flat buffer ``flat`` (writes go through)."""
    w_off, b_off, in_p, _, R, K = head_geometry(lay)
    return flat[w_off : w_off + (1 + K) * R * in_p].reshape(1 + K, R, in_p), flat[b_off : b_off + (1 + K) * R].reshape(1 + K, R)


def soft_shift(lay, params, tau, *, fma=False, shifted_neighbours=False):
    """isdqn_net_soft_shift on a host copy; returns the new flat buffer.  tau = 0 returns the bits of ``params``; tau = 1 the hard
    shift's (head k <- the bits of head k+1, a NaN and the sign of a zero included).  The keyword arguments select the WRONG variants:
    ``fma`` (the sum contracted with the first product) and ``shifted_neighbours`` (the heads walked downward in place, so that head k
    reads the value head k+1 has AFTER its own update)."""
    p = np.array(params, dtype=F32, copy=True)
    tau = F32(tau)
    if tau == 0:
        return p
    old = p.copy()
    K = head_geometry(lay)[5]
    for new, was in zip(head_views(lay, p), head_views(lay, old)):
        if tau == 1:
            new[:K] = was[1:]
            continue
        omt = F32(1.0) - tau
        if shifted_neighbours:
            for k in reversed(range(K)):
                new[k] = blend(omt, tau, new[k], new[k + 1], fma)
        else:
            new[:K] = blend(omt, tau, was[:K], was[1:], fma)
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# The networks of the device tests (tests/test_gpu_soft_shift.py, scripts/soft_shift_bounds_check.py): the kernel sees the last Dense only,
# so an fc torso on 8 observations is enough.  One hidden layer of 20 (in_p pads to 24) or 24 (unpadded); A = 3; K in {1, 3}; scalar,
# histogram (5 bins), quantile (4) and dueling heads (a hidden Dense of even width: 24).  R * (1 + K) is no multiple of 8 in most of them:
# padding rows follow the last head.  "wide": 2 * 18 * 51 rows of 512 columns, 459 workgroups; "stride": 2 * 10 * 256 rows of 1024 columns,
# 655 360 positions, more than the 2048 * 256 lanes of the capped grid -- the one size at which the stride loop takes a second turn.
A = 3
HEADS = {"scalar": {}, "bins": dict(n_bins=5, min_value=-10.0, max_value=10.0, sigma=0.3), "quantiles": dict(n_quantiles=4, huber_delta=1.0),
         "dueling": dict(dueling=True)}
CONFIGS = {f"f{f}-K{K}-{h}": dict(features=(f,), n_actions=A, K=K, options=HEADS[h])
           for f in (20, 24) for K in (1, 3) for h in HEADS if not (h == "dueling" and f == 20)}
CONFIGS["wide"] = dict(features=(512,), n_actions=18, K=1, options=dict(n_bins=51, min_value=-10.0, max_value=10.0, sigma=0.3))
CONFIGS["stride"] = dict(features=(1024,), n_actions=10, K=1, options=dict(n_quantiles=256, huber_delta=1.0))
TAUS = (0.005, 0.5)


def make_engine(name, batch_size=4, **extra):
    """The QNetEngine of CONFIGS[name] (a GPU is needed)."""
    from slimdqn._engine import QNetEngine

    c = CONFIGS[name]
    return QNetEngine((8,), c["n_actions"], 1 + c["K"], c["features"], "fc", False, batch_size, **c["options"], **extra)


def written_extents(lay, mirror=False):
    """[(offset, size)] in floats of everything isdqn_net_soft_shift may read (heads 0 .. K) in the flat buffer: kernel rows, then
    biases.  ``mirror``: the same ranges counted from the start of the workspace region "wsplit", each rounded up to whole groups of 8
    floats -- a group keeps its 8 bf16 high halves in its first 16 bytes and the 8 low halves in the 16 behind them, so the last bias
    of a head block that ends inside a group has its low half past the block's own floats (still inside the padded bias)."""
    w_off, b_off, in_p, _, R, K = head_geometry(lay)
    up = (lambda n: -(-n // 8) * 8) if mirror else (lambda n: n)
    return [(w_off, up((1 + K) * R * in_p)), (b_off, up((1 + K) * R))]
