"""Host-side driver of the HIP Q-network: configuration, parameter import/export between the
reference's Flax pytree layout and the library's internal layout, workspace ownership, and thin
wrappers over the C-ABI entry points.  Pure plumbing: no arithmetic of the hot path lives here.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import math
from typing import Dict, Sequence

import numpy as np
import torch

from slimdqn import _hip
from slimdqn import _conservative
from slimdqn import _mixture
from slimdqn import _optimizer
from slimdqn import _projection
from slimdqn import _sparsity


def _round_up(a, b):
    return (a + b - 1) // b * b


MUNCHAUSEN_DOUBLE_Q_REFUSED = (
    "double_q and munchausen_tau > 0 exclude each other: the Munchausen target bootstraps from the soft value "
    "tau * logsumexp(Q / tau), which has no argmax to decouple")


def check_munchausen(double_q, munchausen_tau) -> None:
    """The one combination the library refuses (ISDQN_ERR_ARG), said before anything is allocated."""
    if double_q and float(munchausen_tau) > 0.0:
        raise ValueError(MUNCHAUSEN_DOUBLE_Q_REFUSED)


QUANTILE_HISTOGRAM_REFUSED = "n_quantiles > 0 and n_bins > 0 exclude each other: a head is either quantile values or a histogram"
QUANTILE_MUNCHAUSEN_REFUSED = (
    "n_quantiles > 0 with munchausen_tau > 0 is not built: the Munchausen target of quantile heads is M-IQN's atom-wise form")
QUANTILE_BATCH_NORM_REFUSED = "n_quantiles > 0 with batch_norm is not built (ISDQN_ERR_UNSUPPORTED)"


def check_quantiles(n_quantiles, n_bins=0, munchausen_tau=0.0, batch_norm=False) -> None:
    """The combinations the library refuses with quantile heads, said before anything is allocated or written."""
    if int(n_quantiles) > 0:
        if int(n_bins) > 0:
            raise ValueError(QUANTILE_HISTOGRAM_REFUSED)
        if float(munchausen_tau) > 0.0:
            raise ValueError(QUANTILE_MUNCHAUSEN_REFUSED)
        if batch_norm:
            raise ValueError(QUANTILE_BATCH_NORM_REFUSED)


CATEGORICAL_NEEDS_HISTOGRAM = "categorical needs the histogram heads: n_bins > 0 (the entry points: -cat modifies -hl)"
CATEGORICAL_QUANTILE_REFUSED = "categorical and n_quantiles > 0 exclude each other: the categorical loss is one of the histogram heads"
CATEGORICAL_MUNCHAUSEN_REFUSED = (
    "categorical with munchausen_tau > 0 is not built: the Munchausen target of a categorical head is an atom-wise form")


def check_categorical(categorical, n_bins=0, n_quantiles=0, munchausen_tau=0.0) -> None:
    """The combinations the library refuses with the categorical loss, said before anything is allocated or written."""
    if categorical:
        if int(n_quantiles) > 0:
            raise ValueError(CATEGORICAL_QUANTILE_REFUSED)
        if int(n_bins) <= 0:
            raise ValueError(CATEGORICAL_NEEDS_HISTOGRAM)
        if float(munchausen_tau) > 0.0:
            raise ValueError(CATEGORICAL_MUNCHAUSEN_REFUSED)


REDO_IMPALA_REFUSED = "ReDo is not built for architecture_type 'impala': the residual adds make a neuron's outgoing weights ambiguous (ISDQN_ERR_UNSUPPORTED)"
REDO_BATCH_NORM_REFUSED = "ReDo is not built for batch_norm: per-position statistics sit between the layers (ISDQN_ERR_UNSUPPORTED)"


def check_redo(architecture_type, batch_norm=False) -> None:
    """The networks whose dormant neurons the library refuses to recycle, said before anything is allocated or written."""
    if architecture_type == "impala":
        raise ValueError(REDO_IMPALA_REFUSED)
    if batch_norm:
        raise ValueError(REDO_BATCH_NORM_REFUSED)


DUELING_IMPALA_REFUSED = "dueling heads are not built for architecture_type 'impala' (ISDQN_ERR_UNSUPPORTED)"
DUELING_BATCH_NORM_REFUSED = "dueling heads are not built for batch_norm (ISDQN_ERR_UNSUPPORTED)"
DUELING_NEEDS_HIDDEN_DENSE = "dueling heads need a hidden Dense layer in front of the head: its two halves are the value and the advantage stream"
DUELING_ODD_WIDTH_REFUSED = "dueling heads split the last hidden Dense into two equal streams: its width must be even"


def check_dueling(dueling, architecture_type, features, batch_norm=False) -> None:
    """The networks the library refuses to give dueling heads, said before anything is allocated or written."""
    if dueling:
        if architecture_type == "impala":
            raise ValueError(DUELING_IMPALA_REFUSED)
        if batch_norm:
            raise ValueError(DUELING_BATCH_NORM_REFUSED)
        feats = [int(f) for f in features]
        if len(feats) <= (0 if architecture_type == "fc" else 3):
            raise ValueError(DUELING_NEEDS_HIDDEN_DENSE)
        if feats[-1] % 2 != 0:
            raise ValueError(DUELING_ODD_WIDTH_REFUSED)


GRAD_CLIP_IMPALA_REFUSED = "gradient clipping is not built for architecture_type 'impala': the torso's backward runs its own optimizer launches (ISDQN_ERR_UNSUPPORTED)"
GRAD_CLIP_BATCH_NORM_REFUSED = "gradient clipping is not built for batch_norm: that learn path runs its own optimizer launches (ISDQN_ERR_UNSUPPORTED)"
GRAD_CLIP_NEGATIVE_REFUSED = "max_grad_norm must be >= 0 (0 = off, inf = measure the gradient norm and never clip)"


def check_grad_clip(max_grad_norm, architecture_type, batch_norm=False) -> None:
    """The thresholds and the networks the library refuses to clip, said before anything is allocated or written."""
    c = float(max_grad_norm)
    if not c >= 0.0:  # (NaN too)
        raise ValueError(GRAD_CLIP_NEGATIVE_REFUSED)
    if c > 0.0:
        if architecture_type == "impala":
            raise ValueError(GRAD_CLIP_IMPALA_REFUSED)
        if batch_norm:
            raise ValueError(GRAD_CLIP_BATCH_NORM_REFUSED)


NOISY_BATCH_NORM_REFUSED = "noisy layers are not built for batch_norm: running statistics would be committed into the composed parameters (ISDQN_ERR_UNSUPPORTED)"
NOISY_IMPALA_REFUSED = "noisy layers are not built for architecture_type 'impala' (ISDQN_ERR_UNSUPPORTED)"
NOISY_GRAD_CLIP_REFUSED = "noisy layers with max_grad_norm > 0 are a follow-up: the global norm must cover the gradient of sigma too (ISDQN_ERR_UNSUPPORTED)"
NOISY_REDO_REFUSED = "noisy layers and ReDo exclude each other: a recycled neuron would keep the sigma it had"


def check_noisy(noisy, architecture_type, batch_norm=False, max_grad_norm=0.0, redo=False) -> None:
    """The networks and options the library refuses to make noisy (in the library's order), said before anything is allocated or written."""
    if noisy:
        if batch_norm:
            raise ValueError(NOISY_BATCH_NORM_REFUSED)
        if architecture_type == "impala":
            raise ValueError(NOISY_IMPALA_REFUSED)
        if float(max_grad_norm) > 0.0:
            raise ValueError(NOISY_GRAD_CLIP_REFUSED)
        if redo:
            raise ValueError(NOISY_REDO_REFUSED)


AUGMENT_FC_REFUSED = "random-shift augmentation shifts image frames: architecture_type 'fc' reads float32 vector observations"
AUGMENT_PAD_REFUSED = "augment_pad must be an integer in [0, 127] (0: off; include/isdqn_hip.h, isdqn_replay_augment_shift)"


def check_augment(pad, architecture_type) -> None:
    """The pads and the torso the random-shift augmentation refuses, said before anything is allocated or written.  0 is off and goes
    with every torso; every torso that reads frames (cnn, impala, with LayerNorm or BatchNorm) takes a pad > 0."""
    if isinstance(pad, bool) or int(pad) != pad or not 0 <= int(pad) <= 127:
        raise ValueError(AUGMENT_PAD_REFUSED)
    if int(pad) > 0 and architecture_type == "fc":
        raise ValueError(AUGMENT_FC_REFUSED)


@dataclasses.dataclass(frozen=True)
class NetOptions:
    """The head, loss and exploration options that the agents (iSDQN, DQN, TFDQN and the analysis agents) and QNetEngine share, as one
    checked value.  Field names are the constructors' keyword names, defaults are QNetEngine's; this is the one place that documents
    them (the agents' docstrings say only what is particular to them).

    ``huber_delta``: 0 keeps the reference's squared TD error (isdqn.py:102); > 0 trains on the Huber loss (with quantile heads: kappa).
    ``n_bins`` > 0: each head predicts a histogram of ``n_bins`` bins over [min_value, max_value] and trains on the HL-Gauss
    cross-entropy with std ``sigma`` (include/isdqn_hip.h, isdqn_net_config::n_bins; n_heads * n_actions * n_bins logits, region
    "logits"); acting and ``forward`` use the expectations.
    ``double_q``: Double Q-learning targets (van Hasselt et al. 2016; include/isdqn_hip.h, isdqn_net_config::double_q) -- iS-DQN's online
    head 1 + k picks the next action that head k values, DQN's online parameters pick the action its target parameters value; off keeps
    the reference's max.  The *_target forms then keep the target network's rows in region "q_target".
    ``munchausen_tau`` > 0: Munchausen targets (Vieillard et al. 2020) -- the bootstrap value is the soft value
    tau * logsumexp(Q / tau) of the value head and ``munchausen_alpha`` * clip(tau ln pi(a|s), ``munchausen_clip``, 0) is added to the
    reward (include/isdqn_hip.h, isdqn_net_config::munchausen_tau); 0 is off.  The *_target forms then keep the target network's rows of
    concat(state, next_state) in region "q_target".  Not together with ``double_q`` (ValueError).
    ``n_quantiles`` > 0: QR-DQN heads -- each action of each head predicts ``n_quantiles`` quantile values and trains on the
    quantile-regression loss with kappa = ``huber_delta`` (include/isdqn_hip.h, isdqn_net_config::n_quantiles); acting uses
    their means.  Not with ``n_bins`` > 0, Munchausen targets or batch_norm (ValueError).
    ``categorical``: with ``n_bins`` > 0, train the histogram heads on the C51 categorical projection loss (include/isdqn_hip.h,
    isdqn_net_config::categorical) instead of HL-Gauss: same heads, same acting, ``sigma`` ignored.  Not without ``n_bins``, nor with
    ``n_quantiles`` > 0 or Munchausen targets (ValueError).
    ``dueling``: dueling value / advantage heads (Wang et al. 2016; include/isdqn_hip.h, isdqn_net_config::dueling) -- the last
    Dense holds a value row and ``n_actions`` advantage rows per head (per bin / quantile with those heads), read from the two
    halves of the last hidden layer and combined on the device; every loss, target and acting rule then runs on the combined
    values.  Needs a hidden Dense layer of even width; not with batch_norm or the impala torso (ValueError).
    ``max_grad_norm`` > 0 (``inf`` allowed): clip the gradient by its global norm in front of Adam, as
    optax.clip_by_global_norm chained with optax.adam does (include/isdqn_hip.h, isdqn_net_config::max_grad_norm); the norm stays on
    the device in region "grad_clip" and an agent's ``update_target_params`` adds ``grad_norm`` (the mean over the interval's gradient
    steps) and ``grad_clipped_fraction`` to its logs.  ``inf`` measures and never clips; 0 is off.  Negative or NaN, batch_norm or the
    impala torso: ValueError.
    ``noisy``: NoisyNet exploration (Fortunato et al. 2018; include/isdqn_hip.h, isdqn_noisy_layout) -- every Dense layer, the head
    included, carries factorised Gaussian noise with a learned scale sigma (initialised to ``noisy_sigma0`` / sqrt(fan-in)).  In an
    agent every acting call on its own parameters draws first (one draw serves all rows of a batched call), every learn step draws
    first, and ``noisy_eval`` = True (or the ``noisy_evaluation()`` context) acts with the mean network; ``get_model()`` then carries
    "sigma_kernel" / "sigma_bias" beside the Dense leaves.  The epsilon schedule is the caller's: set it to 0 to explore by noise
    alone.  Not with batch_norm, the impala torso or ``max_grad_norm`` > 0 (ValueError: ``check_noisy``, which the constructors call
    beside ``check``)."""

    huber_delta: float = 0.0
    n_bins: int = 0
    min_value: float = -100.0
    max_value: float = 100.0
    sigma: float = 3.0
    double_q: bool = False
    munchausen_tau: float = 0.0
    munchausen_alpha: float = 0.9
    munchausen_clip: float = -1.0
    n_quantiles: int = 0
    categorical: bool = False
    dueling: bool = False
    max_grad_norm: float = 0.0
    noisy: bool = False
    noisy_sigma0: float = 0.5

    @classmethod
    def pick(cls, mapping) -> "NetOptions":
        """The options among the entries of ``mapping`` (a constructor's ``locals()``), each converted to the type of its default."""
        return cls(**{f.name: type(f.default)(mapping[f.name]) for f in dataclasses.fields(cls)})

    def check(self, architecture_type, features, batch_norm=False) -> None:
        """The head and loss rules, once, in this order: dueling, gradient clipping, Munchausen with double_q, categorical, quantiles --
        the first rule violated answers.  ``check_noisy`` and ``check_augment`` are not in here, because the constructors place them
        differently around this call: QNetEngine asks ``check_noisy`` first; an agent asks its own rules first (iSDQN: ema_tau;
        TFDQN: double_q, then ema_tau; DQN: Munchausen with double_q in front, ema_tau behind), then this, then ``check_augment``, then
        ``check_noisy`` (tests/golden/options_snapshot.txt holds which refusal answers first for every pair of settings)."""
        check_dueling(self.dueling, architecture_type, features, batch_norm)
        check_grad_clip(self.max_grad_norm, architecture_type, batch_norm)
        check_munchausen(self.double_q, self.munchausen_tau)
        check_categorical(self.categorical, self.n_bins, self.n_quantiles, self.munchausen_tau)
        check_quantiles(self.n_quantiles, self.n_bins, self.munchausen_tau, batch_norm)

    def fill(self, cfg: "_hip.NetConfig") -> None:
        """Write the options into an isdqn_net_config.  An option that is off leaves ``max_grad_norm``, ``categorical`` and ``dueling``
        at the 0 the structure starts with; without ``n_bins`` the three hl_* fields are 0."""
        if self.max_grad_norm > 0.0:
            cfg.max_grad_norm = self.max_grad_norm
        cfg.huber_delta = self.huber_delta
        cfg.n_bins = self.n_bins
        cfg.hl_min, cfg.hl_max, cfg.hl_sigma = (self.min_value, self.max_value, self.sigma) if self.n_bins else (0.0, 0.0, 0.0)
        if self.categorical:
            cfg.categorical = 1
        cfg.n_quantiles = self.n_quantiles
        if self.dueling:
            cfg.dueling = 1
        cfg.double_q = 1 if self.double_q else 0
        cfg.munchausen_tau, cfg.munchausen_alpha, cfg.munchausen_clip = self.munchausen_tau, self.munchausen_alpha, self.munchausen_clip

    def engine_kwargs(self, noisy_seed: int = 0) -> dict:
        """The keywords that build a QNetEngine with these options.  ``noisy_sigma0`` and the seed of the draws go only with ``noisy``:
        an engine without noise reads neither and keeps its defaults."""
        kw = dataclasses.asdict(self)
        if self.noisy:
            kw["noisy_seed"] = noisy_seed
        else:
            del kw["noisy_sigma0"]
        return kw


def dueling_live_mask(n_hidden: int, n_heads: int, n_actions: int, width: int = 1) -> np.ndarray:
    """Which entries of the dueling head's Flax kernel (F, R) are weights (True) and which structural zeros (include/isdqn_hip.h,
    isdqn_net_config::dueling): column ((h * (A + 1)) + c) * width + j is a value column for c = A and reads the hidden units
    [0, F / 2); the advantage columns c < A read [F / 2, F)."""
    F2 = n_hidden // 2
    c = (np.arange(n_heads * (n_actions + 1) * width) // width) % (n_actions + 1)
    first_half = np.arange(n_hidden)[:, None] < F2
    return np.where((c == n_actions)[None, :], first_half, ~first_half)


class QNetEngine:
    """One Q-network (slimdqn/networks/architectures/dqn.py DQNNet + isdqn.py head view) on one GPU."""

    def __init__(
        self,
        observation_dim: Sequence[int],
        n_actions: int,
        n_heads: int,
        features: Sequence[int],
        architecture_type: str,
        layer_norm: bool,
        batch_size: int,
        gamma_n: float = 0.99,
        learning_rate: float = 1e-3,
        adam_eps: float = 1e-8,
        precision: str = "bf16x3",
        device: str | None = None,
        huber_delta: float = 0.0,
        batch_norm: bool = False,
        n_bins: int = 0,
        min_value: float = -100.0,
        max_value: float = 100.0,
        sigma: float = 3.0,
        double_q: bool = False,
        munchausen_tau: float = 0.0,
        munchausen_alpha: float = 0.9,
        munchausen_clip: float = -1.0,
        n_quantiles: int = 0,
        categorical: bool = False,
        dueling: bool = False,
        max_grad_norm: float = 0.0,
        noisy: bool = False,
        noisy_sigma0: float = 0.5,
        noisy_seed: int = 0,
    ):
        """``noisy``: every Dense layer is a factorised noisy layer (include/isdqn_hip.h, isdqn_noisy_layout).  The engine then owns
        ``sigma``, ``sigma_m``, ``sigma_v``, ``noise``, ``eff``, ``grad`` and ``noise_count``; ``init_params`` writes sigma =
        noisy_sigma0 / sqrt(in_f) on the real elements of the Dense kernels and biases (in_f: the true fan-in; the live fan-in F / 2 on
        a dueling head) and 0 elsewhere.  ``mu`` keeps the existing initialiser -- a deviation from the paper, which draws mu uniformly
        from +-1 / sqrt(in_f).  Without ``noisy`` nothing new is allocated and every call takes exactly the code path it had.
        The other option keywords: NetOptions."""
        options = self.options = NetOptions.pick(locals())
        check_noisy(noisy, architecture_type, batch_norm, max_grad_norm)
        options.check(architecture_type, features, batch_norm)
        _hip.require_gpu()
        self.lib = _hip.lib()
        self.device = _hip.resolve_device(device)
        _hip.bind_device(self.device)
        cfg = _hip.NetConfig()
        if architecture_type == "cnn":
            cfg.arch = _hip.ARCH_CNN
            cfg.obs_h, cfg.obs_w, cfg.obs_c = (int(d) for d in observation_dim)
        elif architecture_type == "impala":  # architectures/dqn.py:7-36, 75-88: three Stacks on the generic engine (csrc/impala.h)
            cfg.arch = _hip.ARCH_IMPALA
            cfg.obs_h, cfg.obs_w, cfg.obs_c = (int(d) for d in observation_dim)
        elif architecture_type == "fc":
            cfg.arch = _hip.ARCH_FC
            cfg.obs_h = cfg.obs_w = 1
            cfg.obs_c = int(np.prod(observation_dim))
        else:
            raise NotImplementedError(f"architecture_type={architecture_type!r}: 'cnn', 'impala' or 'fc'")
        feats = [int(f) for f in features]
        if len(feats) > _hip.MAX_FEATURES:
            raise ValueError("too many features")
        cfg.n_features = len(feats)
        for i, f in enumerate(feats):
            cfg.features[i] = f
        cfg.n_actions = int(n_actions)
        cfg.n_heads = int(n_heads)
        cfg.layer_norm = 1 if layer_norm else 0
        cfg.batch_size = int(batch_size)
        cfg.precision = {"bf16x3": _hip.PRECISION_BF16X3, "bf16": _hip.PRECISION_BF16}[precision]
        cfg.gamma_n = float(gamma_n)
        cfg.learning_rate = float(learning_rate)
        cfg.adam_b1, cfg.adam_b2 = 0.9, 0.999
        cfg.adam_eps = float(adam_eps)
        cfg.batch_norm = 1 if batch_norm else 0  # architectures/dqn.py:52-53, 59-60, 66-67, 73-74, 100-101 (csrc/batchnorm.h)
        self.batch_norm = bool(batch_norm)
        options.fill(cfg)
        for name in ("max_grad_norm", "n_bins", "categorical", "n_quantiles", "dueling", "double_q", "munchausen_tau", "munchausen_alpha",
                     "munchausen_clip"):  # (plain attributes of the engine; its ``sigma`` is the noisy tensor, not the histogram's std)
            setattr(self, name, getattr(options, name))
        self.cfg = cfg
        self.features = feats
        self.architecture_type = architecture_type
        self.observation_dim = tuple(int(d) for d in observation_dim)
        self.n_actions, self.n_heads = int(n_actions), int(n_heads)
        self.batch_size = int(batch_size)
        self.precision = precision

        n = ctypes.c_int64()
        cnt = ctypes.c_int32()
        _hip.check(self.lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt)))
        infos = (_hip.TensorInfo * cnt.value)()
        _hip.check(self.lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)))
        self.n_param_floats = int(n.value)
        self.infos = list(infos)
        wb = ctypes.c_int64()
        _hip.check(self.lib.isdqn_net_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)))
        self.workspace_bytes = int(wb.value)
        with torch.cuda.device(self.device):
            # zero-initialised once: padded rows/columns of gradient slabs are never written and must read as 0
            self.workspace = torch.zeros(self.workspace_bytes // 4, dtype=torch.float32, device=self.device)
            self.params = torch.zeros(self.n_param_floats, dtype=torch.float32, device=self.device)
            self.adam_m = torch.zeros_like(self.params)
            self.adam_v = torch.zeros_like(self.params)
            self.adam_count = torch.zeros(1, dtype=torch.int32, device=self.device)
            K = self.n_regressed = self.n_heads - 1 if self.n_heads >= 2 else 1  # a single head (DQN / TF-DQN) regresses itself
            self.losses = torch.zeros(K, dtype=torch.float32, device=self.device)
            self.losses_accum = torch.zeros(K, dtype=torch.float32, device=self.device)
            self.q_values = torch.zeros(batch_size, K, dtype=torch.float32, device=self.device)
            self.targets = torch.zeros(batch_size, K, dtype=torch.float32, device=self.device)
            self.priorities = torch.zeros(batch_size, dtype=torch.float64, device=self.device)
            self.action_out = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.noisy = bool(noisy)
        if self.noisy:
            self.noisy_sigma0, self.noisy_seed = float(noisy_sigma0), int(noisy_seed) & (2**64 - 1)
            nl, total = ctypes.c_int32(), ctypes.c_int64()
            offs, wi, wo = (ctypes.c_int64 * 16)(), (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)()
            _hip.check(self.lib.isdqn_noisy_layout(ctypes.byref(cfg), ctypes.byref(nl), offs, wi, wo, 16, ctypes.byref(total)), "isdqn_noisy_layout")
            self.noise_layout = [(int(offs[i]), int(wi[i]), int(wo[i])) for i in range(nl.value)]  # (offset of ein, in_p, out_p) per Dense
            with torch.cuda.device(self.device):
                self.sigma = torch.zeros_like(self.params)
                self.sigma_m = torch.zeros_like(self.params)
                self.sigma_v = torch.zeros_like(self.params)
                self.eff = torch.zeros_like(self.params)
                self.grad = torch.zeros_like(self.params)
                self.noise = torch.zeros(int(total.value), dtype=torch.float32, device=self.device)
                self.noise_count = torch.zeros(1, dtype=torch.int64, device=self.device)
                # the DQN form's second draw (stream_id = 1) and the target's composed parameters
                self.noise_target = torch.zeros_like(self.noise)
                self.eff_target = torch.zeros_like(self.params)
            self._noise_zero = True  # the buffers above: zero noise, the mean network

    def copy_state_from(self, old: "QNetEngine") -> None:
        """Take over the training state of ``old``, an engine of the same network and options at another batch size (same parameter
        layout, another workspace): parameters, Adam's moments and count, the loss accumulator, and what the options own -- noisy: sigma,
        its moments and the draw counter; clipping: the two gradient-norm accumulators.  Copies on the current stream."""
        self.params.copy_(old.params)
        self.adam_m.copy_(old.adam_m)
        self.adam_v.copy_(old.adam_v)
        self.adam_count.copy_(old.adam_count)
        self.losses_accum.copy_(old.losses_accum)
        if self.noisy:
            for name in ("sigma", "sigma_m", "sigma_v", "noise_count"):
                getattr(self, name).copy_(getattr(old, name))
        if self.max_grad_norm > 0.0:
            self.grad_clip[2:4].copy_(old.grad_clip[2:4])

    # ------------------------------------------------------------------ noisy Dense layers
    noisy = False  # (class default: an engine built without the option, or a host-side stand-in for the layout)
    resample_on_learn = False  # True (the agents set it): every learn call draws new noise first, so that a captured step does too

    def _dense_leaf(self, info) -> bool:
        return info.kind == 1 or (info.kind == 2 and info.name.decode().split("/")[-2].startswith("Dense_"))

    def _sigma_tree(self) -> Dict[str, Dict[str, np.ndarray]]:
        """sigma0 / sqrt(in_f) on the real elements of every Dense kernel and bias, in Flax shapes."""
        head = self.head_kernel_info()
        fan_in, tree = {}, {}
        for info in self.infos:
            if info.kind == 1:
                fan_in[info.name.decode().rsplit("/", 1)[0]] = int(info.flax_shape[0]) // (2 if self.dueling and info.layer == head.layer else 1)
        for info in self.infos:
            if not self._dense_leaf(info):
                continue
            mod, leaf = info.name.decode().rsplit("/", 1)
            v = np.full(tuple(info.flax_shape[: info.ndim]), self.noisy_sigma0 / math.sqrt(fan_in[mod]), np.float32)
            if self.dueling and info.kind == 1 and info.layer == head.layer:
                v = np.where(self.dueling_live_mask(), v, np.float32(0))
            tree.setdefault(mod, {})["sigma_" + leaf] = v
        return tree

    def _import_sigma(self, tree, target: torch.Tensor) -> None:
        flat = np.zeros(self.n_param_floats, np.float32)
        for info in self.infos:
            if self._dense_leaf(info):
                mod, leaf = info.name.decode().rsplit("/", 1)
                flat[info.offset : info.offset + info.size] = self._to_internal(info, tree[mod]["sigma_" + leaf])
        target.copy_(torch.from_numpy(flat))

    def export_sigma(self, source: torch.Tensor | None = None) -> Dict[str, Dict[str, np.ndarray]]:
        """{"Dense_i": {"sigma_kernel", "sigma_bias"}} in Flax shapes from ``sigma`` (or another buffer of its layout)."""
        flat = (self.sigma if source is None else source).detach().cpu().numpy()
        out: Dict[str, Dict[str, np.ndarray]] = {}
        for info in self.infos:
            if self._dense_leaf(info):
                mod, leaf = info.name.decode().rsplit("/", 1)
                out.setdefault(mod, {})["sigma_" + leaf] = self._from_internal(info, flat[info.offset : info.offset + info.size])
        return out

    def resample_noise(self, stream_id: int = 0, noise: torch.Tensor | None = None) -> None:
        """A new factorised draw into ``noise`` on the current stream; the device counter advances by one (nothing is read back)."""
        _hip.check(self.lib.isdqn_noisy_sample(ctypes.byref(self.cfg), self.noisy_seed, int(stream_id), _hip.ptr(self.noise_count),
                                               _hip.ptr(self.noise if noise is None else noise), _hip.stream_ptr(self.device)), "isdqn_noisy_sample")
        if noise is None:
            self._noise_zero = False

    def zero_noise(self) -> None:
        """The mean (evaluation) network: compose then returns mu bit for bit; the DQN form's target draw is zero too until the next resample."""
        self.noise.zero_()
        self.noise_target.zero_()
        self._noise_zero = True

    def compose(self, mu: torch.Tensor | None = None, sigma: torch.Tensor | None = None, noise: torch.Tensor | None = None,
                eff: torch.Tensor | None = None, mirror: bool = True) -> torch.Tensor:
        """eff = mu + sigma * noise on the Dense layers (defaults: the engine's own buffers); ``mirror``: also the workspace's weight
        mirror of eff, so that the next call on eff may trust it."""
        eff = self.eff if eff is None else eff
        _hip.check(self.lib.isdqn_noisy_compose(ctypes.byref(self.cfg), _hip.ptr(self.params if mu is None else mu),
                                                _hip.ptr(self.sigma if sigma is None else sigma), _hip.ptr(self.noise if noise is None else noise),
                                                _hip.ptr(eff), _hip.ptr(self.workspace) if mirror else 0, _hip.stream_ptr(self.device)),
                   "isdqn_noisy_compose")
        if mirror:
            self._mirror_version = None  # (the mirror now holds eff, not params)
        return eff

    def _acting_params(self, params):
        """What a forward / loss / gradient-only call reads: the caller's buffer, or -- noisy, on the engine's own parameters -- eff after a
        compose with the current noise."""
        if params is None and self.noisy:
            return self.compose()
        return self.params if params is None else params

    def _noisy_learn(self, batch: _hip.Batch, eff_target: torch.Tensor | None) -> torch.Tensor:
        _hip.check(
            self.lib.isdqn_noisy_learn_on_batch(
                ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(self.sigma), _hip.ptr(self.adam_m), _hip.ptr(self.adam_v),
                _hip.ptr(self.sigma_m), _hip.ptr(self.sigma_v), _hip.ptr(self.adam_count), _hip.ptr(self.noise), _hip.ptr(self.eff),
                _hip.ptr(eff_target), _hip.ptr(self.grad), ctypes.byref(batch), _hip.ptr(self.losses), _hip.ptr(self.losses_accum),
                _hip.ptr(self.q_values), _hip.ptr(self.targets), _hip.ptr(self.priorities), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_noisy_learn_on_batch",
        )
        self._mirror_version = None  # (the mirror holds eff of this step)
        return self.losses

    # ------------------------------------------------------------------ parameter layout
    def _first_dense_after_conv(self, info) -> bool:
        # (the first Dense behind the torso: layer 3 of the cnn plan, layer 1 behind the impala pseudo-layer)
        return info.kind == 1 and ((self.architecture_type == "cnn" and info.layer == 3) or (self.architecture_type == "impala" and info.layer == 1))

    def _to_internal(self, info, arr: np.ndarray) -> np.ndarray:
        arr = np.asarray(arr, dtype=np.float32)
        d = list(info.dims)
        if info.kind == 0:
            k1, k2, cin, cout = arr.shape
            if self.architecture_type == "cnn" and info.layer == 0 and not self.batch_norm:
                out = np.zeros((d[0], cin, k1 * k2), np.float32)  # [out][plane][ky*8+kx]
                out[:cout] = arr.transpose(3, 2, 0, 1).reshape(cout, cin, k1 * k2)
            else:
                out = np.zeros((d[0], d[1], d[2]), np.float32)  # [out][tap][in_p]
                out[:cout, :, :cin] = arr.transpose(3, 0, 1, 2).reshape(cout, k1 * k2, cin)
            return out.reshape(-1)
        if info.kind == 1:
            in_f, out_f = arr.shape
            out = np.zeros((d[0], d[1]), np.float32)  # [out_p][in_p]
            if self._first_dense_after_conv(info):
                c = self.features[2]
                c_p = _round_up(c, 8)
                npix = in_f // c
                tmp = np.zeros((out_f, npix, c_p), np.float32)
                tmp[:, :, :c] = arr.T.reshape(out_f, npix, c)
                out[:out_f] = tmp.reshape(out_f, npix * c_p)
            else:
                out[:out_f, :in_f] = arr.T
            return out.reshape(-1)
        if info.kind >= 5:  # BatchNorm_i scale / bias / mean / var: dims = [groups, P, C, C padded]
            out = np.zeros(info.size, np.float32)
            if info.ndim == 2:  # spatial site: one value per pixel position, flax shape (H, W)
                out[: d[0]] = arr.reshape(-1)
            else:  # feature site: flax column p * C + c -> internal column p * Cp + c
                out[: d[0]].reshape(d[1], d[3])[:, : d[2]] = arr.reshape(d[1], d[2])
            return out
        out = np.zeros(d[0], np.float32)
        out[: arr.shape[0]] = arr
        return out

    def _from_internal(self, info, flat: np.ndarray) -> np.ndarray:
        d = list(info.dims)
        shape = tuple(info.flax_shape[: info.ndim])
        if info.kind == 0:
            k1, k2, cin, cout = shape
            if self.architecture_type == "cnn" and info.layer == 0 and not self.batch_norm:
                w = flat.reshape(d[0], cin, k1, k2)[:cout]
                return np.ascontiguousarray(w.transpose(2, 3, 1, 0))
            w = flat.reshape(d[0], k1, k2, d[2])[:cout, :, :, :cin]
            return np.ascontiguousarray(w.transpose(1, 2, 3, 0))
        if info.kind == 1:
            in_f, out_f = shape
            w = flat.reshape(d[0], d[1])[:out_f]
            if self._first_dense_after_conv(info):
                c = self.features[2]
                c_p = _round_up(c, 8)
                npix = in_f // c
                w = w.reshape(out_f, npix, c_p)[:, :, :c].reshape(out_f, in_f)
            else:
                w = w[:, :in_f]
            return np.ascontiguousarray(w.T)
        if info.kind >= 5:
            if info.ndim == 2:
                return flat[: d[0]].reshape(shape).copy()
            return np.ascontiguousarray(flat[: d[0]].reshape(d[1], d[3])[:, : d[2]]).reshape(shape)
        return flat[: shape[0]].copy()

    def head_kernel_info(self):
        """The tensor table's entry of the last Dense's kernel."""
        return max((i for i in self.infos if i.kind == 1), key=lambda i: i.layer)

    def dueling_live_mask(self) -> np.ndarray:
        """Boolean (F, R) over the dueling head's Flax kernel: True where a weight lives, False on the structural zeros."""
        assert self.dueling
        return dueling_live_mask(self.features[-1], self.n_heads, self.n_actions, max(self.n_bins, self.n_quantiles, 1))

    def import_flax(self, params: Dict[str, Dict[str, np.ndarray]], target: torch.Tensor | None = None, batch_stats=None) -> None:
        """Load a reference-layout pytree ({"Conv_0": {"kernel": HWIO, "bias"}, "LayerNorm_0": ...}).  BatchNorm networks: the
        running averages come from ``batch_stats`` ({"BatchNorm_0": {"mean", "var"}}, Flax's second collection); without it
        they keep Flax's initial values (mean 0, var 1).  Dueling heads: a non-zero structural zero of the head kernel is refused
        (ValueError) before anything is written."""
        if getattr(self, "dueling", False):  # (a host-side stand-in for the layout has no such attribute: off)
            head = self.head_kernel_info()
            mod, leaf = head.name.decode().rsplit("/", 1)
            live = self.dueling_live_mask()
            if np.any(np.asarray(params[mod][leaf])[~live] != 0):
                raise ValueError(f"{mod}/{leaf}: a structural zero of the dueling head kernel is not zero (value columns read the hidden units "
                                 "[0, F / 2), advantage columns [F / 2, F))")
            params = {**params, mod: {**params[mod], leaf: np.where(live, params[mod][leaf], 0)}}  # (a -0.0 becomes the +0.0f the library keeps)
        flat = np.zeros(self.n_param_floats, np.float32)
        for info in self.infos:
            mod, leaf = info.name.decode().rsplit("/", 1)  # (impala: "Stack_0/Conv_1" / "kernel")
            if info.kind >= 7:
                shape = tuple(info.flax_shape[: info.ndim])
                src = batch_stats[mod][leaf] if batch_stats is not None else (np.zeros(shape, np.float32) if info.kind == 7 else np.ones(shape, np.float32))
                v = self._to_internal(info, src)
            else:
                v = self._to_internal(info, params[mod][leaf])
            assert v.size == info.size, (info.name, v.size, info.size)
            flat[info.offset : info.offset + info.size] = v
        (self.params if target is None else target).copy_(torch.from_numpy(flat))
        # noisy engines: "Dense_i/sigma_kernel" and "Dense_i/sigma_bias" next to kernel / bias load sigma (a tree without them leaves it)
        if getattr(self, "noisy", False) and target is None and any("sigma_kernel" in leaves for leaves in params.values()):
            self._import_sigma(params, self.sigma)

    def export_flax(self, source: torch.Tensor | None = None) -> Dict[str, Dict[str, np.ndarray]]:
        flat = (self.params if source is None else source).detach().cpu().numpy()
        out: Dict[str, Dict[str, np.ndarray]] = {}
        for info in self.infos:
            if info.kind >= 7:  # (running averages: export_batch_stats)
                continue
            mod, leaf = info.name.decode().rsplit("/", 1)  # (impala: "Stack_0/Conv_1" / "kernel")
            out.setdefault(mod, {})[leaf] = self._from_internal(info, flat[info.offset : info.offset + info.size])
        if getattr(self, "noisy", False) and source is None:  # (the engine's own parameters: mu with the sigma leaves beside it)
            for mod, leaves in self.export_sigma().items():
                out[mod].update(leaves)
        return out

    def export_batch_stats(self, source: torch.Tensor | None = None) -> Dict[str, Dict[str, np.ndarray]]:
        """Flax's ``batch_stats`` collection of a BatchNorm network: {"BatchNorm_i": {"mean", "var"}} (empty without BatchNorm)."""
        flat = (self.params if source is None else source).detach().cpu().numpy()
        out: Dict[str, Dict[str, np.ndarray]] = {}
        for info in self.infos:
            if info.kind >= 7:
                mod, leaf = info.name.decode().rsplit("/", 1)
                out.setdefault(mod, {})[leaf] = self._from_internal(info, flat[info.offset : info.offset + info.size])
        return out

    def init_params(self, seed: int) -> None:
        """Flax defaults (dqn.py:49, 90): xavier_uniform for cnn, lecun_normal for fc; biases 0, LN scale 1.
        Draws come from numpy PCG64 (JAX threefry streams are not reproducible offline)."""
        self.import_flax(self._init_tree(seed))
        if getattr(self, "noisy", False):
            self.init_sigma()

    def init_sigma(self) -> None:
        """sigma = noisy_sigma0 / sqrt(in_f) on the real elements of the Dense kernels and biases, +0 everywhere else."""
        self._import_sigma(self._sigma_tree(), self.sigma)

    def fresh_params(self, seed) -> torch.Tensor:
        """A new device tensor in the internal layout holding what ``init_params(seed)`` would leave in ``params`` (the engine's own
        buffers are not touched): the source of re-initialised weights for ``redo``."""
        t = torch.empty_like(self.params)
        self.import_flax(self._init_tree(seed), target=t)
        return t

    def _init_tree(self, seed) -> Dict[str, Dict[str, np.ndarray]]:
        rng = np.random.default_rng(seed)
        params: Dict[str, Dict[str, np.ndarray]] = {}
        for info in self.infos:
            mod, leaf = info.name.decode().rsplit("/", 1)  # (impala: "Stack_0/Conv_1" / "kernel")
            shape = tuple(info.flax_shape[: info.ndim])
            if info.kind in (0, 1):
                if info.kind == 0:
                    rf = shape[0] * shape[1]
                    fan_in, fan_out = rf * shape[2], rf * shape[3]
                else:
                    fan_in, fan_out = shape
                duel_head = getattr(self, "dueling", False) and info.kind == 1 and info.layer == self.head_kernel_info().layer
                if duel_head:  # the live entries of a column are one F / 2-wide stream: drawn at that fan-in, scattered below
                    full_shape, shape = shape, (shape[0] // 2, shape[1])
                    fan_in = shape[0]
                xavier = self.architecture_type == "cnn" or (self.architecture_type == "impala" and (info.kind == 1 or mod.endswith("/Conv_0")))
                if xavier:  # (impala: kernel_init is passed to each Stack's first conv and to the Dense layers only, dqn.py:17-21, 96)
                    lim = math.sqrt(6.0 / (fan_in + fan_out))
                    w = rng.uniform(-lim, lim, size=shape)
                else:
                    std = math.sqrt(1.0 / fan_in) / 0.87962566103423978
                    w = np.empty(int(np.prod(shape)))
                    filled = 0
                    while filled < w.size:
                        draw = rng.standard_normal(w.size - filled)
                        draw = draw[np.abs(draw) <= 2.0]
                        w[filled : filled + draw.size] = draw
                        filled += draw.size
                    w = w.reshape(shape) * std
                if duel_head:
                    live = self.dueling_live_mask()
                    full = np.zeros(full_shape)
                    full.T[live.T] = w.T.reshape(-1)  # column by column: every column has exactly F / 2 live rows, in ascending order
                    w = full
                params.setdefault(mod, {})[leaf] = w.astype(np.float32)
            elif info.kind in (3, 5):  # LayerNorm / BatchNorm scale
                params.setdefault(mod, {})[leaf] = np.ones(shape, np.float32)
            elif info.kind >= 7:  # running averages: import_flax's defaults (mean 0, var 1)
                continue
            else:
                params.setdefault(mod, {})[leaf] = np.zeros(shape, np.float32)
        return params

    # ------------------------------------------------------------------ workspace regions (tests / debugging)
    def region(self, name: str) -> torch.Tensor:
        off, size = ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self.lib.isdqn_net_workspace_region(ctypes.byref(self.cfg), name.encode(), ctypes.byref(off), ctypes.byref(size)))
        return self.workspace[off.value // 4 : (off.value + size.value) // 4]

    @property
    def grad_clip(self) -> torch.Tensor:
        """View of the workspace region "grad_clip" (max_grad_norm > 0 only): [0] the gradient norm of the last learn / gradient-only
        step, [1] the factor its gradient was multiplied by, [2] the running sum of the norms of the update steps, [3] the running count
        of update steps that were clipped.  The caller zeroes [2] and [3] (include/isdqn_hip.h, isdqn_net_config::max_grad_norm)."""
        return self.region("grad_clip")[:4]

    def set_max_grad_norm(self, max_grad_norm: float) -> None:
        """Another threshold for the following steps of an engine built with clipping on (the workspace does not depend on the value:
        any threshold > 0 has the same regions).  A step that is already captured keeps the threshold it was captured with."""
        c = float(max_grad_norm)
        if not (c > 0.0 and self.max_grad_norm > 0.0):
            raise ValueError("set_max_grad_norm: the engine must have been built with max_grad_norm > 0 and the new threshold must be > 0")
        self.cfg.max_grad_norm = c
        self.max_grad_norm = c
        self.options = dataclasses.replace(self.options, max_grad_norm=c)

    weight_decay = 0.0  # AdamW's decoupled weight decay of the following learn steps (set_weight_decay); 0: plain Adam
    decay_kinds = 0     # bit k: tensors of TensorInfo.kind k decay
    _captured = None    # weak set of the captured updates whose batches this engine made (slimdqn/_graph.py)

    def _drop_captured(self) -> None:
        """Destroy every captured update of this engine: what its batches carry changed, so each captures again at its next run."""
        for g in list(self._captured or ()):
            g.destroy()

    def set_weight_decay(self, weight_decay: float, all_kinds: bool = False) -> None:
        """AdamW (Loshchilov & Hutter 2019; optax.adamw, torch.optim.AdamW) for the following learn steps of this engine: every element
        of a decaying tensor also loses ``learning_rate * weight_decay`` times its value before the step (include/isdqn_hip.h,
        isdqn_batch_decay: the definition, three float32 roundings).  The conv and dense kernels decay -- the usual mask --, with
        ``all_kinds`` the biases and the LayerNorm / BatchNorm scales and biases too; running statistics never.  0 is off: the batches
        and the bits of an engine that never heard of it.  The decay travels in every batch ``make_batch`` builds from here on; a step
        that is already captured was captured with the old one, so every captured update of this engine is dropped (it captures again
        at its next run).  Loss-only and gradient-only calls ignore it; noisy engines refuse it (ValueError)."""
        wd = _optimizer.check_weight_decay(weight_decay, noisy=self.noisy)
        self.weight_decay = wd
        self.decay_kinds = _optimizer.decay_kinds(all_kinds) if wd > 0.0 else 0
        self._drop_captured()

    cql_alpha = 0.0  # weight of the conservative term of the following loss / gradient / learn calls (set_conservative); 0: none

    def set_conservative(self, alpha: float) -> None:
        """CQL(H) (Kumar et al. 2020) for the following calls of this engine: every loss, gradient and learn call adds
        ``alpha * (logsumexp_a Q(s, a) - Q(s, a_b))`` per regressed pair to the configured loss, on the device (include/isdqn_hip.h,
        isdqn_batch_conservative: the definition).  q_values, targets and priorities stay those of the configured loss.  0 is off: the
        batches and the bits of an engine that never heard of it.  The weight travels in every batch ``make_batch`` builds from here on;
        every captured update of this engine is dropped and captures again at its next run, as ``set_weight_decay`` does.  Every
        torso, head type, target form and the noisy learn step take it; a learn step on scalar heads leaves the head chain.  Refused
        with alpha > 0 on an engine with a mixture (``set_mixture``): ValueError."""
        alpha = _conservative.check_cql_alpha(alpha)
        if alpha > 0.0 and self.mix_alpha is not None:  # (the library refuses the two together at every call: refuse them here)
            raise ValueError(_mixture.REM_CQL_REFUSED)
        self.cql_alpha = alpha
        self._drop_captured()

    mix_alpha = None  # float32 [n_heads]: the mixture weights of the following loss / gradient / learn calls (set_mixture); None: none
    mix_count = None  # int64 [1]: draws so far (selects the next draw; mixture_draw advances it on the device)

    def set_mixture(self, seed: int) -> None:
        """REM (Agarwal et al. 2020) for the following calls of this engine: every loss, gradient and learn call regresses the mixture
        ``sum_h alpha_h Q_h`` of all ``n_heads`` heads on the same mixture of the value network and spreads the one TD error over the
        heads (include/isdqn_hip.h, isdqn_batch_mixture: the definition).  Allocates ``mix_alpha`` -- uniform, 1 / n_heads, until the
        first draw -- and the draw count; ``mixture_draw`` draws the next weights.  The weights travel in every batch ``make_batch``
        builds from here on; every captured update of this engine is dropped, as ``set_conservative`` does.  Noisy engines, histogram
        and quantile heads, Munchausen targets and a conservative term are refused (ValueError)."""
        _mixture.check_rem_heads(self.n_heads, noisy=self.noisy, n_bins=self.n_bins, n_quantiles=self.n_quantiles,
                                 munchausen_tau=self.munchausen_tau, cql_alpha=self.cql_alpha)
        self.mix_seed = _mixture.mixture_seed(seed)
        with torch.cuda.device(self.device):
            self.mix_alpha = torch.full((self.n_heads,), 1.0 / self.n_heads, dtype=torch.float32, device=self.device)
            self.mix_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._drop_captured()

    def mixture_draw(self) -> None:
        """The next mixture weights into ``mix_alpha`` on the current stream; the device count advances by one (nothing is read back)."""
        _hip.check(self.lib.isdqn_mixture_draw(self.n_heads, self.mix_seed, _hip.ptr(self.mix_count), _hip.ptr(self.mix_alpha),
                                               _hip.stream_ptr(self.device)), "isdqn_mixture_draw")

    # ------------------------------------------------------------------ C-ABI calls
    def make_batch(self, *, frames=None, frame_stride=0, frame_ids=None, state=None, next_state=None, action=None, reward=None, terminal=None,
                   mirror_current: bool = False, priorities_ready: torch.cuda.Event | None = None, loss_weights=None, discount=None) -> _hip.Batch:
        """``mirror_current``: promise that the previous call on this engine was learn_on_batch and nothing wrote the
        parameters since (include/isdqn_hip.h, ISDQN_BATCH_MIRROR_CURRENT) -- only the captured multi-step graphs do.
        ``priorities_ready``: an event (already recorded once, so that its handle exists) the learn call records on the
        caller's stream as soon as q_values / targets / priorities are final.
        ``loss_weights``: float32 [B] device tensor of importance-sampling weights (prioritized replay), None = weight 1.
        ``discount``: float32 [B] device tensor of per-transition discounts that stand in ``gamma_n``'s place (a horizon-window replay's
        ``DeviceBatch.discount``), None = ``gamma_n`` everywhere."""
        if loss_weights is not None:
            assert loss_weights.dtype == torch.float32 and loss_weights.numel() == self.batch_size and loss_weights.is_contiguous()
        if discount is not None:
            assert discount.dtype == torch.float32 and discount.numel() == self.batch_size and discount.is_contiguous()
        b = _hip.Batch() if discount is None else _hip.BatchDiscount()  # (isdqn_batch_discount: the flag announces the pointer behind)
        b.flags = (_hip.BATCH_MIRROR_CURRENT if mirror_current else 0) | (0 if discount is None else _hip.BATCH_DISCOUNT)
        if self.weight_decay > 0.0:  # (isdqn_batch_decay: the batch, its discount slot, then the decay; off: the structs above, as ever)
            b, flags = _hip.BatchDecay(), b.flags
            b.flags = flags | _hip.BATCH_WEIGHT_DECAY
            b.weight_decay, b.decay_kinds = self.weight_decay, self.decay_kinds
        if self.cql_alpha > 0.0:  # (isdqn_batch_conservative: the structs above, then the term's weight; the decay slot is read with its own flag)
            inner, b = b, _hip.BatchConservative()
            b.flags = inner.flags | _hip.BATCH_CONSERVATIVE
            if self.weight_decay > 0.0:
                b.weight_decay, b.decay_kinds = inner.weight_decay, inner.decay_kinds
            b.cql_alpha = self.cql_alpha
        if self.mix_alpha is not None:  # (isdqn_batch_mixture: the structs above, then the weights; the inner slots are read with their own flags)
            inner, b = b, _hip.BatchMixture()
            b.flags = inner.flags | _hip.BATCH_MIXTURE
            if self.weight_decay > 0.0:
                b.weight_decay, b.decay_kinds = inner.weight_decay, inner.decay_kinds
            if self.cql_alpha > 0.0:
                b.cql_alpha = inner.cql_alpha
            b.alpha, b.n_mix = _hip.ptr(self.mix_alpha), self.n_heads
        b.priorities_ready = None if priorities_ready is None else int(priorities_ready.cuda_event)
        b.B = self.batch_size
        b.frames = _hip.ptr(frames)
        b.frame_stride = int(frame_stride)
        b.frame_ids = _hip.ptr(frame_ids)
        b.state = _hip.ptr(state)
        b.next_state = _hip.ptr(next_state)
        b.action = _hip.ptr(action)
        b.reward = _hip.ptr(reward)
        b.terminal = _hip.ptr(terminal)
        b.loss_weights = _hip.ptr(loss_weights)
        if discount is not None:
            b.discount = _hip.ptr(discount)
        # keep the tensors alive for the duration of the asynchronous call
        b._keep = (frames, frame_ids, state, next_state, action, reward, terminal, priorities_ready, loss_weights, discount)
        return b

    def forward(self, *, frames=None, frame_stride=0, frame_ids=None, obs=None, n_rows: int, params=None) -> torch.Tensor:
        q = torch.empty(n_rows, self.n_heads * self.n_actions, dtype=torch.float32, device=self.device)
        p = self._acting_params(params)
        _hip.check(
            self.lib.isdqn_net_forward(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(frames), int(frame_stride), _hip.ptr(frame_ids),
                _hip.ptr(obs), int(n_rows), _hip.ptr(q), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_forward",
        )
        self._mirror_holds(params)
        return q

    def learn_on_batch(self, batch: _hip.Batch, grad_out: torch.Tensor | None = None) -> torch.Tensor:
        """One gradient step in place; returns the device tensor of per-head losses (no sync).  Noisy engines: the noisy learn step
        on the current ``noise`` (the caller resamples); ``grad_out`` then receives a copy of the step's reduced gradient."""
        if self.noisy:
            if self.resample_on_learn:
                self.resample_noise()
            self._noisy_learn(batch, None)
            if grad_out is not None:
                grad_out.copy_(self.grad)
            return self.losses
        args = [
            ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(self.adam_m), _hip.ptr(self.adam_v),
            _hip.ptr(self.adam_count), ctypes.byref(batch), _hip.ptr(self.losses), _hip.ptr(self.losses_accum), _hip.ptr(self.q_values),
            _hip.ptr(self.targets), _hip.ptr(self.priorities), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
        ]
        if grad_out is None:
            rc = self.lib.isdqn_net_learn_on_batch(*args)
        else:
            rc = self.lib.isdqn_net_learn_on_batch_debug(*args, _hip.ptr(grad_out))
        _hip.check(rc, "isdqn_net_learn_on_batch")
        self._mirror_made_current()  # Adam wrote the updated weights in both forms
        return self.losses

    def grad_on_batch(self, batch: _hip.Batch, grad_out: torch.Tensor, target_params: torch.Tensor | None = None, online_head: int = 0,
                      target_head: int = 0, n_pairs: int = 0, params=None) -> torch.Tensor:
        """Gradient of a TD loss into ``grad_out`` (internal layout), nothing updated (analysisdqn.py:156-219): the
        configuration's own loss (n_pairs = 0) or online heads online_head + k on target heads target_head + k; next states
        through ``target_params`` when given.  Returns the device tensor of the loss per pair (the first n_pairs / K entries)."""
        p = self._acting_params(params)
        _hip.check(
            self.lib.isdqn_net_grad_on_batch(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(target_params), ctypes.byref(batch), int(online_head), int(target_head),
                int(n_pairs), _hip.ptr(grad_out), _hip.ptr(self.losses), _hip.ptr(self.q_values), _hip.ptr(self.targets),
                _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_grad_on_batch",
        )
        self._mirror_holds(params)
        return self.losses

    def learn_on_batch_target(self, batch: _hip.Batch, target_params: torch.Tensor, target_sigma: torch.Tensor | None = None) -> torch.Tensor:
        """DQN step (dqn.py:59-72): next states through `target_params`, in-place update of the online parameters.  Noisy engines:
        the target is composed from ``target_params``, ``target_sigma`` (default: the online sigma) and a draw of its own (stream_id = 1;
        zero while the engine's noise is zeroed)."""
        if self.noisy:
            if self.resample_on_learn:
                self.resample_noise()
            if not self._noise_zero:
                self.resample_noise(1, self.noise_target)
            self.compose(target_params, target_sigma, self.noise_target, self.eff_target, mirror=False)
            return self._noisy_learn(batch, self.eff_target)
        _hip.check(
            self.lib.isdqn_net_learn_on_batch_target(
                ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(target_params), _hip.ptr(self.adam_m), _hip.ptr(self.adam_v),
                _hip.ptr(self.adam_count), ctypes.byref(batch), _hip.ptr(self.losses), _hip.ptr(self.losses_accum),
                _hip.ptr(self.q_values), _hip.ptr(self.targets), _hip.ptr(self.priorities), _hip.ptr(self.workspace),
                _hip.stream_ptr(self.device),
            ),
            "isdqn_net_learn_on_batch_target",
        )
        self._mirror_made_current()
        return self.losses

    def loss_on_batch_target(self, batch: _hip.Batch, target_params: torch.Tensor, params=None) -> torch.Tensor:
        p = self._acting_params(params)
        _hip.check(
            self.lib.isdqn_net_loss_on_batch_target(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(target_params), ctypes.byref(batch), _hip.ptr(self.losses),
                _hip.ptr(self.q_values), _hip.ptr(self.targets), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_loss_on_batch_target",
        )
        self._mirror_holds(params)
        return self.losses

    def loss_on_batch(self, batch: _hip.Batch, params=None) -> torch.Tensor:
        p = self._acting_params(params)
        _hip.check(
            self.lib.isdqn_net_loss_on_batch(
                ctypes.byref(self.cfg), _hip.ptr(p), ctypes.byref(batch), _hip.ptr(self.losses),
                _hip.ptr(self.q_values), _hip.ptr(self.targets), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_loss_on_batch",
        )
        self._mirror_holds(params)
        return self.losses

    def commit_batch_stats(self) -> None:
        """params["batch_stats"] <- the collection the last training-mode forward in this workspace returned (the analysis agents keep
        the evaluation batch's: analysisdqn.py:121-131).  The running averages are written in the master alone: the weight mirror is
        marked stale."""
        _hip.check(self.lib.isdqn_net_bn_commit_running(ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(self.workspace),
                                                        _hip.stream_ptr(self.device)), "isdqn_net_bn_commit_running")
        self._mirror_version = None

    def batch_stats_slice(self) -> slice:
        """Where the running averages (tensor kinds 7, 8) sit in the flat parameter buffer: one contiguous block behind the optimised ones."""
        stats = [i for i in self.infos if i.kind in (7, 8)]
        lo, hi = min(i.offset for i in stats), max(i.offset + i.size for i in stats)
        assert all(i.offset + i.size <= lo or i.offset >= hi for i in self.infos if i.kind not in (7, 8)), "running averages are not contiguous"
        return slice(lo, hi)

    def shift_params(self, params=None) -> None:
        p = self.params if params is None else params
        _hip.check(self.lib.isdqn_net_shift_params(ctypes.byref(self.cfg), _hip.ptr(p), _hip.stream_ptr(self.device)))
        if self.noisy and params is None:  # the head blocks of sigma move exactly as those of mu (same layout)
            _hip.check(self.lib.isdqn_net_shift_params(ctypes.byref(self.cfg), _hip.ptr(self.sigma), _hip.stream_ptr(self.device)))
        self._mirror_version = None  # the head rows moved in the master only

    def soft_shift(self, tau: float, params=None) -> None:
        """Soft head shift (include/isdqn_hip.h, isdqn_net_soft_shift): head k <- (1 - tau) * head k + tau * head k+1 on the last Dense,
        k < n_heads - 1, every head reading its neighbour's value from before the call; one stream-ordered launch.  ``params`` None: the
        engine's own parameters, and the same launch stores the weight mirror of the rows it wrote -- a mirror that was current stays
        current, one that was not stays marked so.  A noisy engine shifts ``sigma`` with the same rule and the masters alone (its mirror
        holds the composed parameters, which the next step's compose rebuilds); another buffer of the layout: that buffer alone, master
        only -- handing in the engine's own ``params`` that way marks the mirror stale."""
        own = params is None
        p = self.params if own else params
        ws = _hip.ptr(self.workspace) if own and not self.noisy else 0
        _hip.check(self.lib.isdqn_net_soft_shift(ctypes.byref(self.cfg), _hip.ptr(p), float(tau), ws, _hip.stream_ptr(self.device)),
                   "isdqn_net_soft_shift")
        if not own:
            self._wrote_without_mirror(params)
            return
        if self.noisy:
            _hip.check(self.lib.isdqn_net_soft_shift(ctypes.byref(self.cfg), _hip.ptr(self.sigma), float(tau), 0, _hip.stream_ptr(self.device)),
                       "isdqn_net_soft_shift")
            if tau > 0:
                self._mirror_version = None  # (it held eff of the unshifted masters)
        elif tau == 1:
            self._mirror_holds(None)  # the hard shift's route ends by rebuilding the mirror from the new parameters
        # otherwise the raw-pointer write moved neither torch's version counter nor the relation between master and mirror

    prune_mask = None     # set_pruning: int32 words of the bit mask over the parameter buffer (bit set = kept), all ones at first
    prune_scratch = None  # set_pruning: what the selection counts in
    prune_infos = ()      # set_pruning: per prunable tensor (index into ``infos``, offset, internal size, real element count)

    def set_pruning(self) -> list:
        """Gradual magnitude pruning (include/isdqn_hip.h, isdqn_net_prune_*) for this engine: allocates the bit mask over the parameter
        buffer (all ones: nothing pruned) and the selection's scratch, and returns the real element count of every prunable tensor --
        every conv and Dense kernel but the last Dense's, in layout order.  Nothing else changes: learn steps, batches and captured
        updates are those of an engine that never heard of it until ``prune_update`` / ``prune_apply`` are called.  Calling it again
        starts from a full mask.  Noisy engines, batch_norm and the impala torso are refused (ValueError)."""
        _sparsity.check_network(noisy=self.noisy, batch_norm=self.batch_norm, architecture_type=self.architecture_type)
        n, words, scratch = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        _hip.check(self.lib.isdqn_net_prune_layout(ctypes.byref(self.cfg), ctypes.byref(n), None, 0, ctypes.byref(words), ctypes.byref(scratch)),
                   "isdqn_net_prune_layout")
        infos = (ctypes.c_int64 * (4 * n.value))()
        _hip.check(self.lib.isdqn_net_prune_layout(ctypes.byref(self.cfg), ctypes.byref(n), infos, n.value, None, None), "isdqn_net_prune_layout")
        self.prune_infos = tuple(tuple(int(x) for x in infos[4 * i:4 * i + 4]) for i in range(n.value))
        self.prune_mask = torch.full((int(words.value),), -1, dtype=torch.int32, device=self.device)
        self.prune_scratch = torch.zeros(max(int(scratch.value) // 4, 1), dtype=torch.int32, device=self.device)
        return [i[3] for i in self.prune_infos]

    def _layout_buffer(self, params):
        """(buffer, workspace pointer or 0) of a pruning or projection call: the engine's own parameters go with their mirror."""
        own = params is None
        p = self.params if own else params
        assert p.dtype == torch.float32 and p.numel() == self.n_param_floats and p.is_contiguous() and p.device == self.params.device
        return p, (_hip.ptr(self.workspace) if own else 0)

    def prune_update(self, counts, params=None) -> None:
        """Mask update (include/isdqn_hip.h, isdqn_net_prune_update): of every prunable tensor the ``counts[i]`` real elements of smallest
        (already pruned, |w|, index) are pruned from here on, then the mask is applied.  ``params`` None: the engine's own parameters,
        and the apply launch stores the weight mirror of what it wrote -- a mirror that was current stays current, one that was not stays
        marked so.  Another buffer of the layout: the magnitudes are read there, that buffer alone is written, master only -- handing in
        the engine's own ``params`` that way marks the mirror stale.  Stream-ordered, no host synchronisation."""
        if self.prune_mask is None:
            raise ValueError(_sparsity.PRUNE_NOT_SET_REFUSED)
        p, ws = self._layout_buffer(params)
        if len(counts) != len(self.prune_infos) or any(int(k) != k or not 0 <= int(k) <= i[3] for k, i in zip(counts, self.prune_infos)):
            raise ValueError(_sparsity.PRUNE_COUNTS_REFUSED)
        k = (ctypes.c_int32 * len(self.prune_infos))(*[int(c) for c in counts])
        _hip.check(self.lib.isdqn_net_prune_update(ctypes.byref(self.cfg), _hip.ptr(p), k, _hip.ptr(self.prune_mask), _hip.ptr(self.prune_scratch),
                                                   ws, _hip.stream_ptr(self.device)), "isdqn_net_prune_update")
        if params is not None:
            self._wrote_without_mirror(params)
        # otherwise the raw-pointer write moved neither torch's version counter nor the relation between master and mirror

    def prune_apply(self, params=None) -> None:
        """+0.0 wherever the mask says pruned (include/isdqn_hip.h, isdqn_net_prune_apply): one stream-ordered launch, the node behind
        every gradient step.  ``params`` as in ``prune_update``."""
        if self.prune_mask is None:
            raise ValueError(_sparsity.PRUNE_NOT_SET_REFUSED)
        p, ws = self._layout_buffer(params)
        _hip.check(self.lib.isdqn_net_prune_apply(ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(self.prune_mask), ws, _hip.stream_ptr(self.device)),
                   "isdqn_net_prune_apply")
        if params is not None:
            self._wrote_without_mirror(params)

    project_target = None   # set_weight_projection: float64, the target norm rho_i of every projected tensor
    project_norms_out = None  # set_weight_projection: float64, n_i of the last project_weights / project_norms call, before the projection
    project_scales = None   # set_weight_projection: float32, s_i of the last project_weights call
    project_scratch = None  # set_weight_projection: one double per chunk
    project_infos = ()      # set_weight_projection: per projected tensor (index into ``infos``, offset, internal size, real element count)

    def set_weight_projection(self, target_norms=None) -> list:
        """Normalize-and-Project (include/isdqn_hip.h, isdqn_net_project_*) for this engine: allocates the scratch, ``project_norms_out``,
        ``project_scales`` (ones) and ``project_target``, and returns the target norms as a list of floats, one per projected tensor --
        every conv and Dense kernel but the last Dense's, in layout order.  ``target_norms`` None: the norms of the engine's current
        parameters, measured once on the device (one host read, here and nowhere else).  Nothing else changes: learn steps, batches and
        captured updates are those of an engine that never heard of it until ``project_weights`` / ``project_norms`` are called.
        Noisy engines, batch_norm and the impala torso are refused (ValueError)."""
        _projection.check_engine(noisy=self.noisy, batch_norm=self.batch_norm, architecture_type=self.architecture_type)
        n, scratch = ctypes.c_int32(), ctypes.c_int64()
        _hip.check(self.lib.isdqn_net_project_layout(ctypes.byref(self.cfg), ctypes.byref(n), None, 0, ctypes.byref(scratch)),
                   "isdqn_net_project_layout")
        infos = (ctypes.c_int64 * (4 * n.value))()
        _hip.check(self.lib.isdqn_net_project_layout(ctypes.byref(self.cfg), ctypes.byref(n), infos, n.value, None), "isdqn_net_project_layout")
        if target_norms is not None:
            target_norms = _projection.check_targets(target_norms, n.value)
        self.project_infos = tuple(tuple(int(x) for x in infos[4 * i:4 * i + 4]) for i in range(n.value))
        self.project_scratch = torch.zeros(max(int(scratch.value) // 8, 1), dtype=torch.float64, device=self.device)
        self.project_norms_out = torch.zeros(max(n.value, 1), dtype=torch.float64, device=self.device)
        self.project_scales = torch.ones(max(n.value, 1), dtype=torch.float32, device=self.device)
        self.project_target = torch.zeros(max(n.value, 1), dtype=torch.float64, device=self.device)
        if target_norms is None:
            target_norms = self.project_norms()
        self.project_target[: n.value].copy_(torch.tensor(target_norms, dtype=torch.float64))
        return list(target_norms)

    def project_norms(self, params=None) -> list:
        """The norm of every projected tensor of ``params`` (None: the engine's own) as the device measures it
        (include/isdqn_hip.h, isdqn_net_project_norms): two launches and one host read.  Writes ``project_norms_out`` and no parameter."""
        if self.project_target is None:
            raise ValueError(_projection.NAP_NOT_SET_REFUSED)
        p, _ = self._layout_buffer(params)
        _hip.check(self.lib.isdqn_net_project_norms(ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(self.project_norms_out),
                                                    _hip.ptr(self.project_scratch), _hip.stream_ptr(self.device)), "isdqn_net_project_norms")
        return [float(x) for x in self.project_norms_out[: len(self.project_infos)].cpu()]

    def project_weights(self, params=None) -> None:
        """Every projected tensor back to its target norm (include/isdqn_hip.h, isdqn_net_project_apply): two stream-ordered launches,
        the node behind every gradient step; no host read -- ``project_norms_out`` (before the projection) and ``project_scales`` hold
        what it measured and applied.  ``params`` None: the engine's own parameters, and the weight mirror is stored with them -- a
        mirror that was current stays current, one that was not stays marked so.  Another buffer of the layout: that buffer alone,
        master only -- handing in the engine's own ``params`` that way marks the mirror stale."""
        if self.project_target is None:
            raise ValueError(_projection.NAP_NOT_SET_REFUSED)
        p, ws = self._layout_buffer(params)
        _hip.check(self.lib.isdqn_net_project_apply(ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(self.project_target),
                                                    _hip.ptr(self.project_norms_out), _hip.ptr(self.project_scales),
                                                    _hip.ptr(self.project_scratch), ws, _hip.stream_ptr(self.device)), "isdqn_net_project_apply")
        if params is not None:
            self._wrote_without_mirror(params)

    def best_action(self, *, frames=None, frame_stride=0, frame_ids=None, obs=None, idx_network: int, params=None) -> torch.Tensor:
        p = self._acting_params(params)
        _hip.check(
            self.lib.isdqn_net_best_action(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(frames), int(frame_stride), _hip.ptr(frame_ids),
                _hip.ptr(obs), int(idx_network), _hip.ptr(self.action_out), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_best_action",
        )
        self._mirror_holds(params)
        return self.action_out

    def analysis(self, *, frames=None, frame_stride=0, frame_ids=None, obs=None, n_rows: int, params=None):
        """AnalysisNet.apply (utils/analysis_architecture.py:9-122) on n_rows observations: (features [n_rows, width of the last
        hidden layer], [per-layer sums over the rows of the post-ReLU activations, in the reference's shapes flattened]).  impala:
        the two ReLU outputs of every residual block come first; BatchNorm networks run on the batch statistics of these rows."""
        n_hidden = ctypes.c_int32()
        sizes = (ctypes.c_int64 * 32)()  # (impala: 12 block activations + the torso output + the hidden Dense layers)
        _hip.check(self.lib.isdqn_net_analysis_layout(ctypes.byref(self.cfg), ctypes.byref(n_hidden), sizes, 32))
        sizes = [int(sizes[i]) for i in range(n_hidden.value)]
        feats = torch.empty(n_rows, sizes[-1], dtype=torch.float32, device=self.device)
        scores = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        p = self.params if params is None else params
        _hip.check(
            self.lib.isdqn_net_analysis(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(frames), int(frame_stride), _hip.ptr(frame_ids), _hip.ptr(obs),
                int(n_rows), _hip.ptr(feats), _hip.ptr(scores), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_analysis",
        )
        self._mirror_holds(params)
        return feats, list(torch.split(scores, sizes))

    def redo_layout(self) -> list:
        """Widths of the recyclable layers (include/isdqn_hip.h, isdqn_net_redo_layout): the hidden layers in network order, a conv
        layer counted in output channels."""
        n = ctypes.c_int32()
        widths = (ctypes.c_int32 * 32)()
        _hip.check(self.lib.isdqn_net_redo_layout(ctypes.byref(self.cfg), ctypes.byref(n), widths, 32), "isdqn_net_redo_layout")
        return [int(widths[i]) for i in range(n.value)]

    def redo(self, *, frames=None, frame_stride=0, frame_ids=None, obs=None, n_rows: int, tau: float, fresh: torch.Tensor):
        """ReDo (Sokar et al. 2023; include/isdqn_hip.h, isdqn_net_redo) on the engine's own params / adam_m / adam_v: score the hidden
        neurons on n_rows observations, recycle the dormant ones from ``fresh`` (internal layout: ``fresh_params``).  Returns device
        tensors, split per layer like ``analysis``: (scores, mask (int32 0 / 1), n_recycled int32 [n_layers]); nothing is read back."""
        if self.noisy:
            raise ValueError(NOISY_REDO_REFUSED)
        assert fresh.dtype == torch.float32 and fresh.numel() == self.n_param_floats and fresh.is_contiguous() and fresh.device == self.params.device
        widths = self.redo_layout()
        scores = torch.empty(sum(widths), dtype=torch.float32, device=self.device)
        mask = torch.empty(sum(widths), dtype=torch.int32, device=self.device)
        n_recycled = torch.empty(len(widths), dtype=torch.int32, device=self.device)
        _hip.check(
            self.lib.isdqn_net_redo(
                ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(self.adam_m), _hip.ptr(self.adam_v), _hip.ptr(fresh),
                _hip.ptr(frames), int(frame_stride), _hip.ptr(frame_ids), _hip.ptr(obs), int(n_rows), float(tau),
                _hip.ptr(scores), _hip.ptr(mask), _hip.ptr(n_recycled), _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_redo",
        )
        # The library wrote `params` through the raw pointer, which does not move torch's version counter -- and it rebuilt the
        # mirror from the recycled parameters as its last launch.  So "mirror == params at this version" is exactly what holds now,
        # and _mirror_is_current stays right under trust_mirror = True: a later torch write moves the counter and is seen as before.
        self._mirror_holds(None)
        return list(torch.split(scores, widths)), list(torch.split(mask, widths)), n_recycled

    # ------------------------------------------------------------------ periodic resets, EMA targets
    def reset_layout(self) -> tuple:
        """(n_layers, first_dense_layer) of the layer list ``infos[i].layer`` indexes (include/isdqn_hip.h, isdqn_net_reset_layout)."""
        n, first = ctypes.c_int32(), ctypes.c_int32()
        _hip.check(self.lib.isdqn_net_reset_layout(ctypes.byref(self.cfg), ctypes.byref(n), ctypes.byref(first)), "isdqn_net_reset_layout")
        return int(n.value), int(first.value)

    def reset(self, fresh: torch.Tensor, split_layer: int | None = None, shrink_lower: float = 0.5, perturb_lower: float = 0.5,
              shrink_upper: float = 0.0, perturb_upper: float = 1.0, params: torch.Tensor | None = None, moments: bool = True,
              count: bool = True) -> None:
        """Shrink-and-perturb reset (include/isdqn_hip.h, isdqn_net_reset) towards ``fresh`` (internal layout: ``fresh_params``): tensors of
        layer >= ``split_layer`` (default: the first Dense layer) take the upper factor pair, the others the lower one.  ``params`` None:
        the engine's own parameters, with ``adam_m`` / ``adam_v`` cleared where written (``moments``), ``adam_count`` zeroed (``count``)
        and the weight mirror rebuilt.  Another buffer of the layout (a target copy, a sigma buffer): that buffer alone -- no moments, no
        count, no mirror (the engine's own ``params`` handed in that way are written as any buffer is, and the mirror is marked stale); a
        noisy engine's own ``sigma`` is recognised and takes ``sigma_m`` / ``sigma_v`` as its moments.  One stream-ordered call; no
        pointer moves."""
        assert fresh.dtype == torch.float32 and fresh.numel() == self.n_param_floats and fresh.is_contiguous() and fresh.device == self.params.device
        if split_layer is None:
            split_layer = self.reset_layout()[1]
        own = params is None
        m = v = cnt = None
        if own:
            params = self.params
            if moments:
                m, v = self.adam_m, self.adam_v
            cnt = self.adam_count if count else None
        elif self.noisy and params is self.sigma and moments:
            m, v = self.sigma_m, self.sigma_v
        _hip.check(
            self.lib.isdqn_net_reset(
                ctypes.byref(self.cfg), _hip.ptr(params), _hip.ptr(m), _hip.ptr(v), _hip.ptr(cnt), _hip.ptr(fresh), int(split_layer),
                float(shrink_lower), float(perturb_lower), float(shrink_upper), float(perturb_upper),
                _hip.ptr(self.workspace) if own else 0, _hip.stream_ptr(self.device),
            ),
            "isdqn_net_reset",
        )
        if own:
            # as in redo: the raw-pointer write does not move torch's version counter and the call's last launch rebuilt the mirror from
            # the new parameters (a noisy engine: the mirror no longer holds eff, and _mirror_holds marks it as not holding params)
            self._mirror_holds(None)
        else:
            self._wrote_without_mirror(params)

    def ema(self, target: torch.Tensor, tau: float, online: torch.Tensor | None = None) -> None:
        """target <- (1 - tau) * target + tau * online (include/isdqn_hip.h, isdqn_net_ema; ``online`` None: the engine's parameters) over
        two buffers of the parameter layout, one stream-ordered launch.  The weight mirror is not written: a ``target`` that is the
        engine's own ``params`` marks it stale."""
        online = self.params if online is None else online
        assert target.dtype == torch.float32 and target.numel() == self.n_param_floats and online.numel() == self.n_param_floats
        _hip.check(self.lib.isdqn_net_ema(ctypes.byref(self.cfg), _hip.ptr(target), _hip.ptr(online), float(tau), _hip.stream_ptr(self.device)),
                   "isdqn_net_ema")
        self._wrote_without_mirror(target)

    def fresh_sigma(self) -> torch.Tensor:
        """A new device tensor holding what ``init_sigma`` writes into ``sigma``: the source of a reset of sigma."""
        t = torch.empty_like(self.params)
        self._import_sigma(self._sigma_tree(), t)
        return t

    # ------------------------------------------------------------------ weight-mirror bookkeeping
    # The library keeps a pre-split mirror of the weights in the workspace and rebuilds it at the head of every call unless
    # told that it is current.  DEFAULT: never told -- every entry point outside a captured replay rebuilds (one 8 us launch),
    # and every captured replay rebuilds at its head (slimdqn/_graph.py), so a writer this class cannot see (a raw pointer, a
    # DLPack consumer, `params.data.copy_()`: none of them moves torch's version counter) is still acted on.
    # `trust_mirror = True` is an explicit declaration by the owner of the engine that every parameter write goes through
    # torch operations on `self.params` or through this class: then the rebuild is skipped while (a) the call reads the
    # engine's own buffer, (b) the last call left the mirror equal to it, (c) no torch operation has written the tensor since
    # (version counter) and (d) tensor object and storage are the ones the engine allocated.
    trust_mirror = os.environ.get("ISDQN_TRUST_MIRROR", "0") == "1"

    def _mirror_is_current(self, params) -> bool:
        return bool(self.trust_mirror and params is None and getattr(self, "_mirror_version", None) == self.params._version
                    and self.params.data_ptr() == getattr(self, "_mirror_ptr", None))

    def rebuild_mirror(self) -> None:
        """Rebuild the weight mirror from the engine's parameters (one launch on the current stream), unconditionally."""
        _hip.check(self.lib.isdqn_net_refresh_mirror(ctypes.byref(self.cfg), _hip.ptr(self.params), _hip.ptr(self.workspace),
                                                     _hip.stream_ptr(self.device)), "isdqn_net_refresh_mirror")
        self._mirror_made_current()

    def refresh_mirror(self) -> None:
        """Rebuild the weight mirror from the engine's parameters now (one launch on the current stream) unless it is current."""
        if self._mirror_is_current(None):
            return
        self.rebuild_mirror()

    def invalidate_mirror(self) -> None:
        """Force the next call to rebuild the weight mirror from ``params`` (for writers that bypass torch's version counter)."""
        self._mirror_version = None

    def _wrote_without_mirror(self, buffer: torch.Tensor) -> None:
        """The call just enqueued wrote ``buffer`` through its raw pointer and was handed no workspace.  A buffer of the caller's is
        none of the mirror's business; one whose bytes overlap the engine's own parameter storage (``params=eng.params``, a view or
        a slice of it: the addresses decide, not the object) moved the master alone, and the mirror no longer holds it."""
        lo = self.params.data_ptr()
        at = buffer.data_ptr()
        if at < lo + self.params.numel() * self.params.element_size() and lo < at + buffer.numel() * buffer.element_size():
            self._mirror_version = None

    def _mirror_made_current(self) -> None:
        self._mirror_version = self.params._version
        self._mirror_ptr = self.params.data_ptr()

    def _mirror_holds(self, params) -> None:
        """The call just enqueued rebuilt the mirror from `params` (None = the engine's own buffer)."""
        self._mirror_version = self.params._version if params is None and not self.noisy else None  # (noisy: the mirror holds eff)
        self._mirror_ptr = self.params.data_ptr()

    def best_actions(self, *, frames=None, frame_stride=0, frame_ids=None, obs=None, idx_networks: torch.Tensor | None = None, params=None,
                     out: torch.Tensor | None = None, mirror_current: bool | None = None, mean_heads: bool = False,
                     n_rows: int | None = None) -> torch.Tensor:
        """Greedy actions of n observations in one forward (isdqn.py:127-135 per row): int32 device tensor [n].
        ``mirror_current``: None = decided by the engine's bookkeeping; a captured graph fixes it at capture time.
        ``mean_heads``: the greedy action of the sum of all heads (ISDQN_ACT_MEAN_HEADS: REM's evaluation policy); ``idx_networks`` is
        then not read and may be None, with ``n_rows`` (or ``out``) giving the number of observations."""
        if idx_networks is not None:
            n = int(idx_networks.numel())
        else:
            assert mean_heads and (n_rows is not None or out is not None), "best_actions without idx_networks: mean_heads and n_rows"
            n = int(n_rows) if n_rows is not None else int(out.numel())
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        p = self.params if params is None else params
        if mirror_current is None:
            mirror_current = self._mirror_is_current(params)
        if self.noisy and params is None:  # one draw serves all rows; compose leaves the mirror of eff in the workspace
            p, mirror_current = self.compose(), True
        flags = (_hip.BATCH_MIRROR_CURRENT if mirror_current else 0) | (_hip.ACT_MEAN_HEADS if mean_heads else 0)
        _hip.check(
            self.lib.isdqn_net_best_actions(
                ctypes.byref(self.cfg), _hip.ptr(p), _hip.ptr(frames), int(frame_stride), _hip.ptr(frame_ids), _hip.ptr(obs), n,
                _hip.ptr(idx_networks), _hip.ptr(out), flags, _hip.ptr(self.workspace), _hip.stream_ptr(self.device),
            ),
            "isdqn_net_best_actions",
        )
        self._mirror_holds(params)
        return out

    def internal_to_flax_grads(self, grad_flat: torch.Tensor) -> Dict[str, Dict[str, np.ndarray]]:
        return self.export_flax(grad_flat)
