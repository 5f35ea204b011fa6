"""CPU reference of ReDo (Sokar et al. 2023, "The Dormant Neuron Phenomenon in Deep Reinforcement Learning") as include/isdqn_hip.h
defines it for isdqn_net_redo: numpy on Flax-layout arrays, moved into the library's internal layout by QNetEngine._to_internal.

  * scores: float64, from oracle.analysis.analysis_net's activation sums reduced per channel and divided by rows * positions;
  * dormant: a_c <= tau * mean_l (float64 here: device and reference agree away from the threshold only, which the tests assert);
  * recycle: on flat internal-layout buffers (parameters, Adam moments, fresh parameters).  WHERE the recycle writes is derived from
    Flax-layout indicator arrays through _to_internal -- "the kernel entries whose input index is neuron c" -- plus the two facts the
    internal layout adds: a neuron's incoming weights are one whole row of the leading (output) axis, padded input lanes included,
    and the outgoing zeroing covers the padded output rows too.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np


class HostLayout:
    """What the helper needs of a QNetEngine -- the tensor table of isdqn_net_param_layout (a host-only entry point) and
    _to_internal -- without a GPU.  A QNetEngine can be passed wherever a HostLayout is taken."""

    def __init__(self, observation_dim, n_actions, n_heads, features, architecture_type, layer_norm, batch_size=32, n_bins=0, n_quantiles=0):
        from slimdqn import _hip
        from slimdqn._engine import QNetEngine

        cfg = _hip.NetConfig()
        if architecture_type == "fc":
            cfg.arch, cfg.obs_h, cfg.obs_w, cfg.obs_c = _hip.ARCH_FC, 1, 1, int(np.prod(observation_dim))
        else:
            cfg.arch = _hip.ARCH_CNN if architecture_type == "cnn" else _hip.ARCH_IMPALA
            cfg.obs_h, cfg.obs_w, cfg.obs_c = (int(d) for d in observation_dim)
        cfg.n_features = len(features)
        for i, f in enumerate(features):
            cfg.features[i] = int(f)
        cfg.n_actions, cfg.n_heads, cfg.layer_norm, cfg.batch_size = int(n_actions), int(n_heads), int(bool(layer_norm)), int(batch_size)
        cfg.n_bins, cfg.n_quantiles = int(n_bins), int(n_quantiles)
        if n_bins:
            cfg.hl_min, cfg.hl_max, cfg.hl_sigma = -10.0, 10.0, 0.3
        lib = _hip.lib()
        n, cnt = ctypes.c_int64(), ctypes.c_int32()
        _hip.check(lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), None, 0, ctypes.byref(cnt)))
        infos = (_hip.TensorInfo * cnt.value)()
        _hip.check(lib.isdqn_net_param_layout(ctypes.byref(cfg), ctypes.byref(n), infos, cnt.value, ctypes.byref(cnt)))
        self.cfg, self.lib = cfg, lib
        self.infos, self.n_param_floats = list(infos), int(n.value)
        self.features, self.architecture_type, self.batch_norm = [int(f) for f in features], architecture_type, False
        self._first_dense_after_conv = lambda info: QNetEngine._first_dense_after_conv(self, info)
        self._to_internal = lambda info, arr: QNetEngine._to_internal(self, info, arr)


def to_flat(lay, tree) -> np.ndarray:
    """A Flax-layout pytree as the flat internal-layout buffer (what QNetEngine.import_flax uploads)."""
    flat = np.zeros(lay.n_param_floats, np.float32)
    for info in lay.infos:
        mod, leaf = info.name.decode().rsplit("/", 1)
        flat[info.offset : info.offset + info.size] = lay._to_internal(info, tree[mod][leaf])
    return flat


def hidden_layers(lay):
    """The recyclable layers in network order: every layer but the last Dense.  Per layer the tensor infos of its kernel, bias,
    LayerNorm scale / bias (None without) and of the next layer's kernel, and its width in neurons (conv: output channels)."""
    by_layer: dict = {}
    for info in lay.infos:
        by_layer.setdefault(int(info.layer), {})[int(info.kind)] = info
    order = sorted(by_layer)
    out = []
    for i, nxt in zip(order[:-1], order[1:]):
        t = by_layer[i]
        kernel = t[0] if 0 in t else t[1]
        n = int(kernel.flax_shape[3] if kernel.kind == 0 else kernel.flax_shape[1])
        nk = by_layer[nxt][0] if 0 in by_layer[nxt] else by_layer[nxt][1]
        out.append(SimpleNamespace(kernel=kernel, bias=t[2], ln_scale=t.get(3), ln_bias=t.get(4), next_kernel=nk, n_neurons=n,
                                   module=kernel.name.decode().rsplit("/", 1)[0],
                                   ln_module=t[3].name.decode().rsplit("/", 1)[0] if 3 in t else None))
    return out


def reference_scores(params, states, features, architecture_type, layer_norm):
    """float64 a_c per hidden layer: the mean over rows and pixel positions of neuron c's post-ReLU activation."""
    import torch

    from oracle import analysis as oa
    from oracle import network as onet

    _, sums = oa.analysis_net(onet.to_torch(params, torch.float64), states, list(features), architecture_type, layer_norm)
    n_rows = len(states)
    widths = list(features)
    out = []
    for s, c in zip(sums, widths):
        per_pos = np.asarray(s, np.float64).reshape(-1, c)  # (positions, channels): conv layers are (H, W, C) flattened
        out.append(per_pos.sum(0) / (n_rows * per_pos.shape[0]))
    return out


def dormant_masks(scores, tau):
    """Per layer: a_c <= tau * mean_l.  A layer that is zero everywhere is dormant everywhere."""
    return [np.asarray(a) <= tau * np.asarray(a).mean() for a in scores]


def threshold_margins(scores, tau):
    """Per layer |a_c / mean_l - tau| (inf for a layer with mean 0): how far every neuron is from the decision."""
    out = []
    for a in scores:
        m = np.asarray(a).mean()
        out.append(np.abs(np.asarray(a) / m - tau) if m > 0 else np.full(len(a), np.inf))
    return out


def _outgoing_columns(lay, layer, c) -> np.ndarray:
    """Boolean pattern over one internal row of the next layer's kernel: the entries that read neuron c of `layer`."""
    nk = layer.next_kernel
    shape = tuple(nk.flax_shape[: nk.ndim])
    ind = np.zeros(shape, np.float32)
    if nk.kind == 0:
        ind[:, :, c, :] = 1.0  # HWIO
    elif lay._first_dense_after_conv(nk):
        n = layer.n_neurons  # Flax flattens (H, W, C): input feature p * C + c
        ind.reshape(shape[0] // n, n, shape[1])[:, c, :] = 1.0
    else:
        ind[c, :] = 1.0
    rows = lay._to_internal(nk, ind).reshape(int(nk.dims[0]), -1)
    assert np.array_equal(rows[0], rows[shape[-1] - 1])  # every real output row reads the same columns
    return rows[0] != 0.0


def recycle(lay, params, adam_m, adam_v, fresh, masks):
    """ReDo's recycle on flat internal-layout float32 buffers; returns new (params, adam_m, adam_v).  `masks`: per hidden layer a
    boolean array over its neurons.  Incoming copies first, outgoing zeros second (a weight from a dormant neuron into a dormant
    neuron ends up 0); the moments are cleared wherever a parameter is written; everything else keeps its bits."""
    p, m, v = (np.array(a, dtype=np.float32, copy=True) for a in (params, adam_m, adam_v))
    fresh = np.asarray(fresh, np.float32)
    layers = hidden_layers(lay)
    assert len(layers) == len(masks)

    def view(buf, info):
        return buf[info.offset : info.offset + info.size].reshape(int(info.dims[0]), -1)

    for layer, mask in zip(layers, masks):
        assert len(mask) == layer.n_neurons
        for c in np.flatnonzero(mask):
            for info in (layer.kernel, layer.bias, layer.ln_scale, layer.ln_bias):
                if info is None:
                    continue
                view(p, info)[c] = view(fresh, info)[c]  # (a vector tensor: dims[0] rows of one element)
                view(m, info)[c] = 0.0
                view(v, info)[c] = 0.0
    for layer, mask in zip(layers, masks):
        for c in np.flatnonzero(mask):
            cols = _outgoing_columns(lay, layer, int(c))
            for buf in (p, m, v):
                view(buf, layer.next_kernel)[:, cols] = 0.0  # every row, the padded ones too
    return p, m, v
