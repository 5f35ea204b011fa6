"""Which kernel every convolution of the cnn torso runs on, restated on the host, and the cases of tests/test_gpu_conv_routes.py.

Two halves.  The plan-level half (layers, plan_fields: csrc/net_plan.h) is held to the real code by tests/test_conv_routes_host.py
through tests/helpers/plan_dump.cpp.  The launch-level half (forward_route, dgrad_route, wgrad_route: csrc/net_launch.h) has no host
entry point: it is written from the source, every rule with its file and line, and tests/test_conv_routes_host.py pins its result for
every case as a literal table, so that a moved threshold fails a test instead of moving a case onto another kernel.

Pure Python: no GPU, no torch."""

CONVS = ((8, 4), (4, 2), (3, 1))  # (kernel, stride) of the three convolutions: net_plan.h:316
FC_OBS = (8,)
ATARI = (84, 84, 4)
_ceil = lambda a, b: -(-a // b)
_round_up = lambda a, b: _ceil(a, b) * b

LDS_LIMIT = 158 * 1024  # net_launch.h:103
LDS_ONE_PER_CU = 80 * 1024  # net_launch.h:114, :166
LDS_BWD = 150 * 1024  # net_launch.h:432 (weight gradient), :541 (data gradient)
U8P_WPLANE = 32 * (256 + 16)  # conv_u8_pair.h:36-37
U8P_POSITIONS = 2 * 512  # conv_u8_pair.h:31-32 (U8P_PB * U8P_THREADS)
S8P_CHUNKS = 6 * 256 * 2  # conv_s8_pair.h:20, net_launch.h:171 (S8P_BATCH * GEMM_THREADS * 2)


def same_padding(size, k, s):
    """(output size, leading padding) of a SAME convolution along one axis (net_plan.h same_padding; oracle/network.py)"""
    out = _ceil(size, s)
    return out, max((out - 1) * s + k - size, 0) // 2


# ------------------------------------------------------------------ the plan, restated (net_plan.h)
def layers(cfg):
    """Hidden layers in plan order: name, kind, ln name, true / padded width, pixels, conv (k, s), internal input width.
    cfg: arch, feats, ln and, for a cnn, obs = (h, w, stack) (default: the Atari frame).  Convolutions also carry their whole
    geometry (net_plan.h:296-313 conv_geometry): hin, win, cin, cin_p, h, w (output), pad, u8, i."""
    out, n_ln = [], 0
    if cfg["arch"] == "cnn":
        h, w, c = cfg.get("obs", ATARI)
        cp = c
        for i, (k, s) in enumerate(CONVS):
            (ho, pad), (wo, pad_w) = same_padding(h, k, s), same_padding(w, k, s)
            assert pad == pad_w, "non-square padding is refused by the plan (net_plan.h:330)"
            co = cfg["feats"][i]
            out.append(dict(name=f"Conv_{i}", kind=0, ln=f"LayerNorm_{n_ln}" if cfg["ln"] else None, c=co, cp=_round_up(co, 8), npix=ho * wo,
                            k=k, s=s, h=ho, w=wo, K=c * 64 if i == 0 else k * k * cp,  # net_plan.h:308
                            hin=h, win=w, cin=c, cin_p=cp, pad=pad, u8=i == 0, i=i))
            h, w, c, cp = ho, wo, co, _round_up(co, 8)
            n_ln += cfg["ln"]
        in_p, dense = h * w * cp, cfg["feats"][3:]
    else:
        in_p, dense = _round_up(cfg.get("obs", FC_OBS)[0], 8), cfg["feats"]  # (an fc case may name its own observation width)
    for j, c in enumerate(dense):
        out.append(dict(name=f"Dense_{j}", kind=1, ln=f"LayerNorm_{n_ln}" if cfg["ln"] else None, c=c, cp=_round_up(c, 8), npix=1,
                        K=in_p, in_p=in_p))
        n_ln += cfg["ln"]
        in_p = _round_up(c, 8)
    return out, in_p


def fwd_splits(N2, out_p, K, unpadded):
    """split-K factor of a dense forward GEMM: net_plan.h:497-507 (fwd_narrow, fwd_splits), capped like effective_splits"""
    ft = _ceil(N2, 128) * _ceil(out_p, 128)
    if ft <= 64 and not unpadded and out_p % 64 == 0:
        ft = _ceil(N2, 128) * _ceil(out_p, 64)
    fs = 1 if ft >= 256 else 512 // ft
    return max(1, min(fs, _ceil(K, 32)))


def dense_wgrad_slabs(B, in_p, out_p):
    """split-K slabs of a dense weight gradient: net_plan.h:488-493"""
    tiles = _ceil(out_p, 128) * _ceil(in_p, 128)
    s = 1 if tiles >= 128 else 256 // tiles
    return max(1, min(s, _ceil(B, 32)))


def conv_wgrad_split(B, L):
    """slabs of a convolution's weight gradient on the generic engine: net_plan.h:434-441"""
    return max(1, min(256 // _ceil(L["K"], 64) or 1, _ceil(B * L["npix"], 32)))


def conv_wgrad_image(B, L):
    """(ntw, G, groups) of the image-resident weight gradient, (0, 0, 0) where the plan does not offer it: net_plan.h:461-484"""
    K = L["K"]
    if K % 64 != 0 or not (L["u8"] or L["cin_p"] % 16 == 0):
        return 0, 0, 0
    ntw = 4 if K % 256 == 0 else 3 if K % 192 == 0 else 2 if K % 128 == 0 else 0
    if K == 512:
        ntw = 2
    wide = L["cp"] == 64 and not L["u8"] and K in (512, 576)
    if wide:
        ntw = K // 64
    if not ntw:
        return 0, 0, 0
    ncg = K // (64 * ntw)
    G = (B * ncg + 255) // 256
    if wide:
        G = (B + 127) // 128
        if G > 2:
            G = max(2, (B + 255) // 256)
    G = max(G, 1)
    return ntw, G, _ceil(B, G)


def conv_wgrad_chain(B, L):
    """(K steps in one accumulator, slabs) that bound a convolution's weight gradient whichever kernel takes it: the generic
    engine's slabs, or the image-resident kernel's groups of G images (wgrad_route tells which)."""
    s = conv_wgrad_split(B, L)
    steps, slabs = _ceil(_ceil(B * L["npix"], 32), s), s
    # (callers with layer dicts of their own -- tests/test_gpu_batchnorm.py -- give name, K, k, cp, npix: uint8 pixels are Conv_0's)
    u8 = L["name"] == "Conv_0"
    ntw, G, groups = conv_wgrad_image(B, dict(L, u8=u8, cin_p=4 if u8 else L["K"] // L["k"] ** 2))
    if ntw:
        steps, slabs = max(steps, _ceil(G * L["npix"], 32)), max(s, groups)
    return steps, slabs


def _classes(L):
    """pixels (Ha, Wb) of each stride class of a convolution's input: net_plan.h:448-451, net_launch.h:529-531"""
    s = L["s"]
    return [((L["hin"] - c // s + s - 1) // s, (L["win"] - c % s + s - 1) // s) for c in range(s * s)]


def plan_fields(cfg, B):
    """Per convolution, the plan's tiling decisions as plan_dump prints them: npix, gw_slabs, wgi_ntw / wgi_G / wgi_groups (None where
    not offered), dgi_tiles, dgi_tile_pix (None without tiles), part_rows."""
    ls, _ = layers(cfg)
    out = []
    for L in ls:
        if L["kind"] != 0:
            break
        dgi = 0
        if L["i"] > 0 and L["k"] % L["s"] == 0 and L["cp"] <= 64 and L["cin_p"] <= 64:  # net_plan.h:445
            dgi = sum(_ceil(a * b, 128) for a, b in _classes(L))  # (the 64-pixel tiles are off in the product: net_plan.h:21-22, :455)
        ntw, G, groups = conv_wgrad_image(B, L)
        out.append(dict(npix=L["npix"], gw_slabs=max(conv_wgrad_split(B, L), groups), wgi_ntw=ntw or None, wgi_G=G or None,
                        wgi_groups=groups or None, dgi_tiles=dgi, dgi_tile_pix=128 if dgi else None))
    for i, f in enumerate(out):  # net_plan.h:512-522 part_rows_of (a convolution: kind != 1)
        rows = 256
        if i + 1 < len(out):
            rows = max(rows, B * out[i + 1]["dgi_tiles"])
        elif len(ls) > len(out) and ls[i]["cp"] == 64:
            rows = max(rows, _ceil(B, 64) * ls[i]["npix"])
        f["part_rows"] = rows
    return out


# ------------------------------------------------------------------ the launch side, restated (net_launch.h, conv_img.h)
def _img_geometry(L, b_planes, mt, a_planes, pitch=0):
    """(lds bytes, R, Wp, plane elements): conv_img.h:697-711 conv_img_geometry"""
    rows = L["h"] if L["npix"] <= 128 else (128 + L["w"] - 2) // L["w"] + 1
    rows = min(rows, L["h"])
    R = L["s"] * (rows - 1) + L["k"]
    if L["u8"]:
        Wp = ((L["w"] - 1) * L["s"] + L["k"] + 7) // 8 * 8
        plane = L["cin"] * R * Wp
    else:
        Wp = (L["w"] - 1) * L["s"] + L["k"]
        plane = R * Wp * (pitch or L["cin_p"])
    return (2 * a_planes * (mt * 16) * 48 + b_planes * plane) * 2, R, Wp, plane


def passes_of(L, x3):
    return (2 if L["u8"] else 3) if x3 else 1  # net_launch.h:97, :417


def forward_route(L, x3, n_img):
    """dict(kernel=..., ...) of conv_fwd (net_launch.h:85-196):
    "u8pair" (passes, tiles), "u8img" (mt, passes, tiles), "s8img" (mt, passes, tiles, kg), "s8pair", or "generic" (bm, passes, why:
    "lds", "stack" or "cin8")."""
    mt = 2 if L["cp"] <= 32 else 4  # :96
    p = passes_of(L, x3)
    PP = 0 if L["u8"] else L["cin_p"] + (16 if L["cin_p"] % 64 == 0 else 8)  # :100
    lds, R, Wp, _ = _img_geometry(L, 2 if p >= 3 else 1, mt, 2 if p >= 2 else 1, PP)  # :101
    generic = lambda why: dict(kernel="generic", bm=32 if L["cp"] <= 32 else 64, passes=p, why=why)  # :185-195
    if lds > LDS_LIMIT:  # :104
        return generic("lds")
    if L["u8"] and (L["win"] < 8 or L["cin"] > 4):  # :104
        return generic("stack")
    if not L["u8"] and L["cin_p"] < 16:  # :105
        return generic("cin8")
    tiles = _ceil(L["npix"], 128)  # :129
    stage = (2 if p >= 2 else 1) * (mt * 16) * 48 * 2 * 2  # :113, :164
    if not L["u8"] and L["npix"] <= 128:  # :109-120: the row pitch of a single-tile image
        want = Wp + (L["w"] - Wp) % 8
        lds2 = lds + (2 if p >= 3 else 1) * R * (want - Wp) * PP * 2
        old, new = (lds + stage if lds > LDS_ONE_PER_CU else lds), (lds2 + stage if lds2 > LDS_ONE_PER_CU else lds2)
        if want != Wp and new <= LDS_LIMIT and (old <= LDS_ONE_PER_CU) == (new <= LDS_ONE_PER_CU):
            Wp, lds = want, lds2
    if L["u8"]:
        rows = L["h"] if L["npix"] <= 256 else (256 + L["w"] - 2) // L["w"] + 1  # conv_u8_pair.h:334-338
        Rd = L["s"] * (min(rows, L["h"]) - 1) + L["k"]
        lds_pair = ((2 if p >= 2 else 1) * U8P_WPLANE + 4 * Rd * Wp) * 2  # conv_u8_pair.h:330-332
        if mt == 2 and tiles % 2 == 0 and Rd * (Wp // 8) <= U8P_POSITIONS and lds_pair <= LDS_LIMIT and L["cin"] == 4 and L["K"] == 256:  # :155-156
            return dict(kernel="u8pair", passes=p, tiles=tiles)
        return dict(kernel="u8img", mt=mt, passes=p, tiles=tiles)  # :159-160
    kg2 = mt == 4 and lds > LDS_ONE_PER_CU and lds + stage <= LDS_LIMIT and mt * 16 * 128 * 4 <= lds - stage and L["K"] >= 256  # :166-167
    if p == 3 and mt == 4 and kg2 and tiles == 1 and L["K"] == 512 and n_img % 2 == 0 and R * Wp * (L["cin_p"] // 8) <= S8P_CHUNKS:  # :170-171
        return dict(kernel="s8pair")
    return dict(kernel="s8img", mt=mt, passes=p, tiles=tiles, kg=2 if kg2 else 1)  # :174-177


def dgrad_route(L, x3, B, fields, below_fields):
    """dict(kernel="dgimg", mt, passes, tiles=[per class]) or dict(kernel="generic", why) of data_gradient (learn_step.h:451-454,
    net_launch.h:488-556); `fields` / `below_fields`: plan_fields of this layer and of the one below"""
    if not fields["dgi_tiles"]:  # :491
        return dict(kernel="generic", why="plan")
    if below_fields["part_rows"] < B * fields["dgi_tiles"]:  # :491
        return dict(kernel="generic", why="part_rows")
    T = L["k"] // L["s"]  # :503
    bt = max(T - 1 - L["pad"] // L["s"], 0)  # :511
    need_h, need_w = (L["hin"] - 1 + L["pad"]) // L["s"] + 1, (L["win"] - 1 + L["pad"]) // L["s"] + 1  # :513
    Hd, Wd = bt + max(L["h"], need_h), bt + max(L["w"], need_w)  # :514-515
    PPd = L["cp"] + ((16 - L["cp"] % 32) + 32) % 32  # :517
    mt = 2 if L["cin_p"] <= 32 else 4  # :538
    p = 3 if x3 else 1  # :539
    lds = (2 * (2 if p >= 2 else 1) * 32 * (mt * 16 + 16) + (2 if p >= 3 else 1) * Hd * Wd * PPd) * 2  # :540
    if lds > LDS_BWD:  # :541
        return dict(kernel="generic", why="lds")
    return dict(kernel="dgimg", mt=mt, passes=p, tiles=[_ceil(a * b, 128) for a, b in _classes(L)])  # :529-535, :550-551


def wgrad_route(L, x3, B, fields):
    """dict(kernel="wgimg", mt, ntw, passes, G, groups) or dict(kernel="generic", why, slabs, steps) of conv_wgrad
    (net_launch.h:809-816, :411-478).  why: "plan" (no wgi_ntw), "lds", "stack", "u8ntw3"."""
    def generic(why):  # :558-562 conv_wgrad_slabs, :405-407
        ksteps = _ceil(B * L["npix"], 32)
        sps = _ceil(ksteps, fields["gw_slabs"])
        return dict(kernel="generic", why=why, slabs=_ceil(ksteps, sps), steps=sps)

    ntw = fields["wgi_ntw"]
    if not ntw or _ceil(B, fields["wgi_G"]) > fields["gw_slabs"]:  # :414
        return generic("plan")
    p = passes_of(L, x3)
    mt = 2 if L["cp"] <= 32 else 4  # :418
    _, _, Wp, _ = _img_geometry(L, 1, mt, 1)  # :420
    R = L["s"] * (L["h"] - 1) + L["k"]  # :421
    PPin = L["cin_p"]
    for pad in (0, 8, 16, 24):  # :425-426
        if (L["s"] * (L["cin_p"] + pad)) % 32 == 16:
            PPin = L["cin_p"] + pad
            break
    in_plane = L["cin"] * R * Wp if L["u8"] else R * Wp * PPin  # :427
    PA = L["cp"] + (16 if L["cp"] % 32 == 0 else 8)  # :428
    dz_plane = _round_up(L["npix"], 32) * PA  # :429-430
    lds = ((2 if p >= 2 else 1) * dz_plane + (2 if p >= 3 else 1) * in_plane) * 2  # :431
    if lds > LDS_BWD:  # :432
        return generic("lds")
    if L["u8"] and (L["win"] < 8 or L["cin"] > 4):  # :432
        return generic("stack")
    if L["u8"] and ntw not in (2, 4):  # :455-459, :476: uint8 pixels with three column tiles per wave are not instantiated
        return generic("u8ntw3")
    assert L["u8"] or (mt == 2 and ntw in (2, 3, 4)) or (mt == 4 and ntw in (2, 3, 4, 8, 9)), "an uninstantiated S8 form"  # :461-472
    return dict(kernel="wgimg", mt=mt, ntw=ntw, passes=p, u8=L["u8"], G=fields["wgi_G"], groups=_ceil(B, fields["wgi_G"]))  # :451


def fmt(r):
    """A route as the literal table of tests/test_conv_routes_host.py writes it."""
    k = r["kernel"]
    if k == "u8pair":
        return f"u8pair<{r['passes']}> tiles={r['tiles']}"
    if k == "u8img":
        return f"u8img<{r['mt']},{r['passes']}> tiles={r['tiles']}"
    if k == "s8img":
        return f"s8img<{r['mt']},{r['passes']}{',KG2' if r['kg'] == 2 else ''}> tiles={r['tiles']}"
    if k == "s8pair":
        return "s8pair"
    if k == "dgimg":
        return f"dgimg<{r['mt']},{r['passes']}> tiles={'+'.join(map(str, r['tiles']))}"
    if k == "wgimg":
        return f"wgimg<{r['mt']},{r['ntw']},{r['passes']}{',u8' if r['u8'] else ''}> G={r['G']} groups={r['groups']}"
    if "bm" in r:
        return f"generic<{r['bm']},{r['passes']}>({r['why']})"
    return f"generic({r['why']})" + (f" slabs={r['slabs']} steps={r['steps']}" if "slabs" in r else "")


def routes(cfg, precision):
    """Per convolution: dict(fwd=route at n_img = 2B, fwd1=route at n_img = 1, dgrad=route or None (Conv_0), wgrad=route)."""
    x3 = precision == "bf16x3"
    B = cfg["B"]
    ls, _ = layers(cfg)
    F = plan_fields(cfg, B)
    out = []
    for i, f in enumerate(F):
        L = ls[i]
        out.append(dict(fwd=forward_route(L, x3, 2 * B), fwd1=forward_route(L, x3, 1),
                        dgrad=dgrad_route(L, x3, B, f, F[i - 1]) if i else None, wgrad=wgrad_route(L, x3, B, f)))
    return out


# ------------------------------------------------------------------ the cases
HIDDEN = 32  # the hidden Dense width: small, so that the dense tail costs nothing
CASES = {
    "100x100": dict(obs=(100, 100, 4), feats=(32, 64, 64, HIDDEN), K=3, A=5, B=6, slack=5),  # frame pitch h * w + 5, slack bytes 0xFF
    "160x120": dict(obs=(160, 120, 4), feats=(32, 64, 64, HIDDEN), K=2, A=3, B=3),
    "128x128-w64": dict(obs=(128, 128, 4), feats=(64, 64, 64, HIDDEN), K=2, A=3, B=4),
    "64x64x3": dict(obs=(64, 64, 3), feats=(32, 64, 64, HIDDEN), K=3, A=4, B=6),
    "84-w64-48-24": dict(obs=(84, 84, 4), feats=(64, 48, 24, HIDDEN), K=2, A=5, B=5),
    "40x40x2": dict(obs=(40, 40, 2), feats=(16, 32, 64, HIDDEN), K=3, A=3, B=7),
    "8x8x1": dict(obs=(8, 8, 1), feats=(8, 8, 8, HIDDEN), K=2, A=3, B=3),
}
for _c in CASES.values():
    _c.update(arch="cnn", ln=True)
    _c.setdefault("slack", 0)
BOTH_PRECISIONS = ("100x100", "128x128-w64", "84-w64-48-24")  # their routes change with the precision
RUNS = [(c, "bf16x3") for c in CASES] + [(c, "bf16") for c in BOTH_PRECISIONS]
