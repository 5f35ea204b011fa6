"""Host checks of the float64 bf16 model (tests/helpers/bf16_model.py) the GPU tests hold the kernels to."""
import numpy as np
import torch

from tests.helpers import bf16_model as M


def _specials():
    bits = np.array([0x3F808000, 0x3F818000, 0x3F80C000, 0x3F807FFF, 0xBF808000, 0xBF818000,  # ties to even, up and down; near-ties
                     0x00000001, 0x00008000, 0x00018000, 0x0000FFFF, 0x007FFFFF, 0x80008000,  # denormals and their ties
                     0x7F7FFFFF, 0x7F7F8000, 0xFF7FFFFF, 0x7F800000, 0x00000000, 0x80000000], np.uint32)
    return bits.view(np.float32)


def test_nearest_even_rounding_matches_the_bit_level_reference():
    rng = np.random.default_rng(0)
    x = np.concatenate([_specials(), rng.integers(0, 2**32, 200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[~np.isnan(x)]
    got = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, M.rne_bf16_bits(x))
    # ties: 1 + 2^-8 is halfway between 1 and 1 + 2^-7 -> 1 (even); 1 + 3 2^-8 -> 1 + 2^-6
    assert M.bf16_bits_to_f64(M.rne_bf16_bits(np.float32(1 + 2.0**-8))) == 1.0
    assert M.bf16_bits_to_f64(M.rne_bf16_bits(np.float32(1 + 3 * 2.0**-8))) == 1 + 2.0**-6
    # the largest finite float32 rounds to infinity, a denormal tie to even
    assert M.rne_bf16_bits(np.float32(np.finfo(np.float32).max)) == 0x7F80
    assert M.rne_bf16_bits(np.array([0x00008000], np.uint32).view(np.float32))[0] == 0
    assert M.rne_bf16_bits(np.array([0x00018000], np.uint32).view(np.float32))[0] == 2
    # split(): hi is that rounding, and lo the rounding of the exact float32 remainder
    f = x[np.isfinite(x) & (np.abs(x) < 1e38)]
    hi, lo = M.split(torch.from_numpy(f))
    assert np.array_equal(hi.numpy(), M.bf16_bits_to_f64(M.rne_bf16_bits(f)))
    rem = (f - hi.numpy().astype(np.float32)).astype(np.float32)
    assert np.array_equal(lo.numpy(), M.bf16_bits_to_f64(M.rne_bf16_bits(rem)))


def test_s8_unpack_round_trip():
    rng = np.random.default_rng(1)
    v = (rng.normal(size=(5, 24)) * np.exp(rng.uniform(-30, 30, (5, 24)))).astype(np.float32)
    words = M.split_words(torch.from_numpy(v))  # what the kernels store: [hi x 8][lo x 8] per 8 floats
    region = words.view(torch.float32)
    hi, lo = M.s8_planes(region, 5, 24)
    want_hi, want_lo = M.split(torch.from_numpy(v))
    assert torch.equal(hi, want_hi.reshape(5, 24)) and torch.equal(lo, want_lo.reshape(5, 24))
    assert np.all(np.abs((hi + lo).numpy() - v) <= M.S8_STORE * np.abs(v))
    assert not bool(M.s8_malformed(hi, lo).any())
    # a truncating split is malformed on many elements
    t = torch.from_numpy((v.view(np.uint32) & 0xFFFF0000).view(np.float32))
    tl = (torch.from_numpy(v) - t).to(torch.bfloat16).double()
    assert float(M.s8_malformed(t.double(), tl).double().mean()) > 0.3


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).double().numpy()


def test_float32_sequential_accumulation_stays_inside_the_bound():
    """A numpy float32 accumulation of random bf16 products, in 32-product blocks then split-K slabs, against chain_depth."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for k, slabs in ((32, 1), (512, 1), (7744, 16), (7744, 4), (400 * 64, 64)):
        a = _bf16(rng.normal(size=(64, k)) * np.exp(rng.normal(size=(64, k))))
        b = _bf16(rng.normal(size=k))
        per = -(-k // (32 * slabs)) * 32  # slabs of whole K steps
        out = np.zeros(64, np.float32)
        for s in range(slabs):
            acc = np.zeros(64, np.float32)
            for k0 in range(s * per, min(k, (s + 1) * per), 32):
                blk = (a[:, k0 : k0 + 32] * b[k0 : k0 + 32]).astype(np.float32)  # bf16 products: exact in float32
                t = np.zeros(64, np.float32)
                for j in range(blk.shape[1]):
                    t = (t + blk[:, j]).astype(np.float32)
                acc = (acc + t).astype(np.float32)
            out = (out + acc).astype(np.float32)
        want = a @ b
        S = np.abs(a) @ np.abs(b)
        r = np.abs(out.astype(np.float64) - want) / (M.U * S)
        worst = max(worst, float(r.max()))
        assert np.all(np.abs(out - want) <= M.bound(S, M.chain_depth(k, slabs=slabs)))
    assert worst < 64  # a sequential fp32 chain stays far inside its worst case


def test_negative_control_tells_one_pass_from_three():
    """The same operands at 1 and 3 passes: each model's result is inside its own bound with a float32 accumulation and the
    other model breaks that bound on most elements (forward shapes: K = 256 .. 7744)."""
    rng = np.random.default_rng(3)
    for k in (256, 576, 7744):
        x = torch.from_numpy((rng.normal(size=(48, k)) * (rng.random((48, k)) < 0.6)).astype(np.float32))
        w = torch.from_numpy((rng.normal(size=(k, 40)) / np.sqrt(k)).astype(np.float32))
        xs, ws = M.split(x), M.split(w)
        v1, S1 = M.dense(1, xs, ws)
        v3, S3 = M.dense(3, xs, ws)
        c = M.chain_depth(k, slabs=4)
        # a float32 run of each: the products of the pass summed in float32
        for own, other, S in ((v1, v3, S1), (v3, v1, S3)):
            got = torch.from_numpy(own.numpy().astype(np.float32).astype(np.float64))
            used, ratio, frac = M.check(got, own, M.bound(S, c), S, other, label=f"k={k}")
            assert frac >= 0.5
        # the two-pass form with an exact operand is the three-pass one without the exact operand's lo
        px = (torch.from_numpy(rng.integers(0, 256, (8, k)).astype(np.float64)), None)
        v2, _ = M.dense(2, (ws[0].T, ws[1].T), (px[0].T, None))
        v3x, _ = M.dense(3, (ws[0].T, ws[1].T), (px[0].T, None))
        assert torch.equal(v2, v3x)


def test_ln_relu_backward_matches_autograd():
    rng = np.random.default_rng(4)
    z = torch.from_numpy(rng.normal(size=(6, 5, 64)) * 3 + 1)
    gamma = torch.from_numpy(rng.normal(size=64))
    beta = torch.from_numpy(rng.normal(size=64))
    da = torch.from_numpy(rng.normal(size=(6, 5, 64)))
    zz = z.clone().requires_grad_(True)
    mean = zz.mean(-1, keepdim=True)
    var = ((zz * zz).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
    y = (zz - mean) * torch.rsqrt(var + M.LN_EPS) * gamma + beta
    mask = (y > 0).double().detach()
    (torch.relu(y) * da).sum().backward()
    dz, E = M.ln_relu_bwd(z, gamma, mask, da, torch.zeros_like(da))
    assert torch.allclose(dz, zz.grad, rtol=1e-12, atol=1e-12)
    assert bool((E > 0).all())
