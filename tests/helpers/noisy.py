"""numpy / float64 restatement of the noisy Dense layers, written from the header text alone (include/isdqn_hip.h, isdqn_noisy_layout):

    x        = Philox4x32-10(ctr = {j, (stream_id << 16) | (2 l + v), lo32(count), hi32(count)}, key = {lo32(seed), hi32(seed)})
    u1, u2   = ((x0 >> 8) + 1/2) 2^-24,  (x1 >> 8) 2^-24
    z        = sqrt(-2 ln u1) cos(2 pi u2),      f(z) = sign(z) sqrt|z|
    eff      = mu + fl32(sigma * fl32(eout[o] * ein[i]))   on a Dense kernel,   mu + fl32(sigma_b[o] * eout[o]) on a Dense bias
    g_sigma  = fl32(g * n)

and the wrong readings the tests must be able to tell from it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two.  Returns the four output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def words(n, layer, vec, seed, count, stream_id):
    """(x0, x1) of elements 0 .. n-1 of vector `vec` (0 = in, 1 = out) of noisy layer `layer`."""
    x = philox4x32_10([np.arange(n), (stream_id << 16) | (2 * layer + vec), count & 0xFFFFFFFF, (count >> 32) & 0xFFFFFFFF],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return x[0], x[1]


def uniforms(x0, x1):
    u1 = ((x0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0**-24
    u2 = (x1 >> np.uint32(8)).astype(np.float64) * 2.0**-24
    return u1, u2


def normal(x0, x1):
    """(z, r) in float64: the standard normal and the Box-Muller radius sqrt(-2 ln u1)."""
    u1, u2 = uniforms(x0, x1)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r


def f(z):
    return np.copysign(np.sqrt(np.abs(z)), z)


def sample_vector(n, layer, vec, seed, count, stream_id):
    """float64 f(z) of one noise vector and (z, r) for the error bound."""
    z, r = normal(*words(n, layer, vec, seed, count, stream_id))
    return f(z), z, r


def sample_all(layout, seed, count, stream_id):
    """The whole noise buffer in float64 for `layout` = [(offset of ein, in_p, out_p), ...]; also z and r at the same positions."""
    total = max(off + i + o for off, i, o in layout)
    out, zs, rs = np.zeros(total), np.zeros(total), np.zeros(total)
    for l, (off, n_in, n_out) in enumerate(layout):
        for vec, (a, n) in enumerate(((off, n_in), (off + n_in, n_out))):
            out[a:a + n], zs[a:a + n], rs[a:a + n] = sample_vector(n, l, vec, seed, count, stream_id)
    return out, zs, rs


# ---- compose and gradients on one Dense layer: kernel [out][in] (the internal orientation), bias [out]
def factors(ein, eout):
    """n of the kernel in fp32: one rounded product per element."""
    return np.float32(eout)[:, None] * np.float32(ein)[None, :]


def compose_kernel(mu, sigma, ein, eout):
    """fp32, in the header's order: n = eout * ein, t = sigma * n, eff = mu + t (every step rounded)."""
    t = np.float32(sigma) * factors(ein, eout)
    return np.float32(mu) + t


def compose_bias(mu, sigma, eout):
    return np.float32(mu) + np.float32(sigma) * np.float32(eout)


def g_sigma_kernel(g, ein, eout):
    return np.float32(g) * factors(ein, eout)


def g_sigma_bias(g, eout):
    return np.float32(g) * np.float32(eout)


def adam64(p0, m0, v0, g, t, lr, eps, b1=float(np.float32(0.9)), b2=float(np.float32(0.999))):
    """float64 Adam (optax.adam's expression order); `t` is the step count after the increment.  Returns p, m, v."""
    p0, m0, v0, g = (np.asarray(a, np.float64) for a in (p0, m0, v0, g))
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * (g * g)
    return p0 - lr * (m / (1 - b1**t)) / (np.sqrt(v / (1 - b2**t)) + eps), m, v


def noisy_step64(mu, sigma, state, g, n, t, lr, eps):
    """float64 Adam on both buffers of one tensor from one gradient: mu from g, sigma from fl32(g * n).  `state` = (m_mu, v_mu, m_s, v_s)."""
    gs = (np.float32(g) * np.float32(n)).astype(np.float64)
    mu1, mm, vm = adam64(mu, state[0], state[1], g, t, lr, eps)
    s1, ms, vs = adam64(sigma, state[2], state[3], gs, t, lr, eps)
    return mu1, s1, (mm, vm, ms, vs)


# ---- wrong readings
def compose_kernel_no_f(mu, sigma, zin, zout):
    """the raw normals multiplied, f never applied (zin / zout: the z behind ein / eout)"""
    return compose_kernel(mu, sigma, zin, zout)


def compose_kernel_swapped(mu, sigma, ein, eout):
    """ein indexes the rows and eout the columns (needs a square layer, or compares the overlapping corner)"""
    o, i = np.shape(mu)
    e_in = np.resize(np.float32(ein), o)
    e_out = np.resize(np.float32(eout), i)
    return np.float32(mu) + np.float32(sigma) * (e_in[:, None] * e_out[None, :])


def compose_bias_by_ein(mu, sigma, ein):
    return np.float32(mu) + np.float32(sigma) * np.resize(np.float32(ein), np.shape(mu))


def g_sigma_plain(g, ein, eout):
    """sigma trained with g instead of g * n"""
    return np.float32(g) + np.float32(0) * factors(ein, eout)
