"""numpy restatement of the random-shift augmentation, written from the header text alone (include/isdqn_hip.h,
isdqn_replay_augment_shift):

    t, b     = count + r // rows_per_step,  r % rows_per_step;   half = 0 (state stack) / 1 (next-state stack)
    x        = Philox4x32-10(ctr = {b, 0x80000000 | half, lo32(t), hi32(t)}, key = {lo32(seed), hi32(seed)})
    dx, dy   = ((x0 * (2 pad + 1)) >> 32) - pad,  ((x1 * (2 pad + 1)) >> 32) - pad
    out[y, x] = in[clamp(y + dy, 0, h-1), clamp(x + dx, 0, w-1)]            one draw per (row, half): all `stack` frames share it
    id >= 0 at (r, k) -> r * 2 stack + k and that pool frame written;  id -1 stays -1, its pool frame untouched

the wrong readings the tests must be able to tell from it, and the ramp frames from which a shift can be read back."""
import numpy as np

from tests.helpers.noisy import philox4x32_10

VARIANTS = ("right", "per_frame", "same_halves", "swapped", "zero_pad", "flipped")


def draws(n_rows, rows_per_step, pad, seed, count):
    """(dy, dx), each int64 [n_rows][2]: the shifts of the two halves of every row."""
    r = np.arange(n_rows, dtype=np.int64)
    t = int(count) + r // rows_per_step
    b = r % rows_per_step
    out = np.zeros((2, n_rows, 2), np.int64)
    for half in (0, 1):
        x = philox4x32_10([b, 0x80000000 | half, t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
        out[1, :, half] = ((x[0].astype(np.uint64) * np.uint64(2 * pad + 1)) >> np.uint64(32)).astype(np.int64) - pad  # dx
        out[0, :, half] = ((x[1].astype(np.uint64) * np.uint64(2 * pad + 1)) >> np.uint64(32)).astype(np.int64) - pad  # dy
    return out[0], out[1]


def shift_frame(img, dy, dx, zero_pad=False):
    """out[y, x] = img[clamp(y + dy), clamp(x + dx)] (zero_pad: 0 where the source leaves the frame -- a wrong reading)."""
    h, w = img.shape
    ys, xs = np.arange(h) + int(dy), np.arange(w) + int(dx)
    out = img[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]
    if zero_pad:
        out = out * (((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]).astype(img.dtype)
    return out


def shift_by_pad_and_crop(img, dy, dx, pad):
    """The independent formulation: replicate-pad by `pad`, crop h x w at offset (pad + dy, pad + dx)."""
    h, w = img.shape
    big = np.pad(img, pad, mode="edge")
    return big[pad + dy : pad + dy + h, pad + dx : pad + dx + w]


def augment(frames, h, w, stack, ids, rows_per_step, pad, seed, count, pool=None, variant="right"):
    """frames: uint8 [n_frames][frame_stride]; ids: int32 [n_rows][2*stack].  Returns (pool [n_rows*2*stack][frame_stride], out_ids,
    count behind the call).  `pool`: what the scratch pool held before (bytes the call does not write keep it); default zeros."""
    assert variant in VARIANTS
    n_rows, s2 = ids.shape
    assert s2 == 2 * stack and n_rows % rows_per_step == 0
    stride = frames.shape[1]
    pool = np.zeros((n_rows * s2, stride), np.uint8) if pool is None else pool.copy()
    out_ids = np.full_like(ids, -1)
    dy, dx = draws(n_rows, rows_per_step, pad, seed, count)
    for r in range(n_rows):
        for k in range(s2):
            if ids[r, k] < 0:
                continue
            half = k // stack
            y, x = int(dy[r, half]), int(dx[r, half])
            if variant == "per_frame":  # one shift per frame instead of per stack: a draw of its own at the frame's position
                fy, fx = draws(n_rows * s2, rows_per_step * s2, pad, seed, count)
                y, x = int(fy[r * s2 + k, 0]), int(fx[r * s2 + k, 0])
            elif variant == "same_halves":
                y, x = int(dy[r, 0]), int(dx[r, 0])
            elif variant == "swapped":
                y, x = x, y
            elif variant == "flipped":
                y, x = -y, -x
            img = frames[ids[r, k], : h * w].reshape(h, w)
            pool[r * s2 + k, : h * w] = shift_frame(img, y, x, zero_pad=variant == "zero_pad").reshape(-1)
            out_ids[r, k] = r * s2 + k
    return pool, out_ids, int(count) + n_rows // rows_per_step


def stacks(pool, ids, h, w, stack):
    """The reference-layout (n_rows, h, w, stack) state / next-state arrays of a pool + table (-1: the zero frame)."""
    n_rows = ids.shape[0]
    out = np.zeros((2, n_rows, h, w, stack), np.uint8)
    for r in range(n_rows):
        for k in range(2 * stack):
            if ids[r, k] >= 0:
                out[k // stack, r, :, :, k % stack] = pool[ids[r, k], : h * w].reshape(h, w)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------- ramps: a shift read back from the output
def ramp_frames(n_frames, h, w, stride=None):
    """Frame f holds f(frame, y, x) = (f + 16 y + x) mod 256 with h, w <= 16 interior: inside the frame the value names (y, x) up to the
    frame's own offset, so the shift of an output frame can be read back from its pixels (needs h <= 15, w <= 15: no wrap inside)."""
    assert h <= 15 and w <= 15
    stride = h * w if stride is None else stride
    out = np.zeros((n_frames, stride), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    for f in range(n_frames):
        out[f, : h * w] = ((f + 16 * y + x) % 256).astype(np.uint8).reshape(-1)
    return out


def ramp_case(n_rows=6, h=11, w=13, stack=3, pad=4, n_frames=40):
    """(frames, ids, h, w, stack, pad) of the property test: ramp frames with one spare byte per frame, two -1 ids; h, w > 2 pad, so every
    shift in range gives a different frame."""
    frames = ramp_frames(n_frames, h, w, stride=h * w + 1)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, n_frames, (n_rows, 2 * stack)).astype(np.int32)
    ids[0, 1] = ids[3, stack] = -1
    return frames, ids, h, w, stack, pad


def read_shift(out_img, frame, h, w, pad):
    """The unique (dy, dx) in [-pad, pad]^2 for which replicate-shifting ramp frame `frame` gives out_img, or None."""
    y, x = np.mgrid[0:h, 0:w]
    src = ((frame + 16 * y + x) % 256).astype(np.uint8)
    found = [(dy, dx) for dy in range(-pad, pad + 1) for dx in range(-pad, pad + 1) if np.array_equal(shift_frame(src, dy, dx), out_img)]
    return found[0] if len(found) == 1 else None


def check_ramp_properties(pool, out_ids, ids, h, w, stack, pad, expect_dy=None, expect_dx=None):
    """The property test on ramp frames, from the output alone: every written frame is a replicate shift of its source by a readable
    (dy, dx) in [-pad, pad]^2; the `stack` frames of a half share it; over all rows the two halves do not always agree and dy is not
    always dx.  With expect_dy / expect_dx ([n_rows][2]) the read shifts must equal them (sign and axis).  Returns a list of failures
    (empty: all hold)."""
    fails = []
    n_rows = ids.shape[0]
    read = np.full((n_rows, 2, 2), 10**6, np.int64)
    for r in range(n_rows):
        for half in (0, 1):
            seen = set()
            for c in range(stack):
                k = half * stack + c
                if ids[r, k] < 0:
                    if out_ids[r, k] != -1:
                        fails.append(f"row {r} pos {k}: -1 did not stay -1")
                    continue
                if out_ids[r, k] != r * 2 * stack + k:
                    fails.append(f"row {r} pos {k}: id {out_ids[r, k]}")
                    continue
                s = read_shift(pool[out_ids[r, k], : h * w].reshape(h, w), int(ids[r, k]), h, w, pad)
                if s is None:
                    fails.append(f"row {r} pos {k}: no replicate shift in range gives this frame")
                else:
                    seen.add(s)
            if len(seen) > 1:
                fails.append(f"row {r} half {half}: frames of one stack moved differently: {sorted(seen)}")
            if len(seen) == 1:
                read[r, half] = seen.pop()
    ok = (read[:, :, 0] < 10**6).all(axis=1)
    if ok.any() and pad > 0:
        if (read[ok, 0] == read[ok, 1]).all():
            fails.append("both halves moved alike in every row")
    if expect_dy is not None:
        for r in range(n_rows):
            for half in (0, 1):
                if read[r, half, 0] < 10**6 and (read[r, half, 0], read[r, half, 1]) != (expect_dy[r, half], expect_dx[r, half]):
                    fails.append(f"row {r} half {half}: moved by {tuple(read[r, half])}, the draw is {(expect_dy[r, half], expect_dx[r, half])}")
    return fails
