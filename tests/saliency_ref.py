"""numpy references of the perturbation-saliency definitions
(include/dreamer_hip.h "perturbation saliency").

The occluder comes twice: `occlude32` emulates the kernel's f32 arithmetic --
every fmaf as an exact float64 product plus the addend, rounded to f32 once
(the product of two f32 values is exact in float64), every other f32 operation
rounded to f32 -- and `occlude64` evaluates the same formulas in plain float64
on the same f32 tables.  `guarded` marks the pixels whose float64 value lies
within 1e-3 of a half-integer: only there may a u8 level legitimately differ."""
import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays: the float64 product is exact, one rounding to f32."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def centres(n, s):
    return np.arange(n // s) * s + s // 2


def _blur_axis(I, wb, rb, axis, emulate):
    n = I.shape[axis]
    acc = np.zeros(I.shape, dtype=F32 if emulate else F64)
    for k in range(-rb, rb + 1):
        idx = np.clip(np.arange(n) + k, 0, n - 1)
        v = np.take(I, idx, axis=axis)
        w = wb[k + rb]
        if emulate:
            acc = fma32(np.full(v.shape, w, dtype=F32), v.astype(F32), acc)
        else:
            acc = F64(w) * v.astype(F64) + acc
    return acc


def fill_of(frames, fill, wb, rb, emulate):
    """A [F][3][H][W] (f32 when emulating, else float64) of u8 frames [F][3][H][W]."""
    Fn, _, H, W = frames.shape
    if fill == "blur":
        x = frames.astype(F32 if emulate else F64)
        return _blur_axis(_blur_axis(x, wb, rb, 3, emulate), wb, rb, 2, emulate)
    if fill != "mean":
        raise ValueError(fill)
    s = frames.astype(np.int64).sum(axis=(2, 3))  # the exact integer sum
    if emulate:
        a = (s.astype(F32) / F32(H * W)).astype(F32)  # the sums are below 2^24: (float) is exact
    else:
        a = s.astype(F64) / F64(H * W)
    return np.broadcast_to(a[:, :, None, None], frames.shape).copy()


def _masks(H, W, s, gm, dtype):
    """m [G][H][W] = gm[|y - cy|] * gm[|x - cx|] (one multiply in `dtype`)."""
    cy, cx = centres(H, s), centres(W, s)
    g = gm.astype(dtype)
    my = g[np.abs(np.arange(H)[None, :] - cy[:, None])]  # [Gy][H]
    mx = g[np.abs(np.arange(W)[None, :] - cx[:, None])]  # [Gx][W]
    m = (my[:, None, :, None] * mx[None, :, None, :]).astype(dtype)  # [Gy][Gx][H][W]
    return m.reshape(len(cy) * len(cx), H, W)


def values32(frames, s, fill, wb, rb, gm):
    """v [F][G][3][H][W] f32, the kernel's arithmetic: fmaf(m, A - I, I)."""
    A = fill_of(frames, fill, wb, rb, True)
    I = frames.astype(F32)
    D = (A - I).astype(F32)
    m = _masks(frames.shape[2], frames.shape[3], s, gm, F32)
    shape = (frames.shape[0], m.shape[0]) + frames.shape[1:]
    bc = lambda x: np.broadcast_to(x, shape)
    return fma32(bc(m[None, :, None]), bc(D[:, None]), bc(I[:, None]))


def values64(frames, s, fill, wb, rb, gm):
    """The same in plain float64."""
    A = fill_of(frames, fill, wb, rb, False)
    I = frames.astype(F64)
    m = _masks(frames.shape[2], frames.shape[3], s, gm, F64)
    return m[None, :, None] * (A - I)[:, None] + I[:, None]


def quantise(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _with_variant0(frames, q):
    return np.concatenate((frames[:, None], q), axis=1)


def occlude32(frames, s, fill, wb, rb, gm):
    """u8 [F][G+1][3][H][W]: variant 0 the frame, variant 1 + i Gx + j perturbed at cell (i, j)."""
    return _with_variant0(frames, quantise(values32(frames, s, fill, wb, rb, gm)))


def occlude64(frames, s, fill, wb, rb, gm):
    """(u8 [F][G+1][3][H][W] in float64, guarded [F][G+1][3][H][W]: the float64
    value within 1e-3 of a half-integer; never for variant 0)."""
    v = values64(frames, s, fill, wb, rb, gm)
    g = np.abs(v - np.floor(v) - 0.5) <= 1e-3
    return _with_variant0(frames, quantise(v)), np.concatenate((np.zeros_like(g[:, :1]), g), axis=1)


# ---------------------------------------------------------------------- scores
def _log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def scores64(mu, V, logits, z, F, G, R, C):
    """float64 (actor, value, value_delta, posterior_kl) [F][G] and the exact flips, rows f (G + 1) + g."""
    mu = mu.astype(F64).reshape(F, G + 1, -1)
    V = V.astype(F64).reshape(F, G + 1)
    lp = _log_softmax(logits.astype(F64).reshape(F, G + 1, R, C))
    zi = z.reshape(F, G + 1, R, C).argmax(-1)
    actor = 0.5 * ((mu[:, 1:] - mu[:, :1]) ** 2).sum(-1)
    delta = V[:, 1:] - V[:, :1]
    p0 = np.exp(lp[:, :1])
    kl = (p0 * (lp[:, :1] - lp[:, 1:])).sum((-1, -2))
    flips = (zi[:, 1:] != zi[:, :1]).sum(-1).astype(np.int32)
    return actor, 0.5 * delta ** 2, delta, kl, flips


# ------------------------------------------------------------------------- map
def _axis(n, s):
    """(i0, i1, w) of every pixel along a side of n pixels, the kernel's f32 arithmetic."""
    Gn = n // s
    fp = np.minimum(np.maximum(((np.arange(n) - s // 2).astype(F32) / F32(s)).astype(F32), F32(0)), F32(Gn - 1))
    i0 = np.floor(fp).astype(np.int64)
    return i0, np.minimum(i0 + 1, Gn - 1), (fp - np.floor(fp)).astype(F32)


def map64(scores, scale, H, W, s):
    """map [F][H][W] in float64 from the f32 weights the kernel forms (they are exact: s is small)."""
    i0, i1, wy = _axis(H, s)
    j0, j1, wx = _axis(W, s)
    S = scores.astype(F64)
    wy, wx = wy.astype(F64)[:, None], wx.astype(F64)[None, :]
    g = lambda a, b: S[:, a[:, None], b[None, :]]
    bl = (1 - wy) * (1 - wx) * g(i0, j0) + (1 - wy) * wx * g(i0, j1) + wy * (1 - wx) * g(i1, j0) + wy * wx * g(i1, j1)
    return scale.astype(F64)[:, None, None] * bl


def overlay_values(m, frames, ch):
    """(f32-emulated, float64) values [F][H][W] of the overlay's channel ch for a map m (f32 [F][H][W])."""
    heat = np.minimum(F32(1), np.maximum(F32(0), m.astype(F32)))
    I = frames[:, ch].astype(F32)
    v32 = fma32(heat, (F32(255) - I).astype(F32), I)
    v64 = heat.astype(F64) * (255.0 - I.astype(F64)) + I.astype(F64)
    return v32, v64
