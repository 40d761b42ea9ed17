"""Float64 numpy reference of the sampled-futures metrics (include/dreamer_hip.h
"sampled futures": dr_frame_ssim, dr_ensemble_metrics; dreamer_amd/futures.py),
and their transcription in f32 (one rounding per operation, numpy does not
contract): the yardstick the kernels' error is held against.

SSIM is written non-separably here -- a direct 11 x 11 weighted sum per
position with the weights w_i w_j -- so it states the definition independently
of the kernel's two passes; the f32 transcription follows the header's order
(along W, then along H, taps ascending)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 2.0 ** -24
C1, C2 = 1e-4, 9e-4


def bound(yardstick, cap=1e-4):
    """DESIGN 5h's rule: 8 x the f32 transcription's error, at least 4 x 2^-24,
    at most `cap` (None: no cap -- dr_frame_ssim)."""
    b = max(8.0 * yardstick, 4.0 * U)
    return b if cap is None else min(b, cap)


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|) in float64."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def window():
    """The f32 window: g_k = exp(-(k - 5)^2 / 4.5) normalised in double, rounded to f32 once."""
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / 4.5)
    return (g / g.sum()).astype(np.float32)


def x_of_u8(u8):
    """True value of a stored pixel: (float)u8 / 255.0f - 0.5f, this f32 expression."""
    return np.asarray(u8).astype(np.float32) / np.float32(255.0) - np.float32(0.5)


def clamp(mu):
    return np.minimum(np.float32(0.5), np.maximum(np.float32(-0.5), np.asarray(mu, np.float32)))


def ssim_ref(mu, x):
    """mu (raw prediction), x (true values) [..., 3, H, W] -> (ssim [...], ssim_ch [..., 3]) in float64."""
    p = clamp(mu).astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    w = window().astype(np.float64)
    w2 = np.outer(w, w)

    def filt(a):
        return np.einsum("...ij,ij->...", sliding_window_view(a, (11, 11), axis=(-2, -1)), w2)

    mp, mx = filt(p), filt(x)
    vp, vx, c = filt(p * p) - mp * mp, filt(x * x) - mx * mx, filt(p * x) - mp * mx
    up, ux = mp + 0.5, mx + 0.5
    smap = ((2 * up * ux + C1) * (2 * c + C2)) / ((up * up + ux * ux + C1) * (vp + vx + C2))
    ch = smap.mean(axis=(-2, -1))
    return ch.mean(axis=-1), ch


def ssim_f32(mu, x):
    """The header's order of operations in f32: the yardstick."""
    f = np.float32
    p = clamp(mu)
    x = np.asarray(x, f)
    w = window()
    H, W = p.shape[-2:]

    def filt(a):
        s = np.zeros(a.shape[:-1] + (W - 10,), f)
        for k in range(11):
            s = s + w[k] * a[..., k:k + W - 10]
        o = np.zeros(a.shape[:-2] + (H - 10, W - 10), f)
        for k in range(11):
            o = o + w[k] * s[..., k:k + H - 10, :]
        return o

    mp, mx = filt(p), filt(x)
    vp, vx, c = filt(p * p) - mp * mp, filt(x * x) - mx * mx, filt(p * x) - mp * mx
    up, ux = mp + f(0.5), mx + f(0.5)
    num = (f(2) * up * ux + f(C1)) * (f(2) * c + f(C2))
    den = (up * up + ux * ux + f(C1)) * (vp + vx + f(C2))
    smap = num / den
    ch = smap.reshape(*smap.shape[:-2], -1).sum(-1, dtype=f) / f((H - 10) * (W - 10))
    return ((ch[..., 0] + ch[..., 1]) + ch[..., 2]) / f(3), ch


def ensemble_ref(mu, x, dtype=np.float64):
    """mu [B][M][T][n] f32, x [B][T][n] f32 -> dict of sqerr_mean [B][T], spread
    [B][T], mean [B][T][n], var [B][T][n], sqerr [B][M][T] in `dtype` (float64:
    the reference; float32: the yardstick, m ascending as the kernel)."""
    mu = np.asarray(mu, np.float32).astype(dtype)
    x = np.asarray(x, np.float32).astype(dtype)
    M = mu.shape[1]
    s = np.zeros_like(mu[:, 0])
    for m in range(M):
        s = s + mu[:, m]
    mean = s / dtype(M)
    v = np.zeros_like(mean)
    for m in range(M):
        dv = mu[:, m] - mean
        v = v + dv * dv
    var = v / dtype(M)
    d = mean - x
    return dict(sqerr_mean=(d * d).sum(-1, dtype=dtype), spread=var.sum(-1, dtype=dtype), mean=mean, var=var,
                sqerr=((mu - x[:, None]) ** 2).sum(-1, dtype=dtype))


def quant(mean32):
    """(u8) min(255, max(0, rintf((mean + 0.5f) * 255.0f))) in f32 (np.rint: half to even)."""
    f = np.float32
    v = np.rint((np.asarray(mean32, f) + f(0.5)) * f(255.0))
    return np.minimum(f(255.0), np.maximum(f(0.0), v)).astype(np.uint8)


def quant_std(var32):
    """(u8) min(255, rintf(255.0f * sqrtf(var))) in f32."""
    f = np.float32
    return np.minimum(f(255.0), np.rint(f(255.0) * np.sqrt(np.asarray(var32, f)))).astype(np.uint8)


def best_ref(sqerr):
    """sqerr [B][M][K]: per window the first sample attaining the smallest sum over k >= 1."""
    out = []
    for row in np.asarray(sqerr)[:, :, 1:].sum(-1):
        best = 0
        for m in range(1, len(row)):
            if row[m] < row[best]:
                best = m
        out.append(best)
    return np.asarray(out, np.int64)


def coverage_ref(mu, x):
    """mu [B][M][K][...], x [B][K][...]: per step k the share of x inside [min_m mu, max_m mu]."""
    mu, x = np.asarray(mu), np.asarray(x)
    inside = (mu.min(1) <= x) & (x <= mu.max(1))
    return inside.reshape(inside.shape[0], inside.shape[1], -1).mean(axis=(0, 2))
