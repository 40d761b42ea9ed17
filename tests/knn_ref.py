"""float64 numpy references of the k-nearest-neighbour search and the particle-entropy reward (include/dreamer_hip.h,
DESIGN.md 5p), the error bounds the tests hold the kernels to, and f32 evaluations in the kernels' own order.

Bounds (u = 2^-24):
  Gram form      G_mj = (D + c) u (|x|^2 + |y|^2 + 2 sum_i |x_i||y_i|), c = 3.  The tile kernel's dot product and both
                 norms are single k-ascending fmaf chains from 0 (one rounding per column: D roundings each, the
                 zero-staged columns past D add none), then one rounded sum |x|^2 + |y|^2, an exact doubling and one
                 rounded difference: (D + 2) u to first order, c = 3 covers the second-order terms ((1 + u)^(D+2) - 1 <=
                 (D + 3) u for D u < 0.01).  The clamp at 0 only moves a value towards the true one.
  direct form    E_mj = (ceil(D / 64) + 10) u d2_mj.  Per column one rounded difference (relative u, doubled by the
                 square) and one rounded product: 3 u on every non-negative term; a lane adds its ceil(D / 64) terms in
                 order, wave_sum adds 4 DPP levels and 3 row totals: ceil(D / 64) + 7 rounded adds, each relative u on
                 a sum of non-negative terms.  Differences that underflow are outside it (none in the cases).
  entropy        e = log1p(mean sqrt(d2)): sqrt is correctly rounded (relative E / (2 d2) + u), the k_m adds and the
                 division relative (k_m + 1) u, log1pf within 2 ulp; d log1p(d) / dd = 1 / (1 + d) <= 1:
                 |e - e64| <= d (gamma / 2 + (k_m + 2) u) + 3 u e64 with gamma = (ceil(D / 64) + 10) u."""
import numpy as np

U = 2.0 ** -24
GRAM_C = 3
KN_KNN, KN_ENT, KN_PLAN = 0, 1, 2  # ops of dr_internal_knn_run
MAX_K = 32


def finite_rows(a):
    return np.isfinite(a).all(axis=-1)


def eligible(x, y, qg=None, bg=None):
    """[Mq][Nb] bool: bank row finite, and not (both group arrays given and equal groups)."""
    el = np.broadcast_to(finite_rows(y)[None, :], (x.shape[0], y.shape[0])).copy()
    if qg is not None and bg is not None:
        el &= np.asarray(qg)[:, None] != np.asarray(bg)[None, :]
    return el


def dist2(x, y, rows=16):
    """float64 direct-form squared distances [Mq][Nb] (NaN where a row is not finite)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, x.shape[0], rows):
            df = x[i:i + rows, None, :] - y[None, :, :]
            out[i:i + rows] = np.einsum("mjd,mjd->mj", df, df)
    return out


def select(d2, el, k):
    """The k eligible columns of smallest (d2, index) per row of a distance matrix: (d2 [Mq][k], idx [Mq][k]); unfilled
    slots +inf / -1."""
    Mq, Nb = d2.shape
    key = np.where(el, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]  # stable: ties by the smaller index
    dd = np.take_along_axis(key, order, axis=1)
    idx = np.where(np.isfinite(dd), order, -1)
    if k > Nb:
        dd = np.concatenate([dd, np.full((Mq, k - Nb), np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((Mq, k - Nb), -1, dtype=idx.dtype)], axis=1)
    return np.where(idx >= 0, dd, np.inf), idx.astype(np.int32)


def knn(x, y, k, qg=None, bg=None, d2=None):
    """Brute-force eligible k-NN by the direct form in float64.  A non-finite query row: NaN / -1."""
    d2 = dist2(x, y) if d2 is None else d2
    dd, idx = select(np.where(np.isnan(d2), np.inf, d2), eligible(x, y, qg, bg), k)
    bad = ~finite_rows(x)
    dd[bad], idx[bad] = np.nan, -1
    return dd, idx


def entropy(d2, idx):
    """e_m = log1p(mean over the filled slots of sqrt(d2)); 0 with no filled slot, NaN for a NaN row."""
    filled = idx >= 0
    km = filled.sum(axis=1)
    with np.errstate(invalid="ignore"):
        s = np.where(filled, np.sqrt(np.where(filled, d2, 0.0)), 0.0).sum(axis=1)
        e = np.log1p(s / np.maximum(km, 1))
    e[km == 0] = 0.0
    e[np.isnan(d2[:, 0])] = np.nan
    return e


def gram_bound(x, y, c=GRAM_C):
    """G_mj [Mq][Nb] in float64."""
    x, y = np.abs(x.astype(np.float64)), np.abs(y.astype(np.float64))
    D = x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (D + c) * U * ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] + 2.0 * x @ y.T)


def direct_gamma(D):
    return (-(-D // 64) + 10) * U


def direct_bound(d2, D):
    return direct_gamma(D) * d2


def entropy_bound(d2, idx, D):
    filled = idx >= 0
    km = filled.sum(axis=1)
    d = np.where(filled, np.sqrt(np.where(filled, d2, 0.0)), 0.0).sum(axis=1) / np.maximum(km, 1)
    return d * (direct_gamma(D) / 2 + (km + 2) * U) + 3 * U * np.log1p(d)


# --------------------------------------------------------------------------------------------------------------------
# f32 evaluations in the kernels' order
# --------------------------------------------------------------------------------------------------------------------
def _wave_sum32(v):
    """common.h wave_sum on [..., 64] f32: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, then the four
    row totals in order."""
    lane = np.arange(64)
    for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        v = (v + v[..., perm]).astype(np.float32)
    return ((v[..., 0] + v[..., 16]).astype(np.float32) + v[..., 32]).astype(np.float32) + v[..., 48]


def direct32(x, y):
    """sum (x - y)^2 of paired rows x, y [n][D] as k_knn_merge forms it, in f32."""
    n, D = x.shape
    P = -(-D // 64) * 64
    df = np.zeros((n, P), dtype=np.float32)
    df[:, :D] = x.astype(np.float32) - y.astype(np.float32)
    sq = (df * df).astype(np.float32).reshape(n, P // 64, 64)
    acc = np.zeros((n, 64), dtype=np.float32)
    for c in range(P // 64):
        acc = (acc + sq[:, c]).astype(np.float32)
    return _wave_sum32(acc).astype(np.float32)


def _chain32(a, b):
    """k-ascending fmaf chain of a[..., k] b[..., k] from 0 (the f32 product is exact in float64; one rounding per
    step up to the rare double rounding of the float64 sum)."""
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), dtype=np.float32)
    a, b = a.astype(np.float64), b.astype(np.float64)
    for k in range(a.shape[-1]):
        acc = (acc.astype(np.float64) + a[..., k] * b[..., k]).astype(np.float32)
    return acc


def gram32(x, y):
    """The tile kernel's Gram distances [Mq][Nb] in f32: max(0, (|x|^2 + |y|^2) - 2 x.y)."""
    x, y = x.astype(np.float32), y.astype(np.float32)
    xy = _chain32(x[:, None, :], y[None, :, :])
    na, nb = _chain32(x, x), _chain32(y, y)
    d = ((na[:, None] + nb[None, :]).astype(np.float32) - np.float32(2) * xy).astype(np.float32)
    return np.maximum(d, np.float32(0))


def brute(x, y, k, qg=None, bg=None):
    """An independent scalar brute force (python floats, math.fsum) for small cases: (d2, idx) lists."""
    import math
    out_d, out_i = [], []
    for m in range(x.shape[0]):
        if not all(math.isfinite(float(v)) for v in x[m]):
            out_d.append([math.nan] * k)
            out_i.append([-1] * k)
            continue
        cand = []
        for j in range(y.shape[0]):
            if not all(math.isfinite(float(v)) for v in y[j]):
                continue
            if qg is not None and bg is not None and int(qg[m]) == int(bg[j]):
                continue
            cand.append((math.fsum((float(a) - float(b)) ** 2 for a, b in zip(x[m], y[j])), j))
        cand.sort()
        cand = cand[:k] + [(math.inf, -1)] * (k - min(k, len(cand)))
        out_d.append([c[0] for c in cand])
        out_i.append([c[1] for c in cand])
    return np.array(out_d), np.array(out_i, dtype=np.int32)
