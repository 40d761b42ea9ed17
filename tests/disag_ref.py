"""References of the latent-disagreement ensemble (dreamer_amd/csrc/disag.hip, networks.DisagreementEnsemble), written
from the definitions in numpy and evaluated in float64 (the reference) or float32 (what a correct f32 implementation
may give: the tolerances of tests/disag_cases.py must admit it):

  member k:  p1 = h W0_k^T + b0_k;  x1 = SiLU(LN(p1; g1_k, be1_k));  p2 = x1 W3_k^T + b3_k;  x2 = SiLU(LN(p2; g4_k, be4_k))
             pred_k = x2 W6_k^T + b6_k                       (LayerNorm eps 1e-5, biased variance)
  loss_k = mean over rows and columns of (pred_k - z)^2,  loss = mean_k loss_k
  d[m]   = mean_j sqrt(mean_k (pred_kmj - mean_k pred_kmj)^2)   (population std over the members)

Parameters are the module's stacked arrays: l0_weight (K W, Hd), l0_bias (K W), n1_weight / n1_bias (K, W), l3_weight
(K, W, W), l3_bias (K, W), n4_weight / n4_bias (K, W), l6_weight (K, L, W), l6_bias (K, L)."""
import numpy as np

NAMES = ("l0_weight", "l0_bias", "n1_weight", "n1_bias", "l3_weight", "l3_bias", "n4_weight", "n4_bias", "l6_weight",
         "l6_bias")
U = 2.0 ** -24
DG_VAR, DG_MSE = 0, 1  # op codes of dr_internal_disag_run (disag.hip DG_*)


def shapes(K, W, Hd, L):
    return dict(l0_weight=(K * W, Hd), l0_bias=(K * W,), n1_weight=(K, W), n1_bias=(K, W), l3_weight=(K, W, W),
                l3_bias=(K, W), n4_weight=(K, W), n4_bias=(K, W), l6_weight=(K, L, W), l6_bias=(K, L))


def cast(P, dt):
    return {k: np.asarray(v, dtype=dt) for k, v in P.items()}


def _ln(x, g, b):
    dt = x.dtype
    mean = x.mean(-1, keepdims=True, dtype=dt)
    c = x - mean
    var = (c * c).mean(-1, keepdims=True, dtype=dt)
    rstd = (1.0 / np.sqrt(var + dt.type(1e-5))).astype(dt)
    xh = c * rstd
    return xh * g + b, xh, rstd


def _silu(y):
    return y / (1.0 + np.exp(-y))


def forward(P, h):
    """The members' forward in h's dtype: a dict with pred (K, M, L) and what the backward needs."""
    dt = h.dtype
    P = cast(P, dt)
    K, W = P["n1_weight"].shape
    M = h.shape[0]
    p1 = (h @ P["l0_weight"].T + P["l0_bias"]).reshape(M, K, W).transpose(1, 0, 2)  # (K, M, W)
    y1, xh1, r1 = _ln(p1, P["n1_weight"][:, None, :], P["n1_bias"][:, None, :])
    x1 = _silu(y1)
    p2 = np.einsum("kmw,kvw->kmv", x1, P["l3_weight"]) + P["l3_bias"][:, None, :]
    y2, xh2, r2 = _ln(p2, P["n4_weight"][:, None, :], P["n4_bias"][:, None, :])
    x2 = _silu(y2)
    pred = np.einsum("kmw,klw->kml", x2, P["l6_weight"]) + P["l6_bias"][:, None, :]
    return dict(p1=p1, y1=y1, xh1=xh1, r1=r1, x1=x1, p2=p2, y2=y2, xh2=xh2, r2=r2, x2=x2, pred=pred)


def disagreement(pred):
    """(K, M, L) -> (M,): the definition (mean over the members, deviations, biased variance)."""
    mu = pred.mean(0, keepdims=True, dtype=pred.dtype)
    c = pred - mu
    return np.sqrt((c * c).mean(0, dtype=pred.dtype)).mean(-1, dtype=pred.dtype)


def disagreement_shifted(pred):
    """The same in the form the kernel takes (include/dreamer_hip.h): deviations from member 0 minus their mean.  In
    f32 it is exactly 0 where the members agree, whatever K (dividing a sum of K equal values by K need not give the
    value back; a sum of K zeros does).  The deviations are scaled by a power of two (exact) so that their largest is
    in [1, 2) before they are squared: the squares of 1e-20 would fall below the f32 normals."""
    dt = pred.dtype
    dev = pred - pred[0:1]
    c = dev - dev.sum(0, keepdims=True, dtype=dt) / dt.type(pred.shape[0])
    amax = np.abs(c).max(0)
    e = np.where(np.isfinite(amax) & (amax > 0), np.frexp(amax)[1] - 1, 0).astype(np.int32)
    r = np.ldexp(c, -e[None]).astype(dt)
    std = np.ldexp(np.sqrt((r * r).sum(0, dtype=dt) / dt.type(pred.shape[0])), e).astype(dt)
    return std.mean(-1, dtype=dt)


def losses(pred, z):
    """[loss, loss_0 .. loss_{K-1}] in pred's dtype."""
    dt = pred.dtype
    d = pred - z[None].astype(dt)
    lk = (d * d).mean((1, 2), dtype=dt)
    return np.concatenate([[lk.mean(dtype=dt)], lk]).astype(dt)


def mse_grad(pred, z):
    K, M, L = pred.shape
    return (pred - z[None].astype(pred.dtype)) * pred.dtype.type(2.0 / (K * M * L))


def _ln_silu_bwd(gx, y, xh, rstd, g):
    sg = 1.0 / (1.0 + np.exp(-y))
    gy = gx * (sg * (1.0 + y * (1.0 - sg)))
    gxh = gy * g
    dt = gx.dtype
    c1 = gxh.mean(-1, keepdims=True, dtype=dt)
    c2 = (gxh * xh).mean(-1, keepdims=True, dtype=dt)
    return rstd * (gxh - c1 - xh * c2), gy


def grads(P, h, z):
    """(losses (1 + K,), {name: gradient of the total loss}) in h's dtype; no input gradient exists."""
    dt = h.dtype
    P = cast(P, dt)
    f = forward(P, h)
    K, W = P["n1_weight"].shape
    g = mse_grad(f["pred"], z)
    G = {}
    G["l6_weight"] = np.einsum("kml,kmw->klw", g, f["x2"])
    G["l6_bias"] = g.sum(1, dtype=dt)
    gx2 = np.einsum("kml,klw->kmw", g, P["l6_weight"])
    gp2, gy2 = _ln_silu_bwd(gx2, f["y2"], f["xh2"], f["r2"], P["n4_weight"][:, None, :])
    G["n4_weight"] = (gy2 * f["xh2"]).sum(1, dtype=dt)
    G["n4_bias"] = gy2.sum(1, dtype=dt)
    G["l3_weight"] = np.einsum("kmv,kmw->kvw", gp2, f["x1"])
    G["l3_bias"] = gp2.sum(1, dtype=dt)
    gx1 = np.einsum("kmv,kvw->kmw", gp2, P["l3_weight"])
    gp1, gy1 = _ln_silu_bwd(gx1, f["y1"], f["xh1"], f["r1"], P["n1_weight"][:, None, :])
    G["n1_weight"] = (gy1 * f["xh1"]).sum(1, dtype=dt)
    G["n1_bias"] = gy1.sum(1, dtype=dt)
    G["l0_weight"] = np.einsum("kmw,mh->kwh", gp1, h).reshape(K * W, -1)
    G["l0_bias"] = gp1.sum(1, dtype=dt).reshape(K * W)
    return losses(f["pred"], z), {k: G[k].astype(dt) for k in NAMES}


class AdamW:
    """torch.optim.AdamW (single-tensor op order) after clip_grad_norm_(max_norm) over all gradients, as
    DisagreementEnsemble.train_step applies it: no update when a gradient is non-finite."""

    def __init__(self, P, lr, betas=(0.9, 0.999), eps=1e-5, weight_decay=1e-6, max_norm=100.0):
        self.lr, self.b1, self.b2, self.eps, self.wd, self.max_norm = lr, betas[0], betas[1], eps, weight_decay, max_norm
        self.m = {k: np.zeros_like(v) for k, v in P.items()}
        self.v = {k: np.zeros_like(v) for k, v in P.items()}
        self.t = 0
        self.skipped = 0

    def step(self, P, G):
        dt = next(iter(P.values())).dtype
        if not all(np.isfinite(G[k]).all() for k in NAMES):
            self.skipped += 1
            return P
        sq = sum(float((G[k].astype(np.float64) ** 2).sum()) for k in NAMES)
        clip = dt.type(min(1.0, self.max_norm / (np.sqrt(sq) + 1e-6)))
        self.t += 1
        step_size = dt.type(self.lr / (1.0 - self.b1 ** self.t))
        bc2 = dt.type(np.sqrt(1.0 - self.b2 ** self.t))
        out = {}
        for k in NAMES:
            g = G[k] * clip
            p = P[k] * dt.type(1.0 - self.lr * self.wd)
            self.m[k] = self.m[k] * dt.type(self.b1) + g * dt.type(1.0 - self.b1)
            self.v[k] = self.v[k] * dt.type(self.b2) + g * g * dt.type(1.0 - self.b2)
            denom = np.sqrt(self.v[k]) / bc2 + dt.type(self.eps)
            out[k] = (p - step_size * (self.m[k] / denom)).astype(dt)
        return out


def train(P, h, z, steps, lr, dt=np.float64, **kw):
    """`steps` train_steps on the same rows: (parameters, [loss per step], the optimiser)."""
    P = cast(P, dt)
    h, z = h.astype(dt), z.astype(dt)
    opt = AdamW(P, lr, **kw)
    hist = []
    for _ in range(steps):
        ls, G = grads(P, h, z)
        hist.append(float(ls[0]))
        P = opt.step(P, G)
    return P, hist, opt


# ----------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def var_bound(pred):
    """|d - ref| of k_disag_var, derived from its geometry (a wave per row: a lane adds ceil(L / 64) column stds in
    ascending order, wave_sum adds 7 levels, one division).  Per column, with D = max_k |p_k - p_0|: each deviation
    from member 0 is off by <= u D, their sum (K - 1 adds of partial sums <= K D) and its division by <= u (K + 1) D,
    the centred deviation by <= u (K + 4) D in all; sqrt(mean of squares) is 1-Lipschitz in the max norm of the
    deviations, and forming it (exact power-of-two scaling, K squares and adds, a division, a correctly rounded sqrt)
    adds <= (K / 2 + 2) u std <= (K + 4) u D since std <= 2 D.  So |std_j - ref| <= (2 K + 8) u D_j, and
        |d - ref| <= u [(2 K + 8) mean_j D_j + (ceil(L / 64) + 8) mean_j std_j]  (+ 2^-140: results below the normals)."""
    p = pred.astype(np.float64)
    K, M, L = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.abs(p - p[0:1]).max(0)
        c = p - p.mean(0, keepdims=True)
        std = np.sqrt((c * c).mean(0))
        return U * ((2 * K + 8) * D.mean(-1) + (_cdiv(L, 64) + 8) * std.mean(-1)) + 2.0 ** -140


def mse_bounds(pred, z):
    """(|g - ref| elementwise, |losses - ref| (1 + K,)) of k_disag_mse + k_disag_loss.  g = fl(fl(p - z) fl(scale)): 3
    roundings -> 4 u |g| (+ 2^-149).  A squared difference carries 3 u; a lane adds ceil(L / 64) of them and wave_sum 7
    levels; a thread of the one loss workgroup adds ceil(M / 256) rows, wave_sum 7, the four wave totals 3, the division
    1: |loss_k - ref| <= u (ceil(L / 64) + ceil(M / 256) + 22) loss_k.  The total adds K values and divides:
    + u (K + 1) mean_k loss_k on top of the members' mean bound."""
    p = pred.astype(np.float64)
    K, M, L = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.abs(mse_grad(p, z.astype(np.float64)))
        ls = losses(p, z.astype(np.float64))
    lk = U * (_cdiv(L, 64) + _cdiv(M, 256) + 22) * ls[1:]
    tot = lk.mean() + U * (K + 1) * ls[1:].mean()
    return 4 * U * g + 2.0 ** -149, np.concatenate([[tot], lk])


def _act_bound(pre, e_pre, g, b):
    """First-order |error| of x = SiLU(LN(pre)) given |error| e_pre of pre (float64 arrays, LN over the last axis of
    width W).  LayerNorm: dxh_i = rstd (dp_i - mean(dp) - xh_i mean(xh dp)), so the incoming error gives
    rstd (e_i + mean(e) + |xh_i| mean(|xh| e)); its own f32 evaluation (mean: ceil(W / 64) + 8 adds; centring; the
    variance, rsqrt and product: <= (ceil(W / 64) + 12) u relative) gives rstd (2 u |pre_i| + dmean) + (ceil(W / 64) + 12)
    u |xh_i|.  Affine: |g| times that + 2 u (|xh g| + |b|).  SiLU: slope <= 1.1; evaluated with the hardware exp2 / rcp
    in the GEMM prologue (argument rounding u |y| into the exponential): (8 + 2 |y|) u |x|."""
    W = pre.shape[-1]
    y, xh, rstd = _ln(pre, g, b)
    cw = _cdiv(W, 64)
    dmean = (cw + 8) * U * np.abs(pre).mean(-1, keepdims=True)
    own = rstd * (2 * U * np.abs(pre) + dmean) + (cw + 12) * U * np.abs(xh)
    prop = rstd * (e_pre + e_pre.mean(-1, keepdims=True) + np.abs(xh) * (np.abs(xh) * e_pre).mean(-1, keepdims=True))
    e_y = np.abs(g) * (own + prop) + 2 * U * (np.abs(xh * g) + np.abs(b))
    x = _silu(y)
    return 1.1 * e_y + (8 + 2 * np.abs(y)) * U * np.abs(x)


def _prod_bound(Kdim, absprod, ref):
    """tests/gemm_ref.py f32_bound, in numpy: 2 (K + 4) u (|A| |B| + |bias|) + 2 u |ref|."""
    return 2.0 * (Kdim + 4) * U * absprod + 2.0 * U * np.abs(ref)


def forward_bounds(P, h):
    """(|pred - ref| (K, M, L), |d - ref| (M,)) of dr_disag_fwd against forward() in float64, propagated layer by layer
    to first order -- every f32 product by the project's product bound (gemm_ref.f32_bound), every LN + SiLU by
    _act_bound, an incoming error e through a product as e |W|^T -- and doubled for the terms of second order.
    |d - ref| <= max_kj |pred - ref| over the row (the std over the members is 1-Lipschitz in the max norm, and so is
    the mean over the columns) + var_bound."""
    P = cast(P, np.float64)
    h = h.astype(np.float64)
    f = forward(P, h)
    K, W = P["n1_weight"].shape
    M, Hd = h.shape
    a0 = (np.abs(h) @ np.abs(P["l0_weight"]).T + np.abs(P["l0_bias"])).reshape(M, K, W).transpose(1, 0, 2)
    e1 = _prod_bound(Hd, a0, f["p1"])
    ex1 = _act_bound(f["p1"], e1, P["n1_weight"][:, None, :], P["n1_bias"][:, None, :])
    a3, b3 = np.abs(P["l3_weight"]), np.abs(P["l3_bias"])[:, None, :]
    e2 = _prod_bound(W, np.einsum("kmw,kvw->kmv", np.abs(f["x1"]), a3) + b3, f["p2"]) + np.einsum("kmw,kvw->kmv", ex1, a3)
    ex2 = _act_bound(f["p2"], e2, P["n4_weight"][:, None, :], P["n4_bias"][:, None, :])
    a6, b6 = np.abs(P["l6_weight"]), np.abs(P["l6_bias"])[:, None, :]
    ep = _prod_bound(W, np.einsum("kmw,klw->kml", np.abs(f["x2"]), a6) + b6, f["pred"]) + np.einsum("kmw,klw->kml", ex2, a6)
    ep = 2.0 * ep
    return ep, ep.max((0, 2)) + var_bound(f["pred"])


def loss_bounds(P, h, z):
    """|losses - ref| (1 + K,) of dr_disag_train_grads: (2 |p - z| e + e^2) averaged, e = forward_bounds' |pred - ref|,
    plus mse_bounds' reduction bound."""
    ep, _ = forward_bounds(P, h)
    pred = forward(cast(P, np.float64), h.astype(np.float64))["pred"]
    lk = (2 * np.abs(pred - z[None]) * ep + ep * ep).mean((1, 2))
    return np.concatenate([[lk.mean()], lk]) + mse_bounds(pred, z)[1]
