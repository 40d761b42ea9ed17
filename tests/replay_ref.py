"""Float64 numpy reference of prioritised replay (include/dreamer_hip.h,
"prioritised replay"): the valid starts, the weights and
probabilities, the draw (np.cumsum in slot order), the priority update and the
per-window score of a world-model step (from oracle.wm_losses' per-step
terms).  Written from the definitions, independently of the kernels."""
import numpy as np


def valid_mask(cap, size, next_idx, S):
    """Slot i is a valid start iff 0 <= i < size - S + 1 and not
    (size == cap and i < next_idx < i + S)."""
    ok = np.zeros(cap, dtype=bool)
    for i in range(cap):
        if not 0 <= i < size - S + 1:
            continue
        if size == cap and i < next_idx < i + S:
            continue
        ok[i] = True
    return ok


def valid_mask_fast(cap, size, next_idx, S):
    i = np.arange(cap, dtype=np.int64)
    ok = i < size - S + 1
    if size == cap:
        ok &= ~((i < next_idx) & (next_idx < i + S))
    return ok


def weights(priority, size, next_idx, S, p_floor):
    """w_i = priority[i] on a valid start (non-finite or <= 0: p_floor), else 0; float64."""
    p = np.asarray(priority, dtype=np.float64)
    cap = len(p)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(p) & (p > 0.0)
    w = np.where(good, p, float(p_floor))
    return np.where(valid_mask_fast(cap, size, next_idx, S), w, 0.0)


def probabilities(priority, size, next_idx, S, p_floor):
    w = weights(priority, size, next_idx, S, p_floor)
    return w / np.cumsum(w)[-1]


def sample(priority, size, next_idx, S, p_floor, u):
    """(starts int64 [B], prob float64 [B], margin float64 [B]): the start of
    draw b is the least valid i with C_i > u_b W (C = np.cumsum(w), W = C[-1]),
    the last valid slot if there is none; margin = min_j |u_b W - C_j| / W."""
    w = weights(priority, size, next_idx, S, p_floor)
    C = np.cumsum(w)
    W = C[-1]
    assert W > 0.0, "no valid start"
    t = np.asarray(u, dtype=np.float64) * W
    idx = np.searchsorted(C, t, side="right")  # the first C_i > t; w_i > 0 there, as C rises at i
    last = int(np.nonzero(w > 0.0)[0][-1])
    starts = np.where(idx >= len(w), last, idx).astype(np.int64)
    hi = np.abs(C[np.minimum(idx, len(w) - 1)] - t)
    lo = np.where(idx > 0, np.abs(t - C[np.maximum(idx - 1, 0)]), np.inf)
    assert np.all(w[starts] > 0.0)
    return starts, w[starts] / W, np.minimum(hi, lo) / W


def update(priority, visits, starts, scores, c, beta, alpha, eps, p_new):
    """(priority float64 [cap], visits int64 [cap]) after a step on `starts`
    with `scores`: visits[s] += rows with start s; priority[s] = c beta^visits[s]
    + (max |L| + eps)^alpha over those rows, p_new if one of them is non-finite."""
    p = np.asarray(priority, dtype=np.float64).copy()
    v = np.asarray(visits, dtype=np.int64).copy()
    starts = np.asarray(starts, dtype=np.int64)
    a = np.abs(np.asarray(scores, dtype=np.float64))
    for s in np.unique(starts):
        rows = a[starts == s]
        v[s] += len(rows)
        p[s] = float(p_new) if not np.all(np.isfinite(rows)) else \
            float(c) * float(beta) ** int(v[s]) + (rows.max() + float(eps)) ** float(alpha)
    return p, v


def window_scores(o, cont, T, betas):
    """L_b (float64 [B]), pred_b, kl_b and the per-window mask sums from the
    per-step terms of oracle.wm_losses' result `o` (obs_ll, rew_ll, cont_ll,
    prior, post over steps 1 .. T-1) and the windows' continues (B, S, 1):
    pred_b = sum_t m (sqerr - rew_ll + cont_bce) / (sum_t m + 1e-5),
    kl_b = 1/(T-1) sum_t m sum_g KL, L_b = beta_pred pred_b + (beta_dyn + beta_rep) kl_b
    (no free-bit clamp)."""
    f = lambda t: t.detach().double().numpy()
    m = f(cont)[:, :T - 1, 0]
    sq = -f(o["obs_ll"])
    rew = f(o["rew_ll"])[..., 0]
    bce = f(o["cont_ll"])[..., 0]
    post, prior = f(o["post"]), f(o["prior"])
    lse = lambda x: x - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)) - x.max(-1, keepdims=True)
    lp, lq = lse(post), lse(prior)
    kl = (np.exp(lp) * (lp - lq)).sum(-1).sum(-1)  # (B, T-1)
    msum = m.sum(1)
    pred = (m * (sq - rew + bce)).sum(1) / (msum + 1e-5)
    klb = (m * kl).sum(1) / (T - 1)
    return betas[0] * pred + (betas[1] + betas[2]) * klb, pred, klb, msum
