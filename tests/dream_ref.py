"""References for dr_dream_stats (include/dreamer_hip.h "dream trace"), written
from the formulas: Agent.py:156-172 (lambda returns), Agent.py:105-121
(advantage, log-probability of a tanh-Normal action), and the per-window
statistics the header defines.

dream_ref(..., dt=np.float64) takes the float32 values the kernel sees and
continues in float64; dt=np.float32 is the same formulas with every operation
rounded to f32 in the kernel's order (the accuracy yardstick of
test_gpu_dream_trace.py).  Rows n = b*M + m; inputs rewards, continues [N][H],
Vt, Vo [N][H+1], mus, sigmas, actions [N][H][A]."""
import math

import numpy as np

PER_DREAM = ("R_lambda", "R_mc", "adv", "adv_norm", "weight", "logp", "base_entropy", "saturated")
PER_WINDOW = ("reward_mean", "reward_std", "ret_mean", "ret_std", "logp_mean", "logp_std", "alive", "action_spread",
              "best", "worst", "n_finite")
INT = ("saturated", "best", "worst", "n_finite")
U = 2.0 ** -24


def returns(r, c, V, gamma, lam, dt):
    """R [N][H]: R_{H-1} = r + (gamma c) V_H, R_t = r + (gamma c) ((1 - lam) V_{t+1} + lam R_{t+1})."""
    f = dt
    r, c, V = r.astype(f), c.astype(f), V.astype(f)
    g, l = f(np.float32(gamma)), f(np.float32(lam))
    lc = f(1.0 - float(np.float32(lam)))  # formed in double, rounded once (to dt)
    H = r.shape[1]
    R = np.empty_like(r)
    nxt = r[:, H - 1] + (g * c[:, H - 1]) * V[:, H]
    R[:, H - 1] = nxt
    for t in range(H - 2, -1, -1):
        nxt = r[:, t] + (g * c[:, t]) * ((lc * V[:, t + 1]) + (l * nxt))
        R[:, t] = nxt
    return R


def weights(c, gamma, dt):
    """w [N][H+1]: w_0 = 1, w_{t+1} = w_t (gamma c_t)."""
    f = dt
    c = c.astype(f)
    g = f(np.float32(gamma))
    N, H = c.shape
    w = np.ones((N, H + 1), f)
    for t in range(H):
        w[:, t + 1] = w[:, t] * (g * c[:, t])
    return w


def softplus(x):
    """torch softplus(beta=1, threshold=20) in x's dtype."""
    with np.errstate(over="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, x.dtype.type(30)))))


def logprob(mus, sigmas, actions, dt):
    """(logp, base_entropy) [N][H]: the A terms added in ascending order from 0."""
    f = dt
    y = np.minimum(np.maximum(actions.astype(np.float32), np.float32(-1.0 + 1e-6)), np.float32(1.0 - 1e-6)).astype(f)
    x = np.arctanh(y)
    mu, sg = mus.astype(f), sigmas.astype(f)
    d = x - mu
    var = sg * sg
    lsg = np.log(sg)
    half_log_2pi = f(math.log(math.sqrt(2 * math.pi)))
    log2 = f(math.log(2.0))
    ent0 = f(0.5 + 0.5 * math.log(2 * math.pi))
    lp = -(d * d) / (f(2.0) * var) - lsg - half_log_2pi
    ladj = f(2.0) * (log2 - x - softplus(f(-2.0) * x))
    term = lp - ladj
    acc, ent = np.zeros(term.shape[:-1], f), np.zeros(term.shape[:-1], f)
    for k in range(term.shape[-1]):
        acc = acc + term[..., k]
        ent = ent + (ent0 + lsg[..., k])
    return acc, ent


def mean_var(x, dt):
    """x [B][M][...] -> (mean, population variance) over M: ascending sums from 0, two passes."""
    f = dt
    M = x.shape[1]
    s = np.zeros(x.shape[:1] + x.shape[2:], f)
    for m in range(M):
        s = s + x[:, m]
    mean = s / f(M)
    v = np.zeros_like(s)
    for m in range(M):
        d = x[:, m] - mean
        v = v + d * d
    return mean, v / f(M)


def rank(mc0):
    """mc0 [B][M] -> (best, worst, n_finite) int32 [B]: the largest / smallest
    finite entry, ties to the lower m; no finite entry: 0, 0, 0."""
    B, M = mc0.shape
    best, worst, nf = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for m in range(M):
            v = mc0[b, m]
            if not np.isfinite(v):
                continue
            if nf[b] == 0 or v > mc0[b, best[b]]:
                best[b] = m
            if nf[b] == 0 or v < mc0[b, worst[b]]:
                worst[b] = m
            nf[b] += 1
    return best, worst, nf


def dream_ref(B, M, rewards, continues, Vt, Vo, mus, sigmas, actions, gamma, lam, norm=1.0, sat=0.99, dt=np.float64):
    """Every output of dr_dream_stats as {name: array}, per dream (B,M,...), per window (B,...)."""
    f = dt
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        N, H = rewards.shape
        A = actions.shape[-1]
        assert N == B * M
        Rl = returns(rewards, continues, Vt, gamma, lam, f)
        Rmc = returns(rewards, continues, Vt, gamma, 1.0, f)
        adv = Rl - Vo.astype(f)[:, :H]
        w = weights(continues, gamma, f)
        lp, ent = logprob(mus, sigmas, actions, f)
        sat_n = (np.abs(actions.astype(np.float32)) >= np.float32(sat)).sum(-1).astype(np.int32)
        o = dict(R_lambda=Rl, R_mc=Rmc, adv=adv, adv_norm=adv / f(np.float32(norm)), weight=w, logp=lp,
                 base_entropy=ent, saturated=sat_n)
        o = {k: v.reshape(B, M, *v.shape[1:]) for k, v in o.items()}
        for name, x in (("reward", rewards.astype(f).reshape(B, M, H)), ("ret", o["R_lambda"]), ("logp", o["logp"])):
            mean, var = mean_var(x, f)
            o[name + "_mean"], o[name + "_std"] = mean, np.sqrt(var)
        o["alive"] = mean_var(o["weight"], f)[0]
        _, va = mean_var(actions.astype(f).reshape(B, M, H, A), f)  # (B,H,A)
        s = np.zeros((B, H), f)
        for k in range(A):
            s = s + va[..., k]
        o["action_spread"] = np.sqrt(s / f(A))
        o["best"], o["worst"], o["n_finite"] = rank(o["R_mc"][:, :, 0])
    return o


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|) over the entries where ref is finite; the
    others must agree in kind (NaN with NaN, +-Inf with the same Inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "Inf pattern differs"
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max())


def planted(B, M, H, A, seed=0):
    """f32 inputs of B windows of M dreams with the rows the tests plant, as far
    as the shape has room for them: a continue of exactly 0 mid-dream (dream 0),
    all continues 1 (dream 1), actions of exactly +1 / -1 (dream 0, step 0),
    sigma at the actor's floor 1e-3 (dream 0, last step, H >= 2), dreams 1 and 2
    identical and on top (a tie for best), a NaN reward in dream 3, and window 0
    copied to the last batch position.

    The log-probability is conditioned like |x| / |x - mu| (x = atanh a): an
    error of one f32 step in x is |x| 2^-24 / sigma^2 times |x - mu| in the
    quadratic term.  A bound relative to |logp| can therefore only be asked for
    where sigma is not tiny against |x|: the general rows keep sigma >= 0.05,
    and the row at the floor sigma = 1e-3 has |mu| ~ 0.01, as an actor that has
    collapsed around a small action has."""
    g = np.random.default_rng(1000 * seed + 97 * B + 13 * M + 7 * H + A)
    N = B * M
    f32 = np.float32
    nrm = lambda *s: g.standard_normal(s).astype(f32)
    x = dict(rewards=nrm(N, H) * f32(2), continues=(1 - 0.3 * g.random((N, H))).astype(f32),
             Vt=nrm(N, H + 1) * f32(5), Vo=nrm(N, H + 1) * f32(5), mus=nrm(N, H, A),
             sigmas=(np.log1p(np.exp(g.random((N, H, A)) * 5 - 3)) + 1e-3).astype(f32))
    eps = nrm(N, H, A)
    if H >= 2:
        x["sigmas"][0, H - 1] = f32(1e-3)
        x["mus"][0, H - 1] *= f32(0.01)
    x["actions"] = np.tanh(x["mus"] + x["sigmas"] * eps).astype(f32)
    if H >= 3:
        x["continues"][0, H // 2] = 0.0
    x["actions"][0, 0, 0] = 1.0
    x["actions"][0, 0, A - 1] = -1.0 if A > 1 else 1.0
    if M >= 2:
        x["continues"][1] = 1.0
    if M >= 3:
        x["rewards"][1] += f32(50)
        for k in x:
            x[k][2] = x[k][1]
    if M >= 4:
        x["rewards"][3, min(1, H - 1)] = np.nan
    if B >= 2:
        for k in x:
            x[k][(B - 1) * M:] = x[k][:M]
    return x
