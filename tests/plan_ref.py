"""References of the planner's two kernels (include/dreamer_hip.h "latent
planning", steps 1 and 4 to 7) on the CPU in numpy: every function takes the
dtype it computes in.  np.float64 is the reference the GPU is held to;
np.float32 is a transcription of the same formulas in the kernels' order (one
rounding per operation, numpy does not contract), the yardstick of the
project's accuracy rule: the GPU may be off by 8 x what this transcription is
off against float64 on the same inputs.  Test infrastructure only."""
import numpy as np

U = 2.0 ** -24


def bound(yardstick):
    """The accuracy rule: 8 x the f32 transcription's error, at least 4 * 2^-24, never more than 1e-4."""
    return min(max(8.0 * yardstick, 4.0 * U), 1e-4)


def rel(got, ref):
    """max |got - ref| / max(1, |ref|) (0 for empty arrays)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def sample(mean, std, eps, pol, N_pi, dt):
    """Step 1.  mean, std (E,H*A); eps (E,N,H*A); pol (E,N_pi,H*A) or None -> (E,N,H*A)."""
    mean, std, eps = (np.asarray(t).astype(dt) for t in (mean, std, eps))
    a = np.clip(mean[:, None, :] + std[:, None, :] * eps, dt(-1), dt(1)).astype(dt)
    if N_pi > 0:
        a[:, :N_pi] = np.asarray(pol).astype(dt)
    return a


def scores(r, c, vH, gamma, dt):
    """Step 4.  r, c (B,H); vH (B,) or None -> G (B,): k_lambda_returns' expressions at lam = 1."""
    r, c = np.asarray(r).astype(dt), np.asarray(c).astype(dt)
    B, H = r.shape
    v = np.zeros(B, dt) if vH is None else np.asarray(vH).astype(dt)
    g = dt(np.float32(gamma))
    with np.errstate(all="ignore"):
        nxt = r[:, H - 1] + (g * c[:, H - 1]) * v
        for t in range(H - 2, -1, -1):
            nxt = r[:, t] + (g * c[:, t]) * ((dt(0) * dt(0)) + (dt(1) * nxt))
    return nxt.astype(dt)


def rank(G, K):
    """Step 5 for one environment: the indices of the K' = min(K, finite) elites in rank order."""
    G = np.asarray(G)
    fin = np.flatnonzero(np.isfinite(G))
    order = fin[np.argsort(-G[fin], kind="stable")]  # ties: the lower index first
    return order[:K]


def update(r, c, vH, gamma, temperature, momentum, std_min, std_max, actions, mean, std, K, dt, G=None):
    """Steps 4 to 7.  r, c (E*N,H); vH (E*N,) or None; actions (E,N,H*A); mean, std (E,H*A).
    Returns dict(scores (E,N), elite_idx (E,K) int, elite_w (E,K), n_elite (E,), mean, std).
    G: scores to rank and weigh by instead of this dtype's own (E,N)."""
    actions = np.asarray(actions).astype(dt)
    E, N, HA = actions.shape
    mean, std = np.array(mean).astype(dt), np.array(std).astype(dt)
    sc = scores(r, c, vH, gamma, dt).reshape(E, N) if G is None else np.asarray(G).astype(dt).reshape(E, N)
    T, mom = dt(np.float32(temperature)), dt(np.float32(momentum))
    lo, hi = dt(np.float32(std_min)), dt(np.float32(std_max))
    keep = dt(1) - mom
    eidx = np.full((E, K), -1, np.int64)
    ew = np.zeros((E, K), dt)
    ne = np.zeros(E, np.int64)
    for e in range(E):
        el = rank(sc[e], K)
        Ke = len(el)
        ne[e] = Ke
        if Ke == 0:
            continue
        eidx[e, :Ke] = el
        g = sc[e, el]
        w = np.ones(Ke, dt) if T == 0 else np.exp(((g - g[0]) / T).astype(dt)).astype(dt)
        W = dt(0)
        for j in range(Ke):
            W = dt(W + w[j])
        ew[e, :Ke] = (w / W).astype(dt)
        acc = np.zeros(HA, dt)
        for j in range(Ke):
            acc = (acc + w[j] * actions[e, el[j]]).astype(dt)
        m = (acc / W).astype(dt)
        var = np.zeros(HA, dt)
        for j in range(Ke):
            dv = (actions[e, el[j]] - m).astype(dt)
            var = (var + w[j] * (dv * dv)).astype(dt)
        s = np.sqrt((var / W).astype(dt)).astype(dt)
        mean[e] = (mom * mean[e] + keep * m).astype(dt)
        std[e] = np.minimum(np.maximum(s, lo), hi)
    return dict(scores=sc, elite_idx=eidx, elite_w=ew, n_elite=ne, mean=mean, std=std)


def tie_gaps_ok(G):
    """The index tests' tie guard for one environment's float64 scores: sorted,
    all consecutive scores differ by at least 1e-3 * max(1, |G|)."""
    s = np.sort(np.asarray(G, np.float64))[::-1]
    if len(s) < 2:
        return True
    thr = 1e-3 * np.maximum(1.0, np.maximum(np.abs(s[:-1]), np.abs(s[1:])))
    return bool(np.all(s[:-1] - s[1:] >= thr))


def close_rows(G):
    """Candidates of one environment whose float64 score is within the tie guard of the next better one."""
    G = np.asarray(G, np.float64)
    order = np.argsort(-G, kind="stable")
    s = G[order]
    thr = 1e-3 * np.maximum(1.0, np.maximum(np.abs(s[:-1]), np.abs(s[1:])))
    return order[1:][s[:-1] - s[1:] < thr]


def draw_update_inputs(E, N, H, seed):
    """rewards, continues in [0, 1] with some exact zeros, V_H (all float32, (E*N,H) / (E*N,)), redrawn row by
    row until every environment's float64 scores pass the tie guard at gamma = 0.99."""
    rng = np.random.default_rng(seed)

    def rows(n):
        r = rng.standard_normal((n, H)).astype(np.float32)
        c = rng.uniform(0, 1, (n, H)).astype(np.float32)
        c[rng.uniform(0, 1, (n, H)) < 0.15] = 0.0
        v = (2.0 * rng.standard_normal(n)).astype(np.float32)
        return r, c, v

    r, c, v = rows(E * N)
    for _ in range(10000):
        G = scores(r, c, v, 0.99, np.float64).reshape(E, N)
        bad = np.concatenate([e * N + close_rows(G[e]) for e in range(E)])
        if len(bad) == 0:
            return r, c, v
        r[bad], c[bad], v[bad] = rows(len(bad))
    raise RuntimeError("no tie-free draw")


def spaced_update_inputs(E, N, H, seed):
    """The same kind of inputs for large N, where redrawing cannot satisfy the tie guard: the scores are steered
    onto a shuffled grid that passes it with a margin (steps of 1.3e-3 inside [-1, 1], a ratio of 1.0013
    outside), by solving each row's first reward for its target in float64."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((E * N, H)).astype(np.float32)
    c = rng.uniform(0, 1, (E * N, H)).astype(np.float32)
    c[rng.uniform(0, 1, (E * N, H)) < 0.15] = 0.0
    v = (2.0 * rng.standard_normal(E * N)).astype(np.float32)
    inner = min(N, 1500)
    grid = list((np.arange(inner) - inner // 2) * 1.3e-3)
    k = 1
    while len(grid) < N:
        grid += [(1.0 + 1e-3) * 1.0013 ** k, -(1.0 + 1e-3) * 1.0013 ** k]
        k += 1
    grid = np.asarray(grid[:N], np.float64)
    for e in range(E):
        rows = slice(e * N, (e + 1) * N)
        r[rows, 0] = 0.0
        rest = scores(r[rows], c[rows], v[rows], 0.99, np.float64)        # = (gamma c_0) R_1 with r_0 = 0
        r[rows, 0] = (rng.permutation(grid) - rest).astype(np.float32)
    return r, c, v


def cem_loop(a_star, eps, K, temperature, gamma, std_init, std_min, std_max, momentum, dt):
    """The two kernels' loop on the quadratic problem r_k = -|a_k - a*_k|^2, c = 1, V_H = 0: a_star (E,H,A), eps
    (J,E,N,H*A).  Returns (mean (E,H*A) after J iterations, max |mean - a*| before, after)."""
    a_star = np.asarray(a_star).astype(dt)
    E, H, A = a_star.shape
    J, _, N, HA = eps.shape
    mean, std = np.zeros((E, HA), dt), np.full((E, HA), dt(np.float32(std_init)), dt)
    before = float(np.abs(mean - a_star.reshape(E, HA)).max())
    for j in range(J):
        a = sample(mean, std, eps[j], None, 0, dt)
        d = a.reshape(E, N, H, A) - a_star[:, None]
        r = (-(d * d).sum(-1)).astype(dt).reshape(E * N, H)
        out = update(r, np.ones_like(r), None, gamma, temperature, momentum, std_min, std_max, a, mean, std, K, dt)
        mean, std = out["mean"], out["std"]
    return mean, before, float(np.abs(mean - a_star.reshape(E, HA)).max())


def shifted(mean):
    """PlanResult.shifted in numpy: (E,H,A) moved one step earlier, the last step repeated."""
    mean = np.asarray(mean)
    return np.concatenate((mean[:, 1:], mean[:, -1:]), axis=1)
