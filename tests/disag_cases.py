"""Inputs and tolerances of tests/test_gpu_disag.py, shared with tests/test_disag_host.py (which checks without a GPU
that a correct f32 evaluation stays inside every tolerance here).

Row-kernel cases: K x L x M as below.  The rows of a case take turns through KINDS: random predictions; all members
equal; one member far off; magnitudes 1e-20 and 1e+15; a NaN (in the last member) and an Inf (in member 0); predictions
equal to the target (the squared-error gradient is exactly 0).  A case with fewer rows than kinds starts the turn at
its own index, so every kind meets every K and L.  Predictions sit in a NaN-padded buffer (row stride L + 3, a guard row
per member), the targets likewise: a kernel that reads past a row shows.

Composed cases (K, W, Hd, (rows, cols), M): weights drawn like nn.Linear's (LayerNorm gains 1 +- 0.1, shifts +- 0.05), h
~ N(0, 1), z a one-hot sample per latent row.  Predictions, d and the losses are held to disag_ref.forward_bounds /
loss_bounds (propagated, written down there; composed of worst-case product bounds over three layers they are
wide -- the first run sat at 1e-4 of them -- so each is also held to 4 x its measured error, without the f32 cap:
the measured figure only tightens what the propagation allows).  For the gradients and the parameters after three
train_steps no propagated bound is written (the LayerNorm backward divides differences of errors by sigma twice over);
they follow the project's standing rule: 4 x the error against float64 measured on the first MI355X run, in units of 2^-24 max|ref| of
the tensor (MEASURED below, profiles/disag_errors.txt; DISAG_ERRORS=<file> appends such a table), and never looser than
8 x the largest error of the f32 numpy evaluation of the same tensor of the same case."""
import os

import numpy as np

import disag_ref as R

U = R.U
POISON = 0x7FE5A5A5
ROW_K = (1, 2, 3, 5, 8, 16)
ROW_L = (1, 63, 64, 65, 1056)
ROW_M = (1, 4, 5, 257)
KINDS = ("random", "equal", "far", "tiny", "huge", "nan", "inf", "target")

COMPOSED = ((1, 8, 20, (4, 3), 1), (2, 36, 36, (12, 8), 17), (3, 64, 64, (4, 3), 257), (5, 100, 100, (32, 33), 33),
            (8, 64, 32, (8, 8), 1027), (16, 16, 32, (4, 3), 5))
TRAIN_STEPS, TRAIN_LR = 3, 1e-3

# learning case (test_learning): K = 5, W = 64, Hd = 32, L = 64 (8 x 8), 64 training rows h ~ N(0, 1), 64 held-out rows
# h ~ N(3, 1), 200 train_steps on the training rows at LEARN_LR.  The seed was chosen on the CPU so that the float64
# reference alone ends with mean d(train) <= 0.5 mean d(held-out); its values are recorded here
# (tests/test_disag_host.py recomputes them).
LEARN = dict(K=5, W=64, Hd=32, rows=8, cols=8, M=64, steps=200, lr=3e-3, seed=0)
LEARN_REF = dict(d_train=0.01408721247481793, d_held=0.26407883675747446, loss_first=0.25582251949262147,
                 loss_last=0.00038277069643505806)

# largest |got - ref| / (2^-24 max|ref|) per tensor over the composed cases, first MI355X run (profiles/disag_errors.txt)
MEASURED = {
    "pred": 5.585, "d": 2.987, "losses": 2.009,
    "grad.l0_weight": 13.696, "grad.l0_bias": 13.669, "grad.n1_weight": 13.711, "grad.n1_bias": 11.268,
    "grad.l3_weight": 7.444, "grad.l3_bias": 7.348, "grad.n4_weight": 3.473, "grad.n4_bias": 2.975,
    "grad.l6_weight": 5.844, "grad.l6_bias": 2.235,
    "trained.l0_weight": 9.926, "trained.l0_bias": 3.482, "trained.n1_weight": 2.217, "trained.n1_bias": 1.627,
    "trained.l3_weight": 6.730, "trained.l3_bias": 3.497, "trained.n4_weight": 2.113, "trained.n4_bias": 2.107,
    "trained.l6_weight": 3.866, "trained.l6_bias": 2.263,
}
MEASURING = bool(os.environ.get("DISAG_ERRORS"))


def measured_tol(key, ref, f32=None):
    """(tolerance, scale) of a measured output, one number for the whole tensor: min(4 MEASURED 2^-24 max|ref|,
    8 max|f32 - ref|).  f32 None (predictions, d, losses: they have a propagated bound, which the measured figure
    only tightens): no cap."""
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    cap = float("inf") if f32 is None else 8.0 * float(np.abs(f32.astype(np.float64) - ref).max())
    if key not in MEASURED and MEASURING:
        return float("inf"), scale
    return min(4.0 * MEASURED[key] * U * scale, cap), scale


def rng(*key):
    return np.random.default_rng([20260000, *key])


def poison(*shape):
    return np.full(shape, POISON, dtype=np.int32).view(np.float32)


def is_poison(a):
    return a.view(np.int32) == POISON


# ----------------------------------------------------------------------------------------------------------------
# row kernels
# ----------------------------------------------------------------------------------------------------------------
def row_kinds(K, L, M):
    first = (ROW_K.index(K) * len(ROW_L) + ROW_L.index(L)) if M < len(KINDS) else 0
    return [KINDS[(first + r) % len(KINDS)] for r in range(M)]


def row_case(K, L, M):
    """pred (K, M, L) f32, z (M, L) f32 (0 / 1) and the kind of every row."""
    g = rng(1, K, L, M)
    pred = g.standard_normal((K, M, L)).astype(np.float32)
    z = (g.random((M, L)) < 0.25).astype(np.float32)
    kinds = row_kinds(K, L, M)
    for r, kind in enumerate(kinds):
        if kind == "equal":
            pred[:, r] = pred[0, r]
        elif kind == "far":
            pred[(r + K - 1) % K, r] += np.float32(1e3)
        elif kind == "tiny":
            pred[:, r] *= np.float32(1e-20)
        elif kind == "huge":
            pred[:, r] *= np.float32(1e15)
        elif kind == "nan":
            pred[K - 1, r, (3 * r) % L] = np.nan
        elif kind == "inf":
            pred[0, r, (5 * r) % L] = np.inf if r % 2 else -np.inf
        elif kind == "target":
            pred[:, r] = z[r]
            if K > 1:
                pred[K - 1, r, L // 2] += np.float32(0.5)  # (the members still disagree in one column)
    return pred, z, kinds


def padded_pred(pred, pad=3, guard=1):
    """(buffer (K, M + guard, L + pad) NaN-padded, kstride, ldp)."""
    K, M, L = pred.shape
    b = np.full((K, M + guard, L + pad), np.nan, dtype=np.float32)
    b[:, :M, :L] = pred
    return b, (M + guard) * (L + pad), L + pad


def padded_rows(x, pad=1, guard=1):
    M, L = x.shape
    b = np.full((M + guard, L + pad), np.nan, dtype=np.float32)
    b[:M, :L] = x
    return b, L + pad


def reward_map(M):
    """(rew_T, rew_skip, rew_sb, rew_st, floats of the reward buffer, [buffer index of row m or -1]) -- the engine's
    mapping (rows [B][T1], the first of each group has no reward) where M splits into groups, else one reward per row
    at a stride of 2."""
    if M == 1:
        return 0, 0, 0, 2, 2 * M + 1, [2 * m for m in range(M)]
    T1 = 2 if M == 4 else M
    B, sb = M // T1, T1 + 1
    at = [-1 if m % T1 == 0 else (m // T1) * sb + (m % T1 - 1) for m in range(M)]
    return T1, 1, sb, 1, B * sb + 1, at


REW_W = (0.5, 2.0)  # (w_ext, w_int) of the in-place reward update


# ----------------------------------------------------------------------------------------------------------------
# composed
# ----------------------------------------------------------------------------------------------------------------
def init_params(g, K, W, Hd, L):
    def uni(fan, *s):
        return ((g.random(s) * 2 - 1) / np.sqrt(fan)).astype(np.float32)
    P = dict(l0_weight=uni(Hd, K * W, Hd), l0_bias=uni(Hd, K * W),
             n1_weight=(1 + 0.1 * g.standard_normal((K, W))).astype(np.float32),
             n1_bias=(0.05 * g.standard_normal((K, W))).astype(np.float32),
             l3_weight=uni(W, K, W, W), l3_bias=uni(W, K, W),
             n4_weight=(1 + 0.1 * g.standard_normal((K, W))).astype(np.float32),
             n4_bias=(0.05 * g.standard_normal((K, W))).astype(np.float32),
             l6_weight=uni(W, K, L, W), l6_bias=uni(W, K, L))
    return P


def onehot_rows(g, M, rows, cols):
    idx = g.integers(0, cols, size=(M, rows))
    z = np.zeros((M, rows, cols), dtype=np.float32)
    np.put_along_axis(z, idx[..., None], 1.0, axis=-1)
    return z.reshape(M, rows * cols)


_composed = {}


def composed_case(i):
    """Case i of COMPOSED with its float64 reference and f32 evaluation, computed once and shared."""
    if i in _composed:
        return _composed[i]
    K, W, Hd, (rows, cols), M = COMPOSED[i]
    L = rows * cols
    g = rng(2, i)
    P = init_params(g, K, W, Hd, L)
    h = g.standard_normal((M, Hd)).astype(np.float32)
    z = onehot_rows(g, M, rows, cols)
    c = dict(K=K, W=W, Hd=Hd, L=L, M=M, P=P, h=h, z=z)
    for tag, dt in (("ref", np.float64), ("f32", np.float32)):
        f = R.forward(R.cast(P, dt), h.astype(dt))
        ls, G = R.grads(R.cast(P, dt), h.astype(dt), z.astype(dt))
        Pn, hist, opt = R.train(P, h, z, TRAIN_STEPS, TRAIN_LR, dt=dt)
        c[tag] = dict(pred=f["pred"], d=R.disagreement(f["pred"]) if dt == np.float64 else
                      R.disagreement_shifted(f["pred"]), losses=ls, grads=G, trained=Pn, hist=hist, skipped=opt.skipped)
    c["e_pred"], c["e_d"] = R.forward_bounds(P, h)
    c["e_loss"] = R.loss_bounds(P, h, z)
    _composed[i] = c
    return c


def learn_case():
    g = rng(3, LEARN["seed"])
    K, W, Hd, rows, cols, M = (LEARN[k] for k in ("K", "W", "Hd", "rows", "cols", "M"))
    P = init_params(g, K, W, Hd, rows * cols)
    for k in ("n1_weight", "n4_weight"):
        P[k][:] = 1.0
    for k in ("n1_bias", "n4_bias"):
        P[k][:] = 0.0
    h_train = g.standard_normal((M, Hd)).astype(np.float32)
    h_held = (3.0 + g.standard_normal((M, Hd))).astype(np.float32)
    z = onehot_rows(g, M, rows, cols)
    return P, h_train, h_held, z
