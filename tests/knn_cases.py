"""Inputs and the case table of tests/test_gpu_knn.py, shared with tests/test_knn_host.py (which checks without a GPU
that f32 evaluations in the kernels' order stay inside every bound used there).

A case is (D, (Mq, Nb), k, groups).  Every D of DS, every shape of SHAPES and every k of KS occurs; D = 600 meets the
two shapes of more than one bank tile that keep the float64 reference small, the largest shape (9 bank tiles, the
planner splits it 9 ways) meets D = 5 and D = 64.  k = 32 meets Nb = 1 and Nb = 2 (k > Nb), k = 12 meets "dream" groups
of 5 at Nb = 40 (k > eligible for none, but Nb - 5 < 40) and groups = "self" at Nb = 2 (one eligible row).
groups: None, "self" (group = row index; the queries are the first Mq bank rows) or "dream" (group = row // 5).

Inputs per case:
  ints   integer values in [-8, 8] drawn from few distinct rows: many exact ties and duplicates; every product and sum
         is exact in f32 (D 8^2 4 < 2^24), so indices and distances are held to the reference exactly
  rand   tanh of normals (the range of a GRU state), every 7th bank row a copy of the row 3 before it and every 11th
         that row + 1e-4
Rows sit in NaN-padded buffers (row stride D + 3, one guard row); outputs in poisoned ones."""
import numpy as np

import knn_ref as R

POISON = 0x7FE5A5A5
DS = (1, 3, 4, 5, 63, 64, 65, 600)
SHAPES = ((1, 1), (1, 2), (3, 40), (63, 65), (64, 64), (65, 129), (129, 257), (257, 1030))
KS = (1, 3, 12, 32)
DREAM_T = 5

CASES = (
    (1, (1, 1), 32, None), (3, (1, 2), 32, "self"), (4, (3, 40), 12, "dream"), (5, (63, 65), 3, "self"),
    (63, (64, 64), 12, "self"), (64, (65, 129), 1, None), (65, (129, 257), 32, "dream"), (600, (65, 129), 12, "self"),
    (600, (129, 257), 3, None), (5, (257, 1030), 12, "self"), (64, (257, 1030), 32, "dream"), (1, (63, 65), 12, None),
    (3, (64, 64), 1, "dream"), (4, (1, 2), 3, None), (65, (3, 40), 32, "self"), (63, (1, 1), 1, "self"),
)
REW_W = (0.5, 2.0)


def rng(*key):
    return np.random.default_rng([20261021, *key])


def poison(*shape):
    return np.full(shape, POISON, dtype=np.int32).view(np.float32)


def is_poison(a):
    return a.view(np.int32) == POISON


def padded_rows(x, pad=3, guard=1):
    M, D = x.shape
    b = np.full((M + guard, D + pad), np.nan, dtype=np.float32)
    b[:M, :D] = x
    return b, D + pad


def groups(kind, Mq, Nb):
    if kind is None:
        return None, None
    if kind == "self":
        return np.arange(Mq, dtype=np.int32), np.arange(Nb, dtype=np.int32)
    return (np.arange(Mq, dtype=np.int32) // DREAM_T).astype(np.int32), \
        (np.arange(Nb, dtype=np.int32) // DREAM_T).astype(np.int32)


def ints(i):
    """(queries, bank) of case i, integer-valued."""
    D, (Mq, Nb), k, kind = CASES[i]
    g = rng(1, i)
    pool = g.integers(-8, 9, size=(max(2, Nb // 3), D)).astype(np.float32)
    bank = pool[g.integers(0, pool.shape[0], size=Nb)]
    q = bank[:Mq].copy() if kind else pool[g.integers(0, pool.shape[0], size=Mq)]
    return q, bank


def rand(i):
    """(queries, bank) of case i, tanh of normals with planted duplicates and near-duplicates."""
    D, (Mq, Nb), k, kind = CASES[i]
    g = rng(2, i)
    bank = np.tanh(g.standard_normal((Nb, D))).astype(np.float32)
    for j in range(3, Nb):
        if j % 7 == 0:
            bank[j] = bank[j - 3]
        elif j % 11 == 0:
            bank[j] = bank[j - 3] + np.float32(1e-4)
    q = bank[:Mq].copy() if kind else np.tanh(g.standard_normal((Mq, D))).astype(np.float32)
    if not kind and Mq > 2 and Nb > 2:
        q[1] = bank[2]  # a query that is a bank row
    return q, bank


_refs = {}


def reference(i, which):
    """Case i's inputs with their float64 reference, computed once and shared:
    dict(q, bank, qg, bg, k, D, T (true d2), el, d2, idx, G)."""
    if (i, which) in _refs:
        return _refs[i, which]
    D, (Mq, Nb), k, kind = CASES[i]
    q, bank = (ints if which == "ints" else rand)(i)
    qg, bg = groups(kind, Mq, Nb)
    T = R.dist2(q, bank)
    d2, idx = R.knn(q, bank, k, qg, bg, d2=T)
    c = dict(q=q, bank=bank, qg=qg, bg=bg, k=k, D=D, T=T, el=R.eligible(q, bank, qg, bg), d2=d2, idx=idx,
             G=R.gram_bound(q, bank))
    _refs[i, which] = c
    return c


def check_contract(c, d2, idx):
    """The random-input contract of one case on outputs d2 / idx [Mq][k]; returns a list of failures and the worst
    ratios (reported distance / direct bound, selection slack / 2 max G)."""
    fails, w_direct, w_sel = [], 0.0, 0.0
    T, el, G, k, D = c["T"], c["el"], c["G"], c["k"], c["D"]
    for m in range(T.shape[0]):
        n_el = int(el[m].sum())
        fill = min(k, n_el)
        ii, dd = idx[m], d2[m].astype(np.float64)
        if not (np.all(ii[:fill] >= 0) and np.all(ii[fill:] == -1) and np.all(np.isposinf(dd[fill:]))):
            fails.append(f"row {m}: {fill} slots should be filled: {ii}")
            continue
        ii, dd = ii[:fill], dd[:fill]
        if fill == 0:
            continue
        if len(set(ii.tolist())) != fill or not el[m, ii].all():
            fails.append(f"row {m}: indices repeated or not eligible: {ii}")
            continue
        if not all((dd[n], ii[n]) < (dd[n + 1], ii[n + 1]) for n in range(fill - 1)):
            fails.append(f"row {m}: not in ascending (d2, index) order")
        t = T[m, ii]
        lim = R.direct_bound(t, D)
        if not np.all(np.abs(dd - t) <= lim):
            fails.append(f"row {m}: a reported distance is off its direct-form bound")
        nz = lim > 0
        if nz.any():
            w_direct = max(w_direct, float((np.abs(dd - t)[nz] / lim[nz]).max()))
        slack = 2.0 * float(G[m, el[m]].max())
        elig = np.sort(T[m, el[m]])
        kth = elig[fill - 1]
        worst_in = float(t.max())
        if not worst_in <= kth + slack:
            fails.append(f"row {m}: returned a row at {worst_in!r}, the true k-th is {kth!r} (slack {slack:.3g})")
        out = el[m].copy()
        out[ii] = False
        if out.any():
            nearest_out = float(T[m, out].min())
            if not nearest_out >= worst_in - slack:
                fails.append(f"row {m}: left out a row at {nearest_out!r}, returned one at {worst_in!r}")
            if slack > 0:
                w_sel = max(w_sel, (worst_in - nearest_out) / slack)
    return fails, w_direct, w_sel


def reward_map(M):
    """(rew_T, rew_skip, rew_sb, rew_st, floats of the reward buffer, [buffer index of row m or -1]): the engine's mapping
    (rows [B][T1], the first of each group has no reward) where M splits into groups, else one reward per row at a
    stride of 2 (as disag_cases.reward_map)."""
    T1 = next((t for t in (5, 4, 3) if M % t == 0 and M > t), 0)
    if T1 == 0:
        return 0, 0, 0, 2, 2 * M + 1, [2 * m for m in range(M)]
    B, sb = M // T1, T1 + 1
    at = [-1 if m % T1 == 0 else (m // T1) * sb + (m % T1 - 1) for m in range(M)]
    return T1, 1, sb, 1, B * sb + 1, at
