"""The k-nearest-neighbour references, bounds and cases without a GPU (tests/knn_ref.py, tests/knn_cases.py): the
references against an independent scalar brute force; f32 evaluations of both distance forms in the kernels' order
inside the bounds the GPU tests assert, on every case; the case table covers what it says; config validation; and that
a Dreamer with explore absent, "none" or "entropy" has exactly the state-dict keys of one without the feature."""
import numpy as np
import pytest
import torch

import knn_cases as C
import knn_ref as R
from conftest import state_layout
from formula import SMALL


@pytest.mark.parametrize("i", [0, 1, 2, 3, 12, 13, 14, 15])
def test_reference_equals_brute_force(i):
    for which in ("ints", "rand"):
        c = C.reference(i, which)
        d2, idx = R.brute(c["q"], c["bank"], c["k"], c["qg"], c["bg"])
        assert np.array_equal(idx, c["idx"]), (i, which)
        fin = np.isfinite(d2)
        assert np.array_equal(fin, np.isfinite(c["d2"]))
        assert np.all(np.abs(d2[fin] - c["d2"][fin]) <= 1e-13 * np.abs(d2[fin]))
        if which == "ints":
            assert np.array_equal(d2[fin], c["d2"][fin])


def test_reference_on_non_finite_rows():
    g = C.rng(7)
    q = g.standard_normal((6, 5)).astype(np.float32)
    bank = g.standard_normal((9, 5)).astype(np.float32)
    bank[2, 1], bank[7, 4], q[3, 0] = np.nan, np.inf, np.nan
    d2, idx = R.knn(q, bank, 8)
    b2, bidx = R.brute(q, bank, 8)
    assert np.array_equal(idx, bidx) and not np.isin(idx, [2, 7]).any()
    assert np.isnan(d2[3]).all() and (idx[3] == -1).all()
    assert (idx[[0, 1, 2, 4, 5], 7] == -1).all() and np.isposinf(d2[[0, 1, 2, 4, 5], 7]).all()  # 7 eligible rows
    e = R.entropy(d2, idx)
    assert np.isnan(e[3]) and np.isfinite(np.delete(e, 3)).all()
    assert R.entropy(np.full((1, 3), np.inf), np.full((1, 3), -1))[0] == 0.0
    assert R.entropy(np.zeros((1, 3)), np.arange(3)[None])[0] == 0.0


@pytest.mark.parametrize("i", range(len(C.CASES)))
def test_f32_evaluations_inside_the_bounds(i):
    """Both forms in f32, in the kernels' order (knn_ref.gram32 / direct32), against float64 on every pair of the
    case (the largest shapes: on the first 24 queries), and the contract on the selection made from the f32 Gram
    distances with the f32 direct distances reported."""
    D, (Mq, Nb), k, kind = C.CASES[i]
    for which in ("ints", "rand"):
        c = C.reference(i, which)
        rows = min(Mq, 24)
        q, bank, T, G, el = c["q"][:rows], c["bank"], c["T"][:rows], c["G"][:rows], c["el"][:rows]
        g32 = R.gram32(q, bank).astype(np.float64)
        assert np.all(np.abs(g32 - T) <= G), (i, which, float((np.abs(g32 - T) / np.maximum(G, 1e-300)).max()))
        if which == "ints":
            assert np.array_equal(g32, T)
        assert np.all(g32[T == 0.0] == 0.0)  # bit-identical rows: exactly 0
        dd, idx = R.select(g32, el, k)
        sub = dict(c, T=T, el=el, G=G)
        d2 = np.full((rows, k), np.inf, dtype=np.float32)
        for m in range(rows):
            n = int((idx[m] >= 0).sum())
            if n:
                d2[m, :n] = R.direct32(np.repeat(q[m:m + 1], n, axis=0), bank[idx[m, :n]])
                order = np.lexsort((idx[m, :n], d2[m, :n]))
                d2[m, :n], idx[m, :n] = d2[m, :n][order], idx[m, :n][order]
        fails, w_direct, w_sel = C.check_contract(sub, d2, idx)
        assert not fails, (i, which, fails[:3])
        assert w_direct <= 1.0
        if which == "ints":
            assert np.array_equal(idx, c["idx"][:rows]) and np.array_equal(d2.astype(np.float64), c["d2"][:rows])


def test_case_table_covers_what_it_says():
    assert {c[0] for c in C.CASES} == set(C.DS)
    assert {c[1] for c in C.CASES} == set(C.SHAPES)
    assert {c[2] for c in C.CASES} == set(C.KS)
    assert {c[3] for c in C.CASES} == {None, "self", "dream"}
    assert any(c[2] > c[1][1] for c in C.CASES)  # k > Nb
    assert any(c[0] == 600 and c[1][1] > 128 for c in C.CASES)
    for i in range(len(C.CASES)):
        c = C.reference(i, "rand")
        assert np.isfinite(c["T"]).all()
    # planted duplicates exist where the bank is large enough, and the integer cases have exact ties
    c = C.reference(9, "rand")
    assert (c["T"] == 0.0).sum() > c["T"].shape[0]
    c = C.reference(9, "ints")
    assert (np.diff(c["d2"], axis=1) == 0).any()


def _cfg(**kw):
    c = dict(SMALL)
    c.update(kw)
    return c


@pytest.mark.parametrize("bad", [dict(explore_knn=0), dict(explore_knn=33), dict(explore_knn=2.0),
                                 dict(explore_knn=True), dict(explore_knn_exclude="none"),
                                 dict(explore_knn_exclude=None), dict(explore="curiosity"), dict(explore=None),
                                 dict(explore_scale=-0.1), dict(explore_extrinsic=float("inf"))])
def test_config_validation(bad):
    from dreamer_amd import Dreamer
    for mode in ("none", "disagreement", "entropy"):  # the keys are checked in every mode
        with pytest.raises(ValueError):
            Dreamer(_cfg(**{"explore": mode, **bad}), "cpu")


def test_defaults():
    from dreamer_amd import Dreamer
    from dreamer_amd.networks import explore_config
    e = explore_config(_cfg(explore="entropy"))
    assert (e["explore_knn"], e["explore_knn_exclude"], e["explore_scale"], e["explore_extrinsic"]) == \
        (12, "self", 0.1, 1.0)
    d = Dreamer(_cfg(explore="entropy", explore_knn=5, explore_knn_exclude="dream"), "cpu")
    assert (d.explore, d.explore_knn, d.explore_knn_exclude) == ("entropy", 5, "dream")


def test_off_and_entropy_add_nothing():
    """explore absent, "none" or "entropy": the state-dict keys of a Dreamer without the feature, no explorer
    attribute, the same initial parameters, the global random streams where a plain Dreamer leaves them, and the
    saved training state has the keys of "none"."""
    from dreamer_amd import Dreamer
    today = [k for k, _ in state_layout("small")]

    def build(**kw):
        torch.manual_seed(7)
        np.random.seed(7)
        d = Dreamer(_cfg(**kw), "cpu")
        return d, torch.get_rng_state().clone(), np.random.get_state()[1].copy()

    off, t0, n0 = build()
    none, t1, n1 = build(explore="none")
    ent, t2, n2 = build(explore="entropy", explore_knn=3)
    for d in (off, none, ent):
        assert list(d.state_dict()) == today
        assert not hasattr(d, "explorer")
        assert len(list(d.parameters())) == len(list(off.parameters()))
    assert torch.equal(t0, t1) and torch.equal(t0, t2) and np.array_equal(n0, n1) and np.array_equal(n0, n2)
    for (k, a), (_, b) in zip(off.state_dict().items(), ent.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(RuntimeError, match="explore"):
        ent.disagreement(torch.zeros(2, 64))
    for d in (off, none):
        for method in (d.novelty, d.evaluate_novelty):
            with pytest.raises(RuntimeError, match="explore"):
                method()


def test_read_outs_need_the_gpu_and_valid_arguments():
    from dreamer_amd import Dreamer
    d = Dreamer(_cfg(), "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        d.knn(torch.zeros(4, 8))
    with pytest.raises(ValueError):
        d.knn(torch.zeros(4, 8), k=0)
    with pytest.raises(ValueError):
        d.state_entropy(torch.zeros(4, 8), k=33)


def test_data_parallel_raises():
    from dreamer_amd import Dreamer
    d = Dreamer(_cfg(explore="entropy"), "cpu")
    d.world = (0, 2, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()
    with pytest.raises(ValueError, match="data parallelism"):
        d.evaluate_novelty()
