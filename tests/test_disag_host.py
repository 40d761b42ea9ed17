"""The latent-disagreement references and tolerances, without a GPU (tests/disag_ref.py, tests/disag_cases.py): the
reference's gradients against torch float64 autograd of the same loss; a correct f32 evaluation inside every tolerance
the GPU tests assert; the exact-zero claims in the shifted form; the recorded learning case; config validation; and that
a Dreamer without exploration has exactly the state-dict keys it had before the feature."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disag_cases as C
import disag_ref as R
from conftest import state_layout
from formula import SMALL


def _autograd(c):
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c["P"].items()}
    h, z = torch.tensor(c["h"], dtype=torch.float64), torch.tensor(c["z"], dtype=torch.float64)
    K, W, M = c["K"], c["W"], c["M"]
    p1 = (h @ P["l0_weight"].T + P["l0_bias"]).reshape(M, K, W).transpose(0, 1)
    total = 0.0
    for k in range(K):
        x1 = F.silu(F.layer_norm(p1[k], (W,), P["n1_weight"][k], P["n1_bias"][k], 1e-5))
        x2 = F.silu(F.layer_norm(x1 @ P["l3_weight"][k].T + P["l3_bias"][k], (W,), P["n4_weight"][k], P["n4_bias"][k],
                                 1e-5))
        total = total + ((x2 @ P["l6_weight"][k].T + P["l6_bias"][k] - z) ** 2).mean()
    loss = total / K
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("i", [0, 1, 3, 5])
def test_reference_gradients_equal_autograd(i):
    c = C.composed_case(i)
    loss, G = _autograd(c)
    assert abs(loss - c["ref"]["losses"][0]) <= 1e-14 * abs(loss)
    for n in R.NAMES:
        ref = c["ref"]["grads"][n]
        assert ref.shape == G[n].shape
        assert np.abs(G[n] - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1e-30), n


@pytest.mark.parametrize("i", range(len(C.COMPOSED)))
def test_f32_evaluation_inside_composed_tolerances(i):
    c = C.composed_case(i)
    ref, f32 = c["ref"], c["f32"]
    assert np.all(np.abs(f32["pred"].astype(np.float64) - ref["pred"]) <= c["e_pred"])
    assert np.all(np.abs(f32["d"].astype(np.float64) - ref["d"]) <= c["e_d"])
    assert np.all(np.abs(f32["losses"].astype(np.float64) - ref["losses"]) <= c["e_loss"])
    assert ref["skipped"] == 0 and f32["skipped"] == 0
    assert ref["hist"][-1] < ref["hist"][0]
    # The gradients and the trained parameters follow the standing rule (4 x the MI355X's measured error, capped at
    # 8 x this f32 evaluation's): no derived bound to be inside of.  numpy's f32 einsum adds 1027 rows in one chain
    # and is up to 13 x less accurate than the device there (profiles/disag_errors.txt, case 4), so the rule's
    # tolerance is not one this evaluation has to meet; what is checked is that every such tensor has a table entry
    # and a positive, finite tolerance.
    for key, (a, b) in [(f"grad.{n}", (ref["grads"][n], f32["grads"][n])) for n in R.NAMES] + \
                       [(f"trained.{n}", (ref["trained"][n], f32["trained"][n])) for n in R.NAMES]:
        tol, scale = C.measured_tol(key, a, b)
        assert 0.0 < tol < float("inf") and tol <= 4.0 * C.MEASURED[key] * R.U * scale, key


@pytest.mark.parametrize("K", C.ROW_K)
def test_f32_evaluation_inside_row_tolerances(K):
    for L in C.ROW_L:
        for M in C.ROW_M:
            pred, z, kinds = C.row_case(K, L, M)
            fin = np.array([k not in ("nan", "inf") for k in kinds])
            with np.errstate(invalid="ignore", over="ignore"):
                ref = R.disagreement(pred.astype(np.float64))
                got = R.disagreement_shifted(pred).astype(np.float64)
                assert np.all(np.abs(got - ref)[fin] <= R.var_bound(pred)[fin]), (K, L, M)
                assert not np.isfinite(ref[~fin]).any() and not np.isfinite(got[~fin]).any()
                for r, kind in enumerate(kinds):
                    if kind == "equal" or K == 1 and fin[r]:
                        assert got[r] == 0.0, (K, L, M, r)
                assert np.all(got[fin] >= 0.0)
                eg, el = R.mse_bounds(pred, z)
                g32 = R.mse_grad(pred, z)
                g64 = R.mse_grad(pred.astype(np.float64), z.astype(np.float64))
                ok = np.isfinite(g64)
                assert np.all(np.abs(g32.astype(np.float64) - g64)[ok] <= eg[ok])
                assert np.all(g32[pred == z[None]] == 0.0)
                l32, l64 = R.losses(pred, z).astype(np.float64), R.losses(pred.astype(np.float64), z.astype(np.float64))
                assert np.array_equal(np.isfinite(l32), np.isfinite(l64))
                okl = np.isfinite(l64)
                # (numpy's pairwise f32 sums sit well inside the kernel's chain bound)
                assert np.all(np.abs(l32 - l64)[okl] <= el[okl]), (K, L, M)


def test_every_kind_meets_every_k_and_l():
    for K in C.ROW_K:
        seen = set()
        for L in C.ROW_L:
            for M in C.ROW_M:
                seen |= set(C.row_kinds(K, L, M))
        assert seen == set(C.KINDS)
    assert set(C.row_kinds(16, 1056, 257)) == set(C.KINDS)


def test_shifted_form_is_exactly_zero_where_division_is_not():
    """K equal f32 values: the definition's mean, sum / K, need not give the value back (K = 3, 5, ...), so its
    deviations are not 0; the shifted form's are."""
    g = C.rng(9)
    worst = 0.0
    for K in C.ROW_K:
        row = g.standard_normal((1, 7, 65)).astype(np.float32) * np.float32(1e3)
        pred = np.repeat(row, K, axis=0)
        assert np.all(R.disagreement_shifted(pred) == 0.0)
        worst = max(worst, float(R.disagreement(pred).max()))
    assert worst > 0.0


def test_learning_case_reference():
    P, h_train, h_held, z = C.learn_case()
    Pn, hist, opt = R.train(P, h_train, z, C.LEARN["steps"], C.LEARN["lr"])
    d_train = float(R.disagreement(R.forward(Pn, h_train.astype(np.float64))["pred"]).mean())
    d_held = float(R.disagreement(R.forward(Pn, h_held.astype(np.float64))["pred"]).mean())
    assert opt.skipped == 0
    assert d_train <= 0.5 * d_held
    want = C.LEARN_REF
    for got, key in ((d_train, "d_train"), (d_held, "d_held"), (hist[0], "loss_first"), (hist[-1], "loss_last")):
        assert abs(got - want[key]) <= 1e-9 * abs(want[key]), (key, got)


def _cfg(**kw):
    c = dict(SMALL)
    c.update(kw)
    return c


@pytest.mark.parametrize("bad", [dict(explore="curiosity"), dict(explore=None), dict(explore_ensemble=0),
                                 dict(explore_ensemble=17), dict(explore_ensemble=2.5), dict(explore_width=0),
                                 dict(explore_width=-8), dict(explore_lr=0.0), dict(explore_lr=-1e-4),
                                 dict(explore_scale=-0.1), dict(explore_extrinsic=-1.0),
                                 dict(explore_scale=float("nan"))])
def test_config_validation(bad):
    from dreamer_amd import Dreamer
    for mode in ("none", "disagreement"):  # the keys are checked whether or not the ensemble is built
        with pytest.raises(ValueError):
            Dreamer(_cfg(**{"explore": mode, **bad}), "cpu")


def test_defaults_and_module():
    from dreamer_amd import Dreamer
    d = Dreamer(_cfg(explore="disagreement"), "cpu")
    ex = d.explorer
    assert (ex.members, ex.width, ex.hidden, ex.latent) == (8, SMALL["dyn_pred_hidden_num_nodes_1"], 64, 64)
    assert (d.explore_scale, d.explore_extrinsic) == (0.1, 1.0)
    assert ex._opt[0] == SMALL["world_model_lr"]
    want = R.shapes(8, 32, 64, 64)
    got = {k[len("explorer."):]: tuple(v.shape) for k, v in d.state_dict().items() if k.startswith("explorer.")}
    assert got == {k: tuple(v) for k, v in want.items()}
    for n in ("n1_weight", "n4_weight"):
        assert torch.all(getattr(ex, n) == 1.0)
    b = 1.0 / 64 ** 0.5
    assert float(ex.l0_weight.detach().abs().max()) <= b and float(ex.l0_weight.detach().std()) > 0.4 * b
    # members differ (diversity comes from the initialisation) and the draw is a function of the seed alone
    assert not torch.equal(ex.l3_weight[0], ex.l3_weight[1])
    again = Dreamer(_cfg(explore="disagreement"), "cpu").explorer
    other = Dreamer(_cfg(explore="disagreement", seed=43), "cpu").explorer
    assert all(torch.equal(a, b) for a, b in zip(ex.parameters(), again.parameters()))
    assert not torch.equal(ex.l0_weight, other.l0_weight)


def test_off_is_inert_and_construction_draws_nothing():
    """explore absent or "none": today's state-dict keys, no explorer attribute; with it on, the ensemble's keys come
    after them and the global torch / numpy streams are where a Dreamer without it leaves them."""
    from dreamer_amd import Dreamer
    today = [k for k, _ in state_layout("small")]

    def build(**kw):
        torch.manual_seed(7)
        np.random.seed(7)
        d = Dreamer(_cfg(**kw), "cpu")
        return d, torch.get_rng_state().clone(), np.random.get_state()[1].copy()

    off, t0, n0 = build()
    none, t1, n1 = build(explore="none")
    on, t2, n2 = build(explore="disagreement", explore_ensemble=3)
    assert list(off.state_dict()) == today and list(none.state_dict()) == today
    assert not hasattr(off, "explorer") and not hasattr(none, "explorer")
    keys = list(on.state_dict())
    assert keys[:len(today)] == today and keys[len(today):] == ["explorer." + n for n in R.NAMES]
    assert torch.equal(t0, t1) and torch.equal(t0, t2) and np.array_equal(n0, n1) and np.array_equal(n0, n2)
    for (k, a), (_, b) in zip(off.state_dict().items(), on.state_dict().items()):
        assert torch.equal(a, b), k
    for method in (off.disagreement, off.novelty, off.evaluate_novelty):
        with pytest.raises(RuntimeError, match="explore"):
            method(torch.zeros(2, 64)) if method == off.disagreement else method()


def test_data_parallel_raises():
    from dreamer_amd import Dreamer
    d = Dreamer(_cfg(explore="disagreement", explore_ensemble=2), "cpu")
    d.world = (0, 2, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_world_model()
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()
    d.world = None
    d.world_model.set_data_parallel(0, 2)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_world_model()
