"""Dream trace, host side (no GPU): properties of the references
(dream_ref.py), DreamResult's arithmetic on hand-built tensors, the binding of
dr_dream_stats and the argument checks made before the device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import dream_ref as DR
from conftest import REPO
from formula import SMALL

F32, F64 = np.float32, np.float64


def _inputs(B, M, H, A, seed=0):
    g = np.random.default_rng(seed)
    N = B * M
    f = lambda *s: g.standard_normal(s).astype(F32)
    mus, sig = f(N, H, A), (np.abs(f(N, H, A)) * 0.5 + 1e-3).astype(F32)
    act = np.tanh(mus + sig * f(N, H, A)).astype(F32)
    return dict(rewards=f(N, H) * 2, continues=(1 - 0.3 * g.random((N, H))).astype(F32), Vt=f(N, H + 1) * 5,
                Vo=f(N, H + 1) * 5, mus=mus, sigmas=sig, actions=act)


def _ref(B, M, x, gamma=0.99, lam=0.95, dt=F64, **kw):
    return DR.dream_ref(B, M, x["rewards"], x["continues"], x["Vt"], x["Vo"], x["mus"], x["sigmas"], x["actions"],
                        gamma, lam, dt=dt, **kw)


# ------------------------------------------------------------------ the references' own properties
@pytest.mark.parametrize("dt", [F64, F32])
def test_zero_continue_cuts_the_recursion(dt):
    B, M, H, A = 1, 2, 6, 2
    x = _inputs(B, M, H, A)
    x["continues"][0, 2] = 0.0
    o = _ref(B, M, x, dt=dt)
    assert np.all(o["weight"][0, 0, 3:] == 0) and np.all(o["weight"][0, 0, :3] != 0)
    assert o["R_lambda"][0, 0, 2] == dt(x["rewards"][0, 2]) and o["R_mc"][0, 0, 2] == dt(x["rewards"][0, 2])
    # what lies beyond the cut does not reach the entries up to it
    y = {k: v.copy() for k, v in x.items()}
    y["rewards"][0, 3:] += 7.0
    y["Vt"][0, 3:] *= -3.0
    o2 = _ref(B, M, y, dt=dt)
    for k in ("R_lambda", "R_mc"):
        assert np.array_equal(o[k][0, 0, :3], o2[k][0, 0, :3]) and np.array_equal(o[k][0, 1], o2[k][0, 1])
    assert np.all(o["alive"][:, 0] == 1)


@pytest.mark.parametrize("dt", [F64, F32])
def test_lambda_one_is_the_monte_carlo_return(dt):
    x = _inputs(2, 3, 5, 2, seed=1)
    o = _ref(2, 3, x, lam=1.0, dt=dt)
    assert np.array_equal(o["R_lambda"], o["R_mc"])
    # gamma = 1, c = 1: R_mc[0] = sum r + V_H, and every weight is 1
    x["continues"][:] = 1.0
    o = _ref(2, 3, x, gamma=1.0, dt=F64)
    want = x["rewards"].astype(F64).sum(1) + x["Vt"][:, -1].astype(F64)
    assert np.abs(o["R_mc"][:, :, 0].reshape(-1) - want).max() <= 1e-12
    assert np.all(o["weight"] == 1) and np.all(o["alive"] == 1)


@pytest.mark.parametrize("dt", [F64, F32])
def test_one_dream_has_no_spread(dt):
    x = _inputs(3, 1, 4, 3, seed=2)
    o = _ref(3, 1, x, dt=dt)
    for k in ("reward_std", "ret_std", "logp_std", "action_spread"):
        assert np.all(o[k] == 0), k
    assert np.array_equal(o["ret_mean"], o["R_lambda"][:, 0]) and np.array_equal(o["alive"], o["weight"][:, 0])
    assert o["best"].tolist() == [0, 0, 0] and o["worst"].tolist() == [0, 0, 0] and o["n_finite"].tolist() == [1, 1, 1]


def test_ranking_ties_and_non_finite_returns():
    mc = np.array([[1.0, 3.0, 3.0, -2.0, -2.0],           # ties go to the lower m
                   [np.nan, 0.5, np.inf, 0.25, -np.inf],   # non-finite entries never rank
                   [np.nan, np.nan, np.nan, np.nan, np.nan],
                   [np.nan, np.nan, 4.0, np.nan, np.nan]])
    best, worst, nf = DR.rank(mc)
    assert best.tolist() == [1, 1, 0, 2] and worst.tolist() == [3, 3, 0, 2] and nf.tolist() == [5, 2, 0, 1]
    # through the whole reference: two identical dreams tie, a NaN reward takes its dream out
    B, M, H, A = 1, 4, 3, 2
    x = _inputs(B, M, H, A, seed=3)
    for k in x:
        x[k][2] = x[k][1]
    x["rewards"][1:3] += 50.0
    x["rewards"][3, 1] = np.nan
    o = _ref(B, M, x)
    assert o["best"].tolist() == [1] and o["n_finite"].tolist() == [3] and o["worst"].tolist() == [0]
    assert np.isnan(o["R_mc"][0, 3, 0]) and not np.isnan(o["R_mc"][0, 3, 2])
    assert np.isnan(o["ret_mean"][0, 1]) and np.isnan(o["reward_std"][0, 1]) and not np.isnan(o["ret_mean"][0, 2])
    x["rewards"][:, 0] = np.nan
    o = _ref(B, M, x)
    assert (o["best"].tolist(), o["worst"].tolist(), o["n_finite"].tolist()) == ([0], [0], [0])


def test_reference_against_direct_formulas():
    """The statistics written with numpy's own reductions, and the f32 transcription near the f64 one."""
    B, M, H, A = 2, 5, 4, 3
    x = _inputs(B, M, H, A, seed=4)
    x["actions"][0, 0, 0], x["actions"][1, 1, 2] = 1.0, -1.0
    o = _ref(B, M, x, norm=2.5, sat=0.9)
    a = x["actions"].astype(F64).reshape(B, M, H, A)
    assert np.abs(o["action_spread"] - np.sqrt(a.var(axis=1).mean(-1))).max() <= 1e-12
    assert np.abs(o["ret_std"] - o["R_lambda"].std(axis=1)).max() <= 1e-12
    assert np.abs(o["reward_mean"] - x["rewards"].astype(F64).reshape(B, M, H).mean(1)).max() <= 1e-12
    assert np.abs(o["adv_norm"] * 2.5 - o["adv"]).max() <= 1e-12
    assert np.array_equal(o["saturated"], (np.abs(x["actions"]) >= F32(0.9)).sum(-1).reshape(B, M, H))
    assert o["saturated"].max() >= 1 and np.isfinite(o["logp"]).all()
    t = torch.from_numpy
    y = torch.clamp(t(x["actions"]), -1.0 + 1e-6, 1.0 - 1e-6).double()
    dist = torch.distributions.TransformedDistribution(
        torch.distributions.Normal(t(x["mus"]).double(), t(x["sigmas"]).double()),
        [torch.distributions.transforms.TanhTransform()])
    lp = dist.log_prob(y).sum(-1).numpy().reshape(B, M, H)
    assert DR.rel_err(o["logp"], lp) <= 1e-9
    o32 = _ref(B, M, x, norm=2.5, sat=0.9, dt=F32)
    for k in DR.PER_DREAM + DR.PER_WINDOW:
        if k in DR.INT:
            assert np.array_equal(o32[k], o[k]), k
        else:
            assert o32[k].dtype == F32 and DR.rel_err(o32[k], o[k]) <= 1e-4, k


# ------------------------------------------------------------------ DreamResult arithmetic
def _result(B=2, M=3, H=4, A=2, hw=(4, 5), seed=0, vector=False):
    from dreamer_amd.dream_trace import DreamResult
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    shape = (7,) if vector else (3, *hw)
    best = torch.tensor([2, 0][:B], dtype=torch.int32)
    worst = torch.tensor([1, 1][:B], dtype=torch.int32)
    return DreamResult(
        latents=r(B, M, H + 1, 2, 2), hiddens=r(B, M, H + 1, 3), actions=r(B, M, H, A), mus=r(B, M, H, A),
        sigmas=r(B, M, H, A), rewards=r(B, M, H), continues=r(B, M, H), value=r(B, M, H + 1),
        value_target=r(B, M, H + 1), norm=torch.ones(1), R_lambda=r(B, M, H), R_mc=r(B, M, H), adv=r(B, M, H),
        adv_norm=r(B, M, H), weight=r(B, M, H + 1), logp=r(B, M, H) - 2, base_entropy=r(B, M, H),
        saturated=torch.randint(0, A + 1, (B, M, H), generator=g, dtype=torch.int32), reward_mean=r(B, H),
        reward_std=r(B, H), ret_mean=r(B, H), ret_std=r(B, H), logp_mean=r(B, H), logp_std=r(B, H), alive=r(B, H + 1),
        action_spread=r(B, H), best=best, worst=worst, n_finite=torch.full((B,), M, dtype=torch.int32),
        mu=r(B, M, H + 1, *shape) - 0.5,
        frames=None if vector else torch.randint(0, 256, (B, M, H + 1, *shape), generator=g, dtype=torch.uint8),
        context=3, horizon=H, saturation=0.99)


def test_result_arithmetic():
    from dreamer_amd.dream_trace import CURVES
    B, M, H, A, hw = 2, 3, 4, 2, (4, 5)
    r = _result(B, M, H, A, hw)
    assert r.samples == M and r.frame_elems() == 3 * 4 * 5
    assert torch.equal(r.entropy(), -r.logp)
    c = r.curves()
    assert tuple(c) == CURVES
    assert [c[k].shape[0] for k in CURVES] == [H, H, H + 1, H + 1, H, H, H, H, H, H, H, H]
    assert torch.allclose(c["reward"], r.rewards.reshape(B * M, H).mean(0))
    assert torch.allclose(c["neg_logp"], -r.logp.reshape(B * M, H).mean(0))
    assert torch.allclose(c["sigma"], r.sigmas.permute(2, 0, 1, 3).reshape(H, -1).mean(1))
    assert torch.allclose(c["saturated_frac"], r.saturated.float().reshape(B * M, H).mean(0) / A)
    assert torch.equal(c["alive"], r.alive.mean(0)) and torch.equal(c["ret_std"], r.ret_std.mean(0))
    assert torch.allclose(c["value"], r.value.reshape(B * M, H + 1).mean(0))
    p = r.pick("best")
    assert set(p) == set(r._per_dream)
    for b, m in enumerate([2, 0]):
        assert torch.equal(p["R_mc"][b], r.R_mc[b, m]) and torch.equal(p["frames"][b], r.frames[b, m])
        assert torch.equal(p["latents"][b], r.latents[b, m])
    assert torch.equal(r.pick("worst")["actions"], r.actions[:, 1])
    assert torch.equal(r.pick(2)["weight"], r.weight[:, 2]) and torch.equal(r.pick(np.int64(0))["mu"], r.mu[:, 0])
    for bad in ("median", M, -1, 1.0, True):
        with pytest.raises(ValueError):
            r.pick(bad)
    v = r.video()
    assert v.dtype == torch.uint8 and v.shape == (H + 1, 3, 2 * hw[0], B * hw[1])
    for b in range(B):
        cols = slice(hw[1] * b, hw[1] * (b + 1))
        assert torch.equal(v[0][:, :hw[0], cols], r.frames[b, int(r.best[b]), 0])
        assert torch.equal(v[H][:, hw[0]:, cols], r.frames[b, int(r.worst[b]), H])
    assert r.video(which=("best", 1, "worst")).shape == (H + 1, 3, 3 * hw[0], B * hw[1])


def test_vector_result_has_no_video():
    r = _result(vector=True)
    assert r.frame_elems() == 7 and "frames" not in r.pick("best") and r.pick("best")["mu"].shape == (2, 5, 7)
    with pytest.raises(ValueError):
        r.video()


# ------------------------------------------------------------------ the binding and dr_dream_stats' checks
def test_binding_and_limits():
    from dreamer_amd import _lib as L
    lib = L.load()
    assert {"dr_dream_stats", "dr_actor_draws"} <= set(L.EXPORTED) and hasattr(lib, "dr_dream_stats")
    src = open(os.path.join(REPO, "include", "dreamer_hip.h")).read()
    defs = dict(re.findall(r"#define (DR_DREAM_STATS_\w+) (\d+)", src))
    assert int(defs["DR_DREAM_STATS_MAX_LDS_FLOATS"]) == L.DR_DREAM_STATS_MAX_LDS_FLOATS
    assert int(defs["DR_DREAM_STATS_MAX_DREAMS"]) == L.DR_DREAM_STATS_MAX_DREAMS == L.DR_ENSEMBLE_MAX_SAMPLES == 64
    fields = re.search(r"typedef struct \{([^}]*)\} dr_dream_outputs;", src).group(1)
    assert re.findall(r"\*\s*(\w+)", fields) == [n for n, _ in L.dr_dream_outputs._fields_]
    assert [n for n, _ in L.dr_dream_outputs._fields_] == list(DR.PER_DREAM + DR.PER_WINDOW)
    assert (64 | 1) * (3 * 64 + 2) <= L.DR_DREAM_STATS_MAX_LDS_FLOATS  # H = 64 at M = 64 fits


def _stats(L, B, M, H, A, inputs=(16,) * 7, out=None, outs=True):
    """dr_dream_stats with dummy non-NULL pointers: a valid call stops before the launch only at B = 0."""
    o = L.dr_dream_outputs(R_lambda=16) if out is None else out
    L.call("dr_dream_stats", B, M, H, A, *inputs, 0.99, 0.95, None, 0.99, o if outs else None, None)


def test_dream_stats_checks_arguments_without_a_gpu():
    from dreamer_amd import _lib as L
    _stats(L, 0, 3, 4, 2)  # B = 0: a no-op
    _stats(L, 0, 64, 64, 2)
    bad = [dict(B=-1, M=1, H=1, A=1), dict(B=1, M=0, H=1, A=1), dict(B=1, M=1, H=0, A=1), dict(B=1, M=1, H=1, A=0),
           dict(B=1, M=-2, H=1, A=1)]
    for kw in bad:
        with pytest.raises(L.HipError) as e:
            _stats(L, **kw)
        assert e.value.code == L.DR_E_INVALID, kw
    with pytest.raises(L.HipError) as e:  # no output asked for
        _stats(L, 1, 2, 3, 2, out=L.dr_dream_outputs())
    assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:  # no outputs struct
        _stats(L, 1, 2, 3, 2, outs=False)
    assert e.value.code == L.DR_E_INVALID
    for i in range(7):  # every input is required
        inputs = [16] * 7
        inputs[i] = None
        with pytest.raises(L.HipError) as e:
            _stats(L, 1, 2, 3, 2, inputs=inputs)
        assert e.value.code == L.DR_E_INVALID, i
    with pytest.raises(L.HipError) as e:
        _stats(L, 1, 65, 3, 2)
    assert e.value.code == L.DR_E_UNSUPPORTED
    # the documented LDS bound: (M | 1) * (3 H + 2) floats
    lim = L.DR_DREAM_STATS_MAX_LDS_FLOATS
    for M in (64, 2, 1):
        H = (lim // (M | 1) - 2) // 3
        assert (M | 1) * (3 * H + 2) <= lim < (M | 1) * (3 * (H + 1) + 2)
        _stats(L, 0, M, H, 2)  # inside the bound (B = 0, so nothing is launched)
        with pytest.raises(L.HipError) as e:
            _stats(L, 0, M, H + 1, 2)
        assert e.value.code == L.DR_E_UNSUPPORTED, (M, H)
    assert (lim // 65 - 2) // 3 >= 64
    # dr_actor_draws: no Philox state, no output
    with pytest.raises(L.HipError) as e:
        L.call("dr_actor_draws", 2, 3, 2, L.dr_noise(), 16, None)
    assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:
        L.call("dr_actor_draws", 2, 3, 0, L.dr_noise(None, None, 16, 0, 0), 16, None)
    assert e.value.code == L.DR_E_INVALID
    L.call("dr_actor_draws", 0, 3, 2, L.dr_noise(None, None, 16, 0, 0), 16, None)


# ------------------------------------------------------------------ dream_trace's ValueErrors
def _np_state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_dream_trace_argument_errors_leave_np_random_alone():
    from dreamer_amd import Dreamer
    from dreamer_amd.dream_trace import DREAM_MAX_ROWS, check_dreams
    cfg = dict(SMALL)
    cfg.update(batch_size=2, sequence_length=8, horizon=3)
    d = Dreamer(cfg, torch.device("cpu"))
    S = d.sequence_length
    R, C = d.latent_state_dims
    A = d.action_dims
    assert DREAM_MAX_ROWS == 4096
    check_dreams(1, 1)
    check_dreams(DREAM_MAX_ROWS // 64, 64)
    ones = torch.ones
    good = (ones(4, 2 * R, C), ones(3, 2 * 2 * R, C), ones(3, 2 * 2, A))  # B = 2, M = 2, Tc = 4, H = 3
    cases = [dict(samples=0), dict(samples=65), dict(samples=2.5), dict(samples=True), dict(horizon=0),
             dict(horizon=-3), dict(horizon=1.5), dict(context=0), dict(context=S + 1), dict(context=-1),
             dict(batch_size=DREAM_MAX_ROWS // 64 + 1, samples=64), dict(batch_size=DREAM_MAX_ROWS + 1),
             dict(samples=2, noise=(good[0], good[1])),
             dict(samples=2, noise=(good[0][:3], good[1], good[2])),
             dict(samples=2, noise=(good[0], good[1][:, :-1], good[2])),
             dict(samples=2, noise=(good[0], good[1], ones(3, 2 * 2, A + 1))),
             dict(samples=3, noise=good),
             dict(starts=np.array([0, 9, 20]), samples=2, noise=good)]
    np.random.seed(5)
    before = np.random.get_state()
    for kw in cases:
        with pytest.raises(ValueError):
            d.dream_trace(**kw)
        assert _np_state_equal(before, np.random.get_state()), kw
    with pytest.raises(ValueError):
        d.evaluate_dreams(batches=0)
    with pytest.raises(ValueError):
        d.evaluate_dreams(context=S, real=True)
    assert _np_state_equal(before, np.random.get_state())
