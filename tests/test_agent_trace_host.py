"""Host-side checks of the agent trace that need no GPU: the AgentTraceResult
helpers on hand-made tensors against numpy, the window arithmetic against a
brute-force loop, the length check, and the argument checks of the three new C
entry points, which fail before any device work."""
import math

import numpy as np
import pytest
import torch

from formula import SMALL


def _result(B=3, T=5, A=2, nb=7, seed=0, value=None, returns=None):
    from dreamer_amd import AgentTraceResult
    g = torch.Generator().manual_seed(seed)
    bt = lambda: torch.randn(B, T, generator=g)
    bh = lambda: torch.randn(B, T - 1, generator=g)
    bta = lambda: torch.randn(B, T, A, generator=g)
    return AgentTraceResult(latents=torch.zeros(B, T, 4, 4), hiddens=torch.zeros(B, T, 8),
                            value=bt() if value is None else value, value_target=bt(), value_entropy=bt(),
                            value_std_symlog=bt(), critic_logits=torch.randn(B, T, nb, generator=g), actor_mu=bta(),
                            actor_sigma=bta().abs(), actions=bta().tanh(), action_logprob=bt(),
                            policy_entropy_base=bt(), action_logprob_dims=bta(), reward=bh(), cont=torch.ones(B, T - 1),
                            returns_lambda=bh() if returns is None else returns, returns_mc=bh(), td=bh(),
                            critic_ce=bh(), length=T)


def test_result_helpers_match_numpy():
    B, T = 3, 5
    r = _result(B, T)
    V, R, Rmc = r.value.numpy().astype(np.float64), r.returns_lambda.numpy().astype(np.float64), \
        r.returns_mc.numpy().astype(np.float64)
    adv = r.advantage()
    assert adv.shape == (B, T - 1)
    assert np.allclose(adv.numpy(), R - V[:, :-1], rtol=0, atol=1e-6)
    assert torch.equal(adv, r.returns_lambda - r.value[:, :-1])
    ve = r.value_error()
    assert ve.shape == (B, T - 1) and torch.equal(ve, r.value[:, :-1] - r.returns_mc)
    assert np.allclose(ve.numpy(), V[:, :-1] - Rmc, rtol=0, atol=1e-6)
    ev = float(r.explained_variance())
    want = 1.0 - np.var(R - V[:, :-1]) / np.var(R)  # population variances over all (b, t <= T-2)
    assert math.isclose(ev, want, rel_tol=1e-5, abs_tol=1e-6), (ev, want)
    # a perfect critic explains everything; a constant one nothing
    V1 = torch.cat((r.returns_lambda, torch.zeros(B, 1)), dim=1)
    assert float(_result(B, T, value=V1, returns=r.returns_lambda).explained_variance()) == 1.0
    ev0 = float(_result(B, T, value=torch.full((B, T), 0.25), returns=r.returns_lambda).explained_variance())
    assert abs(ev0) <= 1e-6


def test_explained_variance_zero_variance_is_nan():
    r = _result(2, 4, returns=torch.full((2, 3), 1.5))
    ev = r.explained_variance()
    assert math.isnan(float(ev))
    assert r.advantage().shape == (2, 3)


def test_trace_slots_match_brute_force():
    """State t <-> frame and action slot start + t; the reward / continue flag of
    the transition out of state t sit in the same slot (modulo the ring), for
    every trace length a window of S = 8 allows.  The slot of state t + 1's
    head target in closed_loop is this slot: the two alignments agree."""
    from dreamer_amd.agent_trace import action_step, trace_slots, transition_step
    from dreamer_amd.closed_loop import target_step
    cap, S = 13, 8
    starts = [0, 5, 12, 9]
    for T in range(2, S + 1):
        fs, ts = trace_slots(starts, T, cap)
        assert fs.shape == (len(starts), T) and ts.shape == (len(starts), T - 1)
        for b, s0 in enumerate(starts):
            for t in range(T):
                assert action_step(t) == t and fs[b, t].item() == (s0 + t) % cap
                if t <= T - 2:
                    assert transition_step(t) == t and ts[b, t].item() == (s0 + t) % cap
                    assert target_step(t + 1) == transition_step(t)
    for f in (action_step, transition_step):
        with pytest.raises(ValueError):
            f(-1)


def test_check_length():
    from dreamer_amd.agent_trace import check_length
    check_length(2, 2)
    check_length(2, 8)
    check_length(8, 8)
    for T in (1, 0, 9, -1):
        with pytest.raises(ValueError):
            check_length(T, 8)


def _invalid(L, name, *args):
    with pytest.raises(L.HipError) as e:
        L.call(name, *args)
    assert e.value.code == L.DR_E_INVALID, (name, args)


def test_agent_trace_argument_errors_need_no_gpu():
    """A bad length raises before the device is touched; the three C entry
    points refuse bad dimensions, and good dimensions with null pointers, with
    DR_E_INVALID on the host."""
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    d = Dreamer(dict(SMALL), torch.device("cpu"))
    S = d.sequence_length
    for T in (1, S + 1):
        with pytest.raises(ValueError):
            d.agent_trace(starts=np.array([0]), length=T)
    p = 256  # a non-null address that is never dereferenced: the checks come before any launch
    # dr_replay_returns(B, T, rewards, rew_sb, continues, cont_sb, symlog, V, gamma, lam, R_lambda, R_mc, td, stream)
    for B, T in ((1, 1), (1, 0), (-1, 4)):
        _invalid(L, "dr_replay_returns", B, T, p, 8, p, 8, 0, p, 0.99, 0.95, p, p, p, None)
    _invalid(L, "dr_replay_returns", 1, 4, p, 2, p, 8, 0, p, 0.99, 0.95, p, p, p, None)  # stride < T - 1
    _invalid(L, "dr_replay_returns", 1, 4, None, 8, None, 8, 0, None, 0.99, 0.95, None, None, None, None)
    for k in (2, 4, 7, 10):  # each required pointer in turn
        a = [2, 4, p, 8, p, 8, 1, p, 0.99, 0.95, p, None, None, None]
        a[k] = None
        _invalid(L, "dr_replay_returns", *a)
    # dr_value_stats(B, T, Tt, nb, logits, ldl, buckets, target, entropy, std_symlog, ce, stream)
    for B, T, Tt, nb, ldl in ((1, 3, 2, 1, 8), (1, 3, 2, 1025, 1025), (1, 3, 4, 7, 7), (-1, 3, 2, 7, 7), (1, 0, 0, 7, 7),
                              (1, 3, -1, 7, 7), (1, 3, 2, 7, 6)):
        _invalid(L, "dr_value_stats", B, T, Tt, nb, p, ldl, p, p, p, p, p, None)
    _invalid(L, "dr_value_stats", 1, 3, 2, 7, None, 7, None, None, None, None, None, None)
    _invalid(L, "dr_value_stats", 1, 3, 2, 7, None, 7, p, p, p, p, p, None)   # no logits
    _invalid(L, "dr_value_stats", 1, 3, 2, 7, p, 7, None, p, p, p, p, None)   # no buckets
    _invalid(L, "dr_value_stats", 1, 3, 2, 7, p, 7, p, p, p, p, None, None)   # target without ce
    _invalid(L, "dr_value_stats", 1, 3, 2, 7, p, 7, p, None, p, p, p, None)   # ce without target
    _invalid(L, "dr_value_stats", 1, 3, 0, 7, p, 7, p, p, p, p, p, None)      # Tt = 0 with target and ce
    _invalid(L, "dr_value_stats", 1, 3, 0, 7, p, 7, p, None, None, None, None, None)  # nothing asked for
    # dr_action_logprob(B, T, A, mu, sigma, actions, act_sb, act_st, logp, logp_dims, base_entropy, stream)
    for B, T, A in ((1, 3, 0), (-1, 3, 2), (1, 0, 2), (1, 3, -1)):
        _invalid(L, "dr_action_logprob", B, T, A, p, p, p, 6, 2, p, p, p, None)
    _invalid(L, "dr_action_logprob", 1, 3, 2, None, None, None, 6, 2, None, None, None, None)
    for k in (3, 4, 5, 8):
        a = [1, 3, 2, p, p, p, 6, 2, p, None, None, None]
        a[k] = None
        _invalid(L, "dr_action_logprob", *a)
    # an empty batch is a no-op, not an error (good pointers, nothing launched)
    L.call("dr_replay_returns", 0, 4, p, 8, p, 8, 1, p, 0.99, 0.95, p, None, None, None)
    L.call("dr_value_stats", 0, 3, 2, 7, p, 7, p, p, p, p, p, None)
    L.call("dr_action_logprob", 0, 3, 2, p, p, p, 6, 2, p, None, None, None)
