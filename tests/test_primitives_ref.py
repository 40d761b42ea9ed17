"""The float64 references of tests/primitives_ref.py pinned on the CPU: they
agree with oracle.dreamer_oracle (itself pinned byte-for-byte to the
reference's fixtures, tests/test_oracle_golden.py) on ordinary inputs to
float32 rounding, and the two-hot reference behaves at the edge inputs the GPU
tests use.  Keeps a wrong reference from failing a right kernel, or passing a
wrong one."""
import math

import numpy as np
import pytest
import torch

import primitives_ref as PR
from oracle import dreamer_oracle as O

U = PR.U
BUCKETS = torch.linspace(-20, 20, 255)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_lambda_returns_matches_oracle():
    g = _gen(1)
    B, H = 7, 15
    r = torch.randn(B, H, generator=g)
    c = torch.rand(B, H, generator=g)
    c[2, 4] = 0.0
    V = torch.randn(B, H + 1, generator=g) * 3
    for gamma, lam in ((0.99, 0.95), (1.0, 0.0), (1.0, 1.0), (0.5, 0.3)):
        want = O.lambda_returns(V.unsqueeze(-1), r.unsqueeze(-1), c.unsqueeze(-1), gamma, lam).squeeze(-1)
        got = PR.lambda_returns(r, c, V, gamma, lam)
        A = PR.lambda_returns_abs(r, c, V, gamma, lam)
        # the oracle runs the recursion in float32: 4 roundings a step, and gamma / lam as float32 here
        steps = torch.arange(H, 0, -1, dtype=torch.float64)
        assert bool(((got - want.double()).abs() <= 8 * steps * U * A).all()), (gamma, lam)
    # an episode end cuts the return off exactly
    assert float(PR.lambda_returns(r, c, V, 0.99, 0.95)[2, 4]) == float(r[2, 4])


def test_symlog_symexp_match_oracle():
    x = torch.tensor([-1e9, -30.0, -20.0, -1.5, -1e-3, -0.0, 0.0, 1e-3, 1.5, 20.0, 25.0, 1e9])
    # float32 on the oracle's side: 1 + |x| rounds (absolute U in the log), then the log (relative);
    # exp(|x|) rounds relative to itself before the 1 is taken off
    np.testing.assert_allclose(PR.symlog(x).numpy(), O.symlog(x).double().numpy(), rtol=4 * U, atol=2 * U)
    err = (PR.symexp(x) - O.symexp(x).double()).abs()
    assert bool((err <= 4 * U * torch.exp(x.double().abs().clamp(max=20))).all())
    assert float(PR.symexp(torch.tensor(25.0))) == math.expm1(20.0)
    assert float(PR.symexp(torch.tensor(-1e9))) == -math.expm1(20.0)


def test_bucket_value_matches_oracle():
    g = _gen(2)
    logits = torch.randn(9, 255, generator=g) * 2
    want = O.symexp(torch.sum(torch.softmax(logits, -1) * BUCKETS, dim=-1, keepdim=True)).squeeze(-1)
    got = PR.bucket_value(logits, BUCKETS)
    E, Eabs = PR.bucket_expectation(logits, BUCKETS)
    tol = (255 + 12) * U * Eabs * torch.exp(E.abs()) + 4 * U * torch.exp(E.abs())
    assert bool(((got - want.double()).abs() <= tol).all())


def test_twohot_matches_oracle():
    g = _gen(3)
    v = torch.randn(64, 1, generator=g) * 12  # some beyond +-20
    want = O.twohot(v, BUCKETS)
    got = PR.twohot(v.squeeze(-1), BUCKETS)
    # w = (v - b_lo) / (step + 1e-8) in float32: error about ulp(20) / step
    assert float((got - want.double()).abs().max()) <= 4 * U * 20 / (40 / 254)
    assert int((v.abs() > 20).sum()) > 0 and bool(((want > 0).sum(-1) <= 2).all())


def twohot_edge_values():
    """The symlog values the GPU tests put returns on: exact bucket values
    (first, middle, last but one, last), one float32 step either side of a
    middle bucket, 0, and beyond both ends."""
    b = BUCKETS
    mid = 100
    return {
        "first": float(b[0]), "middle": float(b[mid]), "last_but_one": float(b[253]), "last": float(b[254]),
        "middle_minus": float(np.nextafter(np.float32(b[mid]), np.float32(-np.inf))),
        "middle_plus": float(np.nextafter(np.float32(b[mid]), np.float32(np.inf))),
        "zero": 0.0, "below": float(PR.symlog(torch.tensor(-1e9))), "above": float(PR.symlog(torch.tensor(1e9))),
    }


@pytest.mark.parametrize("name", sorted(twohot_edge_values()))
def test_twohot_edges(name):
    v = twohot_edge_values()[name]
    th = PR.twohot(torch.tensor([v]), BUCKETS)[0]
    assert abs(float(th.sum()) - 1.0) <= 1e-15
    assert float(th.min()) >= 0.0
    assert int((th > 0).sum()) <= 2
    on = {"first": 0, "middle": 100, "last_but_one": 253, "last": 254, "below": 0, "above": 254}
    if name == "zero":  # torch.linspace(-20, 20, 255)[127] is a rounding error away from 0, not 0
        assert abs(float(BUCKETS[127])) <= 20 * 2 * U
        assert float(th[127]) >= 1.0 - 1e-5
    elif name in on:  # wholly on that bucket, up to the 1e-8 of the reference's denominator
        k = on[name]
        assert float(th[k]) >= 1.0 - 1e-7, (name, float(th[k]))
        assert float(BUCKETS[k]) == (v if name not in ("below", "above") else float(BUCKETS[k]))
    else:  # one float32 step off a bucket: almost all of the mass on it, the rest on the neighbour on that side
        assert float(th[100]) >= 1.0 - 1e-4
        other = 99 if name == "middle_minus" else 101
        assert float(th[other]) > 0.0


def test_twohot_expectation_recovers_value():
    """sum(twohot(v) * buckets) == clamp(v): the defining property of the encoding."""
    v = torch.linspace(-23, 23, 1001, dtype=torch.float64)
    th = PR.twohot(v, BUCKETS)
    back = (th * BUCKETS.double()).sum(-1)
    assert float((back - v.clamp(-20, 20)).abs().max()) <= 1e-6  # the 1e-8 in the denominator


def test_tanh_normal_logprob_matches_oracle():
    g = _gen(4)
    a = torch.tanh(torch.randn(33, 5, 3, generator=g))
    a[0, 0, 0], a[0, 0, 1], a[0, 0, 2] = 1.0, -1.0, 0.0
    mu = torch.randn(33, 5, 3, generator=g)
    sigma = torch.rand(33, 5, 3, generator=g) * 2 + 0.0077
    want = O.tanh_normal_logprob(a, mu, sigma)
    terms, mag = PR.tanh_normal_logprob_terms(a, mu, sigma)
    got = terms.sum(-1)
    # ~20 float32 operations per term on the oracle's side, relative to the terms' magnitudes
    assert bool(((got - want.double()).abs() <= 40 * U * mag.sum(-1)).all())
    # the clamp is the float32 one: 1 - 17 * 2^-24
    assert float(PR.clamp_actions(torch.tensor([1.0, -1.0, 1.0 - 1e-7]))[0]) == 1.0 - 17 * U
    assert float(PR.clamp_actions(torch.tensor([1.0 - 1e-7]))[0]) == 1.0 - 17 * U
    assert float(PR.clamp_actions(torch.tensor([-1.0]))[0]) == -(1.0 - 17 * U)


def test_actor_grads_match_closed_form():
    """Autograd of the float64 actor loss equals the closed form the kernel
    implements: dL/dmu = s (nu - adv/norm) d / sigma^2, dL/dsigma = s (nu -
    adv/norm) (d^2 / sigma^3 - 1 / sigma)."""
    g = _gen(5)
    B, H, A = 5, 3, 2
    a = torch.tanh(torch.randn(B, H, A, generator=g))
    mu, sigma = torch.randn(B, H, A, generator=g), torch.rand(B, H, A, generator=g) + 0.1
    R, V = torch.randn(B, H, generator=g), torch.randn(B, H + 1, generator=g)
    loss, gm, gs = PR.actor_loss_and_grads(mu, sigma, a, R, V, 37.5, 3e-4, 0.25)
    d = torch.atanh(PR.clamp_actions(a)) - mu.double()
    gl = 0.25 * (float(np.float32(3e-4)) - (R.double() - V.double()[:, :-1]) / 37.5).unsqueeze(-1)
    s = sigma.double()
    np.testing.assert_allclose(gm.numpy(), (gl * d / s ** 2).numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gs.numpy(), (gl * (d * d / s ** 3 - 1 / s)).numpy(), rtol=1e-11, atol=1e-14)
    want = O.tanh_normal_logprob(a, mu, sigma)
    adv = (R - V[:, :-1]) / 37.5
    ref = torch.mean(-(want * adv) - (3e-4 * (-want)))
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
