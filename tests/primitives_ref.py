"""float64 references of the value-learning and gradient-norm primitives
(dreamer_amd/csrc/ops.hip), written straight from the reference formulas:

  lambda returns             Agent.py:156-172
  symlog / symexp / two-hot  DreamerUtils.py:29-50
  bucket expectation         DynamicsPredictors.py:70-74, Agent.py:237-241
  critic two-hot CE          Agent.py:127-135
  actor loss                 Agent.py:105-125

Every function takes the float32 values the kernel sees and continues in
float64.  The one place where a float32 rounding belongs to the operation
itself is the clamp of the actions to +-(1 - 1e-6) (a float32 constant,
1 - 17 * 2^-24): clamp_actions applies it in float32 first.

tests/test_primitives_ref.py pins these against oracle.dreamer_oracle on the
CPU; tests/test_gpu_primitives.py holds the HIP kernels to them.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of float32

F64 = torch.float64


def f64(x):
    return torch.as_tensor(x).to(F64)


# ----------------------------------------------------------------------------
# DreamerUtils.py
# ----------------------------------------------------------------------------
def symlog(x):  # DreamerUtils.py:29-30
    x = f64(x)
    return torch.sign(x) * torch.log1p(torch.abs(x))


def symexp(x):  # DreamerUtils.py:35-37
    x = torch.clamp(f64(x), -20.0, 20.0)
    return torch.sign(x) * torch.expm1(torch.abs(x))


def twohot_parts(v, buckets):
    """(lo, w) of DreamerUtils.to_twohot (39-50): weight 1 - w on bucket lo and
    w on bucket lo + 1.  v: any shape, buckets: [nb] ascending."""
    v, b = f64(v), f64(buckets)
    nb = b.numel()
    vc = torch.clamp(v, min=float(b.min()), max=float(b.max()))
    lo = torch.searchsorted(b, vc.contiguous(), right=True) - 1
    lo = torch.clamp(lo, max=nb - 2)
    w = (vc - b[lo]) / (b[lo + 1] - b[lo] + 1e-8)
    return lo, w


def twohot(v, buckets):
    """DreamerUtils.to_twohot as a dense [..., nb] float64 tensor."""
    lo, w = twohot_parts(v, buckets)
    nb = int(torch.as_tensor(buckets).numel())
    out = torch.zeros(tuple(lo.shape) + (nb,), dtype=F64)
    out.scatter_(-1, lo.unsqueeze(-1), (1.0 - w).unsqueeze(-1))
    out.scatter_(-1, (lo + 1).unsqueeze(-1), w.unsqueeze(-1))
    return out


# ----------------------------------------------------------------------------
# lambda returns (Agent.py:156-172)
# ----------------------------------------------------------------------------
def lambda_returns(r, c, V, gamma, lam):
    """r, c: [B, H]; V: [B, H + 1]; gamma, lam: the float32 values the entry
    point receives (1 - lam is formed from the float32 lam, as the reference
    forms it from its python float).  Returns R [B, H] in float64."""
    r, c, V = f64(r), f64(c), f64(V)
    gamma, lam = float(np.float32(gamma)), float(np.float32(lam))
    H = r.shape[1]
    nxt = r[:, H - 1] + gamma * c[:, H - 1] * V[:, H]
    out = [nxt]
    for t in reversed(range(H - 1)):
        nxt = r[:, t] + gamma * c[:, t] * ((1.0 - lam) * V[:, t + 1] + lam * nxt)
        out.insert(0, nxt)
    return torch.stack(out, dim=1)


def lambda_returns_abs(r, c, V, gamma, lam):
    """The same recursion on absolute values: A_t bounds every intermediate of
    R_t, so rounding errors of step t are relative to A_t."""
    return lambda_returns(f64(r).abs(), f64(c).abs(), f64(V).abs(), abs(gamma), abs(lam))


# ----------------------------------------------------------------------------
# bucket expectation (DynamicsPredictors.py:70-74, Agent.py:237-241)
# ----------------------------------------------------------------------------
def bucket_expectation(logits, buckets):
    """(E, Eabs): sum softmax(l) * b and sum softmax(l) * |b| per row."""
    p = torch.softmax(f64(logits), dim=-1)
    b = f64(buckets)
    return (p * b).sum(-1), (p * b.abs()).sum(-1)


def bucket_value(logits, buckets):
    return symexp(bucket_expectation(logits, buckets)[0])


# ----------------------------------------------------------------------------
# critic two-hot cross-entropy (Agent.py:127-135)
# ----------------------------------------------------------------------------
def critic_ce_rows(logits, R, buckets):
    """Per-row -sum(twohot(symlog(R)) * log_softmax(logits)); logits [..., nb],
    R [...]."""
    th = twohot(symlog(R), buckets)
    return -(th * torch.log_softmax(f64(logits), dim=-1)).sum(-1)


# ----------------------------------------------------------------------------
# actor loss (Agent.py:105-125)
# ----------------------------------------------------------------------------
def clamp_actions(a):
    """torch.clamp(a, -1 + 1e-6, 1 - 1e-6) on the float32 actions (Agent.py:113-114),
    then float64."""
    a = torch.as_tensor(a, dtype=torch.float32)
    return torch.clamp(a, -1.0 + 1e-6, 1.0 - 1e-6).to(F64)


def tanh_normal_logprob_terms(a, mu, sigma):
    """Per action dimension: log_prob of TransformedDistribution(Normal(mu, sigma),
    [TanhTransform()]) at clamp(a) (Agent.py:110-115), and the sum of the
    magnitudes of the terms it is built from (its condition-weighted size)."""
    y = clamp_actions(a)
    mu, sigma = f64(mu), f64(sigma)
    x = torch.atanh(y)
    d = x - mu
    quad = d * d / (2.0 * sigma * sigma)
    half_log_2pi = math.log(math.sqrt(2.0 * math.pi))
    lp = -quad - torch.log(sigma) - half_log_2pi
    sp = torch.nn.functional.softplus(-2.0 * x)
    ladj = 2.0 * (math.log(2.0) - x - sp)
    D = x.abs() + mu.abs()
    mag = D * D / (2.0 * sigma * sigma) + torch.log(sigma).abs() + half_log_2pi \
        + 2.0 * (math.log(2.0) + x.abs() + sp)
    return lp - ladj, mag


def tanh_normal_logprob(a, mu, sigma):
    return tanh_normal_logprob_terms(a, mu, sigma)[0].sum(-1)


def actor_rows(mu, sigma, a, R, V, norm, nu):
    """Row losses [B, H] of Agent.py:116-124: -(logp * adv / norm) - nu * (-logp),
    adv = R - V[:, :-1].  mu, sigma, a: [B, H, A]; R [B, H]; V [B, H + 1]."""
    logp = tanh_normal_logprob(a, mu, sigma)
    sadv = (f64(R) - f64(V)[:, :-1]) / float(np.float32(norm))
    nu = float(np.float32(nu))
    return -(logp * sadv) - (nu * (-logp))


def actor_loss_and_grads(mu, sigma, a, R, V, norm, nu, scale):
    """(mean row loss, d(scale * sum rows)/dmu, d(scale * sum rows)/dsigma) by
    float64 autograd."""
    mu = f64(mu).clone().requires_grad_(True)
    sigma = f64(sigma).clone().requires_grad_(True)
    rows = actor_rows(mu, sigma, a, R, V, norm, nu)
    g_mu, g_sigma = torch.autograd.grad(float(np.float32(scale)) * rows.sum(), [mu, sigma])
    return rows.detach().mean(), g_mu, g_sigma
