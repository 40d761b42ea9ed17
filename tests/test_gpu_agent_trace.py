"""Agent trace on replay windows (Dreamer.agent_trace, evaluate_values,
dr_replay_returns, dr_value_stats, dr_action_logprob).

The three kernels against the float64 references of tests/primitives_ref.py,
by the project's accuracy rule (test_latent_stats_kernel): the bound is 8 x
the error the same formula evaluated in f32 on the CPU makes against float64
on these inputs, at least 4 * 2^-24 and never more than 1e-4, in the units
each test states.  The one-call path against the separate entry points, bit
for bit, and against oracle.dreamer_oracle teacher-forced on the GPU's own
states.  Run on the MI355X box: pytest -m gpu.  Measured values: DESIGN
section 5i."""
import math

import numpy as np
import pytest
import torch

import primitives_ref as PR
from formula import FULL, SMALL, replay_data
from gpu_helpers import CFG, build, cpu
from oracle import dreamer_oracle as O
from test_gpu_closed_loop import _noise, _oracle
from test_gpu_open_loop import A, N_FILL, _same, _windows

pytestmark = pytest.mark.gpu
U = PR.U
F64 = torch.float64


def _api():
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    return L, hip.stream()


def _bound(yardstick):
    return min(max(8.0 * yardstick, 4.0 * U), 1e-4)


def _rel(got, ref):
    """max |got - ref| / max(1, |ref|)"""
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _nan(*shape, gpu):
    return torch.full(shape, float("nan"), device=gpu)


# ------------------------------------------------------------------ dr_value_stats
def _value_stats(gpu, logits, buckets, B, T, Tt, target, ldl=None, want=("entropy", "std", "ce")):
    """logits [B*T][nb] on the CPU; returns CPU (entropy, std, ce), None where not asked for."""
    L, st = _api()
    nb = logits.shape[1]
    ldl = nb if ldl is None else ldl
    lg = torch.full((B * T, ldl), float("nan"))
    lg[:, :nb] = logits
    lgd, bd = lg.to(gpu), buckets.to(gpu)
    ent = _nan(B, T, gpu=gpu) if "entropy" in want else None
    sd = _nan(B, T, gpu=gpu) if "std" in want else None
    ce = tg = None
    if Tt > 0 and "ce" in want:
        ce, tg = _nan(B, Tt, gpu=gpu), target.reshape(B, Tt).contiguous().to(gpu)
    L.call("dr_value_stats", B, T, Tt if ce is not None else 0, nb, L.ptr(lgd), ldl, L.ptr(bd), L.ptr(tg), L.ptr(ent),
           L.ptr(sd), L.ptr(ce), st)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu()
    return c(ent), c(sd), c(ce)


def _stats_ref(logits, buckets, dt):
    """(entropy, spread) of the issue's formulas in dtype dt on the CPU."""
    l, b = logits.to(dt), buckets.to(dt)
    ls = torch.log_softmax(l, -1)
    p = ls.exp()
    ent = -(p * ls).sum(-1)
    mean = (p * b).sum(-1, keepdim=True)
    return ent, ((p * (b - mean) ** 2).sum(-1)).sqrt()


def _ce32(logits, R, buckets):
    """Agent.py:127-135 in f32 on the CPU (the oracle's symlog and two-hot)."""
    th = O.twohot(O.symlog(R).unsqueeze(-1), buckets)
    return -(th * torch.log_softmax(logits, -1)).sum(-1)


@pytest.mark.parametrize("nb", [255, 65, 7, 2])
def test_value_stats_kernel(nb, gpu):
    """dr_value_stats directly; units: relative to max(1, |ref|).  nb = 255 =
    3 * 64 + 63 covers the lane-stride tail, 65 crosses one wave, 2 the
    lo <= nb - 2 clamp."""
    L, st = _api()
    M = 37
    g = torch.Generator().manual_seed(nb)
    buckets = torch.linspace(-20, 20, nb)
    logits = torch.randn(M, nb, generator=g) * 3
    target = O.symexp(torch.randn(M, generator=g) * 3)
    logits[0] = 1.5                                        # all equal
    logits[1], logits[2] = -80.0, -80.0                    # one-hots
    logits[1, 0], logits[2, nb - 1] = 80.0, 80.0
    target[3], target[4] = 1e12, -1e12                     # clamped to the end buckets
    target[5] = 0.0
    target[6] = float(PR.symexp(buckets[nb // 3]))         # on a bucket (to f32 rounding: either side of it)
    logits[36], target[36] = logits[7], target[7]          # a row copied to another position
    ent64, sd64 = _stats_ref(logits, buckets, F64)
    ce64 = PR.critic_ce_rows(logits, target, buckets)
    ent32, sd32 = _stats_ref(logits, buckets, torch.float32)
    y = dict(entropy=_rel(ent32, ent64), std=_rel(sd32, sd64), ce=_rel(_ce32(logits, target, buckets), ce64))
    b = {k: _bound(v) for k, v in y.items()}
    ent, sd, ce = _value_stats(gpu, logits, buckets, M, 1, 1, target)
    ent, sd, ce = ent.reshape(M), sd.reshape(M), ce.reshape(M)
    e = dict(entropy=_rel(ent, ent64), std=_rel(sd, sd64), ce=_rel(ce, ce64))
    for k in ("entropy", "std", "ce"):
        print(f"value_stats nb={nb} {k}: f32-CPU yardstick {y[k]:.3e}, kernel max rel err {e[k]:.3e} "
              f"(bound {b[k]:.3e})")
    for t in (ent, sd, ce):
        assert bool(torch.isfinite(t).all())
    assert e["entropy"] <= b["entropy"] and e["std"] <= b["std"] and e["ce"] <= b["ce"], (e, b)
    assert abs(ent[0].item() - math.log(nb)) <= b["entropy"] * max(1.0, math.log(nb))
    for r in (1, 2):  # one-hot: no entropy, no spread, a finite loss
        assert abs(ent[r].item()) <= b["entropy"] and abs(sd[r].item()) <= b["std"]
    # the same row at another position, and alone in a call: the same bits
    for t in (ent, sd, ce):
        assert t[36].item() == t[7].item()
    one = _value_stats(gpu, logits[7:8], buckets, 1, 1, 1, target[7:8])
    assert all(o.reshape(1)[0].item() == t[7].item() for o, t in zip(one, (ent, sd, ce)))
    # rows (b, t) of B = 5, T = 4 with a padded row stride; targets for t < 3 only
    B, T, Tt = 5, 4, 3
    rows = torch.arange(B * T).reshape(B, T)
    e2, s2, c2 = _value_stats(gpu, logits[:B * T], buckets, B, T, Tt, target[rows[:, :Tt]], ldl=nb + 3)
    assert torch.equal(e2.reshape(-1), ent[:B * T]) and torch.equal(s2.reshape(-1), sd[:B * T])
    assert c2.shape == (B, Tt) and torch.equal(c2, ce[rows[:, :Tt]])
    # optional outputs may be NULL without changing the others' bits
    for want in (("std", "ce"), ("entropy", "ce"), ("ce",), ("entropy", "std"), ("entropy",), ("std",)):
        got = dict(zip(("entropy", "std", "ce"), _value_stats(gpu, logits, buckets, M, 1, 1, target, want=want)))
        for k, full in (("entropy", ent), ("std", sd), ("ce", ce)):
            if k in want:
                assert torch.equal(got[k].reshape(M), full), (want, k)
            else:
                assert got[k] is None
    # Tt = 0 goes with no target and no ce; a ce given all the same is refused and not touched
    lgd, bd = logits.to(gpu), buckets.to(gpu)
    eo, keep, tg = _nan(M, 1, gpu=gpu), _nan(M, 1, gpu=gpu), target.to(gpu)
    with pytest.raises(L.HipError) as err:
        L.call("dr_value_stats", M, 1, 0, nb, L.ptr(lgd), nb, L.ptr(bd), L.ptr(tg), L.ptr(eo), None, L.ptr(keep), st)
    assert err.value.code == L.DR_E_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(keep).all()) and bool(torch.isnan(eo).all())


# ------------------------------------------------------------------ dr_action_logprob
def _action_logprob(gpu, mu, sigma, actions, B, T, act_sb, act_st, want=("dims", "base")):
    """mu, sigma [B*T][A]; actions: the array the strides index; returns CPU (logp, dims, base)."""
    L, st = _api()
    Ad = mu.shape[-1]
    md, sd, ad = mu.contiguous().to(gpu), sigma.contiguous().to(gpu), actions.contiguous().to(gpu)
    lp = _nan(B, T, gpu=gpu)
    dims = _nan(B, T, Ad, gpu=gpu) if "dims" in want else None
    base = _nan(B, T, gpu=gpu) if "base" in want else None
    L.call("dr_action_logprob", B, T, Ad, L.ptr(md), L.ptr(sd), L.ptr(ad), act_sb, act_st, L.ptr(lp), L.ptr(dims),
           L.ptr(base), st)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu()
    return c(lp), c(dims), c(base)


def _logprob_terms32(a, mu, sigma):
    """tanh_normal_logprob_terms' formula in f32 on the CPU: the yardstick."""
    y = torch.clamp(a, -1.0 + 1e-6, 1.0 - 1e-6)
    x = torch.atanh(y)
    lp = -((x - mu) ** 2) / (2 * sigma ** 2) - sigma.log() - math.log(math.sqrt(2 * math.pi))
    ladj = 2.0 * (math.log(2.0) - x - torch.nn.functional.softplus(-2.0 * x))
    return lp - ladj


@pytest.mark.parametrize("Ad", [3, 1, 8])
def test_action_logprob_kernel(Ad, gpu):
    """dr_action_logprob directly; units: 2^-24 * mag per dimension (mag from
    tanh_normal_logprob_terms), 2^-24 * sum_i mag for the row sum and for
    base_entropy."""
    M = 37
    g = torch.Generator().manual_seed(10 + Ad)
    mu = torch.randn(M, Ad, generator=g) * 2
    sg_min = float(torch.nn.functional.softplus(torch.tensor(-5.0)) + 1e-3)
    sigma = torch.nn.functional.softplus(torch.rand(M, Ad, generator=g) * 7 - 5) + 1e-3
    a = torch.tanh(torch.randn(M, Ad, generator=g) * 1.5)
    a[0], a[1], a[2] = 1.0, -1.0, 0.0
    pat = lambda v: torch.tensor([v[i % 3] for i in range(Ad)])
    a[3], mu[3], sigma[3] = pat((1.0, -1.0, 0.5)), pat((-5.0, 5.0, 0.0)), sg_min  # |logp| ~ 1.3e6
    a[36], mu[36], sigma[36] = a[7], mu[7], sigma[7]
    t64, mag = PR.tanh_normal_logprob_terms(a, mu, sigma)
    base64 = (0.5 + 0.5 * math.log(2 * math.pi) + sigma.double().log()).sum(-1)
    t32 = _logprob_terms32(a, mu, sigma)
    base32 = (0.5 + 0.5 * math.log(2 * math.pi) + sigma.log()).sum(-1)
    units = lambda got, ref, scale: float(((got.double() - ref).abs() / (U * scale)).max())
    y = dict(dims=units(t32, t64, mag), row=units(t32.sum(-1), t64.sum(-1), mag.sum(-1)),
             base=units(base32, base64, mag.sum(-1)))
    b = {k: _bound(v * U) / U for k, v in y.items()}  # in units of 2^-24 * mag
    lp, dims, base = _action_logprob(gpu, mu, sigma, a, M, 1, Ad, Ad)
    lp, dims, base = lp.reshape(M), dims.reshape(M, Ad), base.reshape(M)
    e = dict(dims=units(dims, t64, mag), row=units(lp, t64.sum(-1), mag.sum(-1)),
             base=units(base, base64, mag.sum(-1)))
    for k in ("dims", "row", "base"):
        print(f"action_logprob A={Ad} {k}: f32-CPU yardstick {y[k]:.2f}, kernel max err {e[k]:.2f} "
              f"(bound {b[k]:.2f}) x 2^-24 mag")
    for t in (lp, dims, base):
        assert bool(torch.isfinite(t).all())
    assert abs(lp[3].item()) > 1e6 / 3
    assert e["dims"] <= b["dims"] and e["row"] <= b["row"] and e["base"] <= b["base"], (e, b)
    # logp is the ascending f32 sum of its terms
    acc = np.zeros(M, dtype=np.float32)
    for i in range(Ad):
        acc = (acc + dims[:, i].numpy()).astype(np.float32)
    assert np.array_equal(acc, lp.numpy())
    # position independence; optional outputs
    assert lp[36].item() == lp[7].item() and base[36].item() == base[7].item() and torch.equal(dims[36], dims[7])
    one = _action_logprob(gpu, mu[7:8], sigma[7:8], a[7:8], 1, 1, Ad, Ad)
    assert one[0].item() == lp[7].item() and one[2].item() == base[7].item() and torch.equal(one[1].reshape(Ad), dims[7])
    lp2, d2, b2 = _action_logprob(gpu, mu, sigma, a, M, 1, Ad, Ad, want=())
    assert d2 is None and b2 is None and torch.equal(lp2.reshape(M), lp)
    # rows (b, t) of B = 3, T = 5 read from a [3][8][A] window array
    B, T, S = 3, 5, 8
    win = torch.full((B, S, Ad), float("nan"))
    win[:, :T] = a[:B * T].reshape(B, T, Ad)
    lp3, d3, b3 = _action_logprob(gpu, mu[:B * T], sigma[:B * T], win, B, T, S * Ad, Ad)
    assert torch.equal(lp3.reshape(-1), lp[:B * T]) and torch.equal(d3.reshape(-1, Ad), dims[:B * T])
    assert torch.equal(b3.reshape(-1), base[:B * T])


# ------------------------------------------------------------------ dr_replay_returns
def _replay_returns(gpu, r, c, V, gamma, lam, symlog, stride=None, want=("mc", "td")):
    """r, c [B][H], V [B][H + 1] on the CPU; stride: row stride of the r / c windows."""
    L, st = _api()
    B, H = r.shape
    stride = H if stride is None else stride
    rw, cw = torch.full((B, stride), float("nan")), torch.full((B, stride), float("nan"))
    rw[:, :H], cw[:, :H] = r, c
    rd, cd, Vd = rw.to(gpu), cw.to(gpu), V.contiguous().to(gpu)
    Rl = _nan(B, H, gpu=gpu)
    Rmc = _nan(B, H, gpu=gpu) if "mc" in want else None
    td = _nan(B, H, gpu=gpu) if "td" in want else None
    L.call("dr_replay_returns", B, H + 1, L.ptr(rd), stride, L.ptr(cd), stride, int(symlog), L.ptr(Vd), gamma, lam,
           L.ptr(Rl), L.ptr(Rmc), L.ptr(td), st)
    torch.cuda.synchronize()
    cp = lambda t: None if t is None else t.cpu()
    return cp(Rl), cp(Rmc), cp(td)


def _lambda_returns(gpu, r, c, V, gamma, lam):
    L, st = _api()
    B, H = r.shape
    R = _nan(B, H, gpu=gpu)
    rd, cd, Vd = r.contiguous().to(gpu), c.contiguous().to(gpu), V.contiguous().to(gpu)
    L.call("dr_lambda_returns", B, H, L.ptr(rd), L.ptr(cd), L.ptr(Vd), gamma, lam, L.ptr(R), st)
    torch.cuda.synchronize()
    return R.cpu()


@pytest.mark.parametrize("T", [2, 6])
@pytest.mark.parametrize("B", [1, 70])
def test_replay_returns_kernel(B, T, gpu):
    """dr_replay_returns directly.  B = 70 crosses the 64-thread block."""
    H = T - 1
    g = torch.Generator().manual_seed(100 * B + T)
    r = torch.randn(B, H, generator=g) * 2
    c = 1.0 - 0.5 * torch.rand(B, H, generator=g)
    V = torch.randn(B, T, generator=g) * 5
    cut = H // 2
    c[0, cut] = 0.0  # one window ends an episode in the middle
    worst = 0.0
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
        Rl, Rmc, td = _replay_returns(gpu, r, c, V, gamma, lam, symlog=False)
        for t in (Rl, Rmc, td):
            assert bool(torch.isfinite(t).all())
        # natural-space rewards, contiguous: dr_lambda_returns' bits
        assert torch.equal(Rl, _lambda_returns(gpu, r, c, V, gamma, lam)), (gamma, lam)
        assert torch.equal(Rmc, _lambda_returns(gpu, r, c, V, gamma, 1.0)), (gamma, lam)
        g32 = np.float32(gamma)
        rn, cn, Vn = r.numpy(), c.numpy(), V.numpy()
        td_host = ((rn + (g32 * cn) * Vn[:, 1:]).astype(np.float32) - Vn[:, :-1]).astype(np.float32)
        assert np.array_equal(td.numpy(), td_host), (gamma, lam)
        # the cut: what lies beyond it does not reach the entries up to it
        V2 = V.clone()
        V2[0, cut + 1:] = V2[0, cut + 1:] * -3.0 + 7.0
        for x, y in zip((Rl, Rmc, td), _replay_returns(gpu, r, c, V2, gamma, lam, symlog=False)):
            assert torch.equal(x[0, :cut + 1], y[0, :cut + 1]) and torch.equal(x[1:], y[1:])
        assert Rl[0, cut].item() == r[0, cut].item() and Rmc[0, cut].item() == r[0, cut].item()
        # strided windows, and without the optional outputs: the same bits
        for x, y in zip((Rl, Rmc, td), _replay_returns(gpu, r, c, V, gamma, lam, symlog=False, stride=9)):
            assert torch.equal(x, y)
        assert torch.equal(_replay_returns(gpu, r, c, V, gamma, lam, symlog=False, want=())[0], Rl)
        # symlog rewards against float64: test_lambda_returns' bound 8 (H - t) 2^-24 A_t, plus test_bucket_value's
        # symexp allowance 3 2^-24 e^|x| per reward carried through the same absolute recursion
        rs = r  # N(0, 2^2) read as symlog rewards
        Sl, Smc, _ = _replay_returns(gpu, rs, c, V, gamma, lam, symlog=True, stride=9)
        nat = PR.symexp(rs)
        allow = 3 * U * torch.exp(rs.double().abs().clamp(max=20.0))
        steps = torch.arange(H, 0, -1, dtype=F64)
        for got, lm in ((Sl, lam), (Smc, 1.0)):
            want = PR.lambda_returns(nat, c, V, gamma, lm)
            tol = 8 * steps * U * PR.lambda_returns_abs(nat, c, V, gamma, lm) \
                + PR.lambda_returns_abs(allow, c, torch.zeros(B, T), gamma, lm)
            err = (got.double() - want).abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert bool((err <= tol).all()), (gamma, lm, float((err / tol).max()))
    print(f"dr_replay_returns B={B} T={T}: symlog rewards, worst err/bound {worst:.3g}")


# ------------------------------------------------------------------ the one-call path
def _fill_edited(d, obs, starts, seed=0):
    """test_gpu_open_loop._fill's replay contents with a few stored actions set
    to exactly +-1 and one continue flag to 0 inside the first windows.  obs:
    (h, w) for frames, or the vector rows themselves."""
    s0, s1 = int(starts[0]), int(starts[1])
    fr, ac, rw, ct = replay_data(N_FILL, obs if isinstance(obs, tuple) else (2, 2), A, seed=seed)
    if not isinstance(obs, tuple):
        fr = obs
    ac[s0] = 1.0
    ac[s0 + 1] = (-1.0, 1.0, 0.25)
    ac[s1 + 1, 2] = -1.0
    ct[s1 + 1] = 0.0
    d.buffer.load_arrays(fr, ac, rw, ct)
    return fr, ac, rw, ct


def _direct(d, res, B, T):
    """The separate entry points on the trace's states: (logits, V, V target, mu, sigma)."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    gpu = res.hiddens.device
    ag = d.agent
    dims = d.world_model.dims(ag)
    R, C = d.latent_state_dims
    M, nb, Ad = B * T, ag.buckets, d.action_dims
    hid, lat = res.hiddens.contiguous(), res.latents.contiguous()
    st = hip.stream()
    lg, V, Vt = torch.empty(M, nb, device=gpu), torch.empty(M, device=gpu), torch.empty(M, device=gpu)
    ws = torch.empty(L.query("dr_critic_workspace_bytes", dims, B, T - 1), dtype=torch.uint8, device=gpu)
    L.call("dr_critic_fwd", dims, ag.critic_struct(), M, L.ptr(hid), d.hidden_state_dims, L.ptr(lat), R * C,
           L.ptr(lg), L.ptr(V), None, L.ptr(ws), ws.numel(), st)
    L.call("dr_critic_fwd", dims, ag.critic_struct(target=True), M, L.ptr(hid), d.hidden_state_dims, L.ptr(lat),
           R * C, None, L.ptr(Vt), None, L.ptr(ws), ws.numel(), st)
    a, mu, sg = (torch.empty(M, Ad, device=gpu) for _ in range(3))
    ws2 = torch.empty(L.query("dr_actor_act_workspace_bytes", dims, M), dtype=torch.uint8, device=gpu)
    L.call("dr_actor_act", dims, ag.actor_struct(), M, L.ptr(hid), L.ptr(lat), L.dr_noise(), 1, L.ptr(a), L.ptr(mu),
           L.ptr(sg), L.ptr(ws2), ws2.numel(), st)
    Rl = torch.empty(B, T - 1, device=gpu)
    r, c = res.reward.contiguous(), res.cont.contiguous()
    L.call("dr_lambda_returns", B, T - 1, L.ptr(r), L.ptr(c), L.ptr(res.value_target.contiguous()), ag.gamma,
           ag.lambda_, L.ptr(Rl), st)
    torch.cuda.synchronize()
    return lg.view(B, T, nb), V.view(B, T), Vt.view(B, T), mu.view(B, T, Ad), sg.view(B, T, Ad), Rl


def _check_composition(d, res, q_post, starts, B, T, what):
    """Bit for bit: the one-call path against closed_loop and the separate entry points."""
    R, C = d.latent_state_dims
    gpu = res.hiddens.device
    assert res.length == T and res.latents.shape == (B, T, R, C)
    with torch.no_grad():
        cl = d.closed_loop(starts=np.asarray(starts), length=T, noise=(q_post.to(gpu), torch.ones_like(q_post).to(gpu)),
                           predict=False)
    assert torch.equal(res.latents, cl.latents) and torch.equal(res.hiddens, cl.hiddens), what
    lg, V, Vt, mu, sg, Rl = _direct(d, res, B, T)
    for name, got, want in (("critic_logits", res.critic_logits, lg), ("value", res.value, V),
                            ("value_target", res.value_target, Vt), ("actor_mu", res.actor_mu, mu),
                            ("actor_sigma", res.actor_sigma, sg), ("returns_lambda", res.returns_lambda, Rl)):
        assert got.shape == want.shape and torch.equal(got, want), (what, name)
    nb, Ad = d.agent.buckets, d.action_dims
    shapes = dict(value_entropy=(B, T), value_std_symlog=(B, T), actions=(B, T, Ad), action_logprob=(B, T),
                  policy_entropy_base=(B, T), action_logprob_dims=(B, T, Ad), reward=(B, T - 1), cont=(B, T - 1),
                  returns_mc=(B, T - 1), td=(B, T - 1), critic_ce=(B, T - 1), critic_logits=(B, T, nb))
    for k, s in shapes.items():
        assert tuple(getattr(res, k).shape) == s, (what, k)
        assert bool(torch.isfinite(getattr(res, k)).all()), (what, k)


def _close1e4(got, ref, what):
    """The project's standing 1e-4 relative to max(1, |ref|)."""
    e = _rel(cpu(got), ref.double())
    print(f"{what}: max rel err {e:.3e}")
    assert e <= 1e-4, (what, e)


def _vec_dreamer(gpu, **kw):
    from test_gpu_vector import _dreamer
    return _dreamer(gpu, **kw)


@pytest.mark.parametrize("case", ["small", "full", "vector"])
def test_agent_trace_composition(case, gpu):
    from test_gpu_vector import D_OBS
    B, T = {"small": (3, 5), "full": (2, 3), "vector": (2, 3)}[case]
    S = 8
    starts = {"small": [0, 17, 56], "full": [3, 40], "vector": [1, 33]}[case]
    if case == "vector":
        d = _vec_dreamer(gpu, batch_size=B, sequence_length=S, horizon=3, buffer_size=N_FILL)
        P = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
        rows = torch.randn(N_FILL, D_OBS, generator=torch.Generator().manual_seed(4)).numpy()
        fr, ac, rw, ct = _fill_edited(d, rows, starts, seed=3)
        obs = _windows(fr, starts, S)
    else:
        d, P = build(case, gpu, B=B, H=3, S=S)
        fr, ac, rw, ct = _fill_edited(d, tuple(CFG[case]["observation_dims"]), starts)
        obs = _windows(fr, starts, S).float()
    R, C = d.latent_state_dims
    act = _windows(ac, starts, S)
    q_post, q_prior = _noise(47, T, B, R, C)
    o = _oracle(P, obs, act, T, R, C, q_post, q_prior, heads=False)  # widens q_post where a draw is near a tie
    print(f"{case}: {o['tg'].guarded} guarded groups of {o['tg'].draws} draws")
    with torch.no_grad():
        res = d.agent_trace(starts=np.asarray(starts), length=T, noise=q_post.to(gpu))
    torch.cuda.synchronize()
    _check_composition(d, res, q_post, starts, B, T, case)
    assert torch.equal(cpu(res.latents).argmax(-1), o["lat"].argmax(-1))
    # the ring's slots, bit for bit: actions start + t, the transition's flag start + t
    assert torch.equal(cpu(res.actions), act[:, :T])
    assert torch.equal(cpu(res.cont), _windows(ct, starts, S)[:, :T - 1])
    assert float(cpu(res.actions).abs().max()) == 1.0 and float(cpu(res.cont).min()) == 0.0
    # against the oracle, teacher-forced on the GPU's own (h, z)
    hid, lat = cpu(res.hiddens), cpu(res.latents)
    gamma, lam = d.agent.gamma, d.agent.lambda_
    with torch.no_grad():
        V = O.critic_value(hid, lat, P).squeeze(-1)
        Vt = O.critic_value(hid, lat, P, which="target_critic").squeeze(-1)
        r = O.symexp(_windows(rw, starts, S)[:, :T - 1])
        c = _windows(ct, starts, S)[:, :T - 1]
        Rl = O.lambda_returns(Vt, r, c, gamma, lam)
        Rmc = O.lambda_returns(Vt, r, c, gamma, 1.0)
        buckets = P[O.AG + "critic.buckets_crit"]
        th = O.twohot(O.symlog(Rl).unsqueeze(-1), buckets)
        ce = -(th * torch.log_softmax(O.critic_logits(hid[:, :-1], lat[:, :-1], P), -1)).sum(-1)
        logp = O.tanh_normal_logprob(act[:, :T], cpu(res.actor_mu), cpu(res.actor_sigma))
    _close1e4(res.value, V, f"{case} value")
    _close1e4(res.value_target, Vt, f"{case} value_target")
    _close1e4(res.reward, r, f"{case} reward")
    _close1e4(res.returns_lambda, Rl, f"{case} returns_lambda")
    _close1e4(res.returns_mc, Rmc, f"{case} returns_mc")
    _close1e4(res.critic_ce, ce, f"{case} critic_ce")
    _close1e4(res.action_logprob, logp, f"{case} action_logprob")
    _close1e4(res.td, (r + gamma * c * Vt[:, 1:]) - Vt[:, :-1], f"{case} td")
    # the helpers against numpy on the downloaded tensors
    Rn, Vn = cpu(res.returns_lambda).numpy().astype(np.float64), cpu(res.value).numpy().astype(np.float64)
    assert np.allclose(cpu(res.advantage()).numpy(), Rn - Vn[:, :-1], rtol=1e-6, atol=1e-6)
    ev = 1.0 - np.var(Rn - Vn[:, :-1]) / np.var(Rn)
    assert math.isclose(float(res.explained_variance()), ev, rel_tol=1e-4, abs_tol=1e-5)
    assert torch.equal(res.value_error(), res.value[:, :-1] - res.returns_mc)
    # sample=False is q == 1
    with torch.no_grad():
        m1 = d.agent_trace(starts=np.asarray(starts), length=T, sample=False)
        m2 = d.agent_trace(starts=np.asarray(starts), length=T, noise=torch.ones(T, B * R, C, device=gpu))
    _same({k: v for k, v in vars(m1).items()}, {k: v for k, v in vars(m2).items()})
    for bad in (torch.ones(T - 1, B * R, C, device=gpu), torch.ones(T, B * R, C + 1, device=gpu)):
        with pytest.raises(ValueError):
            d.agent_trace(starts=np.asarray(starts), length=T, noise=bad)


def test_agent_trace_bf16_runs(gpu):
    """precision: "bf16" at B = 3, T = 4: the entry points honour the mode, the
    new kernels are f32; everything is finite and the bit-for-bit composition
    holds as in fp32.  On the FULL widths, like test_closed_loop_consistent's
    bf16 case: the bf16 encoder takes 16, 32 or 64 conv1 filters, and SMALL has
    8 (dr_encoder_features refuses it in this mode, for every caller)."""
    B, T, S = 3, 4, 8
    starts = [0, 17, 56]
    d, _ = build("full", gpu, B=B, H=3, S=S)
    d.precision = d.world_model.precision = "bf16"
    _fill_edited(d, tuple(FULL["observation_dims"]), starts)
    R, C = d.latent_state_dims
    q_post, _ = _noise(48, T, B, R, C)
    with torch.no_grad():
        res = d.agent_trace(starts=np.asarray(starts), length=T, noise=q_post.to(gpu))
    torch.cuda.synchronize()
    for k, v in vars(res).items():
        if isinstance(v, torch.Tensor):
            assert bool(torch.isfinite(v).all()), k
    _check_composition(d, res, q_post, starts, B, T, "bf16")


def test_evaluate_values_leaves_state(gpu):
    """evaluate_values leaves np.random's state and training_state() as it
    found them, returns finite curves of lengths T / T - 1 and the scalar, and
    a following train_Agent() gives the losses of a twin Dreamer that did not
    evaluate."""
    from dreamer_amd import hip
    B, S, H, T = 4, 8, 5, 6

    def run(evaluate):
        np.random.seed(3)
        hip.rng(gpu).reseed(11)
        hip.adhoc(gpu).reseed(12)
        d, _ = build("small", gpu, B=B, H=H, S=S)
        fr, ac, rw, ct = replay_data(N_FILL, tuple(SMALL["observation_dims"]), A, seed=0)
        d.buffer.load_arrays(fr, ac, rw, ct)
        if evaluate:
            before_np, before = np.random.get_state(), d.training_state()
            curves = d.evaluate_values(batches=2, length=T)
            after_np, after = np.random.get_state(), d.training_state()
            assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1])
            assert before_np[2:] == after_np[2:]
            _same(before, after)
            full = ("value", "value_target", "value_entropy", "value_std_symlog", "action_logprob", "actor_sigma")
            part = ("returns_lambda", "returns_mc", "abs_td", "critic_ce", "abs_advantage")
            assert set(curves) == set(full) | set(part) | {"explained_variance"}
            assert all(len(curves[k]) == T for k in full) and all(len(curves[k]) == T - 1 for k in part)
            assert all(np.isfinite(v) for k in full + part for v in curves[k]), curves
            assert isinstance(curves["explained_variance"], float) and np.isfinite(curves["explained_variance"])
        la, lc = d.train_Agent()
        torch.cuda.synchronize()
        return la.detach().cpu().clone(), lc.detach().cpu().clone()

    got, ref = run(True), run(False)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (got, ref)
