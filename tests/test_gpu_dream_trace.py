"""Dream trace on replay windows (Dreamer.dream_trace, evaluate_dreams,
dr_dream_stats, dr_actor_draws).

The kernel against the float64 reference of tests/dream_ref.py by the project's
accuracy rule (test_gpu_agent_trace.py): the bound is 8 x the error the same
formulas evaluated in f32 on the CPU make against float64 on these inputs, at
least 4 * 2^-24 and never more than 1e-4, relative to max(1, |ref|); bit for bit
against dr_lambda_returns and dr_action_logprob on the same device tensors; the
one-call path against context_filter + Dreamer.dream_episodes bit for bit and
against oracle.dreamer_oracle under the tie guard.  Run on the MI355X box:
pytest -m gpu.  Measured values: DESIGN section 5m."""
import numpy as np
import pytest
import torch

import dream_ref as DR
from baseline_case import TieGuard
from formula import SMALL
from gpu_helpers import build, close, cpu
from oracle import dreamer_oracle as O
from test_gpu_open_loop import A, N_FILL, _fill, _quant, _windows

pytestmark = pytest.mark.gpu
U = DR.U
FLOAT = [k for k in DR.PER_DREAM + DR.PER_WINDOW if k not in DR.INT]
GAMMA, LAM, NORM, SAT = 0.99, 0.95, 2.5, 0.99


def _bound(yardstick):
    return min(max(8.0 * yardstick, 4.0 * U), 1e-4)


def _dev(x, gpu):
    return {k: torch.from_numpy(v).contiguous().to(gpu) for k, v in x.items()}


def _run(gpu, B, M, xd, want=None, gamma=GAMMA, lam=LAM, norm=NORM, sat=SAT):
    """dr_dream_stats on device inputs (rows 0 .. B*M-1 of xd), every output unless `want` names some; CPU numpy."""
    from dreamer_amd.dream_trace import PER_DREAM, PER_WINDOW, dream_stats
    N = B * M
    H, Ad = xd["actions"].shape[1:]
    nd = None if norm is None else torch.full((1,), norm, device=gpu)
    out = dream_stats(B, M, H, Ad, *(xd[k][:N].contiguous() for k in ("rewards", "continues", "Vt", "Vo", "mus",
                                                                      "sigmas", "actions")),
                      gamma, lam, nd, sat, want=want or PER_DREAM + PER_WINDOW)
    torch.cuda.synchronize()
    if nd is not None:
        assert nd.item() == np.float32(norm)  # read, never written
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    """Equal bits where finite or infinite, NaN where NaN."""
    if a.dtype.kind == "i":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.int32), b[~nan].view(np.int32))


SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (3, 5, 16, 3), (2, 64, 15, 3), (1, 2, 64, 2)]


# ------------------------------------------------------------------ 1. the kernel against dream_ref
@pytest.mark.parametrize("B,M,H,Ad", SHAPES)
def test_dream_stats_kernel(B, M, H, Ad, gpu):
    x = DR.planted(B, M, H, Ad)
    args = (x["rewards"], x["continues"], x["Vt"], x["Vo"], x["mus"], x["sigmas"], x["actions"], GAMMA, LAM)
    r64 = DR.dream_ref(B, M, *args, norm=NORM, sat=SAT)
    r32 = DR.dream_ref(B, M, *args, norm=NORM, sat=SAT, dt=np.float32)
    xd = _dev(x, gpu)
    got = _run(gpu, B, M, xd)
    worst = {}
    for k in FLOAT:
        assert got[k].shape == r64[k].shape and got[k].dtype == np.float32, k
        y = DR.rel_err(r32[k], r64[k])
        e = DR.rel_err(got[k], r64[k])
        print(f"dream_stats B={B} M={M} H={H} A={Ad} {k}: f32-CPU yardstick {y:.3e}, kernel max rel err {e:.3e} "
              f"(bound {_bound(y):.3e})")
        worst[k] = (e, _bound(y))
    assert all(e <= b for e, b in worst.values()), {k: v for k, v in worst.items() if v[0] > v[1]}
    for k in DR.INT:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], r64[k]), (k, got[k], r64[k])
    # what was planted is there
    assert np.all(got["alive"][:, 0] == 1) and np.all(got["weight"][:, :, 0] == 1)
    assert got["saturated"][0, 0, 0] >= 1 and np.isfinite(got["logp"][0, 0, 0])
    if H >= 2:
        assert x["sigmas"][0, H - 1, 0] == np.float32(1e-3) and np.isfinite(got["logp"][0, 0, H - 1])
    if H >= 3:
        assert np.all(got["weight"][0, 0, H // 2 + 1:] == 0) and got["weight"][0, 0, H // 2] != 0
    if M >= 3:
        assert got["best"][0] == 1  # dreams 1 and 2 tie on top: the lower m
        assert _same_bits(got["R_lambda"][0, 1], got["R_lambda"][0, 2])
    if M >= 4:
        t = min(1, H - 1)
        assert np.isnan(got["R_mc"][0, 3, 0]) and got["n_finite"][0] == M - 1 and got["worst"][0] != 3
        assert np.isnan(got["reward_mean"][0, t]) and np.isnan(got["ret_std"][0, 0])
        assert np.isfinite(got["logp_mean"]).all() and np.isfinite(got["alive"]).all()
    elif M >= 1:
        assert all(np.isfinite(got[k]).all() for k in FLOAT)
    if M == 1:
        assert all(np.all(got[k] == 0) for k in ("reward_std", "ret_std", "logp_std", "action_spread"))
        assert np.all(got["best"] == 0) and np.all(got["worst"] == 0) and np.all(got["n_finite"] == 1)
    # the copied window: the same bits at the other batch position; window 0 alone at B = 1 likewise
    if B >= 2:
        for k in got:
            assert _same_bits(got[k][B - 1], got[k][0]), k
    one = _run(gpu, 1, M, xd)
    for k in got:
        assert _same_bits(one[k][0], got[k][0]), k
    # norm = NULL is 1
    nn = _run(gpu, B, M, xd, want=("adv", "adv_norm"), norm=None)
    assert _same_bits(nn["adv_norm"], nn["adv"]) and _same_bits(nn["adv"], got["adv"])


def test_dream_stats_all_dreams_nan(gpu):
    B, M, H, Ad = 2, 3, 2, 3
    x = DR.planted(B, M, H, Ad)
    x["rewards"][:M, 0] = np.nan
    got = _run(gpu, B, M, _dev(x, gpu))
    assert (got["best"][0], got["worst"][0], got["n_finite"][0]) == (0, 0, 0)
    assert got["n_finite"][1] == M


# ------------------------------------------------------------------ 2. bitwise identities
@pytest.mark.parametrize("B,M,H,Ad", [(3, 5, 16, 3), (2, 64, 15, 3), (1, 1, 1, 1)])
def test_dream_stats_is_the_separate_kernels_bit_for_bit(B, M, H, Ad, gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    N = B * M
    xd = _dev(DR.planted(B, M, H, Ad, seed=1), gpu)
    st = hip.stream()
    for gamma, lam in ((GAMMA, LAM), (1.0, 1.0), (0.9, 0.0)):
        got = _run(gpu, B, M, xd, gamma=gamma, lam=lam)
        for key, lm in (("R_lambda", lam), ("R_mc", 1.0)):
            R = torch.full((N, H), float("nan"), device=gpu)
            L.call("dr_lambda_returns", N, H, L.ptr(xd["rewards"]), L.ptr(xd["continues"]), L.ptr(xd["Vt"]), gamma, lm,
                   L.ptr(R), st)
            torch.cuda.synchronize()
            assert _same_bits(got[key].reshape(N, H), R.cpu().numpy()), (key, gamma, lam)
    lp, be = (torch.full((N, H), float("nan"), device=gpu) for _ in range(2))
    L.call("dr_action_logprob", N, H, Ad, L.ptr(xd["mus"]), L.ptr(xd["sigmas"]), L.ptr(xd["actions"]), H * Ad, Ad,
           L.ptr(lp), None, L.ptr(be), st)
    torch.cuda.synchronize()
    assert _same_bits(got["logp"].reshape(N, H), lp.cpu().numpy())
    assert _same_bits(got["base_entropy"].reshape(N, H), be.cpu().numpy())


# ------------------------------------------------------------------ 3. NULL outputs
def test_any_single_output_alone_has_the_same_bits(gpu):
    B, M, H, Ad = 3, 5, 16, 3
    xd = _dev(DR.planted(B, M, H, Ad, seed=2), gpu)
    full = _run(gpu, B, M, xd)
    for k in DR.PER_DREAM + DR.PER_WINDOW:
        one = _run(gpu, B, M, xd, want=(k,))
        assert set(one) == {k} and _same_bits(one[k], full[k]), k


def test_actor_draws_are_the_unrolls(gpu):
    """dr_actor_draws writes out the N(0,1) variates dr_imagine_fwd's actor draws
    from the same Philox stream: the first action of a Philox dream is
    tanh(mu + eps sigma) of the written-out eps (tanhf's rounding apart)."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, H = 4, 2
    d, _ = build("small", gpu, B=B, H=H, S=8)
    R, C = d.latent_state_dims
    g = torch.Generator().manual_seed(3)
    h0 = (torch.randn(B, d.hidden_state_dims, generator=g) * 0.5).to(gpu)
    z0 = torch.nn.functional.one_hot(torch.randint(0, C, (B, R), generator=g), C).float().to(gpu)
    ar = hip.adhoc(gpu)
    ar.reseed(21)
    with torch.no_grad():
        out = d.dream_episodes(z0, h0)  # the call's stream id: counter 1
    ar.reseed(21)
    eps = torch.full((H, B, A), float("nan"), device=gpu)
    L.call("dr_actor_draws", H, B, A, ar.noise(), L.ptr(eps), hip.stream())
    torch.cuda.synchronize()
    act, mu, sg = (cpu(t) for t in (out[2], out[5], out[6]))
    e = eps.cpu()
    assert bool(torch.isfinite(e).all()) and float(e.std()) > 0.3
    want = torch.tanh(mu[:, 0] + e[0] * sg[:, 0])
    close(act[:, 0], want, 1e-5, 1e-6, "first action from the written-out draws")


# ------------------------------------------------------------------ 4. end to end
def _tensors(r):
    return {k: v for k, v in vars(r).items() if isinstance(v, torch.Tensor)}


def _rerun_stats(d, res):
    from dreamer_amd.dream_trace import dream_stats
    B, M, H = res.rewards.shape
    N = B * M
    Ad = res.actions.shape[-1]
    c = lambda t, *s: t.reshape(N, *s).contiguous()
    out = dream_stats(B, M, H, Ad, c(res.rewards, H), c(res.continues, H), c(res.value_target, H + 1),
                      c(res.value, H + 1), c(res.mus, H, Ad), c(res.sigmas, H, Ad), c(res.actions, H, Ad),
                      d.agent.gamma, d.agent.lambda_, res.norm, res.saturation)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert getattr(res, k).shape == v.shape and torch.equal(getattr(res, k), v), k


def _noise(seed, Tc, H, B, M, R, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(Tc, B * R, C).exponential_(generator=g),
            torch.empty(H, B * M * R, C).exponential_(generator=g), torch.randn(H, B * M, A, generator=g))


def test_dream_trace_end_to_end_small(gpu):
    """SMALL, pixels, (B, M, H) = (2, 3, 4).  A mean over M = 3 equal values need
    not return the value (3x is rounded, and so is the division), so the
    all-dreams-equal case asserts exact zeros at samples=4, where every step of
    the mean is exact, and |std| <= 2^-22 max|x| at samples=3."""
    from dreamer_amd import hip
    from dreamer_amd.replay_eval import context_filter, preserved_rng, window_prologue
    B, M, H, S, Tc = 2, 3, 4, 8, 4
    N = B * M
    d, P = build("small", gpu, B=B, H=H, S=S)
    hw = tuple(SMALL["observation_dims"])
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    fr, ac, rw, ct = _fill(d, hw)
    starts = [5, 40]
    d.agent.S = 3.5
    none = lambda name: None
    # --- samples = 1 under explicit noise: context_filter + dream_episodes, bit for bit
    q_ctx, q1, e1 = (t.to(gpu) for t in _noise(7, Tc, H, B, 1, R, C))
    with torch.no_grad():
        r1 = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=1, noise=(q_ctx, q1, e1))
        w = window_prologue(d, np.asarray(starts), None, Tc, lambda Bn, dev: (q_ctx,), none)
        z0, h0 = context_filter(d, w, Tc, q_ctx, none)
        with hip.noise_override(q=q1, eps=e1):
            lat, hid, act, rew, cont, mus, sgs = d.dream_episodes(z0.view(B, 1, R, C), h0.view(B, 1, Hd))
    torch.cuda.synchronize()
    assert (r1.context, r1.horizon, r1.samples) == (Tc, H, 1)
    for name, got, want in (("latents", r1.latents, lat), ("hiddens", r1.hiddens, hid), ("actions", r1.actions, act),
                            ("mus", r1.mus, mus), ("sigmas", r1.sigmas, sgs), ("rewards", r1.rewards, rew),
                            ("continues", r1.continues, cont)):
        assert got.numel() == want.numel() and torch.equal(got.reshape(want.shape), want), name
    # --- M = 3 against the oracle under the tie guard, the widened draws given to the GPU
    q_ctx, q, eps = _noise(11, Tc, H, B, M, R, C)
    obs, actw = _windows(fr, starts, S).float(), _windows(ac, starts, S)
    with TieGuard() as tg, torch.no_grad():
        z, h = O.warm_start(obs[:, :Tc], actw[:, :Tc], 2 * Tc, P, q_ctx, R, C)
        o = O.dream(z.repeat_interleave(M, 0), h.repeat_interleave(M, 0), P, eps.view(H, N, 1, A), q, H, R, C)
        Vt = O.critic_value(o[1], o[0], P, "target_critic")
        Rl = O.lambda_returns(Vt, o[3], o[4], d.agent.gamma, d.agent.lambda_)
        Rmc = O.lambda_returns(Vt, o[3], o[4], d.agent.gamma, 1.0)
    print(f"dream trace small: {tg.guarded} guarded groups of {tg.draws} draws")
    with torch.no_grad():
        res = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=M,
                            noise=(q_ctx.to(gpu), q.to(gpu), eps.to(gpu)))
    torch.cuda.synchronize()
    assert float(d.agent.S) == 3.5 and res.norm.item() == 3.5
    assert res.latents.shape == (B, M, H + 1, R, C) and res.mu.shape == (B, M, H + 1, 3, *hw)
    assert torch.equal(cpu(res.latents).reshape(N, H + 1, R, C).argmax(-1), o[0].argmax(-1))
    close(res.hiddens.reshape(N, H + 1, Hd), o[1], 2e-4, 2e-5, "hiddens")
    close(res.actions.reshape(N, H, A), o[2], 2e-4, 2e-5, "actions")
    for name, got, want in (("R_lambda", res.R_lambda, Rl), ("R_mc", res.R_mc, Rmc)):
        e = DR.rel_err(cpu(got).reshape(N, H).numpy(), want.reshape(N, H).double().numpy())
        print(f"dream trace small {name}: max rel err {e:.3e}")
        assert e <= 1e-4, (name, e)
    _rerun_stats(d, res)
    assert res.frames.dtype == torch.uint8 and torch.equal(res.frames.cpu(), _quant(res.mu))
    assert bool((res.latents[:, 0, 0] == res.latents[:, 1, 0]).all())  # state 0 is shared
    v = res.video()
    assert v.shape == (H + 1, 3, 2 * hw[0], B * hw[1])
    assert torch.equal(v[0][:, :hw[0], :hw[1]], res.frames[0, int(res.best[0]), 0])
    # --- Philox: the replicas differ, the same RNG state gives the same bits
    with torch.no_grad(), preserved_rng(gpu):
        a = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=M)
    with torch.no_grad(), preserved_rng(gpu):
        b = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=M)
    torch.cuda.synchronize()
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb) and all(torch.equal(ta[k], tb[k]) for k in ta)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ta.values())
    assert not torch.equal(a.actions[:, 0], a.actions[:, 1]) and not torch.equal(a.latents[:, 0, 1:], a.latents[:, 1, 1:])
    assert float(a.action_spread.min()) > 0
    _rerun_stats(d, a)
    # --- modes and tanh(mu): every dream of a window is the same dream
    for Ms in (4, 3):
        with torch.no_grad():
            m = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=Ms, sample=False, deterministic=True,
                              decode=False)
        torch.cuda.synchronize()
        assert m.mu is None and m.frames is None
        for k in m._per_dream:
            t = getattr(m, k)
            assert t is None or bool((t == t[:, :1]).all()), k
        assert float((m.actions - torch.tanh(m.mus)).abs().max()) <= 1e-6
        if Ms == 4:
            assert float(m.ret_std.abs().max()) == 0 and float(m.action_spread.abs().max()) == 0
            assert float(m.reward_std.abs().max()) == 0 and float(m.logp_std.abs().max()) == 0
        else:
            assert float(m.ret_std.max()) <= 2.0 ** -22 * float(m.R_lambda.abs().max())
            assert float(m.action_spread.max()) <= 2.0 ** -22
        assert torch.equal(m.best, torch.zeros_like(m.best)) and torch.equal(m.worst, torch.zeros_like(m.worst))
    # --- modes with Philox actions: the written-out draws differ by row
    with torch.no_grad():
        s = d.dream_trace(starts=np.asarray(starts), context=Tc, samples=M, sample=False, decode=False)
    torch.cuda.synchronize()
    assert not torch.equal(s.actions[:, 0], s.actions[:, 1]) and bool(torch.isfinite(s.logp).all())
    _rerun_stats(d, s)


def _vec(gpu, B, S, H):
    from test_gpu_vector import D_OBS, _dreamer
    from formula import replay_data
    d = _dreamer(gpu, batch_size=B, sequence_length=S, horizon=H, buffer_size=N_FILL)
    _, ac, rw, ct = replay_data(N_FILL, (2, 2), A, seed=3)
    rows = torch.randn(N_FILL, D_OBS, generator=torch.Generator().manual_seed(4)).numpy()
    d.buffer.load_arrays(rows, ac, rw, ct)
    return d, D_OBS


def test_dream_trace_vector_observations(gpu):
    B, M, H, S = 2, 3, 4, 8
    d, D = _vec(gpu, B, S, 2)
    with torch.no_grad():
        res = d.dream_trace(starts=np.array([1, 33]), horizon=H, samples=M)  # H above the model's own horizon
    torch.cuda.synchronize()
    assert (res.context, res.horizon) == (S // 2, H)
    assert res.mu.shape == (B, M, H + 1, D) and res.frames is None
    assert all(bool(torch.isfinite(t.float()).all()) for t in _tensors(res).values())
    with torch.no_grad():
        P = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
        mu_ref = O.decoder_forward(cpu(res.hiddens).flatten(0, 1), cpu(res.latents).flatten(0, 1), P, None)
    close(res.mu.flatten(0, 1), mu_ref, 1e-4, 1e-5, "vector mu")
    _rerun_stats(d, res)
    assert "frames" not in res.pick("worst")
    with pytest.raises(ValueError):
        res.video()


# ------------------------------------------------------------------ 5. evaluate_dreams
def test_evaluate_dreams(gpu):
    from dreamer_amd import hip
    from dreamer_amd.dream_trace import CURVES
    B, S, H, M = 3, 8, 3, 4
    d, _ = _vec(gpu, B, S, H)
    d.agent.S = 2.0
    np.random.seed(3)
    ar = hip.adhoc(gpu)
    ar.reseed(12)

    def state():
        return np.random.get_state(), ar.state.clone(), ar.counter, float(d.agent.S)

    def same(a, b):
        return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and \
            torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]

    before = state()
    two = d.evaluate_dreams(batches=2, samples=M)
    assert same(before, state())
    assert tuple(two) == CURVES
    assert [len(two[k]) for k in CURVES] == [H, H, H + 1, H + 1] + [H] * 8
    assert all(np.isfinite(v) for k in CURVES for v in two[k]), two
    assert two["alive"][0] == 1.0
    # the same two batches by hand, from the same starting random state
    with torch.no_grad():
        c = [d.dream_trace(samples=M, decode=False).curves() for _ in range(2)]
    want = {k: ((c[0][k] + c[1][k]) / 2.0).cpu().tolist() for k in CURVES}
    assert not same(before, state())
    assert two == want
    np.random.set_state(before[0])
    ar.state.copy_(before[1])
    ar.counter = before[2]
    # real = True: a finite gap, the curves of the mode-filtered dreams, the state left alone
    out = d.evaluate_dreams(batches=1, samples=M, real=True)
    assert same(before, state())
    assert set(out) == set(CURVES) | {"gap"} and np.isfinite(out["gap"])
    assert all(np.isfinite(v) for k in CURVES for v in out[k])
