"""Posterior trace on replay windows (Dreamer.closed_loop, evaluate_filter,
WorldModel.observe_sequence, dr_observe_trace, dr_latent_stats) against
dr_observe_scan's launch form, bit for bit, and against the CPU oracle composed
from oracle.dreamer_oracle:

    z_0, lq_0 = O.encode(0, x_0, q_post[0])
    z_t, h_t, lq_t = O.observe_step(z_{t-1}, h_{t-1}, a_{t-1}, x_t, q_post[t])
    lp = O.prior_logits(h);  z~_t = O.prior_predict(h_t, q_prior[t])

under baseline_case.TieGuard, whose widened draws are what the GPU gets, so
every latent index must match exactly.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

from baseline_case import TieGuard
from formula import FULL, SMALL, replay_data
from gpu_helpers import CFG, build, close, cpu
from oracle import dreamer_oracle as O
from test_gpu_open_loop import A, N_FILL, _fields, _fill, _quant, _same, _sqerr_bound_check, _windows, _x_of_u8

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ latent statistics
def _stats64(post, prior):
    """float64 reference on the given f32 logits [M][R][C]: (kl, post entropy, prior entropy) per row."""
    p, q = post.double(), prior.double()
    ent = lambda x: -(torch.log_softmax(x, -1).exp() * torch.log_softmax(x, -1)).sum((-1, -2))
    return O._cat_kl(p, q).sum(-1), ent(p), ent(q)


def _stats32(post, prior):
    """The same formulas evaluated in f32 on the CPU: the yardstick."""
    ent = lambda x: -(torch.log_softmax(x, -1).exp() * torch.log_softmax(x, -1)).sum((-1, -2))
    return O._cat_kl(post, prior).sum(-1), ent(post), ent(prior)


def _rel(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


def _stats_bounds(post, prior, what):
    """(kl bound, entropy bound): 8 x the f32-CPU error of the formulas against
    float64 on these inputs, never more than 1e-4; relative to max(1, |ref|)."""
    ref = _stats64(post, prior)
    y = _stats32(post, prior)
    y_kl, y_ent = _rel(y[0], ref[0]), max(_rel(y[1], ref[1]), _rel(y[2], ref[2]))
    print(f"{what}: f32-CPU yardstick kl {y_kl:.3e}, entropy {y_ent:.3e}")
    return ref, min(8 * y_kl, 1e-4), min(8 * y_ent, 1e-4)


def _latent_stats(post, prior, gpu, groups=False):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    M, R, C = post.shape
    pd = post.contiguous().to(gpu)
    qd = None if prior is None else prior.contiguous().to(gpu)
    hq = torch.full((M,), float("nan"), device=gpu)
    kl = hp = kg = None
    if prior is not None:
        kl, hp = torch.full((M,), float("nan"), device=gpu), torch.full((M,), float("nan"), device=gpu)
        kg = torch.full((M, R), float("nan"), device=gpu) if groups else None
    L.call("dr_latent_stats", M, R, C, L.ptr(pd), L.ptr(qd), L.ptr(kl), L.ptr(hq), L.ptr(hp), L.ptr(kg), hip.stream())
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu()
    return c(kl), c(hq), c(hp), c(kg)


@pytest.mark.parametrize("RC", [(32, 32), (8, 8), (3, 7)])
def test_latent_stats_kernel(RC, gpu):
    """dr_latent_stats directly.  Measured on the MI355X (max relative error
    against float64, kl / entropy; f32-CPU yardstick in brackets): see DESIGN
    section 5h."""
    from dreamer_amd import _lib as L
    R, C = RC
    M = 37
    g = torch.Generator().manual_seed(100 * R + C)
    post, prior = torch.randn(M, R, C, generator=g) * 3, torch.randn(M, R, C, generator=g) * 3
    post[0], prior[0] = 1.5, -0.25                      # all equal in both
    prior[1] = post[1]                                  # prior == posterior
    post[2], prior[2] = -80.0, -80.0                    # peaked on different classes
    post[2, :, 0], prior[2, :, 1] = 80.0, 80.0
    prior[3] = 0.0                                      # posterior random, flat prior
    post[36], prior[36] = post[4], prior[4]             # a row copied to another position
    (kl64, hq64, hp64), b_kl, b_ent = _stats_bounds(post, prior, f"latent_stats {RC}")
    kl, hq, hp, kg = _latent_stats(post, prior, gpu, groups=True)
    e_kl, e_hq, e_hp = _rel(kl, kl64), _rel(hq, hq64), _rel(hp, hp64)
    print(f"latent_stats {RC}: kernel max rel err kl {e_kl:.3e} (bound {b_kl:.3e}), entropy "
          f"{max(e_hq, e_hp):.3e} (bound {b_ent:.3e})")
    for t in (kl, hq, hp, kg):
        assert bool(torch.isfinite(t).all())
    assert e_kl <= b_kl and e_hq <= b_ent and e_hp <= b_ent
    assert kl[0].item() == 0.0 and bool((kg[0] == 0).all())
    assert abs(hq[0].item() - R * np.log(C)) <= b_ent * max(1.0, R * np.log(C))
    assert abs(hp[0].item() - R * np.log(C)) <= b_ent * max(1.0, R * np.log(C))
    assert abs(kl[1].item()) <= b_kl
    assert abs(kl[2].item() - 160.0 * R) <= b_kl * 160.0 * R
    # the same row at another position, and alone in a call with M = 1: the same bits
    for t in (kl, hq, hp):
        assert t[36].item() == t[4].item()
    assert torch.equal(kg[36], kg[4])
    one = _latent_stats(post[4:5], prior[4:5], gpu, groups=True)
    assert one[0][0].item() == kl[4].item() and one[1][0].item() == hq[4].item() and one[2][0].item() == hp[4].item()
    assert torch.equal(one[3][0], kg[4])
    # the group terms sum to kl
    assert _rel(kg.double().sum(-1), kl.double()) <= b_kl
    # NULL prior: the same post_entropy bits, nothing else asked for
    _, hq2, _, _ = _latent_stats(post, None, gpu)
    assert torch.equal(hq2, hq)
    # kl_groups is optional
    kl3, hq3, hp3, _ = _latent_stats(post, prior, gpu)
    assert torch.equal(kl3, kl) and torch.equal(hq3, hq) and torch.equal(hp3, hp)
    x = torch.zeros(1, 4, 4, device=gpu)
    o = torch.zeros(1, device=gpu)
    for Rb, Cb in ((4, 65), (0, 4)):
        with pytest.raises(L.HipError) as e:
            L.call("dr_latent_stats", 1, Rb, Cb, L.ptr(x), L.ptr(x), L.ptr(o), L.ptr(o), L.ptr(o), None, None)
        assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:  # kl without a prior
        L.call("dr_latent_stats", 1, 4, 4, L.ptr(x), None, L.ptr(o), L.ptr(o), None, None, None)
    assert e.value.code == L.DR_E_INVALID


# ------------------------------------------------------------------ trace == scan prefixes
def _trace(d, dims, B, T, feat, act_ptr, act_sb, q, h_init=None, z_init=None, heads=True):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    gpu = feat.device
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    lat, plog, prlog = (torch.empty(B, T, R * C, device=gpu) for _ in range(3))
    hid = torch.empty(B, T, Hd, device=gpu)
    rew, cont = (torch.empty(B, T, device=gpu), torch.empty(B, T, device=gpu)) if heads else (None, None)
    ws = torch.empty(L.query("dr_observe_trace_workspace_bytes", dims, B, T), dtype=torch.uint8, device=gpu)
    L.call("dr_observe_trace", dims, d.world_model.packed(), B, T, L.ptr(feat), act_ptr, act_sb, A, L.ptr(h_init),
           L.ptr(z_init), hip.explicit_noise(q=q, device=gpu), L.ptr(lat), L.ptr(hid), L.ptr(plog), L.ptr(prlog),
           L.ptr(rew), L.ptr(cont), L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return lat, hid, plog, prlog, rew, cont


def _scan(d, dims, B, T, feat, act, q):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    gpu = feat.device
    R, C = d.latent_state_dims
    z, lg = torch.empty(B, R * C, device=gpu), torch.empty(B, R * C, device=gpu)
    h = torch.empty(B, d.hidden_state_dims, device=gpu)
    ws = torch.empty(L.query("dr_observe_workspace_bytes", dims, B), dtype=torch.uint8, device=gpu)
    L.call("dr_observe_scan", dims, d.world_model.packed(), B, T, L.ptr(feat), L.ptr(act), act.shape[1] * A, A, None,
           None, hip.explicit_noise(q=q, device=gpu), L.ptr(z), L.ptr(h), L.ptr(lg), L.ptr(ws), ws.numel(),
           hip.stream())
    torch.cuda.synchronize()
    return z, h, lg


@pytest.mark.parametrize("case", ["small", "full"])
def test_trace_equals_scan_prefixes(case, gpu):
    """Entry t of the trace is dr_observe_scan's launch form on the prefix
    t + 1, bit for bit; the default scan (persistent where it applies) agrees
    on the final state; a trace in two time chunks equals the whole trace.
    B = 130: the smallest ragged batch on the grouped hidden-product / weight-
    plane branch (and, continuing, on its gh_pre branch)."""
    B, T, T1 = {"small": (3, 5, 2), "full": (130, 3, 1)}[case]
    d, _ = build(case, gpu, B=B, H=3, S=8)
    R, C = d.latent_state_dims
    dims = d.world_model.dims()
    g = torch.Generator().manual_seed(7)
    feat = (torch.randn(T * B, dims.enc_hidden, generator=g) * 0.5).to(gpu)
    act = (torch.rand(B, T, A, generator=g) * 2 - 1).to(gpu)
    q = torch.empty(T, B * R, C).exponential_(generator=g).to(gpu)
    lat, hid, plog, _, _, _ = _trace(d, dims, B, T, feat, act.data_ptr(), T * A, q)
    launch = d.world_model.dims()
    launch.launch_form = 1
    for t in range(T):
        z, h, lg = _scan(d, launch, B, t + 1, feat, act, q)
        assert torch.equal(z, lat[:, t]), (case, t, "z")
        assert torch.equal(h, hid[:, t]), (case, t, "h")
        assert torch.equal(lg, plog[:, t]), (case, t, "logits")
    z, h, _ = _scan(d, dims, B, T, feat, act, q)
    assert torch.equal(z.view(B, R, C).argmax(-1), lat[:, T - 1].reshape(B, R, C).argmax(-1))
    close(h, hid[:, T - 1], 2e-4, 2e-5, "default scan h")
    # two chunks through h_init / z_init: action T1 - 1 drives frame T1, draws T1.. follow
    a1 = _trace(d, dims, B, T1, feat, act.data_ptr(), T * A, q[:T1].contiguous())
    a2 = _trace(d, dims, B, T - T1, feat[T1 * B:].contiguous(), act.data_ptr() + 4 * (T1 - 1) * A, T * A,
                q[T1:].contiguous(), h_init=a1[1][:, T1 - 1].contiguous(), z_init=a1[0][:, T1 - 1].contiguous())
    whole = _trace(d, dims, B, T, feat, act.data_ptr(), T * A, q)
    for k, name in enumerate(("latents", "hiddens", "post_logits")):
        assert torch.equal(torch.cat((a1[k], a2[k]), dim=1), whole[k]), (case, name)
    # (the prior and the heads run once over all rows of a call: same values, the contract promises no bits)
    for k, name in ((3, "prior_logits"), (4, "rewards"), (5, "continues")):
        close(torch.cat((a1[k], a2[k]), dim=1), whole[k], 2e-4, 2e-5, f"{case} chunked {name}")


# ------------------------------------------------------------------ against the oracle
def _noise(seed, T, B, R, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(T, B * R, C).exponential_(generator=g), torch.empty(T, B * R, C).exponential_(generator=g))


def _oracle(P, obs, act, T, R, C, q_post, q_prior, heads=True):
    """The issue's recipe; q_post / q_prior are widened in place by the guard."""
    obs = obs if obs.dim() == 3 else O.normalise_obs(obs)
    B = obs.shape[0]
    hidden = P[O.WM + "sequence_model.GRU.weight_hh"].shape[1]
    with TieGuard() as tg, torch.no_grad():
        h = torch.zeros(B, 1, hidden)
        z, lg = O.encode(h, obs[:, 0:1], P, q_post[0], R, C)
        zs, hs, lgs = [z], [h], [lg]
        for t in range(1, T):
            z, h, lg = O.observe_step(z, h, act[:, t - 1:t], obs[:, t:t + 1], P, q_post[t], R, C)
            zs.append(z); hs.append(h); lgs.append(lg)
        cat = lambda xs: torch.cat(xs, dim=1)
        lat, hid, plog = cat(zs), cat(hs), cat(lgs)
        prlog = O.prior_logits(hid, P, R, C)
        zp = cat([O.prior_predict(hid[:, t:t + 1], P, q_prior[t], R, C)[0] for t in range(T)])
        rew = cont = None
        if heads and T > 1:
            rew = O.reward_predict(hid[:, 1:], lat[:, 1:], P)
            cont = O.continue_forward(hid[:, 1:], lat[:, 1:], P)[0]
    return dict(lat=lat, hid=hid, plog=plog, prlog=prlog, zp=zp, rew=rew, cont=cont, tg=tg)


def _check_stats(res, what):
    """kl and the entropies against float64 on the GPU's own logits, by test 1's bound."""
    B, T, R, C = res.post_logits.shape
    post, prior = cpu(res.post_logits).reshape(B * T, R, C), cpu(res.prior_logits).reshape(B * T, R, C)
    (kl64, hq64, hp64), b_kl, b_ent = _stats_bounds(post, prior, what)
    e = (_rel(cpu(res.kl).reshape(-1), kl64), _rel(cpu(res.post_entropy).reshape(-1), hq64),
         _rel(cpu(res.prior_entropy).reshape(-1), hp64))
    print(f"{what}: max rel err kl {e[0]:.3e} (bound {b_kl:.3e}), entropies {e[1]:.3e} {e[2]:.3e} (bound {b_ent:.3e})")
    assert e[0] <= b_kl and e[1] <= b_ent and e[2] <= b_ent, (what, e)


def _check_against_oracle(res, o, what):
    assert torch.equal(cpu(res.latents).argmax(-1), o["lat"].argmax(-1)), what
    assert torch.equal(cpu(res.latents_prior).argmax(-1), o["zp"].argmax(-1)), what
    assert float((cpu(res.latents) - o["lat"]).abs().max()) <= 1.2e-7
    assert float((cpu(res.latents_prior) - o["zp"]).abs().max()) <= 1.2e-7
    close(res.hiddens, o["hid"], 2e-4, 2e-5, f"{what} hiddens")
    close(res.post_logits, o["plog"], 2e-4, 2e-5, f"{what} post_logits")
    close(res.prior_logits, o["prlog"], 2e-4, 2e-5, f"{what} prior_logits")
    if o["rew"] is not None:
        close(res.reward_pred, O.symlog(o["rew"]), 2e-4, 2e-5, f"{what} reward_pred (symlog)")
        close(res.continue_pred, o["cont"], 2e-4, 2e-5, f"{what} continue_pred")


CASES = {"small-B4": ("small", 4, 8, 6, [0, 5, 17, 56]),
         "full-B2": ("full", 2, 8, 6, [3, 56]),
         # the smallest batch that takes the grouped hidden-product branch
         "full-B128": ("full", 128, 4, 3, [(7 * i) % 61 for i in range(128)])}


@pytest.mark.parametrize("case", list(CASES))
def test_closed_loop_matches_oracle(case, gpu):
    which, B, S, T, starts = CASES[case]
    d, P = build(which, gpu, B=B, H=3, S=S)
    hw = tuple(CFG[which]["observation_dims"])
    R, C = d.latent_state_dims
    fr, ac, rw, ct = _fill(d, hw)
    obs, act = _windows(fr, starts, S).float(), _windows(ac, starts, S)
    q_post, q_prior = _noise(43, T, B, R, C)
    o = _oracle(P, obs, act, T, R, C, q_post, q_prior)
    print(f"{case}: {o['tg'].guarded} guarded groups of {o['tg'].draws} draws")
    with torch.no_grad():
        res = d.closed_loop(starts=np.asarray(starts), length=T, noise=(q_post.to(gpu), q_prior.to(gpu)))
    torch.cuda.synchronize()
    assert res.length == T and res.latents.shape == (B, T, R, C)
    _check_against_oracle(res, o, case)
    # the decoder on the GPU's own states
    with torch.no_grad():
        close(res.mu_post, O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, hw), 1e-4, 1e-5, "mu_post")
        close(res.mu_prior, O.decoder_forward(cpu(res.hiddens), cpu(res.latents_prior), P, hw), 1e-4, 1e-5, "mu_prior")
    _check_stats(res, case)
    x = _x_of_u8(res.frames_true.cpu())
    _sqerr_bound_check(res.sqerr_post, res.mu_post, x, f"{case} post")
    _sqerr_bound_check(res.sqerr_prior, res.mu_prior, x, f"{case} prior")
    # alignment: frames against slot start + t, the targets of state t >= 1 against slot start + t - 1, bit for bit
    rt, ctn, ft = cpu(res.reward_true), cpu(res.continue_true), res.frames_true.cpu()
    assert rt.shape == (B, T - 1, 1) and ctn.shape == (B, T - 1, 1) and ft.shape == (B, T, 3, *hw)
    for b, s0 in enumerate(starts):
        for t in range(T):
            assert np.array_equal(ft[b, t].numpy(), fr[s0 + t]), (b, t)
            if t >= 1:
                assert rt[b, t - 1, 0].item() == rw[s0 + t - 1], (b, t)
                assert ctn[b, t - 1, 0].item() == ct[s0 + t - 1], (b, t)


MODE_FILL_SEED = 0  # replay seed at which no group of the q == 1 draws needs the tie guard (found on the CPU)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_closed_loop_consistent(precision, gpu):
    """Self-consistency of one result (FULL, B = 2, T = 4): two calls with the
    same noise agree bit for bit, every field is finite, the latents are
    one-hots, frames_* are the quantisation of mu_*, the helpers have the stated
    shapes and layout, predict=False drops the prior fields and changes nothing
    else, sample=False is explicit q == 1 -- and, fp32, the oracle's mode.  bf16
    mode is held to these checks only, for the reason
    test_open_loop_metrics_consistent gives."""
    B, S, T = 2, 8, 4
    d, P = build("full", gpu, B=B, H=3, S=S)
    d.precision = d.world_model.precision = precision
    hw = tuple(FULL["observation_dims"])
    R, C = d.latent_state_dims
    fr, ac, _, _ = _fill(d, hw, seed=MODE_FILL_SEED)
    noise = tuple(t.to(gpu) for t in _noise(5, T, B, R, C))
    starts = np.array([10, 44])
    with torch.no_grad():
        r1 = d.closed_loop(starts=starts, length=T, noise=noise)
        r2 = d.closed_loop(starts=starts, length=T, noise=noise)
        r3 = d.closed_loop(starts=starts, length=T, noise=noise, predict=False)
    torch.cuda.synchronize()
    f1, f2, f3 = _fields(r1), _fields(r2), _fields(r3)
    prior_fields = {"mu_prior", "latents_prior", "sqerr_prior", "frames_prior"}
    assert set(f1) == {"latents", "hiddens", "post_logits", "prior_logits", "kl", "post_entropy", "prior_entropy",
                       "mu_post", "sqerr_post", "frames_post", "frames_true", "reward_pred", "reward_true",
                       "continue_pred", "continue_true"} | prior_fields
    assert set(f3) == set(f1) - prior_fields and all(getattr(r3, k) is None for k in prior_fields)
    for k in f1:
        assert torch.equal(f1[k], f2[k]), k
        assert bool(torch.isfinite(f1[k].float()).all()), k
        if k not in prior_fields:
            assert torch.equal(f1[k], f3[k]), k
    for lat in (cpu(r1.latents), cpu(r1.latents_prior)):
        assert float((lat.sum(-1) - 1).abs().max()) <= 1e-6 and float((lat.max(-1).values - 1).abs().max()) <= 1e-6
    x = _x_of_u8(r1.frames_true.cpu())
    _sqerr_bound_check(r1.sqerr_post, r1.mu_post, x, f"closed_loop post {precision}")
    _sqerr_bound_check(r1.sqerr_prior, r1.mu_prior, x, f"closed_loop prior {precision}")
    _check_stats(r1, f"closed_loop {precision}")
    assert torch.equal(r1.frames_post.cpu(), _quant(r1.mu_post))
    assert torch.equal(r1.frames_prior.cpu(), _quant(r1.mu_prior))
    n = 3 * hw[0] * hw[1]
    assert torch.equal(r1.mse_post(), r1.sqerr_post / n) and r1.mse_post().shape == (B, T)
    assert torch.equal(r1.mse_prior(), r1.sqerr_prior / n)
    for ps, frames in ((r1.psnr_post(), r1.frames_post), (r1.psnr_prior(), r1.frames_prior)):
        dq = frames.float() - r1.frames_true.float()
        assert ps.shape == (B, T)
        close(ps, 10 * torch.log10(255.0 ** 2 / dq.pow(2).flatten(2).mean(-1)), 1e-6, 0, "psnr")
    v = r1.video()
    assert v.dtype == torch.uint8 and v.shape == (T, 3, 3 * hw[0], B * hw[1])
    for b in range(B):
        for t in range(T):
            cols = slice(b * hw[1], (b + 1) * hw[1])
            assert torch.equal(v[t][:, :hw[0], cols], r1.frames_true[b][t])
            assert torch.equal(v[t][:, hw[0]:2 * hw[0], cols], r1.frames_post[b][t])
            assert torch.equal(v[t][:, 2 * hw[0]:, cols], r1.frames_prior[b][t])
    # the mode: sample=False is q == 1 for both draws
    ones = torch.ones(T, B * R, C, device=gpu)
    with torch.no_grad():
        m1 = d.closed_loop(starts=starts, length=T, sample=False)
        m2 = d.closed_loop(starts=starts, length=T, noise=(ones, ones))
    g1, g2 = _fields(m1), _fields(m2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    if precision == "fp32":
        qa, qb = torch.ones(T, B * R, C), torch.ones(T, B * R, C)
        o = _oracle(P, _windows(fr, starts, S).float(), _windows(ac, starts, S), T, R, C, qa, qb)
        assert o["tg"].guarded == 0 and bool((qa == 1).all()) and bool((qb == 1).all()), \
            f"{o['tg'].guarded} guarded groups: pick another MODE_FILL_SEED"
        _check_against_oracle(m1, o, "mode")


def test_closed_loop_vector_and_deep(gpu):
    """Vector observations (observation_dims = [24], test_gpu_vector.py's widths,
    B = 4, T = 4) against the oracle as in test_closed_loop_matches_oracle, with
    no frame fields; and the depth-5 VAE (128 x 128, test_gpu_deep_vae.py's
    config at B = 2, T = 2): mu against O.decoder_forward on the GPU's own states,
    the statistics and sqerr by their bounds."""
    from test_gpu_deep_vae import _dreamer as deep_dreamer
    from test_gpu_vector import D_OBS, _dreamer as vec_dreamer
    params = lambda dr: {k: v.detach().cpu().clone() for k, v in dr.state_dict().items()}
    # --- vector
    B, S, T = 4, 8, 4
    d = vec_dreamer(gpu, batch_size=B, sequence_length=S, horizon=3, buffer_size=N_FILL)
    P = params(d)
    R, C = d.latent_state_dims
    _, ac, rw, ct = replay_data(N_FILL, (2, 2), A, seed=3)
    rows = torch.randn(N_FILL, D_OBS, generator=torch.Generator().manual_seed(4)).numpy()
    d.buffer.load_arrays(rows, ac, rw, ct)
    starts = [1, 20, 33, 56]
    obs, act = _windows(rows, starts, S), _windows(ac, starts, S)
    q_post, q_prior = _noise(17, T, B, R, C)
    o = _oracle(P, obs, act, T, R, C, q_post, q_prior)
    print(f"vector: {o['tg'].guarded} guarded groups of {o['tg'].draws} draws")
    with torch.no_grad():
        res = d.closed_loop(starts=np.asarray(starts), length=T, noise=(q_post.to(gpu), q_prior.to(gpu)))
    _check_against_oracle(res, o, "vector")
    assert res.mu_post.shape == (B, T, D_OBS) and res.mu_prior.shape == (B, T, D_OBS)
    with torch.no_grad():
        close(res.mu_post, O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, None), 1e-4, 1e-5, "vector mu_post")
        close(res.mu_prior, O.decoder_forward(cpu(res.hiddens), cpu(res.latents_prior), P, None), 1e-4, 1e-5,
              "vector mu_prior")
    x = torch.stack([torch.from_numpy(rows[s0:s0 + T]) for s0 in starts])
    _sqerr_bound_check(res.sqerr_post, res.mu_post, x, "vector closed_loop post")
    _sqerr_bound_check(res.sqerr_prior, res.mu_prior, x, "vector closed_loop prior")
    _check_stats(res, "vector")
    assert res.frames_post is None and res.frames_prior is None and res.frames_true is None
    assert res.mse_post().shape == (B, T) and res.mse_prior().shape == (B, T)
    for f in (res.video, res.psnr_post, res.psnr_prior):
        with pytest.raises(ValueError):
            f()
    # --- depth 5
    B, S, T = 2, 4, 2
    d = deep_dreamer(gpu, batch_size=B, sequence_length=S, horizon=2, buffer_size=N_FILL)
    P = params(d)
    fr, _, _, _ = _fill(d, (128, 128), seed=6)
    starts = [2, 60]
    with torch.no_grad():
        res = d.closed_loop(starts=np.asarray(starts), length=T)
        close(res.mu_post, O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, (128, 128)), 1e-4, 1e-5,
              "deep mu_post")
        close(res.mu_prior, O.decoder_forward(cpu(res.hiddens), cpu(res.latents_prior), P, (128, 128)), 1e-4, 1e-5,
              "deep mu_prior")
    assert res.mu_post.shape == (B, T, 3, 128, 128)
    for b, s0 in enumerate(starts):
        assert np.array_equal(res.frames_true[b].cpu().numpy(), fr[s0:s0 + T])
    x = _x_of_u8(res.frames_true.cpu())
    _sqerr_bound_check(res.sqerr_post, res.mu_post, x, "deep closed_loop post")
    _sqerr_bound_check(res.sqerr_prior, res.mu_prior, x, "deep closed_loop prior")
    _check_stats(res, "deep")
    assert torch.equal(res.frames_post.cpu(), _quant(res.mu_post))
    assert torch.equal(res.frames_prior.cpu(), _quant(res.mu_prior))


def test_evaluate_filter_leaves_state(gpu):
    """evaluate_filter leaves np.random's state and training_state() as it found
    them, returns finite curves of lengths T / T - 1, and a following
    train_Agent() gives the losses of a twin Dreamer that did not evaluate."""
    from dreamer_amd import hip
    B, S, H, T = 4, 8, 5, 6

    def run(evaluate):
        np.random.seed(3)
        hip.rng(gpu).reseed(11)
        hip.adhoc(gpu).reseed(12)
        d, _ = build("small", gpu, B=B, H=H, S=S)
        _fill(d, tuple(SMALL["observation_dims"]))
        if evaluate:
            before_np, before = np.random.get_state(), d.training_state()
            curves = d.evaluate_filter(batches=2, length=T)
            after_np, after = np.random.get_state(), d.training_state()
            assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1])
            assert before_np[2:] == after_np[2:]
            _same(before, after)
            full = ("kl", "post_entropy", "prior_entropy", "mse_post", "mse_prior", "psnr_post", "psnr_prior")
            assert set(curves) == set(full) | {"reward_abs_err", "continue_bce"}
            assert all(len(curves[k]) == T for k in full)
            assert len(curves["reward_abs_err"]) == T - 1 and len(curves["continue_bce"]) == T - 1
            assert all(np.isfinite(v) for k in curves for v in curves[k]), curves
        la, lc = d.train_Agent()
        torch.cuda.synchronize()
        return la.detach().cpu().clone(), lc.detach().cpu().clone()

    got, ref = run(True), run(False)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (got, ref)


def test_closed_loop_argument_errors(gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, S = 2, 8
    d, _ = build("small", gpu, B=B, H=3, S=S)
    _fill(d, tuple(SMALL["observation_dims"]))
    starts = np.array([0, 9])
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    for T in (0, S + 1):
        with pytest.raises(ValueError):
            d.closed_loop(starts=starts, length=T)
    good = torch.ones(4, B * R, C, device=gpu)
    for bad in ((good, good[:3]), (good[:, :-1], good), (good[..., :-1], good[..., :-1])):
        with pytest.raises(ValueError):
            d.closed_loop(starts=starts, length=4, noise=bad)
    # T = 1: no GRU step, empty head fields
    r = d.closed_loop(starts=starts, length=1)
    torch.cuda.synchronize()
    assert r.latents.shape == (B, 1, R, C) and r.kl.shape == (B, 1) and r.sqerr_prior.shape == (B, 1)
    assert r.reward_pred.shape == (B, 0, 1) and r.continue_true.shape == (B, 0, 1)
    assert bool((r.hiddens == 0).all()) and bool(torch.isfinite(r.kl).all())
    # the C entry point
    wmod = d.world_model
    dims, wm = wmod.dims(), wmod.packed()
    T = 3
    feat = torch.zeros(T * B, dims.enc_hidden, device=gpu)
    act = torch.zeros(B, T, A, device=gpu)
    lat, hid = torch.empty(B, T, R * C, device=gpu), torch.empty(B, T, Hd, device=gpu)
    rew, cont = torch.empty(B, T, device=gpu), torch.empty(B, T, device=gpu)
    need = L.query("dr_observe_trace_workspace_bytes", dims, B, T)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    nz = hip.explicit_noise(q=torch.ones(T, B * R, C, device=gpu), device=gpu)

    def call(f=feat, a=act, out=lat, h=hid, r=rew, c=cont, nbytes=need):
        L.call("dr_observe_trace", dims, wm, B, T, L.ptr(f), L.ptr(a), T * A, A, None, None, nz, L.ptr(out), L.ptr(h),
               None, None, L.ptr(r), L.ptr(c), L.ptr(ws), nbytes, hip.stream())

    call()  # the arguments are good as they stand (post_logits / prior_logits may be NULL)
    call(r=None, c=None)
    torch.cuda.synchronize()
    for kw in (dict(f=None), dict(a=None), dict(out=None), dict(h=None), dict(r=None), dict(c=None)):
        with pytest.raises(L.HipError) as e:
            call(**kw)
        assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:
        call(nbytes=need - 1)
    assert e.value.code == L.DR_E_WORKSPACE
