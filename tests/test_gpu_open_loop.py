"""Open-loop world-model prediction on replay windows (Dreamer.open_loop,
WorldModel.imagine_actions, dr_imagine_actions, dr_frame_metrics) against the
CPU oracle composed from oracle.dreamer_oracle:

    z, h = O.warm_start(obs[:, :Tc], act[:, :Tc], 2 Tc, ...)      state 0
    h, z, r, c = O.imagine_step(h, z, act[:, Tc+k-2], ..., q[k-1]) state k = 1..H
    mu = O.decoder_forward(states 0..H)

under baseline_case.TieGuard, whose widened draws are what the GPU gets, so
every latent index must match exactly.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

from baseline_case import TieGuard
from formula import FULL, SMALL, replay_data
from gpu_helpers import CFG, build, close, cpu
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
A = 3
N_FILL = 64


def _fill(d, hw, seed=0):
    fr, ac, rw, ct = replay_data(N_FILL, hw, A, seed=seed)
    d.buffer.load_arrays(fr, ac, rw, ct)
    return fr, ac, rw, ct


def _windows(arr, starts, S):
    idx = np.asarray(starts)[:, None] + np.arange(S)[None, :]
    return torch.from_numpy(arr[idx])


def _noise(seed, Tc, H, B, R, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(Tc, B * R, C).exponential_(generator=g), torch.empty(H, B * R, C).exponential_(generator=g))


def _oracle(P, obs, act, Tc, H, R, C, q_ctx, q, hw):
    """The issue's recipe; q_ctx / q are widened in place by the guard."""
    with TieGuard() as tg, torch.no_grad():
        z, h = O.warm_start(obs[:, :Tc], act[:, :Tc], 2 * Tc, P, q_ctx, R, C)
        zs, hs, rs, cs = [z], [h], [], []
        for k in range(1, H + 1):
            h, z, r, c = O.imagine_step(h, z, act[:, Tc + k - 2:Tc + k - 1], P, q[k - 1], R, C)
            zs.append(z); hs.append(h); rs.append(r); cs.append(c)
        cat = lambda xs: torch.cat(xs, dim=1)
        lat, hid = cat(zs), cat(hs)
        mu = O.decoder_forward(hid, lat, P, hw)
    return lat, hid, cat(rs), cat(cs), mu, tg


def _sqerr_bound_check(sqerr, mu, x32, what):
    """sqerr against the float64 sum of (mu - x)^2 with x formed in f32, within
    relative (n + 8) 2^-24 (one rounding in the subtraction, two in the square,
    at most n - 1 in any summation order of non-negative terms)."""
    mu64 = cpu(mu).double().flatten(2)
    ref = (mu64 - x32.double().flatten(2)).pow(2).sum(-1)
    n = mu64.shape[-1]
    got = cpu(sqerr).double()
    rel = ((got - ref).abs() / ref).max().item()
    print(f"{what}: sqerr max rel err {rel:.3e} (bound {(n + 8) * 2.0 ** -24:.3e}, n = {n})")
    assert rel <= (n + 8) * 2.0 ** -24, (what, rel)


def _x_of_u8(u8):
    """True pixel: (float)u8 / 255.0f - 0.5f, this exact f32 expression."""
    return torch.from_numpy(u8.numpy().astype(np.float32) / np.float32(255.0) - np.float32(0.5))


def _quant(mu):
    """(u8) min(255, max(0, rintf((mu + 0.5f) * 255.0f))) in numpy f32 (np.rint rounds half to even)."""
    m = cpu(mu).numpy().astype(np.float32)
    v = np.rint((m + np.float32(0.5)) * np.float32(255.0))
    return torch.from_numpy(np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), v)).astype(np.uint8))


CASES = {"small-B4": ("small", 4, 8, 4, 4, [0, 5, 17, 56]),
         "full-B2": ("full", 2, 8, 4, 4, [3, 56]),
         # the smallest batch that takes the grouped hidden-product branch
         "full-B128": ("full", 128, 4, 2, 2, [(7 * i) % 61 for i in range(128)])}


@pytest.mark.parametrize("case", list(CASES))
def test_open_loop_matches_oracle(case, gpu):
    which, B, S, Tc, H, starts = CASES[case]
    d, P = build(which, gpu, B=B, H=H, S=S)
    hw = tuple(CFG[which]["observation_dims"])
    R, C = d.latent_state_dims
    fr, ac, rw, ct = _fill(d, hw)
    obs, act = _windows(fr, starts, S).float(), _windows(ac, starts, S)
    q_ctx, q = _noise(41, Tc, H, B, R, C)
    lat, hid, r, c, _, tg = _oracle(P, obs, act, Tc, H, R, C, q_ctx, q, hw)
    print(f"{case}: {tg.guarded} guarded groups of {tg.draws} draws")
    with torch.no_grad():
        res = d.open_loop(starts=np.asarray(starts), context=Tc, horizon=H, noise=(q_ctx.to(gpu), q.to(gpu)))
    torch.cuda.synchronize()
    assert (res.context, res.horizon) == (Tc, H)
    # latent indices exact at every k (no row left out), straight-through values within 1.2e-7
    assert torch.equal(cpu(res.latents).argmax(-1), lat.argmax(-1))
    assert float((cpu(res.latents) - lat).abs().max()) <= 1.2e-7
    close(res.hiddens, hid, 2e-4, 2e-5, "hiddens")
    close(res.reward_pred, O.symlog(r), 2e-4, 2e-5, "reward_pred (symlog)")
    close(res.continue_pred, c, 2e-4, 2e-5, "continue_pred")
    # the decoder on the GPU's own states
    with torch.no_grad():
        mu_ref = O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, hw)
    close(res.mu, mu_ref, 1e-4, 1e-5, "mu")
    # alignment: state k >= 1 against slot start + Tc + k - 2, frames against start + Tc - 1 + k, bit for bit
    rt, ctn, ft = cpu(res.reward_true), cpu(res.continue_true), res.frames_true.cpu()
    assert rt.shape == (B, H, 1) and ctn.shape == (B, H, 1) and ft.shape == (B, H + 1, 3, *hw)
    for b, s0 in enumerate(starts):
        for k in range(1, H + 1):
            assert rt[b, k - 1, 0].item() == rw[s0 + Tc + k - 2], (b, k)
            assert ctn[b, k - 1, 0].item() == ct[s0 + Tc + k - 2], (b, k)
        for k in range(H + 1):
            assert np.array_equal(ft[b, k].numpy(), fr[s0 + Tc - 1 + k]), (b, k)


def _dims(h=0, w=0, obs_dim=0):
    from dreamer_amd import _lib as L
    d = L.dr_dims()
    d.img_h, d.img_w, d.obs_dim = h, w, obs_dim
    return d


def _halfway_values():
    """f32 mu with (mu + 0.5f) * 255.0f exactly k + 0.5 (k even and odd)."""
    out = {}
    for k in range(255):
        m = np.float32((k + 0.5) / 255.0 - 0.5)
        for cand in (m, np.nextafter(m, np.float32(1)), np.nextafter(m, np.float32(-1))):
            if (cand + np.float32(0.5)) * np.float32(255.0) == np.float32(k + 0.5):
                out[k] = cand
                break
    return out


@pytest.mark.parametrize("hw", [(32, 32), (64, 64)])
def test_frame_metrics_kernel(hw, gpu):
    """dr_frame_metrics directly: exact u8 quantisation (round-half-even, clamp),
    exact copy of the true frames, sqerr within the derived bound, and the same
    bits for the same frame at another (b, t) and in a call with another B."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, T, cap = 3, 2, 11
    n = 3 * hw[0] * hw[1]
    g = torch.Generator().manual_seed(9)
    mu = torch.rand(B, T, n, generator=g) * 2 - 1
    half = _halfway_values()
    assert any(k % 2 for k in half) and any(k % 2 == 0 for k in half) and len(half) >= 8, half
    special = [-1.0, -0.5, 0.5, 1.0, -0.75, 0.75] + [float(v) for v in half.values()]
    for b in range(B):
        for t in range(T):
            mu[b, t, 5:5 + len(special)] = torch.tensor(special)
    q = ((mu + 0.5) * 255.0)
    assert bool((q < 0).any()) and bool((q > 255).any())  # the clamp matters
    ring = torch.randint(0, 256, (cap, n), generator=g, dtype=torch.uint8)
    starts = torch.tensor([4, 9, 3])  # t0 = 1: window 1 wraps (slots 10, 0); (2, 1) is the slot of (0, 0)
    mu[2, 1] = mu[0, 0]
    slots = (starts[:, None] + 1 + torch.arange(T)[None, :]) % cap
    truth = ring[slots]  # (B, T, n) u8
    x = _x_of_u8(truth)
    mu_d, ring_d, st_d = mu.to(gpu), ring.to(gpu), starts.to(gpu)
    d = _dims(*hw)

    def run(fr, Bc=B, Tc=T, mu_t=mu_d):
        sq = torch.empty(Bc, Tc, device=gpu)
        pu = torch.empty(Bc, Tc, n, dtype=torch.uint8, device=gpu)
        tu = torch.empty(Bc, Tc, n, dtype=torch.uint8, device=gpu)
        L.call("dr_frame_metrics", d, Bc, Tc, L.ptr(mu_t), fr, L.ptr(sq), L.ptr(pu), L.ptr(tu), hip.stream())
        torch.cuda.synchronize()
        return sq, pu.cpu(), tu.cpu()

    sq, pu, tu = run(L.dr_frames(L.ptr(ring_d), cap, L.ptr(st_d), None, 0, 0, 1, 1))
    assert torch.equal(pu, _quant(mu))
    assert torch.equal(tu, truth)
    _sqerr_bound_check(sq, mu, x, f"ring {hw}")
    assert cpu(sq)[2, 1].item() == cpu(sq)[0, 0].item()  # same frame, another (b, t): same bits
    # the f32 form (values 0..255, raw255) holds the same frames at window steps 1..T
    obs = torch.zeros(B, T + 1, n)
    obs[:, 1:] = truth.float()
    obs_d = obs.to(gpu)
    sq2, pu2, tu2 = run(L.dr_frames(None, 0, None, L.ptr(obs_d), (T + 1) * n, n, 1, 1))
    assert torch.equal(cpu(sq2), cpu(sq)) and torch.equal(pu2, pu) and torch.equal(tu2, truth)
    # ... and in a call with another B (one frame alone)
    one = torch.tensor([int(slots[0, 0]) - 1]).to(gpu)
    sq3, _, tu3 = run(L.dr_frames(L.ptr(ring_d), cap, L.ptr(one), None, 0, 0, 1, 1), 1, 1, mu_d[0, 0].contiguous())
    assert cpu(sq3)[0, 0].item() == cpu(sq)[0, 0].item() and torch.equal(tu3[0, 0], truth[0, 0])
    # pred_u8 / true_u8 may be NULL
    sq4 = torch.empty(B, T, device=gpu)
    L.call("dr_frame_metrics", d, B, T, L.ptr(mu_d), L.dr_frames(L.ptr(ring_d), cap, L.ptr(st_d), None, 0, 0, 1, 1),
           L.ptr(sq4), None, None, hip.stream())
    assert torch.equal(cpu(sq4), cpu(sq))


@pytest.mark.parametrize("D", [24, 7])
def test_frame_metrics_vector_rows(D, gpu):
    """Vector rows (D = 24: 16-byte loads; D = 7: the scalar path): sqerr by the
    bound through the f32 ring and the f32 form, pred_u8 = NULL accepted, a
    non-NULL pred_u8 refused."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, T, cap = 3, 2, 9
    g = torch.Generator().manual_seed(D)
    mu = torch.randn(B, T, D, generator=g)
    ring = torch.randn(cap, D, generator=g)
    starts = torch.tensor([0, 7, 2])
    x = ring[(starts[:, None] + 1 + torch.arange(T)[None, :]) % cap]
    d = _dims(obs_dim=D)
    mu_d, ring_d, st_d, x_d = mu.to(gpu), ring.to(gpu), starts.to(gpu), x.contiguous().to(gpu)
    sq = torch.empty(B, T, device=gpu)
    fr = L.dr_frames(L.ptr(ring_d), cap, L.ptr(st_d), None, 0, 0, 0, 1)
    L.call("dr_frame_metrics", d, B, T, L.ptr(mu_d), fr, L.ptr(sq), None, None, hip.stream())
    _sqerr_bound_check(sq, mu, x, f"vector ring D={D}")
    sq2 = torch.empty(B, T, device=gpu)
    L.call("dr_frame_metrics", d, B, T, L.ptr(mu_d), L.dr_frames(None, 0, None, L.ptr(x_d), T * D, D, 0, 0),
           L.ptr(sq2), None, None, hip.stream())
    assert torch.equal(cpu(sq2), cpu(sq))
    pu = torch.empty(B, T, D, dtype=torch.uint8, device=gpu)
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_metrics", d, B, T, L.ptr(mu_d), fr, L.ptr(sq), L.ptr(pu), None, hip.stream())
    assert e.value.code == L.DR_E_INVALID


def _fields(r):
    return {k: v for k, v in vars(r).items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_open_loop_metrics_consistent(precision, gpu):
    """Self-consistency of one result (FULL, B = 2): sqerr and frames_pred follow
    from the returned mu and frames_true, the helper methods have the stated
    shapes and layout, and two calls with the same explicit noise agree bit for
    bit.  bf16 mode is held to these checks and to finite, one-hot-valid outputs
    only: at these sizes one flipped latent index is already above
    test_gpu_bf16.py's flip-fraction bound, so an oracle comparison would prove
    nothing."""
    B, S, Tc, H = 2, 8, 4, 4
    d, _ = build("full", gpu, B=B, H=H, S=S)
    d.precision = d.world_model.precision = precision
    hw = tuple(FULL["observation_dims"])
    R, C = d.latent_state_dims
    _fill(d, hw)
    q_ctx, q = (t.to(gpu) for t in _noise(5, Tc, H, B, R, C))
    starts = np.array([10, 44])
    with torch.no_grad():
        r1 = d.open_loop(starts=starts, context=Tc, horizon=H, noise=(q_ctx, q))
        r2 = d.open_loop(starts=starts, context=Tc, horizon=H, noise=(q_ctx, q))
    torch.cuda.synchronize()
    f1, f2 = _fields(r1), _fields(r2)
    assert set(f1) == {"latents", "hiddens", "mu", "frames_pred", "frames_true", "sqerr", "reward_pred",
                       "reward_true", "continue_pred", "continue_true"}
    for k in f1:
        assert torch.equal(f1[k], f2[k]), k
        assert bool(torch.isfinite(f1[k].float()).all()), k
    lat = cpu(r1.latents)
    assert float((lat.sum(-1) - 1).abs().max()) <= 1e-6 and float((lat.max(-1).values - 1).abs().max()) <= 1e-6
    _sqerr_bound_check(r1.sqerr, r1.mu, _x_of_u8(r1.frames_true.cpu()), f"open_loop {precision}")
    assert torch.equal(r1.frames_pred.cpu(), _quant(r1.mu))
    n = 3 * hw[0] * hw[1]
    assert torch.equal(r1.mse(), r1.sqerr / n) and r1.mse().shape == (B, H + 1)
    ps = r1.psnr()
    dq = r1.frames_pred.float() - r1.frames_true.float()
    assert ps.shape == (B, H + 1)
    close(ps, 10 * torch.log10(255.0 ** 2 / dq.pow(2).flatten(2).mean(-1)), 1e-6, 0, "psnr")
    v = r1.video()
    assert v.dtype == torch.uint8 and v.shape == (H + 1, 3, 2 * hw[0], B * hw[1])
    for b in range(B):
        for k in range(H + 1):
            cols = slice(b * hw[1], (b + 1) * hw[1])
            assert torch.equal(v[k][:, :hw[0], cols], r1.frames_true[b][k])
            assert torch.equal(v[k][:, hw[0]:, cols], r1.frames_pred[b][k])


MODE_STATE_SEED = 2  # no group of the q == 1 draws needed the tie guard at this state seed


def test_imagine_actions_mode(gpu):
    """sample=False is the prior's mode: the oracle run with q == 1, indices
    exact (the guard, on a copy of the ones tensor, has nothing to widen at
    MODE_STATE_SEED)."""
    B, H = 4, 3
    d, P = build("full", gpu, B=B, H=H, S=8)
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    g = torch.Generator().manual_seed(MODE_STATE_SEED)
    h0 = torch.randn(B, 1, Hd, generator=g) * 0.5
    z0 = torch.nn.functional.one_hot(torch.randint(0, C, (B, 1, R), generator=g), C).float()
    act = torch.rand(B, H, A, generator=g) * 2 - 1
    ones = torch.ones(H, B * R, C)
    qg = ones.clone()
    with TieGuard() as tg, torch.no_grad():
        h, z = h0, z0
        zs, hs, rs, cs = [z], [h], [], []
        for k in range(H):
            h, z, r, c = O.imagine_step(h, z, act[:, k:k + 1], P, qg[k], R, C)
            zs.append(z); hs.append(h); rs.append(r); cs.append(c)
    assert tg.guarded == 0 and torch.equal(qg, ones), f"{tg.guarded} guarded groups: pick another MODE_STATE_SEED"
    with torch.no_grad():
        lat, hid, rew, cont = d.world_model.imagine_actions(h0.to(gpu), z0.to(gpu), act.to(gpu), sample=False)
    assert lat.shape == (B, H + 1, R, C) and hid.shape == (B, H + 1, Hd)
    assert rew.shape == (B, H, 1) and cont.shape == (B, H, 1)
    assert torch.equal(cpu(lat).argmax(-1), torch.cat(zs, 1).argmax(-1))
    close(hid, torch.cat(hs, 1), 2e-4, 2e-5, "hiddens")
    close(rew, torch.cat(rs, 1), 2e-4, 2e-5, "rewards")
    close(cont, torch.cat(cs, 1), 2e-4, 2e-5, "continues")
    # explicit noise goes through the same path: q == 1 given by the caller is the same call
    with torch.no_grad():
        lat2, hid2, _, _ = d.world_model.imagine_actions(h0.to(gpu), z0.to(gpu), act.to(gpu), noise_q=ones.to(gpu))
    assert torch.equal(lat2, lat) and torch.equal(hid2, hid)


def test_open_loop_vector_and_deep(gpu):
    """Vector observations (observation_dims = [24], test_gpu_vector.py's widths,
    B = 4) against the oracle as in test_open_loop_matches_oracle, with no frame
    fields; and the depth-5 VAE (128 x 128, test_gpu_deep_vae.py's config at
    B = 2, H = 2): mu against O.decoder_forward on the GPU's own states and sqerr
    by the bound."""
    from test_gpu_deep_vae import _dreamer as deep_dreamer
    from test_gpu_vector import D_OBS, _dreamer as vec_dreamer
    params = lambda dr: {k: v.detach().cpu().clone() for k, v in dr.state_dict().items()}
    # --- vector
    B, S, Tc, H = 4, 8, 4, 4
    d = vec_dreamer(gpu, batch_size=B, sequence_length=S, horizon=H, buffer_size=N_FILL)
    P = params(d)
    R, C = d.latent_state_dims
    _, ac, rw, ct = replay_data(N_FILL, (2, 2), A, seed=3)
    rows = torch.randn(N_FILL, D_OBS, generator=torch.Generator().manual_seed(4)).numpy()
    d.buffer.load_arrays(rows, ac, rw, ct)
    starts = [1, 20, 33, 56]
    obs, act = _windows(rows, starts, S), _windows(ac, starts, S)
    q_ctx, q = _noise(17, Tc, H, B, R, C)
    lat, hid, _, _, _, tg = _oracle(P, obs, act, Tc, H, R, C, q_ctx, q, None)
    print(f"vector: {tg.guarded} guarded groups of {tg.draws} draws")
    with torch.no_grad():
        res = d.open_loop(starts=np.asarray(starts), context=Tc, horizon=H, noise=(q_ctx.to(gpu), q.to(gpu)))
    assert torch.equal(cpu(res.latents).argmax(-1), lat.argmax(-1))
    close(res.hiddens, hid, 2e-4, 2e-5, "vector hiddens")
    assert res.mu.shape == (B, H + 1, D_OBS)
    with torch.no_grad():
        close(res.mu, O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, None), 1e-4, 1e-5, "vector mu")
    x = torch.stack([torch.from_numpy(rows[s0 + Tc - 1:s0 + Tc + H]) for s0 in starts])
    _sqerr_bound_check(res.sqerr, res.mu, x, "vector open_loop")
    assert res.frames_pred is None and res.frames_true is None
    assert res.mse().shape == (B, H + 1)
    with pytest.raises(ValueError):
        res.video()
    # --- depth 5
    B, S, Tc, H = 2, 4, 2, 2
    d = deep_dreamer(gpu, batch_size=B, sequence_length=S, horizon=H, buffer_size=N_FILL)
    P = params(d)
    fr, _, _, _ = _fill(d, (128, 128), seed=6)
    starts = [2, 60]
    with torch.no_grad():
        res = d.open_loop(starts=np.asarray(starts), context=Tc, horizon=H)
        close(res.mu, O.decoder_forward(cpu(res.hiddens), cpu(res.latents), P, (128, 128)), 1e-4, 1e-5, "deep mu")
    assert res.mu.shape == (B, H + 1, 3, 128, 128)
    for b, s0 in enumerate(starts):
        assert np.array_equal(res.frames_true[b].cpu().numpy(), fr[s0 + Tc - 1:s0 + Tc + H])
    _sqerr_bound_check(res.sqerr, res.mu, _x_of_u8(res.frames_true.cpu()), "deep open_loop")
    assert torch.equal(res.frames_pred.cpu(), _quant(res.mu))


def _same(a, b, path="state"):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    else:
        assert a == b, path


def test_evaluate_world_model_leaves_state(gpu):
    """evaluate_world_model leaves np.random's state and training_state() as it
    found them, returns finite curves of lengths H+1 / H, and a following
    train_Agent() gives the losses of a twin Dreamer that did not evaluate."""
    from dreamer_amd import hip
    B, S, H = 4, 8, 5

    def run(evaluate):
        np.random.seed(3)
        hip.rng(gpu).reseed(11)
        hip.adhoc(gpu).reseed(12)
        d, _ = build("small", gpu, B=B, H=H, S=S)
        _fill(d, tuple(SMALL["observation_dims"]))
        if evaluate:
            before_np, before = np.random.get_state(), d.training_state()
            curves = d.evaluate_world_model(batches=2, context=3, horizon=4)
            after_np, after = np.random.get_state(), d.training_state()
            assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1])
            assert before_np[2:] == after_np[2:]
            _same(before, after)
            assert [len(curves[k]) for k in ("mse", "psnr", "reward_abs_err", "continue_bce")] == [5, 5, 4, 4]
            assert all(np.isfinite(v) for k in curves for v in curves[k]), curves
        la, lc = d.train_Agent()
        torch.cuda.synchronize()
        return la.detach().cpu().clone(), lc.detach().cpu().clone()

    got, ref = run(True), run(False)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (got, ref)


def test_open_loop_argument_errors(gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, S, H = 2, 8, 3
    d, _ = build("small", gpu, B=B, H=H, S=S)
    _fill(d, tuple(SMALL["observation_dims"]))
    starts = np.array([0, 9])
    for Tc, Hh in ((0, 3), (4, 0), (4, S + 1 - 4)):
        with pytest.raises(ValueError):
            d.open_loop(starts=starts, context=Tc, horizon=Hh)
    wmod = d.world_model
    dims, wm = wmod.dims(), wmod.packed()
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    z0, h0 = torch.zeros(B, R * C, device=gpu), torch.zeros(B, Hd, device=gpu)
    z0.view(B, R, C)[..., 0] = 1
    act = torch.zeros(B, H, A, device=gpu)
    lat, hid = torch.empty(B, H + 1, R * C, device=gpu), torch.empty(B, H + 1, Hd, device=gpu)
    rew, cont = torch.empty(B, H, device=gpu), torch.empty(B, H, device=gpu)
    need = L.query("dr_imagine_actions_workspace_bytes", dims, B, H)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    q = torch.ones(H, B * R, C, device=gpu)
    nz = hip.explicit_noise(q=q, device=gpu)

    def call(z=z0, a=act, out=lat, nbytes=need):
        L.call("dr_imagine_actions", dims, wm, B, H, L.ptr(z), L.ptr(h0), L.ptr(a), H * A, A, nz, L.ptr(out),
               L.ptr(hid), L.ptr(rew), L.ptr(cont), L.ptr(ws), nbytes, hip.stream())

    call()  # the arguments are good as they stand
    torch.cuda.synchronize()
    for kw in (dict(z=None), dict(a=None), dict(out=None)):
        with pytest.raises(L.HipError) as e:
            call(**kw)
        assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:
        call(nbytes=need - 1)
    assert e.value.code == L.DR_E_WORKSPACE
    fdims = wmod.dims()
    mu = torch.zeros(1, 1, 3, fdims.img_h, fdims.img_w, device=gpu)
    sq = torch.empty(1, 1, device=gpu)
    st = torch.zeros(1, dtype=torch.int64, device=gpu)
    good = d.buffer.frames_struct(st)
    L.call("dr_frame_metrics", fdims, 1, 1, L.ptr(mu), good, L.ptr(sq), None, None, hip.stream())
    torch.cuda.synchronize()
    for args in ((None, good, L.ptr(sq)), (L.ptr(mu), None, L.ptr(sq)), (L.ptr(mu), good, None),
                 (L.ptr(mu), L.dr_frames(None, 0, None, None, 0, 0, 1, 0), L.ptr(sq))):
        with pytest.raises(L.HipError) as e:
            L.call("dr_frame_metrics", fdims, 1, 1, args[0], args[1], args[2], None, None, hip.stream())
        assert e.value.code == L.DR_E_INVALID
