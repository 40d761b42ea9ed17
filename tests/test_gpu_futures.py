"""Sampled futures on replay windows (Dreamer.sample_futures, evaluate_futures,
dr_frame_ssim, dr_ensemble_metrics) against the float64 reference of
futures_ref.py.  Bounds are DESIGN 5h's rule -- 8 x the error of the f32
transcription on the same inputs, relative to max(1, |ref|), at least 4 x
2^-24 -- with the 1e-4 cap kept for dr_ensemble_metrics and dropped for
dr_frame_ssim (DESIGN 5k has the measured tables).  Run on the MI355X box:
pytest -m gpu."""
import numpy as np
import pytest
import torch

import futures_ref as FR
from formula import SMALL, replay_data
from gpu_helpers import build, cpu

pytestmark = pytest.mark.gpu
A = 3
N_FILL = 64


def _dims(h=0, w=0, obs_dim=0):
    from dreamer_amd import _lib as L
    d = L.dr_dims()
    d.img_h, d.img_w, d.obs_dim = h, w, obs_dim
    return d


def _offset(t, k, gpu):
    """A device copy of t whose base is k elements past an aligned allocation."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=gpu)
    out = flat[k:k + t.numel()].view(t.shape)
    out.copy_(t)
    return out


# ---------------------------------------------------------------- dr_frame_ssim
KINDS = ("noise", "near", "clamp", "ramp", "const_eq", "const_ne")
SSIM_STARTS, SSIM_CAP, SSIM_T0 = [4, 9, 1], 11, 1  # slots (5,6) (10,0) (2,3): window 1 wraps


def _ssim_inputs(hw):
    """Six frames (B = 3, T = 2), one per kind: mu (3,2,3,h,w) f32 and the true u8 frames."""
    h, w = hw
    g = np.random.default_rng(h * 1000 + w)
    tru = g.integers(0, 256, size=(6, 3, h, w), dtype=np.uint8)
    mu = np.empty((6, 3, h, w), np.float32)
    mu[0] = g.random((3, h, w), dtype=np.float32) - np.float32(0.5)
    mu[1] = FR.x_of_u8(tru[1]) + np.float32(0.02) * g.standard_normal((3, h, w)).astype(np.float32)
    mu[2] = np.float32(2.0) * FR.x_of_u8(tru[2]) + np.float32(0.1) * g.standard_normal((3, h, w)).astype(np.float32)
    ramp = (np.arange(h)[:, None] * 255.0 / (h - 1) * 0.5 + np.arange(w)[None, :] * 255.0 / (w - 1) * 0.5)
    tru[3] = np.rint(ramp).astype(np.uint8)[None]
    mu[3] = (np.arange(w, dtype=np.float32)[None, None, :] / np.float32(w - 1) - np.float32(0.5)) \
        * np.ones((3, h, 1), np.float32)
    tru[4] = 77
    mu[4] = FR.x_of_u8(np.uint8(77))
    tru[5] = 200
    mu[5] = np.float32(-0.3)
    assert float(np.abs(mu[2]).max()) > 0.5  # the clamp matters
    return mu.reshape(3, 2, 3, h, w), tru.reshape(3, 2, 3, h, w)


def _ssim_call(d, B, T, mu_d, fr, gpu, ch=True):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    s = torch.full((B, T), -7.0, device=gpu)
    c = torch.full((B, T, 3), -7.0, device=gpu) if ch else None
    L.call("dr_frame_ssim", d, B, T, L.ptr(mu_d), fr, L.ptr(s), L.ptr(c), hip.stream())
    torch.cuda.synchronize()
    return cpu(s).numpy(), (cpu(c).numpy() if ch else None)


@pytest.mark.parametrize("hw", [(11, 11), (12, 13), (32, 32), (64, 64), (128, 128), (33, 70)])
def test_frame_ssim_kernel(hw, gpu):
    """dr_frame_ssim against the float64 reference on six kinds of frames, from
    the u8 ring (starts with a wrap, t0 = 1) at aligned and unaligned bases and
    from the f32 form; exact 1.0f on equal frames; the same bits at every base,
    source, position and batch size, and on a second run.

    Measured on the MI355X (max rel err of ssim / ssim_ch; yardstick in
    brackets): see DESIGN 5k."""
    from dreamer_amd import _lib as L
    h, w = hw
    n = 3 * h * w
    B, T = 3, 2
    mu, tru = _ssim_inputs(hw)
    x = FR.x_of_u8(tru)
    ref, ref_ch = FR.ssim_ref(mu, x)
    y32, y32_ch = FR.ssim_f32(mu, x)
    ring = np.zeros((SSIM_CAP, n), np.uint8)
    for b in range(B):
        for t in range(T):
            ring[(SSIM_STARTS[b] + SSIM_T0 + t) % SSIM_CAP] = tru[b, t].reshape(-1)
    d = _dims(h, w)
    st_d = torch.tensor(SSIM_STARTS, dtype=torch.int64, device=gpu)
    mu_t, ring_t = torch.from_numpy(mu), torch.from_numpy(ring)
    runs = {}
    for name, k in (("aligned", 0), ("unaligned", 1)):
        mu_d, ring_d = _offset(mu_t, k, gpu), _offset(ring_t, k, gpu)
        assert mu_d.data_ptr() % 16 == 4 * k and ring_d.data_ptr() % 4 == k
        runs[name] = _ssim_call(d, B, T, mu_d, L.dr_frames(L.ptr(ring_d), SSIM_CAP, L.ptr(st_d), None, 0, 0, 1, SSIM_T0),
                                gpu)
    mu_d = mu_t.to(gpu)
    obs = torch.zeros(B, T + SSIM_T0, n)
    obs[:, SSIM_T0:] = torch.from_numpy(tru.reshape(B, T, n)).float()
    obs_d = obs.to(gpu)
    runs["f32 raw255"] = _ssim_call(d, B, T, mu_d, L.dr_frames(None, 0, None, L.ptr(obs_d), (T + SSIM_T0) * n, n, 1,
                                                               SSIM_T0), gpu)
    xs = torch.zeros(B, T + SSIM_T0, n)
    xs[:, SSIM_T0:] = torch.from_numpy(x.reshape(B, T, n))
    xs_d = _offset(xs, 1, gpu)
    runs["f32 normalised, unaligned"] = _ssim_call(d, B, T, mu_d, L.dr_frames(None, 0, None, L.ptr(xs_d),
                                                                              (T + SSIM_T0) * n, n, 0, SSIM_T0), gpu)
    got, got_ch = runs["aligned"]
    for name, (s, c) in runs.items():  # the staging differs, the arithmetic and its order do not
        assert np.array_equal(s, got) and np.array_equal(c, got_ch), name
    # the bound: the constant unequal frame on its own yardstick, the other five on theirs
    flat = lambda a: a.reshape(6, *a.shape[2:])
    for sel, what in ((slice(0, 5), "textured"), (slice(5, 6), "const_ne")):
        y = max(FR.rel_err(flat(y32)[sel], flat(ref)[sel]), FR.rel_err(flat(y32_ch)[sel], flat(ref_ch)[sel]))
        e = max(FR.rel_err(flat(got)[sel], flat(ref)[sel]), FR.rel_err(flat(got_ch)[sel], flat(ref_ch)[sel]))
        print(f"frame_ssim {h}x{w} {what}: kernel max rel err {e:.3e} (f32-CPU yardstick {y:.3e}, "
              f"bound {FR.bound(y, None):.3e})")
        assert e <= FR.bound(y, None), (hw, what, e, y)
    per = {k: float(flat(got)[i]) for i, k in enumerate(KINDS)}
    print(f"frame_ssim {h}x{w}: " + ", ".join(f"{k} {v:.4f}" for k, v in per.items()))
    assert per["const_eq"] == 1.0 and np.all(flat(got_ch)[4] == np.float32(1.0))  # exactly 1.0f
    assert np.array_equal(got, ((got_ch[..., 0] + got_ch[..., 1]) + got_ch[..., 2]) / np.float32(3))
    ring_al = ring_t.to(gpu)
    # a frame alone, and at another position of a larger call: the same bits
    for b, t in ((0, 0), (1, 1), (2, 0)):
        one = torch.tensor([SSIM_STARTS[b] + t], dtype=torch.int64, device=gpu)
        s1, c1 = _ssim_call(d, 1, 1, mu_d[b, t].contiguous(), L.dr_frames(L.ptr(ring_al), SSIM_CAP, L.ptr(one),
                                                                          None, 0, 0, 1, SSIM_T0), gpu)
        assert s1[0, 0] == got[b, t] and np.array_equal(c1[0, 0], got_ch[b, t]), (b, t)
    perm = [5, 0, 3, 1, 4, 2, 0, 5]  # B = 2, T = 4 from the six frames in another order
    mu_p = torch.from_numpy(flat(mu)[perm].reshape(2, 4, n)).to(gpu)
    x_p = torch.from_numpy(flat(x)[perm].reshape(2, 4, n)).to(gpu)
    s2, c2 = _ssim_call(d, 2, 4, mu_p, L.dr_frames(None, 0, None, L.ptr(x_p), 4 * n, n, 0, 0), gpu)
    assert np.array_equal(s2.reshape(-1), flat(got)[perm]) and np.array_equal(c2.reshape(8, 3), flat(got_ch)[perm])
    # ssim_ch may be NULL
    s3, _ = _ssim_call(d, 2, 4, mu_p, L.dr_frames(None, 0, None, L.ptr(x_p), 4 * n, n, 0, 0), gpu, ch=False)
    assert np.array_equal(s3, s2)


def test_frame_ssim_refusals(gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    mu = torch.zeros(1, 1, 3 * 10 * 64, device=gpu)
    x = torch.zeros(1, 1, 3 * 10 * 64, device=gpu)
    out = torch.full((1, 1), -7.0, device=gpu)
    fr = L.dr_frames(None, 0, None, L.ptr(x), 3 * 10 * 64, 3 * 10 * 64, 0, 0)
    for hw in ((10, 64), (64, 10)):
        with pytest.raises(L.HipError) as e:
            L.call("dr_frame_ssim", _dims(*hw), 1, 1, L.ptr(mu), fr, L.ptr(out), None, hip.stream())
        assert e.value.code == L.DR_E_UNSUPPORTED
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_ssim", _dims(obs_dim=24), 1, 1, L.ptr(mu), fr, L.ptr(out), None, hip.stream())
    assert e.value.code == L.DR_E_INVALID
    torch.cuda.synchronize()
    assert float(out[0, 0]) == -7.0  # nothing was launched


# ---------------------------------------------------------- dr_ensemble_metrics
ENS_STARTS, ENS_CAP, ENS_T0 = [0, 7, 2], 9, 1  # window 1 wraps


def _ens_call(d, B, M, T, mu_d, fr, gpu, u8, n):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    sq, sp = torch.full((B, T), -7.0, device=gpu), torch.full((B, T), -7.0, device=gpu)
    mq = torch.zeros(B, T, n, dtype=torch.uint8, device=gpu) if u8 else None
    sd = torch.zeros(B, T, n, dtype=torch.uint8, device=gpu) if u8 else None
    mf = torch.zeros(B, T, n, device=gpu)
    L.call("dr_ensemble_metrics", d, B, M, T, L.ptr(mu_d), fr, L.ptr(sq), L.ptr(sp), L.ptr(mq), L.ptr(sd), L.ptr(mf),
           hip.stream())
    torch.cuda.synchronize()
    return dict(sqerr_mean=cpu(sq).numpy(), spread=cpu(sp).numpy(), mean_u8=mq.cpu().numpy() if u8 else None,
                std_u8=sd.cpu().numpy() if u8 else None, mean=cpu(mf).numpy())


def _frame_metrics(d, rows, T, mu_d, fr, gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    sq = torch.empty(rows, T, device=gpu)
    L.call("dr_frame_metrics", d, rows, T, L.ptr(mu_d), fr, L.ptr(sq), None, None, hip.stream())
    torch.cuda.synchronize()
    return cpu(sq).numpy()


@pytest.mark.parametrize("kind", ["pixels32", "vector24", "vector7"])
@pytest.mark.parametrize("M", [1, 2, 5, 64])
def test_ensemble_metrics_kernel(M, kind, gpu):
    """dr_ensemble_metrics against float64 (sqerr_mean, spread: the rule with the
    1e-4 cap; the inputs -- samples at the truth plus N(0, 0.05^2) for pixels,
    N(0,1) rows for vectors -- keep the yardstick under 1.25e-5), the mean frame
    and both u8 frames exactly (the f32 transcription has the kernel's order per
    element), M = 1 against dr_frame_metrics bit for bit, one window alone and a
    second run with the same bits, and the decomposition against
    dr_frame_metrics on the B*M rows."""
    from dreamer_amd import _lib as L
    B, T = 3, 2
    g = np.random.default_rng(100 * M + len(kind))
    pixels = kind == "pixels32"
    if pixels:
        n, d = 3 * 32 * 32, _dims(32, 32)
        ring = g.integers(0, 256, size=(ENS_CAP, n), dtype=np.uint8)
        xr = FR.x_of_u8(ring)
    else:
        n = int(kind[6:])
        d = _dims(obs_dim=n)
        ring = g.standard_normal((ENS_CAP, n)).astype(np.float32)
        xr = ring
    slots = (np.asarray(ENS_STARTS)[:, None] + ENS_T0 + np.arange(T)[None, :]) % ENS_CAP
    x = xr[slots]  # (B,T,n)
    noise = g.standard_normal((B, M, T, n)).astype(np.float32)
    mu = (x[:, None] + np.float32(0.05) * noise) if pixels else noise
    mu = np.ascontiguousarray(mu, np.float32)
    ref, y32 = FR.ensemble_ref(mu, x), FR.ensemble_ref(mu, x, np.float32)
    mu_d, ring_d = torch.from_numpy(mu).to(gpu), torch.from_numpy(ring).to(gpu)
    st_d = torch.tensor(ENS_STARTS, dtype=torch.int64, device=gpu)
    fr = L.dr_frames(L.ptr(ring_d), ENS_CAP, L.ptr(st_d), None, 0, 0, 1 if pixels else 0, ENS_T0)
    got = _ens_call(d, B, M, T, mu_d, fr, gpu, pixels, n)
    for k in ("sqerr_mean", "spread"):
        y, e = FR.rel_err(y32[k], ref[k]), FR.rel_err(got[k], ref[k])
        print(f"ensemble_metrics {kind} M={M} {k}: kernel max rel err {e:.3e} (f32-CPU yardstick {y:.3e}, "
              f"bound {FR.bound(y):.3e})")
        assert y < 1.25e-5, (k, y)
        assert e <= FR.bound(y), (k, e, y)
    # per element the kernel's operations are the transcription's, in its order
    assert np.array_equal(got["mean"], y32["mean"])
    if pixels:
        assert np.array_equal(got["mean_u8"], FR.quant(y32["mean"]))
        assert np.array_equal(got["std_u8"], FR.quant_std(y32["var"]))
        # ... and away from the rounding halves they are the float64 values' u8
        qm = (ref["mean"] + 0.5) * 255.0
        qs = 255.0 * np.sqrt(ref["var"])
        for q, u8 in ((qm, got["mean_u8"]), (qs, got["std_u8"])):
            away = np.abs(q - np.floor(q) - 0.5) > 1e-3
            assert away.mean() > 0.99
            assert np.array_equal(u8[away], np.clip(np.rint(q), 0, 255).astype(np.uint8)[away])
    # M = 1
    if M == 1:
        assert np.all(got["spread"] == 0.0)
        assert np.array_equal(got["sqerr_mean"], _frame_metrics(d, B, T, mu_d, fr, gpu))
    # the decomposition, between the two kernels' outputs
    st_rep = st_d.repeat_interleave(M)
    fr_rep = L.dr_frames(L.ptr(ring_d), ENS_CAP, L.ptr(st_rep), None, 0, 0, 1 if pixels else 0, ENS_T0)
    per = _frame_metrics(d, B * M, T, mu_d, fr_rep, gpu).reshape(B, M, T)
    lhs = per.astype(np.float64).mean(1)
    rhs = got["sqerr_mean"].astype(np.float64) + got["spread"].astype(np.float64)
    y_dec = max(FR.rel_err(y32["sqerr"].astype(np.float64).mean(1),
                           y32["sqerr_mean"].astype(np.float64) + y32["spread"].astype(np.float64)),
                FR.rel_err(y32["sqerr_mean"], ref["sqerr_mean"]), FR.rel_err(y32["spread"], ref["spread"]))
    print(f"ensemble_metrics {kind} M={M} decomposition: {FR.rel_err(lhs, rhs):.3e} (yardstick {y_dec:.3e})")
    assert FR.rel_err(lhs, rhs) <= FR.bound(y_dec)
    # window (1, 1) alone, and everything on a second run: the same bits
    one = torch.tensor([ENS_STARTS[1] + 1], dtype=torch.int64, device=gpu)
    fr1 = L.dr_frames(L.ptr(ring_d), ENS_CAP, L.ptr(one), None, 0, 0, 1 if pixels else 0, ENS_T0)
    g1 = _ens_call(d, 1, M, 1, mu_d[1, :, 1].contiguous(), fr1, gpu, pixels, n)
    assert g1["sqerr_mean"][0, 0] == got["sqerr_mean"][1, 1] and g1["spread"][0, 0] == got["spread"][1, 1]
    assert np.array_equal(g1["mean"][0, 0], got["mean"][1, 1])
    again = _ens_call(d, B, M, T, mu_d, fr, gpu, pixels, n)
    for k, v in got.items():
        assert v is None or np.array_equal(v, again[k]), k


def _halfway(scale_only):
    """f32 v with (v + 0.5f) * 255.0f (or 255.0f * v, scale_only) exactly k + 0.5."""
    f = np.float32
    out = {}
    for k in range(255):
        m = f((k + 0.5) / 255.0) if scale_only else f((k + 0.5) / 255.0 - 0.5)
        for cand in (m, np.nextafter(m, f(1)), np.nextafter(m, f(-1))):
            q = f(255.0) * cand if scale_only else (cand + f(0.5)) * f(255.0)
            if q == f(k + 0.5):
                out[k] = cand
                break
    return out


def test_ensemble_metrics_exact_halves(gpu):
    """Means and standard deviations that land exactly on k + 0.5 round half to
    even, as rintf does."""
    from dreamer_amd import _lib as L
    hm, hs = _halfway(False), _halfway(True)
    for hv in (hm, hs):
        assert len(hv) >= 8 and any(k % 2 for k in hv) and any(k % 2 == 0 for k in hv)
    n = 3 * 16 * 16
    mu = np.zeros((1, 2, 1, n), np.float32)
    km, ks = list(hm), list(hs)
    for i, k in enumerate(km):      # both samples at the halfway mean: mean exact, std 0
        mu[0, :, 0, i] = hm[k]
    for i, k in enumerate(ks):      # +-s around 0: mean 0, var = fl(s^2), sqrtf gives s back
        mu[0, 0, 0, len(km) + i] = hs[k]
        mu[0, 1, 0, len(km) + i] = -hs[k]
    assert len(km) + len(ks) <= n
    x = torch.zeros(1, 1, n, device=gpu)
    got = _ens_call(_dims(16, 16), 1, 2, 1, torch.from_numpy(mu).to(gpu),
                    L.dr_frames(None, 0, None, L.ptr(x), n, n, 0, 0), gpu, True, n)
    even = lambda k: k if k % 2 == 0 else k + 1  # k + 0.5 to even
    assert got["mean_u8"][0, 0, :len(km)].tolist() == [even(k) for k in km]
    assert got["std_u8"][0, 0, len(km):len(km) + len(ks)].tolist() == [even(k) for k in ks]
    y32 = FR.ensemble_ref(mu, np.zeros((1, 1, n), np.float32), np.float32)
    assert np.array_equal(got["mean_u8"], FR.quant(y32["mean"])) and np.array_equal(got["std_u8"], FR.quant_std(y32["var"]))


# ------------------------------------------------------- Dreamer.sample_futures
def _fill(d, hw, seed=0):
    fr, ac, rw, ct = replay_data(N_FILL, hw, A, seed=seed)
    d.buffer.load_arrays(fr, ac, rw, ct)
    return fr, ac, rw, ct


def _noise(seed, Tc, H, B, M, R, C):
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(Tc, B * R, C).exponential_(generator=g),
            torch.empty(H, B * M * R, C).exponential_(generator=g))


SHARED = ("latents", "hiddens", "mu", "frames_pred", "sqerr", "reward_pred", "continue_pred")


@pytest.fixture(scope="module")
def small(gpu):
    """One SMALL Dreamer with a filled ring, shared by the tests below (none of them changes it)."""
    B, S, H = 3, 8, 3
    d, _ = build("small", gpu, B=B, H=H, S=S)
    _fill(d, tuple(SMALL["observation_dims"]))
    return d


def test_sample_futures_one_sample_is_open_loop(small, gpu):
    d = small
    B, Tc, H = 3, 4, 3
    R, C = d.latent_state_dims
    starts = np.array([0, 21, 56])
    q_ctx, q = (t.to(gpu) for t in _noise(3, Tc, H, B, 1, R, C))
    with torch.no_grad():
        f = d.sample_futures(starts=starts, context=Tc, horizon=H, samples=1, noise=(q_ctx, q))
        o = d.open_loop(starts=starts, context=Tc, horizon=H, noise=(q_ctx, q))
    torch.cuda.synchronize()
    assert (f.context, f.horizon, f.samples) == (Tc, H, 1)
    for k in SHARED:
        assert torch.equal(getattr(f, k)[:, 0], getattr(o, k)), k
    for k in ("frames_true", "reward_true", "continue_true"):
        assert torch.equal(getattr(f, k), getattr(o, k)), k
    assert torch.equal(f.mu_mean, o.mu) and torch.equal(f.frames_mean, o.frames_pred)
    assert torch.equal(f.sqerr_mean, o.sqerr) and bool((f.spread == 0).all()) and bool((f.frames_std == 0).all())
    assert torch.equal(f.ssim[:, 0], o.ssim()) and torch.equal(f.ssim_ensemble, o.ssim())
    assert f.best().tolist() == [0, 0, 0]


def test_sample_futures_equal_noise_blocks(small, gpu):
    d = small
    B, M, Tc, H = 3, 4, 4, 3
    R, C = d.latent_state_dims
    starts = np.array([5, 30, 41])
    q_ctx, q1 = (t.to(gpu) for t in _noise(4, Tc, H, B, 1, R, C))
    q = q1.view(H, B, 1, R, C).expand(H, B, M, R, C).reshape(H, B * M * R, C).contiguous()
    with torch.no_grad():
        f = d.sample_futures(starts=starts, context=Tc, horizon=H, samples=M, noise=(q_ctx, q))
    torch.cuda.synchronize()
    for k in SHARED + ("ssim",):
        v = getattr(f, k)
        for m in range(1, M):
            assert torch.equal(v[:, m], v[:, 0]), (k, m)
    assert bool((f.spread == 0).all()) and torch.equal(f.mu_mean, f.mu[:, 0])
    x = torch.from_numpy(FR.x_of_u8(f.frames_true.cpu().numpy())).to(gpu)
    assert torch.equal(f.truth(), x)
    assert torch.equal(f.coverage(), (f.mu[:, 0] == x).flatten(2).float().mean((0, 2)))
    assert f.best().tolist() == [0, 0, 0]  # an exact tie of all four: the lowest index


def test_sample_futures_samples_are_open_loop_rollouts(small, gpu):
    d = small
    B, M, Tc, H = 3, 4, 4, 3
    R, C = d.latent_state_dims
    hw = tuple(SMALL["observation_dims"])
    starts = np.array([2, 33, 50])
    q_ctx, q = (t.to(gpu) for t in _noise(6, Tc, H, B, M, R, C))
    with torch.no_grad():
        f = d.sample_futures(starts=starts, context=Tc, horizon=H, samples=M, noise=(q_ctx, q))
        for m in range(M):
            qm = q.view(H, B, M, R, C)[:, :, m].reshape(H, B * R, C).contiguous()
            o = d.open_loop(starts=starts, context=Tc, horizon=H, noise=(q_ctx, qm))
            for k in ("latents", "mu", "sqerr", "hiddens", "frames_pred", "reward_pred", "continue_pred"):
                assert torch.equal(getattr(f, k)[:, m], getattr(o, k)), (k, m)
            assert torch.equal(f.ssim[:, m], o.ssim()), m
    torch.cuda.synchronize()
    assert not torch.equal(f.latents[:, 0, 1:], f.latents[:, 1, 1:])  # the draws do differ
    assert torch.equal(f.latents[:, 0, 0], f.latents[:, 1, 0])        # state 0 is shared
    assert f.latents.shape == (B, M, H + 1, R, C) and f.mu.shape == (B, M, H + 1, 3, *hw)
    assert f.ssim.shape == (B, M, H + 1) and f.reward_pred.shape == (B, M, H, 1)
    # best() and coverage against the reference, the ensemble fields against float64
    sq = cpu(f.sqerr).numpy()
    assert f.best().tolist() == FR.best_ref(sq).tolist()
    mu = cpu(f.mu).numpy().reshape(B, M, H + 1, -1)
    x = FR.x_of_u8(f.frames_true.cpu().numpy()).reshape(B, H + 1, -1)
    assert np.allclose(cpu(f.coverage()).numpy(), FR.coverage_ref(mu, x), atol=1e-6)
    ref, y32 = FR.ensemble_ref(mu, x), FR.ensemble_ref(mu, x, np.float32)
    for k in ("sqerr_mean", "spread"):
        assert FR.rel_err(cpu(getattr(f, k)).numpy(), ref[k]) <= FR.bound(FR.rel_err(y32[k], ref[k])), k
    assert np.array_equal(cpu(f.mu_mean).numpy().reshape(B, H + 1, -1), y32["mean"])
    assert np.array_equal(f.frames_mean.cpu().numpy().reshape(B, H + 1, -1), FR.quant(y32["mean"]))
    assert np.array_equal(f.frames_std.cpu().numpy().reshape(B, H + 1, -1), FR.quant_std(y32["var"]))
    sref, _ = FR.ssim_ref(cpu(f.mu).numpy(), FR.x_of_u8(f.frames_true.cpu().numpy())[:, None])
    s32, _ = FR.ssim_f32(cpu(f.mu).numpy(), FR.x_of_u8(f.frames_true.cpu().numpy())[:, None])
    assert FR.rel_err(cpu(f.ssim).numpy(), sref) <= FR.bound(FR.rel_err(s32, sref), None)
    from dreamer_amd.futures import frame_ssim
    assert torch.equal(f.ssim_ensemble, frame_ssim(f.mu_mean, f.frames_true))
    # curves and the video
    assert bool((f.mse("best") <= f.mse("mean")).all())
    v = f.video()
    assert v.dtype == torch.uint8 and v.shape == (H + 1, 3, 4 * hw[0], B * hw[1])
    # ssim=False leaves the SSIM fields out and changes nothing else
    with torch.no_grad():
        f2 = d.sample_futures(starts=starts, context=Tc, horizon=H, samples=M, noise=(q_ctx, q), ssim=False)
    assert f2.ssim is None and f2.ssim_ensemble is None and torch.equal(f2.sqerr, f.sqerr)
    assert torch.equal(f2.spread, f.spread)


def test_sample_futures_argument_errors(small, gpu):
    d = small
    starts = np.array([0, 9])
    for kw in (dict(samples=0), dict(samples=65), dict(samples=2.5), dict(context=0), dict(context=6, horizon=3)):
        with pytest.raises(ValueError):
            d.sample_futures(starts=starts, **kw)
    R, C = d.latent_state_dims
    q_ctx, q = _noise(1, 4, 3, 2, 1, R, C)
    with pytest.raises(ValueError):  # q is sized for one sample, two are asked for
        d.sample_futures(starts=starts, context=4, horizon=3, samples=2, noise=(q_ctx.to(gpu), q.to(gpu)))
    with pytest.raises(ValueError):
        d.sample_futures(starts=np.zeros(1025, dtype=np.int64), samples=32)  # above PLAN_MAX_ROWS


def test_sample_futures_vector_and_deep(gpu):
    """A vector model (observation_dims = [24], B = 4, M = 3): no u8 / SSIM
    fields, every sample an open_loop rollout bit for bit, the ensemble fields by
    the bound; and the depth-5 VAE at 128 x 128 (B = 2, M = 2, H = 2): samples
    against open_loop, SSIM and the ensemble fields against float64."""
    from test_gpu_deep_vae import _dreamer as deep_dreamer
    from test_gpu_vector import D_OBS, _dreamer as vec_dreamer
    B, M, S, Tc, H = 4, 3, 8, 4, 4
    d = vec_dreamer(gpu, batch_size=B, sequence_length=S, horizon=H, buffer_size=N_FILL)
    R, C = d.latent_state_dims
    _, ac, rw, ct = replay_data(N_FILL, (2, 2), A, seed=3)
    rows = torch.randn(N_FILL, D_OBS, generator=torch.Generator().manual_seed(4)).numpy()
    d.buffer.load_arrays(rows, ac, rw, ct)
    starts = [1, 20, 33, 56]
    q_ctx, q = (t.to(gpu) for t in _noise(17, Tc, H, B, M, R, C))
    with torch.no_grad():
        f = d.sample_futures(starts=np.asarray(starts), context=Tc, horizon=H, samples=M, noise=(q_ctx, q))
        for m in range(M):
            qm = q.view(H, B, M, R, C)[:, :, m].reshape(H, B * R, C).contiguous()
            o = d.open_loop(starts=np.asarray(starts), context=Tc, horizon=H, noise=(q_ctx, qm))
            for k in ("latents", "mu", "sqerr"):
                assert torch.equal(getattr(f, k)[:, m], getattr(o, k)), (k, m)
    assert f.mu.shape == (B, M, H + 1, D_OBS) and f.mu_mean.shape == (B, H + 1, D_OBS)
    for k in ("frames_pred", "frames_mean", "frames_std", "frames_true", "ssim", "ssim_ensemble"):
        assert getattr(f, k) is None, k
    x = np.stack([rows[s0 + Tc - 1:s0 + Tc + H] for s0 in starts])
    assert np.array_equal(cpu(f.x_true).numpy(), x)
    ref, y32 = FR.ensemble_ref(cpu(f.mu).numpy(), x), FR.ensemble_ref(cpu(f.mu).numpy(), x, np.float32)
    for k in ("sqerr_mean", "spread"):
        assert FR.rel_err(cpu(getattr(f, k)).numpy(), ref[k]) <= FR.bound(FR.rel_err(y32[k], ref[k])), k
    assert f.mse("ensemble").shape == (B, H + 1) and f.coverage().shape == (H + 1,)
    assert f.reward_spread().shape == (B, H)
    for call in (f.psnr, f.ssim_curve, f.video):
        with pytest.raises(ValueError):
            call()
    curves = d.evaluate_futures(batches=1, context=Tc, horizon=H, samples=2)
    assert curves["psnr_mean"] is None and curves["ssim_best"] is None and len(curves["mse_ensemble"]) == H + 1
    # --- depth 5
    B, M, S, Tc, H = 2, 2, 4, 2, 2
    d = deep_dreamer(gpu, batch_size=B, sequence_length=S, horizon=H, buffer_size=N_FILL)
    R, C = d.latent_state_dims
    _fill(d, (128, 128), seed=6)
    starts = np.asarray([2, 60])
    q_ctx, q = (t.to(gpu) for t in _noise(8, Tc, H, B, M, R, C))
    with torch.no_grad():
        f = d.sample_futures(starts=starts, context=Tc, horizon=H, samples=M, noise=(q_ctx, q))
        for m in range(M):
            qm = q.view(H, B, M, R, C)[:, :, m].reshape(H, B * R, C).contiguous()
            o = d.open_loop(starts=starts, context=Tc, horizon=H, noise=(q_ctx, qm))
            for k in ("latents", "mu", "sqerr"):
                assert torch.equal(getattr(f, k)[:, m], getattr(o, k)), (k, m)
            assert torch.equal(f.frames_true, o.frames_true)
    assert f.mu.shape == (B, M, H + 1, 3, 128, 128)
    xt = FR.x_of_u8(f.frames_true.cpu().numpy())
    mu = cpu(f.mu).numpy()
    sref, s32 = FR.ssim_ref(mu, xt[:, None])[0], FR.ssim_f32(mu, xt[:, None])[0]
    assert FR.rel_err(cpu(f.ssim).numpy(), sref) <= FR.bound(FR.rel_err(s32, sref), None)
    ref = FR.ensemble_ref(mu.reshape(B, M, H + 1, -1), xt.reshape(B, H + 1, -1))
    y32 = FR.ensemble_ref(mu.reshape(B, M, H + 1, -1), xt.reshape(B, H + 1, -1), np.float32)
    for k in ("sqerr_mean", "spread"):
        assert FR.rel_err(cpu(getattr(f, k)).numpy(), ref[k]) <= FR.bound(FR.rel_err(y32[k], ref[k])), k


# ------------------------------------------------------ Dreamer.evaluate_futures
def _same(a, b, path="state"):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    else:
        assert a == b, path


def test_evaluate_futures_leaves_state(gpu):
    """evaluate_futures leaves np.random's state and training_state() as it
    found them, returns finite curves of lengths H+1 / H with mse_best <= mse_mean
    and mse_ensemble <= mse_mean (+ rounding) at every step, and a following
    train_Agent() gives the losses of a twin Dreamer that did not evaluate."""
    from dreamer_amd import hip
    from dreamer_amd.futures import CURVES
    B, S, H = 4, 8, 5

    def run(evaluate):
        np.random.seed(3)
        hip.rng(gpu).reseed(11)
        hip.adhoc(gpu).reseed(12)
        d, _ = build("small", gpu, B=B, H=H, S=S)
        _fill(d, tuple(SMALL["observation_dims"]))
        if evaluate:
            before_np, before = np.random.get_state(), d.training_state()
            curves = d.evaluate_futures(batches=2, context=3, horizon=4, samples=4)
            after_np, after = np.random.get_state(), d.training_state()
            assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1])
            assert before_np[2:] == after_np[2:]
            _same(before, after)
            assert set(curves) == set(CURVES)
            assert [len(curves[k]) for k in CURVES] == [5] * 9 + [4]
            assert all(np.isfinite(v) for k in curves for v in curves[k]), curves
            n = 3 * 32 * 32
            for t in range(5):
                assert curves["mse_best"][t] <= curves["mse_mean"][t], t
                # mean = ensemble + spread up to the rounding of three f32 sums of n terms
                tol = (n + 8) * 2.0 ** -24 * curves["mse_mean"][t]
                assert curves["mse_ensemble"][t] <= curves["mse_mean"][t] + tol, t
                assert abs(curves["mse_ensemble"][t] + curves["spread"][t] - curves["mse_mean"][t]) <= 3 * tol, t
                assert curves["psnr_best"][t] >= curves["psnr_mean"][t] and curves["ssim_best"][t] >= curves["ssim_mean"][t]
                assert 0.0 <= curves["coverage"][t] <= 1.0
            assert all(v >= 0 for v in curves["reward_spread"])
            with pytest.raises(ValueError):
                d.evaluate_futures(batches=0)
        la, lc = d.train_Agent()
        torch.cuda.synchronize()
        return la.detach().cpu().clone(), lc.detach().cpu().clone()

    got, ref = run(True), run(False)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (got, ref)


# ------------------------------------------- OpenLoopResult / ClosedLoopResult
def test_result_ssim_methods(small, gpu):
    """OpenLoopResult.ssim() and ClosedLoopResult.ssim() are dr_frame_ssim on the
    result's mu against the ring's frames."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    d = small
    B, Tc, H, S = 3, 4, 3, 8
    starts = np.array([7, 19, 44])
    st = torch.as_tensor(starts, dtype=torch.int64).to(gpu)
    dims = d.world_model.dims(d.agent)

    def by_hand(mu, T, t0):
        out = torch.empty(B, T, device=gpu)
        truth = d.buffer.frames_struct(st)
        truth.t0 = t0
        L.call("dr_frame_ssim", dims, B, T, L.ptr(mu.contiguous()), truth, L.ptr(out), None, hip.stream())
        return out

    with torch.no_grad():
        o = d.open_loop(starts=starts, context=Tc, horizon=H)
        c = d.closed_loop(starts=starts)
        fields = {k: v.clone() for k, v in vars(o).items() if isinstance(v, torch.Tensor)}
        so = o.ssim()
        assert so.shape == (B, H + 1) and torch.equal(so, by_hand(o.mu, H + 1, Tc - 1))
        for k, v in fields.items():  # a new method only: the result is as it was
            assert torch.equal(getattr(o, k), v), k
        sq, sp = c.ssim()
        assert sq.shape == (B, S) and torch.equal(sq, by_hand(c.mu_post, S, 0)) and torch.equal(sq, c.ssim_post())
        assert torch.equal(sp, by_hand(c.mu_prior, S, 0)) and torch.equal(sp, c.ssim_prior())
        c2 = d.closed_loop(starts=starts, predict=False)
        assert c2.ssim()[1] is None
        with pytest.raises(ValueError):
            c2.ssim_prior()
    assert bool((so <= 1.0).all()) and bool((sq <= 1.0).all())
