"""Host-side checks of the closed-loop (posterior trace) path that need no GPU:
the ClosedLoopResult helpers on hand-made tensors, the window arithmetic
against a brute-force loop, the length check, and the argument checks of the
new C entry points that fail before any device work."""
import math

import numpy as np
import pytest
import torch

from formula import SMALL


def _result(B=2, T=3, h=2, w=3, vector=False, predict=True):
    from dreamer_amd import ClosedLoopResult
    g = torch.Generator().manual_seed(0)
    u8 = lambda: torch.randint(0, 256, (B, T, 3, h, w), generator=g, dtype=torch.uint8)
    if vector:
        mu, mp, fq, fp, ft = torch.randn(B, T, 5, generator=g), torch.randn(B, T, 5, generator=g), None, None, None
    else:
        mu, mp = torch.rand(B, T, 3, h, w, generator=g) - 0.5, torch.rand(B, T, 3, h, w, generator=g) - 0.5
        fq, fp, ft = u8(), u8(), u8()
    z = torch.zeros(B, T, 4, 4)
    bt = lambda: torch.rand(B, T, generator=g)
    hd = lambda: torch.zeros(B, T - 1, 1)
    return ClosedLoopResult(latents=z, hiddens=torch.zeros(B, T, 8), post_logits=z.clone(), prior_logits=z.clone(),
                            kl=bt(), post_entropy=bt(), prior_entropy=bt(), mu_post=mu,
                            mu_prior=mp if predict else None, latents_prior=z.clone() if predict else None,
                            sqerr_post=bt(), sqerr_prior=bt() if predict else None, frames_post=fq,
                            frames_prior=fp if predict else None, frames_true=ft, reward_pred=hd(), reward_true=hd(),
                            continue_pred=hd(), continue_true=hd(), length=T)


def test_result_mse_psnr_video():
    B, T, h, w = 2, 3, 2, 3
    r = _result(B, T, h, w)
    n = 3 * h * w
    assert torch.equal(r.mse_post(), r.sqerr_post / n) and torch.equal(r.mse_prior(), r.sqerr_prior / n)
    for ps, fr in ((r.psnr_post(), r.frames_post), (r.psnr_prior(), r.frames_prior)):
        assert ps.shape == (B, T)
        for b in range(B):
            for t in range(T):
                d = fr[b, t].double() - r.frames_true[b, t].double()
                assert math.isclose(ps[b, t].item(), 10 * math.log10(255.0 ** 2 / d.pow(2).mean().item()),
                                    rel_tol=1e-5)
    v = r.video()
    assert v.dtype == torch.uint8 and v.shape == (T, 3, 3 * h, B * w)
    for b in range(B):
        for t in range(T):
            cols = slice(b * w, (b + 1) * w)
            assert torch.equal(v[t][:, :h, cols], r.frames_true[b][t])
            assert torch.equal(v[t][:, h:2 * h, cols], r.frames_post[b][t])
            assert torch.equal(v[t][:, 2 * h:, cols], r.frames_prior[b][t])
    # identical frames: infinite PSNR, not NaN
    r.frames_post = r.frames_true.clone()
    assert bool(torch.isinf(r.psnr_post()).all())


def test_result_vector_observations_and_no_prediction():
    r = _result(vector=True)
    assert r.frames_post is None and r.frames_prior is None and r.frames_true is None
    assert torch.equal(r.mse_post(), r.sqerr_post / 5) and torch.equal(r.mse_prior(), r.sqerr_prior / 5)
    for f in (r.video, r.psnr_post, r.psnr_prior):
        with pytest.raises(ValueError):
            f()
    r = _result(predict=False)
    assert r.mse_post().shape == (2, 3) and r.psnr_post().shape == (2, 3)
    for f in (r.video, r.mse_prior, r.psnr_prior):
        with pytest.raises(ValueError):
            f()


def test_target_slots_match_brute_force():
    """State t <-> frame slot start + t, reward / continue slot start + t - 1
    (modulo the ring), for every trace length a window of S = 8 allows."""
    from dreamer_amd.closed_loop import frame_step, target_slots, target_step
    cap, S = 13, 8
    starts = [0, 5, 12, 9]
    for T in range(1, S + 1):
        fs, ts = target_slots(starts, T, cap)
        assert fs.shape == (len(starts), T) and ts.shape == (len(starts), T - 1)
        for b, s0 in enumerate(starts):
            for t in range(T):
                assert frame_step(t) == t and fs[b, t].item() == (s0 + t) % cap
                if t >= 1:
                    assert ts[b, t - 1].item() == (s0 + t - 1) % cap
                    # unroll_model's alignment: the target sits one step before the state's frame
                    assert target_step(t) == frame_step(t) - 1
    with pytest.raises(ValueError):
        target_step(0)
    with pytest.raises(ValueError):
        frame_step(-1)


def test_check_length():
    from dreamer_amd.closed_loop import check_length
    check_length(1, 1)
    check_length(1, 8)
    check_length(8, 8)
    for T in (0, 9, -1):
        with pytest.raises(ValueError):
            check_length(T, 8)


def test_closed_loop_argument_errors_need_no_gpu():
    """A bad length raises before the device is touched; the C entry points
    refuse null pointers and a bad (R, C) with DR_E_INVALID and answer the
    workspace query on the host."""
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    d = Dreamer(dict(SMALL), torch.device("cpu"))
    S = d.sequence_length
    for T in (0, S + 1):
        with pytest.raises(ValueError):
            d.closed_loop(starts=np.array([0]), length=T)
    dims = d.world_model.dims()
    q1, q4 = (L.query("dr_observe_trace_workspace_bytes", dims, 4, T) for T in (1, 4))
    assert q4 > q1 > L.query("dr_observe_workspace_bytes", dims, 4)
    with pytest.raises(L.HipError) as e:
        L.call("dr_observe_trace", dims, L.dr_world_model(), 1, 1, None, None, 0, 0, None, None, L.dr_noise(), None,
               None, None, None, None, None, None, 0, None)
    assert e.value.code == L.DR_E_INVALID
    for M, R, C in ((1, 4, 65), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        with pytest.raises(L.HipError) as e:
            L.call("dr_latent_stats", M, R, C, None, None, None, None, None, None, None)
        assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:  # good sizes, no pointers
        L.call("dr_latent_stats", 1, 4, 4, None, None, None, None, None, None, None)
    assert e.value.code == L.DR_E_INVALID
