"""Sampled futures, host side (no GPU): properties of the float64 reference
(futures_ref.py), FuturesResult's arithmetic on hand-built tensors, and the
argument checks made before the device is touched."""
import numpy as np
import pytest
import torch

import futures_ref as FR


def _frames(seed, shape):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, size=shape, dtype=np.uint8)


def test_window_is_normalised_and_symmetric():
    w = FR.window()
    assert w.dtype == np.float32 and w.shape == (11,)
    assert np.array_equal(w, w[::-1])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-7
    assert int(np.argmax(w)) == 5


@pytest.mark.parametrize("hw", [(11, 11), (12, 13), (20, 17)])
def test_ssim_reference_properties(hw):
    x = FR.x_of_u8(_frames(1, (2, 3, *hw)))
    y = FR.x_of_u8(_frames(2, (2, 3, *hw)))
    s, ch = FR.ssim_ref(x, x)
    assert np.abs(s - 1.0).max() <= 1e-12 and np.abs(ch - 1.0).max() <= 1e-12
    sxy, cxy = FR.ssim_ref(x, y)
    syx, cyx = FR.ssim_ref(y, x)
    assert np.abs(sxy - syx).max() <= 1e-12 and np.abs(cxy - cyx).max() <= 1e-12
    assert sxy.shape == (2,) and cxy.shape == (2, 3)
    assert float(np.abs(sxy).max()) < 0.5  # noise against noise is far from 1
    # the clamp: a prediction beyond +-0.5 scores as the clamped one
    assert np.array_equal(FR.ssim_ref(4.0 * x, y)[0], FR.ssim_ref(FR.clamp(4.0 * x), y)[0])
    # the f32 transcription stays near the reference, and gives exactly 1 on equal frames
    s32, _ = FR.ssim_f32(x, y)
    assert FR.rel_err(s32, sxy) <= 1e-5
    assert np.all(FR.ssim_f32(x, x)[0] == np.float32(1.0))


def test_ssim_reference_against_direct_loop():
    """One position written out with plain loops."""
    x = FR.x_of_u8(_frames(3, (3, 11, 11))).astype(np.float64)
    y = FR.x_of_u8(_frames(4, (3, 11, 11))).astype(np.float64)
    w = FR.window().astype(np.float64)
    vals = []
    for c in range(3):
        mp = mx = pp = xx = px = 0.0
        for i in range(11):
            for j in range(11):
                ww = w[i] * w[j]
                mp += ww * x[c, i, j]; mx += ww * y[c, i, j]
                pp += ww * x[c, i, j] ** 2; xx += ww * y[c, i, j] ** 2; px += ww * x[c, i, j] * y[c, i, j]
        vp, vx, cv = pp - mp * mp, xx - mx * mx, px - mp * mx
        up, ux = mp + 0.5, mx + 0.5
        vals.append(((2 * up * ux + 1e-4) * (2 * cv + 9e-4)) / ((up * up + ux * ux + 1e-4) * (vp + vx + 9e-4)))
    s, ch = FR.ssim_ref(x.astype(np.float32), y.astype(np.float32))
    assert np.abs(ch - np.asarray(vals)).max() <= 1e-12 and abs(s - np.mean(vals)) <= 1e-12


@pytest.mark.parametrize("M", [1, 2, 5, 64])
def test_variance_decomposition(M):
    g = np.random.default_rng(M)
    mu = g.standard_normal((2, M, 3, 50)).astype(np.float32)
    x = g.standard_normal((2, 3, 50)).astype(np.float32)
    r = FR.ensemble_ref(mu, x)
    lhs = r["sqerr"].mean(1)
    rhs = r["sqerr_mean"] + r["spread"]
    assert (np.abs(lhs - rhs) / np.maximum(1.0, np.abs(lhs))).max() <= 1e-12
    if M == 1:
        assert np.all(r["spread"] == 0) and np.array_equal(r["sqerr_mean"], r["sqerr"][:, 0])
        r32 = FR.ensemble_ref(mu, x, np.float32)
        assert np.all(r32["spread"] == 0) and np.array_equal(r32["mean"], mu[:, 0])


def test_quantisers():
    assert FR.quant(np.float32([-1.0, -0.5, 0.0, 0.5, 1.0])).tolist() == [0, 0, 128, 255, 255]
    # rint: halves go to even
    assert FR.quant_std(np.float32([0.0, 1.0, 4.0, (0.5 / 255.0) ** 2, (1.5 / 255.0) ** 2])).tolist()[:3] == [0, 255, 255]
    assert np.rint(np.float32(0.5)) == 0 and np.rint(np.float32(1.5)) == 2


def _result(sqerr, B, M, K, hw=(4, 4), seed=0):
    """A FuturesResult on the CPU around a given sqerr (B,M,K)."""
    from dreamer_amd.futures import FuturesResult
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(B, M, K, 3, *hw, generator=g) - 0.5
    ft = torch.randint(0, 256, (B, K, 3, *hw), generator=g, dtype=torch.uint8)
    fp = torch.randint(0, 256, (B, M, K, 3, *hw), generator=g, dtype=torch.uint8)
    fm = torch.randint(0, 256, (B, K, 3, *hw), generator=g, dtype=torch.uint8)
    fs = torch.randint(0, 256, (B, K, 3, *hw), generator=g, dtype=torch.uint8)
    H = K - 1
    return FuturesResult(latents=torch.zeros(B, M, K, 2, 2), hiddens=torch.zeros(B, M, K, 3), mu=mu, frames_pred=fp,
                         sqerr=sqerr, ssim=torch.rand(B, M, K, generator=g), reward_pred=torch.rand(B, M, H, 1, generator=g),
                         continue_pred=torch.rand(B, M, H, 1, generator=g), mu_mean=mu.mean(1),
                         sqerr_mean=torch.rand(B, K, generator=g), spread=torch.rand(B, K, generator=g),
                         ssim_ensemble=torch.rand(B, K, generator=g), frames_mean=fm, frames_std=fs, frames_true=ft,
                         x_true=None, reward_true=torch.zeros(B, H, 1), continue_true=torch.ones(B, H, 1),
                         context=2, horizon=H)


def test_best_with_ties():
    B, M, K = 4, 5, 3
    sq = torch.tensor([[[9, 1, 1], [0, 1, 1], [5, 0.5, 1.5], [0, 3, 0], [0, 2, 0.5]],   # totals 2,2,2,3,2.5 -> 0
                       [[0, 4, 4], [0, 1, 2], [0, 2, 1], [0, 3, 3], [0, 1, 2]],         # 8,3,3,6,3 -> 1
                       [[0, 4, 4], [0, 1, 2], [0, 2, 0], [0, 3, 3], [0, 1, 1]],         # 8,3,2,6,2 -> 2
                       [[0, 1, 1], [0, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 1]]],        # -> 4
                      dtype=torch.float32)
    r = _result(sq, B, M, K)
    assert r.best().tolist() == [0, 1, 2, 4]   # state 0 never counts; exact ties go to the lower index
    assert r.best().tolist() == FR.best_ref(sq.numpy()).tolist()
    assert r.samples == M and r.frame_elems() == 48


def test_curve_arithmetic():
    B, M, K = 3, 4, 4
    g = torch.Generator().manual_seed(5)
    sq = torch.rand(B, M, K, generator=g) * 10
    r = _result(sq, B, M, K)
    n = 48.0
    best = FR.best_ref(sq.numpy())
    assert torch.equal(r.mse("mean"), sq.mean(1) / n)
    assert torch.equal(r.mse("best"), sq.min(1).values / n)
    assert torch.equal(r.mse("best_sample"), torch.stack([sq[b, best[b]] for b in range(B)]) / n)
    assert torch.equal(r.mse("ensemble"), r.sqerr_mean / n)
    assert bool((r.mse("best") <= r.mse("mean")).all()) and bool((r.mse("best") <= r.mse("best_sample")).all())
    d = r.frames_pred.float() - r.frames_true.float().unsqueeze(1)
    ps = 10 * torch.log10(255.0 ** 2 / d.pow(2).flatten(3).mean(-1))
    assert torch.allclose(r.psnr("mean"), ps.mean(1)) and torch.allclose(r.psnr("best"), ps.max(1).values)
    de = r.frames_mean.float() - r.frames_true.float()
    assert torch.allclose(r.psnr("ensemble"), 10 * torch.log10(255.0 ** 2 / de.pow(2).flatten(2).mean(-1)))
    assert torch.equal(r.ssim_curve("mean"), r.ssim.mean(1)) and torch.equal(r.ssim_curve("best"), r.ssim.max(1).values)
    assert torch.equal(r.ssim_curve("best_sample"), torch.stack([r.ssim[b, best[b]] for b in range(B)]))
    assert torch.equal(r.ssim_curve("ensemble"), r.ssim_ensemble)
    x = FR.x_of_u8(r.frames_true.numpy())
    assert np.array_equal(r.truth().numpy(), x)
    cov = r.coverage()
    assert cov.shape == (K,) and np.allclose(cov.numpy(), FR.coverage_ref(r.mu.numpy(), x), atol=1e-7)
    rs = r.reward_spread()
    assert rs.shape == (B, K - 1)
    assert torch.allclose(rs, torch.from_numpy(r.reward_pred.squeeze(-1).numpy().std(axis=1)))
    v = r.video()
    assert v.dtype == torch.uint8 and v.shape == (K, 3, 16, B * 4)
    for b in range(B):
        cols = slice(4 * b, 4 * b + 4)
        assert torch.equal(v[1][:, 0:4, cols], r.frames_true[b, 1])
        assert torch.equal(v[1][:, 4:8, cols], r.frames_pred[b, best[b], 1])
        assert torch.equal(v[1][:, 8:12, cols], r.frames_mean[b, 1])
        assert torch.equal(v[1][:, 12:16, cols], r.frames_std[b, 1])
    with pytest.raises(ValueError):
        r.mse("median")


def test_vector_result_has_no_pixel_curves():
    r = _result(torch.rand(2, 3, 3), 2, 3, 3)
    r.x_true = torch.rand(2, 3, 7)
    r.mu = torch.rand(2, 3, 3, 7)
    r.frames_true = r.frames_pred = r.frames_mean = r.frames_std = r.ssim = r.ssim_ensemble = None
    assert r.frame_elems() == 7 and r.mse("best").shape == (2, 3) and r.coverage().shape == (3,)
    for call in (r.psnr, r.ssim_curve, r.video):
        with pytest.raises(ValueError):
            call()


def test_argument_errors():
    from dreamer_amd import _lib as L
    from dreamer_amd.futures import check_futures
    from dreamer_amd.plan import PLAN_MAX_ROWS
    assert L.DR_ENSEMBLE_MAX_SAMPLES == 64
    check_futures(1, 1)
    check_futures(PLAN_MAX_ROWS // 64, 64)
    for B, M in ((1, 0), (1, 65), (1, -1), (1, 2.0), (1, 1.5), (1, True), (0, 4), (PLAN_MAX_ROWS // 64 + 1, 64),
                 (PLAN_MAX_ROWS, 2)):
        with pytest.raises(ValueError):
            check_futures(B, M)
    assert {"dr_frame_ssim", "dr_ensemble_metrics"} <= set(L.EXPORTED)


def test_entry_points_check_arguments_without_a_gpu():
    """NULL arguments, vector dims, small frames and M out of range are refused before any launch."""
    from dreamer_amd import _lib as L
    d = L.dr_dims()
    d.img_h, d.img_w = 32, 32
    fr = L.dr_frames(None, 0, None, 16, 0, 0, 0, 0)  # (a non-NULL obs pointer: never read, the call stops before)
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_ssim", d, 1, 1, None, fr, None, None, None)
    assert e.value.code == L.DR_E_INVALID
    d.img_h = 10
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_ssim", d, 1, 1, 16, fr, 16, None, None)
    assert e.value.code == L.DR_E_UNSUPPORTED
    d.img_h, d.obs_dim = 32, 5
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_ssim", d, 1, 1, 16, fr, 16, None, None)
    assert e.value.code == L.DR_E_INVALID
    for M in (0, 65):
        with pytest.raises(L.HipError) as e:
            L.call("dr_ensemble_metrics", d, 1, M, 1, 16, fr, 16, 16, None, None, None, None)
        assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:  # vector observations have no u8 outputs
        L.call("dr_ensemble_metrics", d, 1, 2, 1, 16, fr, 16, 16, 16, None, None, None)
    assert e.value.code == L.DR_E_INVALID
