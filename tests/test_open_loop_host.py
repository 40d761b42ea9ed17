"""Host-side checks of the open-loop prediction path that need no GPU: the
OpenLoopResult helpers on hand-made tensors, the window arithmetic against a
brute-force loop, and the argument checks that fail before any device work."""
import math

import numpy as np
import pytest
import torch

from formula import SMALL


def _result(B=2, H=2, h=2, w=3, vector=False):
    from dreamer_amd import OpenLoopResult
    K = H + 1
    g = torch.Generator().manual_seed(0)
    if vector:
        mu, fp, ft = torch.randn(B, K, 5, generator=g), None, None
    else:
        mu = torch.rand(B, K, 3, h, w, generator=g) - 0.5
        fp = torch.randint(0, 256, (B, K, 3, h, w), generator=g, dtype=torch.uint8)
        ft = torch.randint(0, 256, (B, K, 3, h, w), generator=g, dtype=torch.uint8)
    z = torch.zeros(B, K, 4, 4)
    return OpenLoopResult(latents=z, hiddens=torch.zeros(B, K, 8), mu=mu, frames_pred=fp, frames_true=ft,
                          sqerr=torch.rand(B, K, generator=g), reward_pred=torch.zeros(B, H, 1),
                          reward_true=torch.zeros(B, H, 1), continue_pred=torch.zeros(B, H, 1),
                          continue_true=torch.zeros(B, H, 1), context=3, horizon=H)


def test_result_mse_psnr_video():
    B, H, h, w = 2, 2, 2, 3
    r = _result(B, H, h, w)
    assert torch.equal(r.mse(), r.sqerr / (3 * h * w))
    ps = r.psnr()
    assert ps.shape == (B, H + 1)
    for b in range(B):
        for k in range(H + 1):
            d = r.frames_pred[b, k].double() - r.frames_true[b, k].double()
            assert math.isclose(ps[b, k].item(), 10 * math.log10(255.0 ** 2 / d.pow(2).mean().item()), rel_tol=1e-5)
    v = r.video()
    assert v.dtype == torch.uint8 and v.shape == (H + 1, 3, 2 * h, B * w)
    for b in range(B):
        for k in range(H + 1):
            assert torch.equal(v[k][:, :h, b * w:(b + 1) * w], r.frames_true[b][k])
            assert torch.equal(v[k][:, h:, b * w:(b + 1) * w], r.frames_pred[b][k])
    # identical frames: infinite PSNR, not NaN
    r.frames_pred = r.frames_true.clone()
    assert bool(torch.isinf(r.psnr()).all())


def test_result_vector_observations():
    r = _result(vector=True)
    assert r.frames_pred is None and r.frames_true is None
    assert torch.equal(r.mse(), r.sqerr / 5)
    with pytest.raises(ValueError):
        r.video()
    with pytest.raises(ValueError):
        r.psnr()


def test_target_slots_match_brute_force():
    """State k <-> reward / continue slot start + Tc + k - 2, frame slot start +
    Tc - 1 + k (modulo the ring), for every (Tc, H) a window of S = 8 allows."""
    from dreamer_amd.open_loop import frame_step, target_slots, target_step
    cap, S = 13, 8
    starts = [0, 5, 12, 9]
    for Tc in range(1, S):
        for H in range(1, S - Tc + 1):
            fs, ts = target_slots(starts, Tc, H, cap)
            assert fs.shape == (len(starts), H + 1) and ts.shape == (len(starts), H)
            for b, s0 in enumerate(starts):
                for k in range(H + 1):
                    assert frame_step(Tc, k) == Tc - 1 + k
                    assert fs[b, k].item() == (s0 + Tc - 1 + k) % cap
                    if k >= 1:
                        assert target_step(Tc, k) == Tc + k - 2
                        assert ts[b, k - 1].item() == (s0 + Tc + k - 2) % cap
                        # unroll_model's alignment: the target sits one step before the state's frame
                        assert target_step(Tc, k) == frame_step(Tc, k) - 1
            assert frame_step(Tc, H) <= S - 1
    with pytest.raises(ValueError):
        target_step(4, 0)


def test_check_lengths():
    from dreamer_amd.open_loop import check_lengths
    check_lengths(1, 1, 2)
    check_lengths(4, 4, 8)
    for Tc, H in ((0, 3), (4, 0), (4, 5), (-1, 2)):
        with pytest.raises(ValueError):
            check_lengths(Tc, H, 8)


def test_open_loop_argument_errors_need_no_gpu():
    """Bad lengths raise before the device is touched; the C entry points refuse
    null pointers with DR_E_INVALID and answer the workspace query on the host."""
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    d = Dreamer(dict(SMALL), torch.device("cpu"))
    S = d.sequence_length
    for Tc, H in ((0, 3), (4, 0), (4, S + 1 - 4)):
        with pytest.raises(ValueError):
            d.open_loop(starts=np.array([0]), context=Tc, horizon=H)
    dims = d.world_model.dims()
    assert L.query("dr_imagine_actions_workspace_bytes", dims, 4, 4) > 4 * 5 * d.hidden_state_dims * 4
    assert L.query("dr_imagine_actions_workspace_bytes", dims, 4, 4) < L.query("dr_imagine_workspace_bytes", dims, 4, 4)
    with pytest.raises(L.HipError) as e:
        L.call("dr_imagine_actions", dims, L.dr_world_model(), 1, 1, None, None,
               None, 0, 0, L.dr_noise(), None, None, None, None, None, 0, None)
    assert e.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as e:
        L.call("dr_frame_metrics", dims, 1, 1, None, None, None, None, None, None)
    assert e.value.code == L.DR_E_INVALID
