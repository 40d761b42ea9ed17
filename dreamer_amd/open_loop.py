"""Open-loop world-model prediction on replay windows: ``Dreamer.open_loop``
and ``evaluate_world_model``, their result container and the window arithmetic
they share with the tests (the front end is replay_eval.py's).

A window b is S = sequence_length consecutive ring slots from starts[b].
Rollout state 0 is the posterior after the context frames 0 .. Tc-1
(warm_start_generator's convention, Dreamer.py:244-262); state k = 1 .. H is
the prior rolled forward under the recorded actions (imagine_step with a given
action, WorldModel.py:72-77).  State k's decoded frame is compared with the
true frame at window step Tc-1+k; its reward / continue heads (k >= 1) with the
values stored at window step Tc+k-2 -- unroll_model's alignment, the state at
frame t+1 against rew[t] (WorldModel.py:113-123)."""
from dataclasses import dataclass
from typing import Optional

import torch

from .replay_eval import (FrameResult, average_curves, check_window, context_filter, decode_and_score, head_errors,
                          psnr_u8, resolve_noise, ring_slots, video_rows, window_prologue)
from .utils import symlog


def frame_step(context, k):
    """Window step of the true frame state k is compared with."""
    return context - 1 + k


def target_step(context, k):
    """Window step of the stored reward / continue state k >= 1 is compared with."""
    if k < 1:
        raise ValueError("state 0 is a posterior: it has no reward / continue target")
    return context + k - 2


def target_slots(starts, context, horizon, capacity):
    """(frame slots [B][H+1], reward / continue slots [B][H]) in the ring, as int64 tensors."""
    return ring_slots(starts, context - 1, horizon + 1, capacity), ring_slots(starts, context - 1, horizon, capacity)


def check_lengths(context, horizon, sequence_length):
    check_window(context >= 1 and horizon >= 1 and context + horizon <= sequence_length,
                 "open loop needs context >= 1, horizon >= 1 and context + horizon <= sequence_length",
                 f"{context} + {horizon}", sequence_length)


def window_lengths(dr, context, horizon):
    """(Tc, H) with open_loop's defaults -- context S // 2 (the warm start's),
    horizon min(dr.horizon, S - Tc) -- checked against S."""
    S = dr.sequence_length
    Tc = S // 2 if context is None else int(context)
    H = min(dr.horizon, S - Tc) if horizon is None else int(horizon)
    check_lengths(Tc, H, S)
    return Tc, H


@dataclass
class OpenLoopResult(FrameResult):
    """Device tensors of one open-loop prediction over B windows.

    latents (B,H+1,R,C), hiddens (B,H+1,hidden): rollout states 0..H.
    mu: decoded frames (B,H+1,3,h,w), or (B,H+1,D) for vector observations.
    frames_pred / frames_true: u8 (B,H+1,3,h,w); None for vector observations.
    sqerr (B,H+1): sum over the frame of (mu - true)^2 (WorldModel.py:129).
    reward_pred / reward_true (B,H,1): both in symlog space (the symlog of the
    head's value; the stored symlog reward).  continue_pred / continue_true
    (B,H,1): the head's probability and the stored flag.  Entry k-1 of the head
    fields belongs to state k."""
    latents: torch.Tensor
    hiddens: torch.Tensor
    mu: torch.Tensor
    frames_pred: Optional[torch.Tensor]
    frames_true: Optional[torch.Tensor]
    sqerr: torch.Tensor
    reward_pred: torch.Tensor
    reward_true: torch.Tensor
    continue_pred: torch.Tensor
    continue_true: torch.Tensor
    context: int
    horizon: int

    def mse(self):
        """Mean squared error per frame (B,H+1), on the model's [-0.5, 0.5] scale."""
        return self.sqerr / float(self.frame_elems())

    def psnr(self):
        """PSNR per frame (B,H+1) in dB on the u8 scale: 10 log10(255^2 / mean((pred - true)^2))."""
        self._need_frames("psnr()")
        return psnr_u8(self.frames_pred, self.frames_true)

    def ssim(self):
        """SSIM per frame (B,H+1) of mu against the true frames (dr_frame_ssim:
        11-tap Gaussian window, sigma 1.5, data range 1), computed on demand on
        the current stream."""
        self._need_frames("ssim()")
        from .futures import frame_ssim
        return frame_ssim(self.mu, self.frames_true)

    def video(self):
        """u8 [H+1][3][2h][B*w]: per step, the true frames above the predicted
        ones, the B windows side by side."""
        self._need_frames("video()")
        return video_rows(self.frames_true, self.frames_pred)


def open_loop(dr, starts=None, batch_size=None, context=None, horizon=None, sample=True, noise=None, _mark=None):
    """Dreamer.open_loop (see its docstring)."""
    mark = _mark or (lambda name: None)
    Tc, H = window_lengths(dr, context, horizon)
    R, C = dr.latent_state_dims
    A, S = dr.action_dims, dr.sequence_length

    def draws(B, dev):
        shapes = ((Tc, B * R, C), (H, B * R, C))
        return resolve_noise(noise, sample, shapes, f"noise must be ({Tc}, {B * R}, {C}) and ({H}, {B * R}, {C})", dev)

    w = window_prologue(dr, starts, batch_size, Tc, draws, mark)
    q_ctx, q = w.noise
    z0, h0 = context_filter(dr, w, Tc, q_ctx, mark)
    # the prior under the recorded actions: action Tc-1+k drives state k -> k+1
    lat, hid, r, c = dr.world_model._imagine_actions(w.d, w.B, H, z0, h0, w.act.data_ptr() + 4 * (Tc - 1) * A, S * A,
                                                     A, q)
    mark("unroll")
    # decode states 0..H and compare with the ring's frames Tc-1 .. Tc-1+H
    ((mu, sqerr, pred),), true, _ = decode_and_score(dr, w, w.st, (w.B, H + 1), Tc - 1, hid, (lat,), True, mark)
    sl = slice(Tc - 1, Tc - 1 + H)  # state k = 1..H against window step Tc+k-2
    return OpenLoopResult(latents=lat, hiddens=hid, mu=mu, frames_pred=pred, frames_true=true, sqerr=sqerr,
                          reward_pred=symlog(r), reward_true=w.rew[:, sl].unsqueeze(-1).clone(),
                          continue_pred=c, continue_true=w.cont[:, sl].unsqueeze(-1).clone(), context=Tc, horizon=H)


CURVES = ("mse", "psnr", "reward_abs_err", "continue_bce")


def curves_of(r):
    return [r.mse().mean(0), r.psnr().mean(0) if r.frames_pred is not None else None] + head_errors(r)


def evaluate_world_model(dr, batches=1, batch_size=None, context=None, horizon=None, sample=True):
    """Dreamer.evaluate_world_model (see its docstring)."""
    return average_curves("evaluate_world_model", dr, batches, CURVES, lambda: dr.open_loop(
        batch_size=batch_size, context=context, horizon=horizon, sample=sample), curves_of)
