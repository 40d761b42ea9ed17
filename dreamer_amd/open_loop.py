"""Open-loop world-model prediction on replay windows: the result container
of ``Dreamer.open_loop`` and the window arithmetic it shares with the tests.

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
    st = torch.as_tensor(starts, dtype=torch.int64).reshape(-1, 1)
    kf = torch.arange(0, horizon + 1, dtype=torch.int64).reshape(1, -1)
    kt = torch.arange(1, horizon + 1, dtype=torch.int64).reshape(1, -1)
    return (st + (context - 1) + kf) % capacity, (st + context + kt - 2) % capacity


def check_lengths(context, horizon, sequence_length):
    if context < 1 or horizon < 1 or context + horizon > sequence_length:
        raise ValueError(f"open loop needs context >= 1, horizon >= 1 and context + horizon <= sequence_length "
                         f"(got {context} + {horizon} vs {sequence_length})")


@dataclass
class OpenLoopResult:
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

    def frame_elems(self):
        n = 1
        for s in self.mu.shape[2:]:
            n *= int(s)
        return n

    def mse(self):
        """Mean squared error per frame (B,H+1), on the model's [-0.5, 0.5] scale."""
        return self.sqerr / float(self.frame_elems())

    def _need_frames(self, what):
        if self.frames_pred is None or self.frames_true is None:
            raise ValueError(f"{what} needs pixel observations (vector observations have no u8 frames)")

    def psnr(self):
        """PSNR per frame (B,H+1) in dB on the u8 scale: 10 log10(255^2 / mean((pred - true)^2))."""
        self._need_frames("psnr()")
        d = self.frames_pred.float() - self.frames_true.float()
        m = d.pow(2).flatten(2).mean(-1)
        return 10.0 * torch.log10(255.0 ** 2 / m)

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
        row = lambda f: torch.cat(list(f.transpose(0, 1).unbind(1)), dim=-1)  # (B,K,3,h,w) -> (K,3,h,B*w)
        return torch.cat((row(self.frames_true), row(self.frames_pred)), dim=-2).contiguous()
