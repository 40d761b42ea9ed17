"""Closed-loop (posterior) trace on replay windows: the result container of
``Dreamer.closed_loop`` and the window arithmetic it shares with the tests.

A window b is S = sequence_length consecutive ring slots from starts[b].  The
filter is warm_start_generator's (Dreamer.py:244-262): h_0 = 0, z_0 ~
posterior(h_0, x_0); for t >= 1 h_t = GRU(z_{t-1}, a_{t-1}, h_{t-1}) and z_t ~
posterior(h_t, x_t).  State t is kept for every t < T.  Its decoded frame (from
the posterior sample, and from a sample of the prior of h_t: the one-step
prediction) is compared with the true frame at window step t; its reward /
continue heads (t >= 1) with the values stored at window step t - 1 --
unroll_model's alignment (WorldModel.py:113-123)."""
from dataclasses import dataclass
from typing import Optional

import torch


def frame_step(t):
    """Window step of the true frame state t is compared with."""
    if t < 0:
        raise ValueError("state index must be >= 0")
    return t


def target_step(t):
    """Window step of the stored reward / continue state t >= 1 is compared with."""
    if t < 1:
        raise ValueError("state 0 follows no action: it has no reward / continue target")
    return t - 1


def target_slots(starts, length, capacity):
    """(frame slots [B][T], reward / continue slots [B][T-1]) in the ring, as int64 tensors."""
    st = torch.as_tensor(starts, dtype=torch.int64).reshape(-1, 1)
    kf = torch.arange(0, length, dtype=torch.int64).reshape(1, -1)
    kt = torch.arange(1, length, dtype=torch.int64).reshape(1, -1)
    return (st + kf) % capacity, (st + kt - 1) % capacity


def check_length(length, sequence_length):
    if length < 1 or length > sequence_length:
        raise ValueError(f"closed loop needs 1 <= length <= sequence_length (got {length} vs {sequence_length})")


@dataclass
class ClosedLoopResult:
    """Device tensors of one posterior trace over B windows of T = length steps.

    latents (B,T,R,C), hiddens (B,T,hidden): the filtered states.
    post_logits / prior_logits (B,T,R,C): the encoder's raw logits and
    dynamics_predictor.logit_net(h_t) (t = 0: the prior of the zero state).
    kl, post_entropy, prior_entropy (B,T): sum over the R groups of KL(posterior
    || prior) and of the two entropies, on the raw logits (no unimix, no free
    bits, no mask).
    mu_post: Decoder(h_t, z_t), (B,T,3,h,w) or (B,T,D) for vector observations.
    latents_prior (B,T,R,C): a sample of the prior of h_t; mu_prior its decode:
    what the model expected before frame t arrived.  None with predict=False, as
    are sqerr_prior and frames_prior.
    sqerr_post / sqerr_prior (B,T): sum over the frame of (mu - true)^2
    (WorldModel.py:129).
    frames_post / frames_prior / frames_true: u8 (B,T,3,h,w); None for vector
    observations.
    reward_pred / reward_true (B,T-1,1): both in symlog space.  continue_pred /
    continue_true (B,T-1,1): the head's probability and the stored flag.  Entry
    t-1 of the head fields belongs to state t."""
    latents: torch.Tensor
    hiddens: torch.Tensor
    post_logits: torch.Tensor
    prior_logits: torch.Tensor
    kl: torch.Tensor
    post_entropy: torch.Tensor
    prior_entropy: torch.Tensor
    mu_post: torch.Tensor
    mu_prior: Optional[torch.Tensor]
    latents_prior: Optional[torch.Tensor]
    sqerr_post: torch.Tensor
    sqerr_prior: Optional[torch.Tensor]
    frames_post: Optional[torch.Tensor]
    frames_prior: Optional[torch.Tensor]
    frames_true: Optional[torch.Tensor]
    reward_pred: torch.Tensor
    reward_true: torch.Tensor
    continue_pred: torch.Tensor
    continue_true: torch.Tensor
    length: int

    def frame_elems(self):
        n = 1
        for s in self.mu_post.shape[2:]:
            n *= int(s)
        return n

    def _need_prior(self, what):
        if self.sqerr_prior is None:
            raise ValueError(f"{what} needs the one-step prediction (closed_loop(predict=True))")

    def mse_post(self):
        """Mean squared reconstruction error per frame (B,T), on the model's [-0.5, 0.5] scale."""
        return self.sqerr_post / float(self.frame_elems())

    def mse_prior(self):
        """Mean squared one-step prediction error per frame (B,T)."""
        self._need_prior("mse_prior()")
        return self.sqerr_prior / float(self.frame_elems())

    def _need_frames(self, what):
        if self.frames_post is None or self.frames_true is None:
            raise ValueError(f"{what} needs pixel observations (vector observations have no u8 frames)")

    def _psnr(self, frames):
        d = frames.float() - self.frames_true.float()
        m = d.pow(2).flatten(2).mean(-1)
        return 10.0 * torch.log10(255.0 ** 2 / m)

    def psnr_post(self):
        """PSNR of the reconstruction per frame (B,T) in dB on the u8 scale: 10 log10(255^2 / mean((pred - true)^2))."""
        self._need_frames("psnr_post()")
        return self._psnr(self.frames_post)

    def psnr_prior(self):
        """PSNR of the one-step prediction per frame (B,T), as psnr_post."""
        self._need_frames("psnr_prior()")
        self._need_prior("psnr_prior()")
        return self._psnr(self.frames_prior)

    def ssim_post(self):
        """SSIM of the reconstruction per frame (B,T) (dr_frame_ssim), computed
        on demand on the current stream."""
        self._need_frames("ssim_post()")
        from .futures import frame_ssim
        return frame_ssim(self.mu_post, self.frames_true)

    def ssim_prior(self):
        """SSIM of the one-step prediction per frame (B,T), as ssim_post."""
        self._need_frames("ssim_prior()")
        self._need_prior("ssim_prior()")
        from .futures import frame_ssim
        return frame_ssim(self.mu_prior, self.frames_true)

    def ssim(self):
        """(ssim_post(), ssim_prior()); the second is None without the one-step prediction."""
        return self.ssim_post(), (self.ssim_prior() if self.sqerr_prior is not None else None)

    def video(self):
        """u8 [T][3][3h][B*w]: per step, the true frames above the posterior
        reconstructions above the one-step predictions, the B windows side by side."""
        self._need_frames("video()")
        self._need_prior("video()")
        row = lambda f: torch.cat(list(f.transpose(0, 1).unbind(1)), dim=-1)  # (B,T,3,h,w) -> (T,3,h,B*w)
        return torch.cat((row(self.frames_true), row(self.frames_post), row(self.frames_prior)), dim=-2).contiguous()
