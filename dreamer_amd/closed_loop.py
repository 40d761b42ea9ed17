"""Closed-loop (posterior) trace on replay windows: ``Dreamer.closed_loop`` and
``evaluate_filter``, their result container and the window arithmetic they
share with the tests (the front end is replay_eval.py's).

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

from . import _lib as L
from . import hip
from .replay_eval import (FrameResult, average_curves, check_window, decode_and_score, head_errors, psnr_u8,
                          resolve_noise, ring_slots, video_rows, window_prologue)
from .utils import symlog


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
    return ring_slots(starts, 0, length, capacity), ring_slots(starts, 0, length - 1, capacity)


def check_length(length, sequence_length):
    check_window(1 <= length <= sequence_length, "closed loop needs 1 <= length <= sequence_length", length,
                 sequence_length)


@dataclass
class ClosedLoopResult(FrameResult):
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

    _mu, _u8 = "mu_post", ("frames_post", "frames_true")

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

    def psnr_post(self):
        """PSNR of the reconstruction per frame (B,T) in dB on the u8 scale: 10 log10(255^2 / mean((pred - true)^2))."""
        self._need_frames("psnr_post()")
        return psnr_u8(self.frames_post, self.frames_true)

    def psnr_prior(self):
        """PSNR of the one-step prediction per frame (B,T), as psnr_post."""
        self._need_frames("psnr_prior()")
        self._need_prior("psnr_prior()")
        return psnr_u8(self.frames_prior, self.frames_true)

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
        return video_rows(self.frames_true, self.frames_post, self.frames_prior)


def closed_loop(dr, starts=None, batch_size=None, length=None, sample=True, noise=None, predict=True, _mark=None):
    """Dreamer.closed_loop (see its docstring)."""
    mark = _mark or (lambda name: None)
    S = dr.sequence_length
    T = S if length is None else int(length)
    check_length(T, S)
    R, C = dr.latent_state_dims
    A = dr.action_dims

    def draws(B, dev):
        shape = (T, B * R, C)
        return resolve_noise(noise, sample, (shape, shape), f"noise must be two tensors of shape ({T}, {B * R}, {C})",
                             dev)

    w = window_prologue(dr, starts, batch_size, T, draws, mark)
    B, dev = w.B, w.st.device
    q_post, q_prior = w.noise
    # action t-1 drives frame t; state t's heads are compared with window step t-1
    lat, hid, plog, prlog, r, c = dr.world_model._observe_trace(w.d, B, T, w.feat, w.act.data_ptr(), S * A, A, None,
                                                                None, q_post)
    mark("trace")
    M = B * T
    kl, hq, hp = (torch.empty(B, T, device=dev) for _ in range(3))
    L.call("dr_latent_stats", M, R, C, L.ptr(plog), L.ptr(prlog), L.ptr(kl), L.ptr(hq), L.ptr(hp), None, w.stream)
    mark("stats")
    zp = None
    if predict:
        # the prior's own draw t for row (b, t): explicit draws are given time-major, the rows are [B][T]
        zp = torch.empty(B, T, R, C, device=dev)
        if q_prior is not None:
            qp = q_prior.view(T, B, R, C).transpose(0, 1).contiguous()
            nz = hip.explicit_noise(q=qp, device=dev)
        else:
            nz = hip.adhoc(dev).noise()
        L.call("dr_categorical_sample", M, R, C, L.ptr(prlog), nz, L.ptr(zp), None, None, w.stream)
        mark("prior_sample")
    ((mu_q, sq_q, fr_q), (mu_p, sq_p, fr_p)), true, _ = decode_and_score(dr, w, w.st, (B, T), 0, hid, (lat, zp), True,
                                                                         mark)
    return ClosedLoopResult(latents=lat, hiddens=hid, post_logits=plog, prior_logits=prlog, kl=kl, post_entropy=hq,
                            prior_entropy=hp, mu_post=mu_q, mu_prior=mu_p, latents_prior=zp, sqerr_post=sq_q,
                            sqerr_prior=sq_p, frames_post=fr_q, frames_prior=fr_p, frames_true=true,
                            reward_pred=symlog(r[:, 1:]), reward_true=w.rew[:, :T - 1].unsqueeze(-1).clone(),
                            continue_pred=c[:, 1:].clone(), continue_true=w.cont[:, :T - 1].unsqueeze(-1).clone(),
                            length=T)


CURVES = ("kl", "post_entropy", "prior_entropy", "mse_post", "mse_prior", "psnr_post", "psnr_prior", "reward_abs_err",
          "continue_bce")


def curves_of(r):
    px = r.frames_post is not None
    return [r.kl.mean(0), r.post_entropy.mean(0), r.prior_entropy.mean(0), r.mse_post().mean(0),
            r.mse_prior().mean(0), r.psnr_post().mean(0) if px else None,
            r.psnr_prior().mean(0) if px else None] + head_errors(r)


def evaluate_filter(dr, batches=1, batch_size=None, length=None, sample=True):
    """Dreamer.evaluate_filter (see its docstring)."""
    return average_curves("evaluate_filter", dr, batches, CURVES, lambda: dr.closed_loop(
        batch_size=batch_size, length=length, sample=sample), curves_of)
