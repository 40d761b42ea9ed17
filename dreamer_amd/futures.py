"""Sampled futures on replay windows: M rollouts of the stochastic prior per
window (Dreamer.sample_futures, evaluate_futures), their result container, and
SSIM for the open-loop / closed-loop results (include/dreamer_hip.h "sampled
futures" has the definitions the kernels fix).

The windows, the context filter and the alignment of states with frames and
reward / continue targets are open_loop.py's.  The B posteriors after the
context are replicated M times (rollout row b*M + m is sample m of window b),
rolled forward under the recorded actions in one dr_imagine_actions call --
the categorical draws are keyed by row, so the replicas differ -- and decoded
in one dr_decoder_fwd.  dr_frame_metrics (on the B*M rows, starts repeated) and
dr_frame_ssim give the per-sample errors, dr_ensemble_metrics the error of the
mean frame and the spread; by the variance decomposition
mean_m sqerr_m = sqerr_mean + spread (up to rounding)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import hip
from .open_loop import target_slots, window_lengths
from .replay_eval import (FrameResult, average_curves, context_filter, decode_and_score, psnr_u8, resolve_noise,
                          video_rows, window_prologue)
from .utils import symlog

WHICH = ("mean", "best", "best_sample", "ensemble")


def check_futures(B, M):
    """Raise ValueError unless B windows of M samples can be run: M an integer
    in 1 .. DR_ENSEMBLE_MAX_SAMPLES, B >= 1, B * M <= plan.PLAN_MAX_ROWS (the
    row count dr_imagine_actions has been run at)."""
    from .plan import PLAN_MAX_ROWS
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)):
        raise ValueError(f"futures: samples must be an integer (got {M!r})")
    if not 1 <= M <= L.DR_ENSEMBLE_MAX_SAMPLES:
        raise ValueError(f"futures: samples must be in 1 .. {L.DR_ENSEMBLE_MAX_SAMPLES} (got {M})")
    if B < 1:
        raise ValueError(f"futures: need at least one window (got {B})")
    if B * M > PLAN_MAX_ROWS:
        raise ValueError(f"futures: {B} windows x {M} samples is above {PLAN_MAX_ROWS} rollout rows")


def best_index(score):
    """Per row of score (B, M) the lowest index holding the row's minimum: the
    candidates are the positions equal to the minimum, the answer the smallest
    of them (no reliance on argmin's choice among ties).  A row without a
    minimum (all NaN) gives 0."""
    M = score.shape[1]
    mn = score.min(dim=1, keepdim=True).values
    idx = torch.arange(M, device=score.device).expand_as(score)
    cand = torch.where(score == mn, idx, torch.full_like(idx, M))
    best = cand.min(dim=1).values
    return torch.where(best == M, torch.zeros_like(best), best)


def frame_ssim(mu, frames_u8):
    """dr_frame_ssim of mu (B,T,3,h,w) f32 against u8 frames (B,T,3,h,w): (B,T)
    on the current stream.  The u8 frames are read as a ring of B*T slots with
    starts b*T, so they go through the kernel's u8 path as the replay ring does."""
    L.require_gpu(mu)
    if mu.dim() != 5 or frames_u8 is None or tuple(frames_u8.shape) != tuple(mu.shape):
        raise ValueError("ssim needs pixel observations: mu (B,T,3,h,w) and u8 frames of the same shape")
    B, T = mu.shape[:2]
    d = L.dr_dims()
    d.img_h, d.img_w = int(mu.shape[3]), int(mu.shape[4])
    mu_c = mu.float().contiguous()
    fr = frames_u8.contiguous()
    starts = torch.arange(B, device=mu.device, dtype=torch.int64) * T
    out = torch.empty(B, T, device=mu.device)
    truth = L.dr_frames(L.ptr(fr), B * T, L.ptr(starts), None, 0, 0, 1, 0)
    L.call("dr_frame_ssim", d, B, T, L.ptr(mu_c), truth, L.ptr(out), None, hip.stream())
    return out


@dataclass
class FuturesResult(FrameResult):
    """Device tensors of M sampled futures over B windows.

    Per sample: latents (B,M,H+1,R,C), hiddens (B,M,H+1,hidden), mu
    (B,M,H+1,3,h,w) or (B,M,H+1,D), frames_pred u8 like mu (None for vector
    observations), sqerr (B,M,H+1), ssim (B,M,H+1) (None for vector observations
    or ssim=False), reward_pred / continue_pred (B,M,H,1) (symlog space / the
    head's probability).  State 0 is the posterior after the context: the same
    for the M samples of a window.
    Ensemble: mu_mean (B,H+1,...) the mean frame, sqerr_mean (B,H+1) its squared
    error, spread (B,H+1) the population variance over the samples summed over
    the frame, ssim_ensemble (B,H+1) the mean frame's SSIM, frames_mean /
    frames_std u8 (B,H+1,3,h,w) the mean frame and min(255, rint(255 std)).
    Truth: frames_true u8 (B,H+1,3,h,w) (None for vector observations), x_true
    (B,H+1,D) for vector observations only, reward_true / continue_true
    (B,H,1) as open_loop returns them."""
    latents: torch.Tensor
    hiddens: torch.Tensor
    mu: torch.Tensor
    frames_pred: Optional[torch.Tensor]
    sqerr: torch.Tensor
    ssim: Optional[torch.Tensor]
    reward_pred: torch.Tensor
    continue_pred: torch.Tensor
    mu_mean: torch.Tensor
    sqerr_mean: torch.Tensor
    spread: torch.Tensor
    ssim_ensemble: Optional[torch.Tensor]
    frames_mean: Optional[torch.Tensor]
    frames_std: Optional[torch.Tensor]
    frames_true: Optional[torch.Tensor]
    x_true: Optional[torch.Tensor]
    reward_true: torch.Tensor
    continue_true: torch.Tensor
    context: int
    horizon: int

    @property
    def samples(self):
        return int(self.sqerr.shape[1])

    _lead, _u8 = 3, ("frames_true",)

    def best(self):
        """Per window the sample with the smallest sum over states 1..H of
        sqerr (state 0 is shared), ties to the lower index: (B,) int64."""
        return best_index(self.sqerr[:, :, 1:].sum(-1))

    def _pick(self, per_sample, which, largest):
        """(B,M,K) per-sample curves -> (B,K): the mean over the samples, the
        per-step best-of-M (min, or max for a similarity), or best()'s sample."""
        if which == "mean":
            return per_sample.mean(1)
        if which == "best":
            return per_sample.max(1).values if largest else per_sample.min(1).values
        if which == "best_sample":
            i = self.best().view(-1, 1, 1).expand(-1, 1, per_sample.shape[2])
            return per_sample.gather(1, i).squeeze(1)
        raise ValueError(f"which must be one of {WHICH} (got {which!r})")

    def mse(self, which="mean"):
        """Mean squared error per frame (B,H+1) on the model's [-0.5, 0.5] scale:
        "mean" over the samples, "best" the smallest of the M at each step (never
        above "mean"), "best_sample" the curve of best()'s sample, "ensemble" the
        error of the mean frame (mean = ensemble + spread / n)."""
        n = float(self.frame_elems())
        if which == "ensemble":
            return self.sqerr_mean / n
        return self._pick(self.sqerr, which, False) / n

    def psnr(self, which="mean"):
        """PSNR per frame (B,H+1) in dB on the u8 scale, as OpenLoopResult.psnr;
        the variants as mse ("best": the largest of the M at each step)."""
        self._need_frames("psnr()")
        if which == "ensemble":
            return psnr_u8(self.frames_mean, self.frames_true)
        return self._pick(psnr_u8(self.frames_pred, self.frames_true.unsqueeze(1)), which, True)

    def ssim_curve(self, which="mean"):
        """SSIM per frame (B,H+1) (dr_frame_ssim); the variants as psnr,
        "ensemble" the mean frame's SSIM."""
        self._need_frames("ssim_curve()")
        if self.ssim is None:
            raise ValueError("ssim_curve() needs sample_futures(ssim=True)")
        if which == "ensemble":
            return self.ssim_ensemble
        return self._pick(self.ssim, which, True)

    def truth(self):
        """The true frames (B,H+1,...) on the model's scale, or the stored rows
        for vector observations.  The 256 values (float)u8 / 255.0f - 0.5f come
        from a host table in IEEE f32, the kernels' bits (a device division by
        a scalar may multiply by the reciprocal instead)."""
        if self.frames_true is None:
            return self.x_true
        lut = np.arange(256, dtype=np.float32) / np.float32(255.0) - np.float32(0.5)
        return torch.from_numpy(lut).to(self.frames_true.device)[self.frames_true.long()]

    def coverage(self):
        """Per step (H+1,) the share of true pixels inside the samples'
        [min, max] envelope (over the B windows and the frame).  One torch
        reduction over mu per call."""
        x = self.truth()
        inside = (self.mu.min(1).values <= x) & (x <= self.mu.max(1).values)
        return inside.flatten(2).float().mean((0, 2))

    def reward_spread(self):
        """Std over the samples (population) of the symlog reward prediction, (B,H)."""
        return self.reward_pred.squeeze(-1).std(dim=1, unbiased=False)

    def video(self):
        """u8 [H+1][3][4h][B*w]: per step the true frames above best()'s sample
        above the ensemble mean above the std map, the B windows side by side."""
        self._need_frames("video()")
        i = self.best().view(-1, 1, 1, 1, 1, 1).expand(-1, 1, *self.frames_pred.shape[2:])
        best = self.frames_pred.gather(1, i).squeeze(1)
        return video_rows(self.frames_true, best, self.frames_mean, self.frames_std)


def sample_futures(dr, starts=None, batch_size=None, context=None, horizon=None, samples=8, noise=None, ssim=True,
                   _mark=None, _metrics=None):
    """Dreamer.sample_futures (see there).  _metrics: tools/futures_timing.py's
    replacement of the SSIM / ensemble stage (called with the stage's inputs)."""
    mark = _mark or (lambda name: None)
    Tc, H = window_lengths(dr, context, horizon)
    buf = dr.buffer
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims

    def draws(B, dev):
        BM = B * int(samples)
        return resolve_noise(noise, True, ((Tc, B * R, C), (H, BM * R, C)),
                             f"noise must be ({Tc}, {B * R}, {C}) and ({H}, {BM * R}, {C})", dev)

    w = window_prologue(dr, starts, batch_size, Tc, draws, mark, check=lambda B: check_futures(B, samples))
    st, B, M, d, stream = w.st, w.B, int(samples), w.d, w.stream
    dev = st.device
    q_ctx, q = w.noise
    # the posterior after the context frames, once per window
    z0, h0 = context_filter(dr, w, Tc, q_ctx, mark)
    # rows b*M + m: the states and the recorded actions Tc-1 .. Tc-2+H, M times each
    BM = B * M
    zr, hr = z0.repeat_interleave(M, dim=0), h0.repeat_interleave(M, dim=0)
    ar = w.act[:, Tc - 1:Tc - 1 + H].repeat_interleave(M, dim=0).contiguous()
    st_rep = st.repeat_interleave(M)
    mark("replicate")
    lat, hid, r, c = dr.world_model._imagine_actions(d, BM, H, zr, hr, ar.data_ptr(), H * A, A, q)
    mark("unroll")
    K = H + 1
    vector = buf.vector
    ((mu, sqerr, pred),), _, truth_rep = decode_and_score(dr, w, st_rep, (B, M, K), Tc - 1, hid, (lat,), False, mark)
    shape = tuple(mu.shape[3:])
    truth = buf.frames_struct(st)
    truth.t0 = Tc - 1
    mu_mean = torch.empty(B, K, *shape, device=dev)
    sq_mean, spread = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
    f_mean = f_std = ss = ss_ens = None
    do_ssim = bool(ssim) and not vector
    if _metrics is not None:
        f_mean, f_std, ss, ss_ens = _metrics(mu, truth_rep, truth, mu_mean, sq_mean, spread, do_ssim)
    else:
        if do_ssim:
            ss = torch.empty(B, M, K, device=dev)
            L.call("dr_frame_ssim", d, BM, K, L.ptr(mu), truth_rep, L.ptr(ss), None, stream)
            mark("ssim")
        if not vector:
            f_mean = torch.empty(B, K, *shape, dtype=torch.uint8, device=dev)
            f_std = torch.empty_like(f_mean)
        L.call("dr_ensemble_metrics", d, B, M, K, L.ptr(mu), truth, L.ptr(sq_mean), L.ptr(spread), L.ptr(f_mean),
               L.ptr(f_std), L.ptr(mu_mean), stream)
        if do_ssim:
            ss_ens = torch.empty(B, K, device=dev)
            L.call("dr_frame_ssim", d, B, K, L.ptr(mu_mean), truth, L.ptr(ss_ens), None, stream)
        mark("ensemble")
    frames = buf._mirror()["frames"][target_slots(st, Tc, H, buf.capacity)[0]]  # the true frames, on the device
    f_true, x_true = (None, frames) if vector else (frames, None)
    sl = slice(Tc - 1, Tc - 1 + H)  # state k = 1..H against window step Tc+k-2
    return FuturesResult(latents=lat.view(B, M, K, R, C), hiddens=hid.view(B, M, K, Hd), mu=mu, frames_pred=pred,
                         sqerr=sqerr, ssim=ss, reward_pred=symlog(r).view(B, M, H, 1),
                         continue_pred=c.view(B, M, H, 1), mu_mean=mu_mean, sqerr_mean=sq_mean, spread=spread,
                         ssim_ensemble=ss_ens, frames_mean=f_mean, frames_std=f_std, frames_true=f_true,
                         x_true=x_true, reward_true=w.rew[:, sl].unsqueeze(-1).clone(),
                         continue_true=w.cont[:, sl].unsqueeze(-1).clone(), context=Tc, horizon=H)


CURVES = ("mse_mean", "mse_best", "mse_ensemble", "spread", "psnr_mean", "psnr_best", "ssim_mean", "ssim_best",
          "coverage", "reward_spread")


def curves_of(r):
    """The per-step curves of one FuturesResult, averaged over its windows, in
    CURVES' order (device tensors; the pixel-only ones None for vector
    observations)."""
    px = r.frames_true is not None
    n = float(r.frame_elems())
    return [r.mse("mean").mean(0), r.mse("best").mean(0), r.mse("ensemble").mean(0), (r.spread / n).mean(0),
            r.psnr("mean").mean(0) if px else None, r.psnr("best").mean(0) if px else None,
            r.ssim_curve("mean").mean(0) if px else None, r.ssim_curve("best").mean(0) if px else None,
            r.coverage(), r.reward_spread().mean(0)]


def evaluate_futures(dr, batches=1, batch_size=None, context=None, horizon=None, samples=8):
    """Dreamer.evaluate_futures (see there)."""
    return average_curves("evaluate_futures", dr, batches, CURVES, lambda: dr.sample_futures(
        batch_size=batch_size, context=context, horizon=horizon, samples=samples), curves_of)
