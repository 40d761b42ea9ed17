"""Dream trace on replay windows: M imagined rollouts under the current actor
per window (``Dreamer.dream_trace``, ``evaluate_dreams``) and their result
container (include/dreamer_hip.h "dream trace" has the definitions the kernel
fixes).

This is what train_Agent learns from (Dreamer.py:143-175, Agent.py:96-135),
kept instead of reduced to two losses.  The windows and the context filter are
open_loop.py's: state 0 of every dream of window b is the posterior after the
window's first `context` frames.  The B posteriors are replicated M times
(rollout row n = b*M + m is dream m of window b) and rolled forward H steps in
one dr_imagine_fwd -- Philox is keyed by row, so the replicas differ --; one
dr_critic_fwd each for the online and the target critic values the N*(H+1)
states; dr_dream_stats turns rewards, continues, values and the actor's
distributions into the lambda-returns, advantages, discount weights,
log-probabilities and saturation counts of every dream and their spread over a
window's dreams, in one launch; one dr_decoder_fwd decodes all states.  The
agent's return normaliser max(S, 1) (Agent.py:78-88) is read, not updated."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import hip
from .replay_eval import FrameResult, average_curves, check_window, context_filter, video_rows, window_prologue

# the largest row count an epoch test runs dr_imagine_fwd at
DREAM_MAX_ROWS = 4096

PER_DREAM = ("R_lambda", "R_mc", "adv", "adv_norm", "weight", "logp", "base_entropy", "saturated")
PER_WINDOW = ("reward_mean", "reward_std", "ret_mean", "ret_std", "logp_mean", "logp_std", "alive", "action_spread",
              "best", "worst", "n_finite")
_INT = ("saturated", "best", "worst", "n_finite")


def _integer(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_dreams(B, M):
    """Raise ValueError unless B windows of M dreams can be run: M an integer in
    1 .. DR_DREAM_STATS_MAX_DREAMS, B >= 1, B * M <= DREAM_MAX_ROWS."""
    if not _integer(M):
        raise ValueError(f"dream trace: samples must be an integer (got {M!r})")
    if not 1 <= M <= L.DR_DREAM_STATS_MAX_DREAMS:
        raise ValueError(f"dream trace: samples must be in 1 .. {L.DR_DREAM_STATS_MAX_DREAMS} (got {M})")
    if B < 1:
        raise ValueError(f"dream trace: need at least one window (got {B})")
    if B * M > DREAM_MAX_ROWS:
        raise ValueError(f"dream trace: {B} windows x {M} dreams is above {DREAM_MAX_ROWS} rollout rows")


def dream_lengths(dr, context, horizon):
    """(Tc, H): context defaults to S // 2 (the warm start's), horizon to
    dr.horizon; 1 <= Tc <= S and H >= 1 -- a dream needs no ring frames, so H is
    not bounded by the window."""
    S = dr.sequence_length
    Tc = S // 2 if context is None else context
    H = dr.horizon if horizon is None else horizon
    if not _integer(Tc) or not _integer(H):
        raise ValueError(f"dream trace: context and horizon must be integers (got {Tc!r}, {H!r})")
    check_window(1 <= Tc <= S, "dream trace needs 1 <= context <= sequence_length", Tc, S)
    if H < 1:
        raise ValueError(f"dream trace needs horizon >= 1 (got {H})")
    return int(Tc), int(H)


def dream_stats(B, M, H, A, rewards, continues, V_target, V_online, mus, sigmas, actions, gamma, lam, norm=None,
                saturation=0.99, want=PER_DREAM + PER_WINDOW, stream=None):
    """One dr_dream_stats call on contiguous f32 device tensors of N = B*M rows
    (rewards, continues [N][H], values [N][H+1], mus / sigmas / actions
    [N][H][A]; norm a device scalar or None).  Returns {name: tensor} for the
    outputs named in `want`: per dream (B,M,H) -- weight (B,M,H+1) --, per
    window (B,H) -- alive (B,H+1), best / worst / n_finite (B,); saturated and
    those three int32."""
    dev = rewards.device
    shape = dict(weight=(B, M, H + 1), alive=(B, H + 1), best=(B,), worst=(B,), n_finite=(B,))
    out = {}
    for k in want:
        s = shape.get(k, (B, M, H) if k in PER_DREAM else (B, H))
        out[k] = torch.empty(*s, dtype=torch.int32 if k in _INT else torch.float32, device=dev)
    o = L.dr_dream_outputs(**{k: L.ptr(t) for k, t in out.items()})
    L.call("dr_dream_stats", B, M, H, A, L.ptr(rewards), L.ptr(continues), L.ptr(V_target), L.ptr(V_online),
           L.ptr(mus), L.ptr(sigmas), L.ptr(actions), gamma, lam, L.ptr(norm), saturation, o,
           hip.stream() if stream is None else stream)
    return out


def quantise(mu):
    """u8 of decoded frames as dr_frame_metrics quantises them:
    min(255, max(0, rint((x + 0.5) * 255))) in f32, halves to even."""
    return ((mu + 0.5) * 255.0).round().clamp(0.0, 255.0).to(torch.uint8)


CURVES = ("reward", "cont", "alive", "value", "ret_lambda", "advantage", "advantage_norm", "neg_logp", "sigma",
          "saturated_frac", "action_spread", "ret_std")


@dataclass
class DreamResult(FrameResult):
    """Device tensors of M dreams of H steps over B windows.

    The rollout: latents (B,M,H+1,R,C), hiddens (B,M,H+1,hidden) -- state 0 is
    the posterior after the context, the same for a window's M dreams --,
    actions, mus, sigmas (B,M,H,A): the action taken at state t and the actor's
    distribution there; rewards (natural space), continues (B,M,H): entry t
    belongs to state t+1, the transition out of state t (Dreamer.py:158-164).
    value, value_target (B,M,H+1): critic.value / target_critic.value of the
    states.  norm (1,): max(S, 1) as the statistics read it.
    dr_dream_stats' outputs under its names: R_lambda, R_mc, adv, adv_norm,
    logp, base_entropy (B,M,H), weight (B,M,H+1), saturated (B,M,H) int32;
    reward_mean, reward_std, ret_mean, ret_std, logp_mean, logp_std,
    action_spread (B,H), alive (B,H+1), best, worst, n_finite (B,) int32.
    mu: the decoded states (B,M,H+1,3,h,w) or (B,M,H+1,D), frames their u8
    quantisation (pixel models); both None with decode=False, frames None for
    vector observations."""
    latents: torch.Tensor
    hiddens: torch.Tensor
    actions: torch.Tensor
    mus: torch.Tensor
    sigmas: torch.Tensor
    rewards: torch.Tensor
    continues: torch.Tensor
    value: torch.Tensor
    value_target: torch.Tensor
    norm: torch.Tensor
    R_lambda: torch.Tensor
    R_mc: torch.Tensor
    adv: torch.Tensor
    adv_norm: torch.Tensor
    weight: torch.Tensor
    logp: torch.Tensor
    base_entropy: torch.Tensor
    saturated: torch.Tensor
    reward_mean: torch.Tensor
    reward_std: torch.Tensor
    ret_mean: torch.Tensor
    ret_std: torch.Tensor
    logp_mean: torch.Tensor
    logp_std: torch.Tensor
    alive: torch.Tensor
    action_spread: torch.Tensor
    best: torch.Tensor
    worst: torch.Tensor
    n_finite: torch.Tensor
    mu: Optional[torch.Tensor]
    frames: Optional[torch.Tensor]
    context: int
    horizon: int
    saturation: float

    _lead, _u8 = 3, ("frames",)
    # what pick() gathers: the fields with a dream axis
    _per_dream = ("latents", "hiddens", "actions", "mus", "sigmas", "rewards", "continues", "value", "value_target",
                  "R_lambda", "R_mc", "adv", "adv_norm", "weight", "logp", "base_entropy", "saturated", "mu", "frames")

    @property
    def samples(self):
        return int(self.rewards.shape[1])

    def entropy(self):
        """-logp (B,M,H): the one-sample estimate of the policy's entropy the
        actor loss keeps (Agent.py:110-121)."""
        return -self.logp

    def curves(self):
        """{name: per-step mean over the windows and their dreams}, CURVES'
        keys: reward, cont, ret_lambda, advantage, advantage_norm, neg_logp,
        sigma (also over the action dimensions), saturated_frac (the share of
        action dimensions at |a| >= saturation), action_spread, ret_std (H,);
        alive, value (H+1,)."""
        A = float(self.actions.shape[-1])
        return dict(reward=self.rewards.mean((0, 1)), cont=self.continues.mean((0, 1)), alive=self.alive.mean(0),
                    value=self.value.mean((0, 1)), ret_lambda=self.R_lambda.mean((0, 1)),
                    advantage=self.adv.mean((0, 1)), advantage_norm=self.adv_norm.mean((0, 1)),
                    neg_logp=self.entropy().mean((0, 1)), sigma=self.sigmas.mean((0, 1, 3)),
                    saturated_frac=self.saturated.float().mean((0, 1)) / A,
                    action_spread=self.action_spread.mean(0), ret_std=self.ret_std.mean(0))

    def pick(self, which):
        """One dream per window: "best" / "worst" (the kernel's ranking by
        R_mc[.][0]) or an integer m for every window.  Returns {field: (B,...)}
        over the fields with a dream axis (mu / frames only when present)."""
        B, M = self.rewards.shape[:2]
        if isinstance(which, str):
            if which not in ("best", "worst"):
                raise ValueError(f"which must be 'best', 'worst' or a dream index (got {which!r})")
            idx = getattr(self, which).long()
        elif _integer(which) and 0 <= which < M:
            idx = torch.full((B,), int(which), dtype=torch.int64, device=self.rewards.device)
        else:
            raise ValueError(f"which must be 'best', 'worst' or a dream index in 0 .. {M - 1} (got {which!r})")
        rows = torch.arange(B, device=idx.device)
        return {k: getattr(self, k)[rows, idx] for k in self._per_dream if getattr(self, k) is not None}

    def video(self, which=("best", "worst")):
        """u8 [H+1][3][n*h][B*w]: per step the picked dreams one above the
        other in the order of `which`, the B windows side by side.  Frame 0 is
        the decoded posterior of the last context frame."""
        self._need_frames("video()")
        return video_rows(*[self.pick(k)["frames"] for k in which])


def _check_noise(noise, shapes):
    if noise is None:
        return
    want = " , ".join(str(s) for s in shapes)
    try:
        got = tuple(tuple(t.shape) for t in noise)
    except (TypeError, AttributeError):
        got = None
    if got != tuple(shapes):
        raise ValueError(f"noise must be three tensors (q_context, q_dream, eps) of shapes {want}")


def dream_trace(dr, starts=None, batch_size=None, context=None, horizon=None, samples=1, deterministic=False,
                sample=True, noise=None, decode=True, saturation=0.99, _mark=None):
    """Dreamer.dream_trace (see there)."""
    mark = _mark or (lambda name: None)
    Tc, H = dream_lengths(dr, context, horizon)
    check_dreams(1, samples)
    M = int(samples)
    sat = float(saturation)
    buf, ag = dr.buffer, dr.agent
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims

    def check(B):
        check_dreams(B, M)
        _check_noise(noise, ((Tc, B * R, C), (H, B * M * R, C), (H, B * M, A)))

    def draws(B, dev):
        if noise is not None:
            return tuple(t.to(dev).float().contiguous() for t in noise)
        if sample:
            return None, None, None
        return torch.ones(Tc, B * R, C, device=dev), torch.ones(H, B * M * R, C, device=dev), None

    w = window_prologue(dr, starts, batch_size, Tc, draws, mark, check=check)
    B, d, stream = w.B, w.d, w.stream
    dev = w.st.device
    N = B * M
    q_ctx, q, eps = w.noise
    z0, h0 = context_filter(dr, w, Tc, q_ctx, mark)
    zr, hr = z0.repeat_interleave(M, dim=0), h0.repeat_interleave(M, dim=0)
    mark("replicate")
    # one unroll under the current actor, as Dreamer._imagine_raw at any H
    ag._ensure_flat()
    if q is None:
        nz = hip.adhoc(dev).noise()
    else:
        if eps is None and not deterministic:
            # modes for the categoricals, Philox for the actor: its draws written out, so that the
            # unroll reads both kinds from arrays
            eps = torch.empty(H, N, A, device=dev)
            L.call("dr_actor_draws", H, N, A, hip.adhoc(dev).noise(), L.ptr(eps), stream)
        nz = hip.explicit_noise(q=q, eps=eps, device=dev)
    lat, hid = torch.empty(N, H + 1, R, C, device=dev), torch.empty(N, H + 1, Hd, device=dev)
    act, mus, sgs = (torch.empty(N, H, A, device=dev) for _ in range(3))
    rew, cont = torch.empty(N, H, device=dev), torch.empty(N, H, device=dev)
    tape = hip.workspace(dev).get("dream_tape", L.query("dr_imagine_tape_bytes", d, N, H))
    ws = hip.workspace(dev).get("im", L.query("dr_imagine_workspace_bytes", d, N, H))
    L.call("dr_imagine_fwd", d, w.wm, ag.actor_struct(), N, H, L.ptr(zr), L.ptr(hr), nz, int(bool(deterministic)),
           L.ptr(lat), L.ptr(hid), L.ptr(act), L.ptr(rew), L.ptr(cont), L.ptr(mus), L.ptr(sgs), L.ptr(tape), L.ptr(ws),
           ws.numel(), stream)
    mark("dream")
    rows = N * (H + 1)
    V, Vt = torch.empty(N, H + 1, device=dev), torch.empty(N, H + 1, device=dev)
    ws = hip.workspace(dev).get("at_crit", L.query("dr_critic_workspace_bytes", d, N, H))
    L.call("dr_critic_fwd", d, ag.critic_struct(), rows, L.ptr(hid), Hd, L.ptr(lat), R * C, None, L.ptr(V), None,
           L.ptr(ws), ws.numel(), stream)
    L.call("dr_critic_fwd", d, ag.critic_struct(target=True), rows, L.ptr(hid), Hd, L.ptr(lat), R * C, None, L.ptr(Vt),
           None, L.ptr(ws), ws.numel(), stream)
    mark("critics")
    norm = ag.S_dev.detach().clamp(min=1.0).reshape(1)  # max(S, 1), formed on the device: S itself is left alone
    stats = dream_stats(B, M, H, A, rew, cont, Vt, V, mus, sgs, act, ag.gamma, ag.lambda_, norm, sat, stream=stream)
    mark("stats")
    mu = frames = None
    if decode:
        vector = buf.vector
        shape = (d.obs_dim,) if vector else (3, d.img_h, d.img_w)
        mu = torch.empty(B, M, H + 1, *shape, device=dev)
        ws = hip.workspace(dev).get("dec", L.query("dr_decoder_workspace_bytes", d, rows))
        L.call("dr_decoder_fwd", d, dr.world_model.packed_decoder(), rows, L.ptr(hid), Hd, L.ptr(lat), R * C, L.ptr(mu),
               L.ptr(ws), ws.numel(), stream)
        if not vector:
            frames = quantise(mu)
        mark("decoder")
    return DreamResult(latents=lat.view(B, M, H + 1, R, C), hiddens=hid.view(B, M, H + 1, Hd),
                       actions=act.view(B, M, H, A), mus=mus.view(B, M, H, A), sigmas=sgs.view(B, M, H, A),
                       rewards=rew.view(B, M, H), continues=cont.view(B, M, H), value=V.view(B, M, H + 1),
                       value_target=Vt.view(B, M, H + 1), norm=norm, mu=mu, frames=frames, context=Tc, horizon=H,
                       saturation=sat, **stats)


def evaluate_dreams(dr, batches=1, batch_size=None, context=None, horizon=None, samples=8, real=False):
    """Dreamer.evaluate_dreams (see there)."""
    Tc, _ = dream_lengths(dr, context, horizon)
    S = dr.sequence_length
    if real and Tc > S - 1:
        raise ValueError(f"evaluate_dreams(real=True) needs context <= sequence_length - 1 (got {Tc} vs {S}): the "
                         "real return at state context - 1 needs the transition out of it")
    gaps = []

    def call():
        if not real:
            return dr.dream_trace(batch_size=batch_size, context=context, horizon=horizon, samples=samples,
                                  decode=False)
        # the same starts for both, both filters at the posterior's mode: the same states
        starts = dr.buffer.sample_eval_starts(batch_size or dr.batch_size)
        r = dr.dream_trace(starts=starts, context=context, horizon=horizon, samples=samples, sample=False,
                           decode=False)
        tr = dr.agent_trace(starts=starts, length=S, sample=False)
        gaps.append(float((r.R_mc[:, :, 0].mean(1) - tr.returns_mc[:, Tc - 1]).mean()))
        return r

    def curves(r):
        c = r.curves()
        return [c[k] for k in CURVES]

    out = average_curves("evaluate_dreams", dr, batches, CURVES, call, curves)
    if real:
        out["gap"] = sum(gaps) / float(batches)
    return out
