"""Perturbation saliency: which part of the frame the actor, the critic and
the posterior rest on (Dreamer.saliency_frames, saliency, evaluate_saliency;
Greydanus et al. 2018, "Visualizing and Understanding Atari Agents").

A blurred copy of the frame is blended into one small region, the agent runs
again, and the score is how far its outputs moved; this is repeated over a
grid of regions.  include/dreamer_hip.h "perturbation saliency" has the
definitions the kernels fix (grid, tables, fill, perturbed pixel, scores, map
and overlay).  Pixel models only.

Frame f comes with the hidden state h_f that is about to encode it (on replay
windows: entry t of the filter's hiddens).  Its G + 1 variants -- variant 0 the
frame itself -- go through dr_occlude_frames, dr_encoder_features,
dr_observe_scan (T = 1 from h_f), dr_actor_act (deterministic) and
dr_critic_fwd (the online critic) as one batch of rows f (G + 1) + g, and
dr_saliency_scores compares row g >= 1 with row 0 of the same frame: never with
the trace's own outputs, so a score is 0 exactly when the perturbation changed
nothing.  All variants of a frame share one block of Exp(1) draws (common random
numbers).  The work is cut into passes of at most PASS_VARIANTS variant frames,
so the workspaces stay at the size of a training epoch's."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import hip
from .agent_trace import check_length
from .replay_eval import average_curves, resolve_noise, ring_slots, video_rows, window_prologue

PASS_VARIANTS = 8192  # variant frames of one pass (a B = 256, T = 32 training epoch's encoder batch)
SCORES = ("actor", "value", "posterior_kl")
FILLS = {"blur": 0, "mean": 1}


# ------------------------------------------------------------- host arithmetic
def grid_dims(H, W, stride):
    """(Gy, Gx) of the stride-s grid on an H x W frame; ValueError unless the
    stride divides both sides and G = Gy Gx <= DR_SALIENCY_MAX_CELLS."""
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
        raise ValueError(f"saliency: stride must be a positive integer (got {stride!r})")
    if H % stride or W % stride:
        raise ValueError(f"saliency: stride {stride} does not divide the {H} x {W} frame")
    Gy, Gx = H // stride, W // stride
    if Gy * Gx > L.DR_SALIENCY_MAX_CELLS:
        raise ValueError(f"saliency: {Gy} x {Gx} cells is above {L.DR_SALIENCY_MAX_CELLS}")
    return Gy, Gx


def cell_centres(n, stride):
    """Integer centres i s + s / 2 (integer division) of the n / s cells along a side of n pixels."""
    return [i * stride + stride // 2 for i in range(n // stride)]


def blur_radius(sigma):
    """rb = ceil(3 sigma_b); ValueError unless sigma > 0 and rb <= DR_SALIENCY_MAX_RADIUS."""
    if not (isinstance(sigma, (int, float, np.floating, np.integer)) and math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"saliency: blur_sigma must be a positive number (got {sigma!r})")
    rb = int(math.ceil(3.0 * float(sigma)))
    if rb > L.DR_SALIENCY_MAX_RADIUS:
        raise ValueError(f"saliency: blur radius ceil(3 * {sigma}) = {rb} is above {L.DR_SALIENCY_MAX_RADIUS}")
    return rb


def blur_taps(sigma):
    """(wb f32 [2 rb + 1], rb): exp(-k^2 / (2 sigma^2)), k = -rb .. rb, normalised
    to sum 1 in float64 and rounded to f32 once."""
    rb = blur_radius(sigma)
    k = np.arange(-rb, rb + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32), rb


def mask_profile(sigma, n):
    """gm f32 [n]: exp(-k^2 / (2 sigma^2)), k = 0 .. n-1, in float64, rounded to f32 once."""
    if not (isinstance(sigma, (int, float, np.floating, np.integer)) and math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"saliency: mask_sigma must be a positive number (got {sigma!r})")
    k = np.arange(int(n), dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * float(sigma) ** 2)).astype(np.float32)


def default_mask_sigma(H):
    """Greydanus' 5 px at 80 px, scaled to the frame."""
    return 5.0 * H / 80.0


def pass_frames(G, limit=PASS_VARIANTS):
    """Source frames of one pass: floor(limit / (G + 1)), at least 1."""
    return max(1, int(limit) // (G + 1))


def check_fill(fill):
    if fill not in FILLS:
        raise ValueError(f"saliency: fill must be one of {tuple(FILLS)} (got {fill!r})")
    return FILLS[fill]


def check_pixels(dr):
    if dr.world_model.vector_obs:
        raise ValueError("saliency needs pixel observations (vector observations have no frame to perturb)")


def check_steps(steps, T):
    """The window steps to score, as a list (default: all T)."""
    if steps is None:
        return list(range(T))
    out = [int(t) for t in steps]
    if not out or any(t < 0 or t >= T for t in out):
        raise ValueError(f"saliency: steps must be a non-empty list of window steps in 0 .. {T - 1} (got {steps!r})")
    return out


@dataclass
class Setup:
    """The checked arguments of one call: grid, tables (host), fill code."""
    H: int
    W: int
    stride: int
    Gy: int
    Gx: int
    fill: int
    wb: np.ndarray
    rb: int
    gm: np.ndarray

    @property
    def G(self):
        return self.Gy * self.Gx


def setup(H, W, stride, fill, blur_sigma, mask_sigma):
    """Every check on the perturbation's arguments, then the tables."""
    Gy, Gx = grid_dims(H, W, stride)
    code = check_fill(fill)
    wb, rb = blur_taps(blur_sigma)
    gm = mask_profile(default_mask_sigma(H) if mask_sigma is None else mask_sigma, max(H, W))
    return Setup(H, W, int(stride), Gy, Gx, code, wb, rb, gm)


# --------------------------------------------------------------------- result
def _u8_ring(frames):
    """(contiguous u8 (M,3,H,W), dr_frames reading it as a ring of M slots with starts 0 .. M-1)."""
    fr = frames.reshape(-1, *frames.shape[-3:]).contiguous()
    starts = torch.arange(fr.shape[0], device=fr.device, dtype=torch.int64)
    return fr, starts, L.dr_frames(L.ptr(fr), fr.shape[0], L.ptr(starts), None, 0, 0, 1, 0)


@dataclass
class SaliencyResult:
    """Device tensors of one saliency call.  lead = (N,) for saliency_frames,
    (B, K) for saliency on K steps of B windows.

    actor, value, value_delta, posterior_kl (*lead, Gy, Gx) f32 and latent_flips
    (*lead, Gy, Gx) int32: the scores of the cell's variant against the
    unperturbed frame (include/dreamer_hip.h).  mu, sigma (*lead, A), value_clean
    (*lead), latents (*lead, R, C): the agent on the unperturbed frame.  frames
    u8 (*lead, 3, H, W); stride the grid's."""
    actor: torch.Tensor
    value: torch.Tensor
    value_delta: torch.Tensor
    posterior_kl: torch.Tensor
    latent_flips: torch.Tensor
    mu: torch.Tensor
    sigma: torch.Tensor
    value_clean: torch.Tensor
    latents: torch.Tensor
    frames: torch.Tensor
    stride: int

    def _lead(self):
        return tuple(self.actor.shape[:-2])

    def _score(self, which):
        if which not in SCORES:
            raise ValueError(f"which must be one of {SCORES} (got {which!r})")
        return getattr(self, which)

    def _scale(self, s, normalise):
        """Per-frame scale (M,) of the grids s (M, Gy, Gx): "frame" 1 / the frame's
        largest score, "global" 1 / the largest of all (0 where that is 0), or a number."""
        M = s.shape[0]
        if isinstance(normalise, str):
            if normalise == "frame":
                mx = s.flatten(1).max(dim=1).values
            elif normalise == "global":
                mx = s.max().expand(M)
            else:
                raise ValueError(f'normalise must be "frame", "global" or a number (got {normalise!r})')
            return torch.where(mx > 0, 1.0 / mx, torch.zeros_like(mx)).contiguous()
        return torch.full((M,), float(normalise), device=s.device)

    def _map(self, which, normalise, channel):
        s = self._score(which)
        lead, (H, W) = self._lead(), self.frames.shape[-2:]
        s = s.reshape(-1, *s.shape[-2:]).float().contiguous()
        M = s.shape[0]
        d = L.dr_dims()
        d.img_h, d.img_w = int(H), int(W)
        scale = self._scale(s, normalise)
        out = torch.empty(M, H, W, device=s.device)
        over = fr = None
        ring = None
        if channel is not None:
            if not 0 <= int(channel) <= 2:
                raise ValueError(f"channel must be 0, 1 or 2 (got {channel!r})")
            fr, starts, ring = _u8_ring(self.frames)
            over = torch.empty(M, 3, H, W, dtype=torch.uint8, device=s.device)
        L.call("dr_saliency_map", d, M, self.stride, L.ptr(s), L.ptr(scale), ring, int(channel or 0), L.ptr(out),
               L.ptr(over), hip.stream())
        return out.view(*lead, H, W), None if over is None else over.view(*lead, 3, H, W)

    def maps(self, which="actor", normalise="frame"):
        """The score grid as a heat map (*lead, H, W): scale * the bilinear
        interpolation between the cell centres (dr_saliency_map)."""
        return self._map(which, normalise, None)[0]

    def overlay(self, which="actor", channel=2, normalise="frame"):
        """u8 (*lead, 3, H, W): the frames with the heat map (clamped to [0, 1])
        blended towards 255 in `channel`."""
        return self._map(which, normalise, channel)[1]

    def video(self):
        """u8 [K][3][3h][B*w]: per step the true frames above the actor overlay
        (blue) above the value overlay (red), the B windows side by side; the N
        frames of a saliency_frames result are the steps of one window."""
        rows = (self.frames, self.overlay("actor", 2), self.overlay("value", 0))
        if len(self._lead()) == 1:
            rows = tuple(r.unsqueeze(0) for r in rows)
        return video_rows(*rows)

    def concentration(self, which="actor", top=0.1):
        """Per frame (*lead) the share of the total score held by the ceil(top * G)
        highest cells; a frame whose scores are all 0 gives the uniform share."""
        if not 0.0 < float(top) <= 1.0:
            raise ValueError(f"top must be in (0, 1] (got {top!r})")
        s = self._score(which).flatten(-2)
        G = s.shape[-1]
        k = min(G, max(1, int(math.ceil(float(top) * G))))
        tot = s.sum(-1)
        share = s.topk(k, dim=-1).values.sum(-1) / torch.where(tot > 0, tot, torch.ones_like(tot))
        return torch.where(tot > 0, share, torch.full_like(tot, k / G))


# ----------------------------------------------------------------- the stages
def _frames_to_device(frames, H, W, dev):
    """u8 (N,3,H,W) on the device from (N,H,W,3) numpy frames or a (N,3,H,W) device tensor."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (3, H, W):
            raise ValueError(f"saliency: a frame tensor must be u8 (N, 3, {H}, {W}) (got {frames.dtype}, "
                             f"{tuple(frames.shape)})")
        L.require_gpu(frames)
        return frames.contiguous()
    fr = np.asarray(frames)
    if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[1:] != (H, W, 3):
        raise ValueError(f"saliency: numpy frames must be u8 (N, {H}, {W}, 3) (got {fr.dtype}, {fr.shape})")
    return torch.from_numpy(np.ascontiguousarray(fr.transpose(0, 3, 1, 2))).to(dev)


def run_frames(dr, frames, hiddens, su, sample, noise, mark, pass_limit=PASS_VARIANTS):
    """The passes over N checked device frames (N,3,H,W) with hiddens (N,hidden):
    a SaliencyResult with lead (N,).  noise: None, or explicit draws (N*R, C)."""
    dev = frames.device
    N = int(frames.shape[0])
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    G, V1 = su.G, su.G + 1
    ag = dr.agent
    ag._ensure_flat()
    d = dr.world_model.dims(ag)
    wm = dr.world_model.packed()
    stream = hip.stream()
    n_elems = 3 * su.H * su.W
    wb, gm = torch.from_numpy(su.wb).to(dev), torch.from_numpy(su.gm).to(dev)
    starts = torch.arange(N, device=dev, dtype=torch.int64)
    rng = None
    if noise is None and sample:
        with hip.noise_override_suspended():
            rng = hip.adhoc(dev).noise()  # one stream for the call; a frame's rows are keyed by its index
    actor, value, delta, kl = (torch.empty(N, G, device=dev) for _ in range(4))
    flips = torch.empty(N, G, dtype=torch.int32, device=dev)
    mu0, sg0 = torch.empty(N, A, device=dev), torch.empty(N, A, device=dev)
    v0, z0 = torch.empty(N, device=dev), torch.empty(N, R * C, device=dev)
    Fp = pass_frames(G, pass_limit)
    n_max = min(Fp, N) * V1
    var = torch.empty(n_max, 3, su.H, su.W, dtype=torch.uint8, device=dev)
    vstarts = torch.arange(n_max, device=dev, dtype=torch.int64)
    feat = torch.empty(n_max, d.enc_hidden, device=dev)
    z, logits = torch.empty(n_max, R * C, device=dev), torch.empty(n_max, R * C, device=dev)
    h_out = torch.empty(n_max, Hd, device=dev)
    mu, sg, a_mode = (torch.empty(n_max, A, device=dev) for _ in range(3))
    val = torch.empty(n_max, device=dev)
    wsp = hip.workspace(dev)
    for f0 in range(0, N, Fp):
        F = min(Fp, N - f0)
        n = F * V1
        src = L.dr_frames(L.ptr(frames), N, L.ptr(starts[f0:]), None, 0, 0, 1, 0)
        ws = wsp.get("occlude", L.query("dr_occlude_workspace_bytes", d, F))
        L.call("dr_occlude_frames", d, src, F, su.stride, su.fill, L.ptr(wb), su.rb, L.ptr(gm), L.ptr(var), L.ptr(ws),
               ws.numel(), stream)
        mark("occlude")
        fr = L.dr_frames(L.ptr(var), n, L.ptr(vstarts), None, 0, 0, 1, 0)
        ws = wsp.get("enc", L.query("dr_encoder_workspace_bytes", d, n))
        L.call("dr_encoder_features", d, wm, fr, n, 1, L.ptr(feat), L.ptr(ws), ws.numel(), stream)
        mark("encoder")
        # every variant of a frame: the frame's hidden state and the frame's draws
        h_rep = hiddens[f0:f0 + F].repeat_interleave(V1, dim=0).contiguous()
        if noise is not None:
            q = noise[f0 * R:(f0 + F) * R]
        elif rng is not None:
            q = torch.empty(F * R, C, device=dev)
            L.call("dr_saliency_draws", F * R, C, L.dr_noise(None, None, rng.rng, f0 * R, rng.stream), L.ptr(q), stream)
        else:
            q = None
        q_rep = torch.ones(n * R, C, device=dev) if q is None else \
            q.view(F, 1, R, C).expand(F, V1, R, C).reshape(n * R, C).contiguous()
        ws = wsp.get("obs", L.query("dr_observe_workspace_bytes", d, n))
        L.call("dr_observe_scan", d, wm, n, 1, L.ptr(feat), None, 0, 0, L.ptr(h_rep), None,
               hip.explicit_noise(q=q_rep, device=dev), L.ptr(z), L.ptr(h_out), L.ptr(logits), L.ptr(ws), ws.numel(),
               stream)
        mark("posterior")
        ws = wsp.get("act", L.query("dr_actor_act_workspace_bytes", d, n))
        L.call("dr_actor_act", d, ag.actor_struct(), n, L.ptr(h_rep), L.ptr(z), L.dr_noise(), 1, L.ptr(a_mode),
               L.ptr(mu), L.ptr(sg), L.ptr(ws), ws.numel(), stream)
        mark("actor")
        ws = wsp.get("at_crit", L.query("dr_critic_workspace_bytes", d, n, 0))
        L.call("dr_critic_fwd", d, ag.critic_struct(), n, L.ptr(h_rep), Hd, L.ptr(z), R * C, None, L.ptr(val), None,
               L.ptr(ws), ws.numel(), stream)
        mark("critic")
        sl = slice(f0, f0 + F)
        L.call("dr_saliency_scores", F, G, A, R, C, L.ptr(mu), L.ptr(val), L.ptr(logits), L.ptr(z), L.ptr(actor[sl]),
               L.ptr(value[sl]), L.ptr(delta[sl]), L.ptr(kl[sl]), L.ptr(flips[sl]), stream)
        mark("scores")
        mu0[sl], sg0[sl] = mu[:n:V1], sg[:n:V1]
        v0[sl], z0[sl] = val[:n:V1], z[:n:V1]
        mark("collect")
    g = lambda t: t.view(N, su.Gy, su.Gx)
    return SaliencyResult(actor=g(actor), value=g(value), value_delta=g(delta), posterior_kl=g(kl),
                          latent_flips=g(flips), mu=mu0, sigma=sg0, value_clean=v0, latents=z0.view(N, R, C),
                          frames=frames, stride=su.stride)


def _frame_size(dr):
    return tuple(int(s) for s in dr.buffer.observation_buffer.shape[2:])


def saliency_frames(dr, frames, hiddens, stride=4, fill="blur", blur_sigma=3.0, mask_sigma=None, sample=False,
                    noise=None, _mark=None, _pass_limit=PASS_VARIANTS):
    """Dreamer.saliency_frames (see there)."""
    mark = _mark or (lambda name: None)
    check_pixels(dr)
    H, W = _frame_size(dr)
    su = setup(H, W, stride, fill, blur_sigma, mask_sigma)
    R, C = dr.latent_state_dims
    dev = dr.buffer.device
    fr = _frames_to_device(frames, H, W, dev)
    N = int(fr.shape[0])
    if N < 1:
        raise ValueError("saliency: need at least one frame")
    if not isinstance(hiddens, torch.Tensor) or tuple(hiddens.shape) != (N, dr.hidden_state_dims):
        raise ValueError(f"saliency: hiddens must be a ({N}, {dr.hidden_state_dims}) tensor")
    q = None
    if noise is not None:
        (q,) = resolve_noise((noise,), sample, ((N * R, C),), f"noise must be one tensor of shape ({N * R}, {C})", dev)
    L.require_gpu(hiddens)
    L.require_gpu(fr)
    return run_frames(dr, fr, hiddens.float().contiguous(), su, sample, q, mark, _pass_limit)


def saliency(dr, starts=None, batch_size=None, length=None, steps=None, stride=4, fill="blur", blur_sigma=3.0,
             mask_sigma=None, sample=False, noise=None, _mark=None, _pass_limit=PASS_VARIANTS):
    """Dreamer.saliency (see there)."""
    mark = _mark or (lambda name: None)
    check_pixels(dr)
    S = dr.sequence_length
    T = S if length is None else int(length)
    check_length(T, S)
    ts = check_steps(steps, T)
    K = len(ts)
    H, W = _frame_size(dr)
    su = setup(H, W, stride, fill, blur_sigma, mask_sigma)
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    if noise is not None and (not isinstance(noise, (tuple, list)) or len(noise) != 2):
        raise ValueError("noise must be a pair: the trace's draws and the variants' draws")

    def shapes(B):
        return ((T, B * R, C), (B * K * R, C)), f"noise must be ({T}, {B * R}, {C}) and ({B * K * R}, {C})"

    def check(B):  # (before the starts are sampled)
        if noise is not None and tuple(tuple(q.shape) for q in noise) != shapes(B)[0]:
            raise ValueError(shapes(B)[1])

    def draws(B, dev):
        return resolve_noise(noise, sample, *shapes(B), dev)

    w = window_prologue(dr, starts, batch_size, T, draws, mark, check=check)
    B, dev = w.B, w.st.device
    # closed_loop's filter without the prior and the heads: hiddens[t] is about to encode frame t
    _, hid, _, _, _, _ = dr.world_model._observe_trace(w.d, B, T, w.feat, w.act.data_ptr(), S * A, A, None, None,
                                                       w.noise[0], heads=False, prior=False)
    mark("trace")
    sel = torch.as_tensor(ts, dtype=torch.int64, device=dev)
    slots = ring_slots(w.st, 0, T, dr.buffer.capacity)[:, sel]
    frames = dr.buffer._mirror()["frames"][slots].reshape(B * K, 3, H, W)
    h_sel = hid[:, sel].reshape(B * K, Hd).contiguous()
    mark("frames")
    r = run_frames(dr, frames, h_sel, su, sample, w.noise[1], mark, _pass_limit)
    lead = lambda t: t.view(B, K, *t.shape[1:])
    return SaliencyResult(actor=lead(r.actor), value=lead(r.value), value_delta=lead(r.value_delta),
                          posterior_kl=lead(r.posterior_kl), latent_flips=lead(r.latent_flips), mu=lead(r.mu),
                          sigma=lead(r.sigma), value_clean=lead(r.value_clean), latents=lead(r.latents),
                          frames=lead(r.frames), stride=r.stride)


def evaluate_saliency(dr, batches=1, batch_size=None, length=None, steps=None, top=0.1, **kw):
    """Dreamer.evaluate_saliency (see there)."""
    keys = SCORES + tuple(f"concentration_{k}" for k in SCORES)
    # (the checks that need no window, before the random state is even looked at)
    check_pixels(dr)
    setup(*_frame_size(dr), kw.get("stride", 4), kw.get("fill", "blur"), kw.get("blur_sigma", 3.0),
          kw.get("mask_sigma"))

    def curves(r):
        lead = tuple(range(len(r.actor.shape) - 2))
        return [getattr(r, k).mean(lead) for k in SCORES] + [r.concentration(k, top).mean() for k in SCORES]

    out = average_curves("evaluate_saliency", dr, batches, keys, lambda: saliency(
        dr, batch_size=batch_size, length=length, steps=steps, **kw), curves)
    out["concentration"] = {k: out.pop(f"concentration_{k}") for k in SCORES}
    return out
