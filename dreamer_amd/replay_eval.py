"""The front end the replay-window evaluation entry points share (open_loop,
closed_loop, agent_trace, sample_futures and their evaluate_* averages).

A window b is S = sequence_length consecutive ring slots from starts[b].
Here: the slot arithmetic and the length check; the prologue every entry point
opens with (resolve the starts, resolve the noise, dr_replay_gather,
dr_encoder_features on the ring's frames); the context filter (dr_observe_scan
to the posterior after the context frames); the decode-and-score stage
(dr_decoder_fwd + dr_frame_metrics); the helpers of the result containers; and
what the evaluate_* methods are made of (random state preserved, per-step
curves averaged over sampled batches).

Every argument check fires before np.random is drawn from, and everything is
enqueued on the current stream without a sync.  The ad-hoc Philox draws are
taken in the order the stages are enqueued: a stage given explicit draws (or
the mode, q == 1) takes none."""
import math
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import hip


# ------------------------------------------------------------ window arithmetic
def ring_slots(starts, first, count, capacity):
    """Ring slots [B][count] of window steps first .. first+count-1, as an int64
    tensor on the device of `starts` (a tensor, or anything torch.as_tensor takes)."""
    st = torch.as_tensor(starts, dtype=torch.int64).reshape(-1, 1)
    return (st + torch.arange(first, first + count, dtype=torch.int64, device=st.device).reshape(1, -1)) % capacity


def check_window(ok, needs, got, sequence_length):
    if not ok:
        raise ValueError(f"{needs} (got {got} vs {sequence_length})")


# --------------------------------------------------------------------- prologue
def resolve_noise(noise, sample, shapes, message, dev):
    """One tensor of Exp(1) draws per shape: the caller's `noise` (as contiguous
    f32; ValueError(message) unless the shapes are these), ones (the mode of
    every categorical) with sample=False, else None: Philox."""
    if noise is not None:
        qs = tuple(t.float().contiguous() for t in noise)
        if tuple(tuple(q.shape) for q in qs) != tuple(shapes):
            raise ValueError(message)
        return qs
    if sample:
        return (None,) * len(shapes)
    ones = {}
    for s in shapes:
        if s not in ones:
            ones[s] = torch.ones(*s, device=dev)
    return tuple(ones[s] for s in shapes)


@dataclass
class Windows:
    """What window_prologue leaves: the int64 device starts (B,), the resolved
    noise, the model's dims / packed world model, the stream, the gathered
    actions (B,S,A), rewards and continues (B,S) and the encoder features of
    the first T frames (T*B, enc_hidden)."""
    st: torch.Tensor
    B: int
    noise: tuple
    d: object
    wm: object
    stream: object
    act: torch.Tensor
    rew: torch.Tensor
    cont: torch.Tensor
    feat: torch.Tensor


def window_prologue(dr, starts, batch_size, T, draws, mark, check=None):
    """starts: the window starts, or None to sample batch_size (default
    dr.batch_size) of them.  check(B), if given, runs before the sampling and
    on the final B.  draws(B, dev) resolves the call's noise (resolve_noise)
    once B is known, before the gather.  Marks "gather" and "encoder".
    The sampled starts are uniform (buffer.sample_eval_starts) also with
    replay = "curious": evaluation sees the data distribution, not the
    training distribution.  With replay_episodes = "respect" they are an
    unweighted device draw among the windows that lie inside one stream."""
    buf, wmod = dr.buffer, dr.world_model
    dev = buf.device
    if starts is None:
        n_win = batch_size or dr.batch_size
        if check is not None:
            check(int(n_win))
        starts = buf.sample_eval_starts(n_win)
    st = starts.to(dev, torch.int64) if isinstance(starts, torch.Tensor) else \
        torch.as_tensor(np.asarray(starts), dtype=torch.int64).to(dev)
    B = int(st.numel())
    if check is not None:
        check(B)
    noise = draws(B, dev)
    S, A = dr.sequence_length, dr.action_dims
    d = wmod.dims(dr.agent)
    wm = wmod.packed()
    stream = hip.stream()
    m = buf._mirror()
    act = torch.empty(B, S, A, device=dev)
    rew, cont = torch.empty(B, S, device=dev), torch.empty(B, S, device=dev)
    L.call("dr_replay_gather", buf.capacity, B, S, 0, A, None, L.ptr(m["actions"]), L.ptr(m["rewards"]),
           L.ptr(m["continues"]), L.ptr(st), None, L.ptr(act), L.ptr(rew), L.ptr(cont), stream)
    mark("gather")
    fr = buf.frames_struct(st)
    feat = torch.empty(T * B, d.enc_hidden, device=dev)
    ws = hip.workspace(dev).get("enc", L.query("dr_encoder_workspace_bytes", d, T * B))
    L.call("dr_encoder_features", d, wm, fr, B, T, L.ptr(feat), L.ptr(ws), ws.numel(), stream)
    mark("encoder")
    return Windows(st, B, noise, d, wm, stream, act, rew, cont, feat)


def context_filter(dr, w, Tc, q_ctx, mark):
    """The posterior (z0 (B,R*C), h0 (B,hidden)) after the first Tc frames of
    the windows (warm_start_generator's scan, Dreamer.py:244-262).  Marks "scan"."""
    R, C = dr.latent_state_dims
    S, A = dr.sequence_length, dr.action_dims
    dev = w.st.device
    z0, h0 = torch.empty(w.B, R * C, device=dev), torch.empty(w.B, dr.hidden_state_dims, device=dev)
    nz = hip.explicit_noise(q=q_ctx, device=dev) if q_ctx is not None else hip.adhoc(dev).noise()
    ws = hip.workspace(dev).get("obs", L.query("dr_observe_workspace_bytes", w.d, w.B))
    L.call("dr_observe_scan", w.d, w.wm, w.B, Tc, L.ptr(w.feat), L.ptr(w.act), S * A, A, None, None, nz, L.ptr(z0),
           L.ptr(h0), None, L.ptr(ws), ws.numel(), w.stream)
    mark("scan")
    return z0, h0


def decode_and_score(dr, w, st, lead, t0, hid, latents, want_true, mark):
    """Decode the states (hid, z) for every z of `latents` (a None entry is
    skipped) into mu (*lead, frame...), then compare each with the ring's
    frames t0 .. t0+K-1 of the windows `st`: lead = (rows..., K), st holds one
    start per row.  Returns ([(mu, sqerr (*lead), u8 prediction or None)] -- all
    None for a skipped entry --, the u8 true frames (want_true, pixel models,
    written beside the first entry), the dr_frames the scores were taken
    against).  Marks "decoder" and "metrics"."""
    buf = dr.buffer
    dev = hid.device
    R, C = dr.latent_state_dims
    d = w.d
    K = lead[-1]
    rows = math.prod(lead[:-1])
    vector = buf.vector
    shape = (d.obs_dim,) if vector else (3, d.img_h, d.img_w)
    ws = hip.workspace(dev).get("dec", L.query("dr_decoder_workspace_bytes", d, rows * K))
    dec = dr.world_model.packed_decoder()
    out = []
    for z in latents:
        if z is None:
            out.append((None, None, None))
            continue
        mu = torch.empty(*lead, *shape, device=dev)
        L.call("dr_decoder_fwd", d, dec, rows * K, L.ptr(hid), dr.hidden_state_dims, L.ptr(z), R * C, L.ptr(mu),
               L.ptr(ws), ws.numel(), w.stream)
        out.append((mu, torch.empty(*lead, device=dev),
                    None if vector else torch.empty(*lead, *shape, dtype=torch.uint8, device=dev)))
    mark("decoder")
    true = torch.empty(*lead, *shape, dtype=torch.uint8, device=dev) if want_true and not vector else None
    truth = buf.frames_struct(st)
    truth.t0 = t0
    for k, (mu, sq, pred) in enumerate(out):
        if mu is not None:
            L.call("dr_frame_metrics", d, rows, K, L.ptr(mu), truth, L.ptr(sq), L.ptr(pred),
                   L.ptr(true) if k == 0 else None, w.stream)
    mark("metrics")
    return out, true, truth


# ------------------------------------------------------------ result containers
class FrameResult:
    """What the result containers with decoded frames share.  _mu names the
    decoded-frame field, _lead its leading (non-frame) dims, _u8 the u8 fields
    the pixel-only methods need."""
    _mu, _lead, _u8 = "mu", 2, ("frames_pred", "frames_true")

    def frame_elems(self):
        return math.prod(int(s) for s in getattr(self, self._mu).shape[self._lead:])

    def _need_frames(self, what):
        if any(getattr(self, k) is None for k in self._u8):
            raise ValueError(f"{what} needs pixel observations (vector observations have no u8 frames)")


def psnr_u8(pred, true):
    """PSNR per frame in dB on the u8 scale: 10 log10(255^2 / mean((pred - true)^2)), u8 (...,3,h,w) -> (...)."""
    d = pred.float() - true.float()
    return 10.0 * torch.log10(255.0 ** 2 / d.pow(2).flatten(-3).mean(-1))


def video_rows(*frames):
    """u8 (B,K,3,h,w) each -> (K,3,n*h,B*w): per step the given frames one above
    the other, the B windows side by side."""
    row = lambda f: torch.cat(list(f.transpose(0, 1).unbind(1)), dim=-1)  # (B,K,3,h,w) -> (K,3,h,B*w)
    return torch.cat([row(f) for f in frames], dim=-2).contiguous()


# ------------------------------------------------------------------- evaluate_*
@contextmanager
def preserved_rng(device):
    """np.random's state and the ad-hoc Philox {seed, offset} and stream
    counter are put back on exit, also when the body raises."""
    np_state = np.random.get_state()
    ar = hip.adhoc(device)
    rng_state, rng_counter = ar.state.clone(), ar.counter
    try:
        yield
    finally:
        np.random.set_state(np_state)
        ar.state.copy_(rng_state)
        ar.counter = rng_counter


def average_curves(name, dr, batches, keys, call, curves):
    """{key: CPU float list} of curves(call()) -- per-step device curves in the
    order of `keys`, None for one the model does not have -- averaged over
    `batches` calls, with the random state left as found."""
    if int(batches) < 1:
        raise ValueError(f"{name} needs batches >= 1")
    acc = None
    with preserved_rng(dr.device), torch.no_grad():
        for _ in range(int(batches)):
            cur = curves(call())
            acc = cur if acc is None else [None if a is None else a + b for a, b in zip(acc, cur)]
    return {k: None if a is None else (a / float(batches)).cpu().tolist() for k, a in zip(keys, acc)}


def head_errors(r):
    """[|reward error| in symlog space, continue BCE], each (steps,), of a result
    with reward_pred / reward_true / continue_pred / continue_true (B,steps,1)."""
    return [(r.reward_pred - r.reward_true).abs().mean((0, 2)),
            torch.nn.functional.binary_cross_entropy(r.continue_pred.clamp(0.0, 1.0), r.continue_true,
                                                     reduction="none").mean((0, 2))]
