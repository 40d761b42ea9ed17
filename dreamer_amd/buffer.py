"""Replay buffer with the reference's API (Buffer.py).

The host numpy ring keeps the reference's exact storage and sampling
semantics (np.random.randint starts, one redraw for windows straddling the
write head).  A device mirror of the ring (u8 frames, f32 actions, symlog
rewards, continues) lives in HBM; new transitions are uploaded lazily before
sampling, and windows are gathered on the device -- the fused train_Agent path
never materialises the float32 window at all: the encoder's first conv reads
the u8 frames straight from the ring (dr_frames).

replay = "curious" (Dreamer's config key) adds prioritised
sampling on the device: one priority (f32) and one visit count (i32) per ring
slot beside the mirror, sample_start_indices_device / update_priorities /
sampling_probabilities on libdreamer_hip (include/dreamer_hip.h has the
semantics).  sample_start_indices and everything else of the uniform path are
untouched, and in uniform mode no priority tensor is ever allocated.

replay_episodes = "respect"  keeps the device sampler inside one
stream of data: a per-slot `first` flag (u8) beside the ring, the window spans
(dr_replay_spans, recomputed when the mirror takes in new slots) and draws
masked by span >= sequence_length, with the priorities of curious mode or with
none (replay = "uniform").  With "ignore" (the default) none of it exists."""
import numpy as np
import torch

from . import _lib as L
from . import hip
from .utils import symlog_np


REPLAY_MODES = ("uniform", "curious")
EPISODE_MODES = ("ignore", "respect")
REPLAY_DEFAULTS = dict(replay_c=1e4, replay_beta=0.7, replay_alpha=0.7, replay_eps=0.01, replay_p_new=1e5)


def check_replay(replay, c, beta, alpha, eps, p_new):
    """ValueError for an unknown mode or a constant outside its range."""
    if replay not in REPLAY_MODES:
        raise ValueError(f"replay must be one of {REPLAY_MODES}, got {replay!r}")
    for name, v, ok in (("replay_beta", beta, 0.0 < beta <= 1.0), ("replay_alpha", alpha, alpha > 0.0),
                        ("replay_eps", eps, eps > 0.0), ("replay_c", c, c >= 0.0),
                        ("replay_p_new", p_new, p_new > 0.0)):
        if not ok:  # a NaN fails every comparison
            raise ValueError(f"{name} = {v!r} is out of range (beta in (0, 1], alpha > 0, eps > 0, c >= 0, p_new > 0)")


def check_replay_episodes(mode):
    if mode not in EPISODE_MODES:
        raise ValueError(f"replay_episodes must be one of {EPISODE_MODES}, got {mode!r}")


def valid_starts(size, capacity, next_idx, seq_len):
    """Boolean [capacity]: slot i is a valid window start iff 0 <= i < size - S + 1
    and not (size == capacity and i < next_idx < i + S)."""
    i = np.arange(capacity, dtype=np.int64)
    ok = i < size - seq_len + 1
    if size == capacity:
        ok &= ~((i < next_idx) & (next_idx < i + seq_len))
    return ok


def valid_window_exists(size, capacity, next_idx, seq_len):
    """valid_starts(...).any() without the array: the starts before the tail
    minus those in the straddle zone [next_idx - S + 1, next_idx - 1]."""
    n = size - seq_len + 1
    if n <= 0:
        return False
    if size != capacity:
        return True
    lo, hi = max(0, next_idx - seq_len + 1), min(next_idx - 1, n - 1)
    return n - max(0, hi - lo + 1) > 0


class Buffer:
    def __init__(self, buffer_size, sequence_length, action_size, observation_dims, device="cpu"):
        # observation_dims = [D]: f32 vector observations (BASELINE configs[4]); else u8 frames
        self.vector = len(tuple(observation_dims)) == 1
        self.observation_buffer = np.zeros((buffer_size, observation_dims[0]), dtype=np.float32) if self.vector \
            else np.zeros((buffer_size, 3, *observation_dims), dtype=np.uint8)
        self.action_buffer = np.zeros((buffer_size, action_size), dtype=np.float32)
        self.reward_buffer = np.zeros((buffer_size, 1), dtype=np.float32)
        self.continue_buffer = np.zeros((buffer_size, 1), dtype=np.float32)
        self.capacity = buffer_size
        self.sequence_length = sequence_length
        self.device = torch.device(device)
        self.next_idx = 0
        self.size = 0
        self._dev = None
        self._dirty = []  # slot indices not yet mirrored on the device
        # prioritised replay (set by Dreamer from the config; the constructor stays the reference's)
        self.replay = "uniform"
        self.replay_c, self.replay_beta, self.replay_alpha, self.replay_eps, self.replay_p_new = (
            REPLAY_DEFAULTS[k] for k in ("replay_c", "replay_beta", "replay_alpha", "replay_eps", "replay_p_new"))
        # episode-aware replay (set by Dreamer from the config): first_buffer[j] != 0 says that slot j begins a
        # new stream; only "respect" ever looks at it
        self.replay_episodes = "ignore"
        self.first_buffer = np.zeros(buffer_size, dtype=np.uint8)
        self._span_key = None  # (size, next_idx) the device spans were computed for
        self._n_valid = 0

    # ---- host side (Buffer.py:19-30) -----------------------------------------
    def add_to_buffer(self, observation, action, reward, continue_, first=False):
        """first=True: this transition begins a new stream of data (replay_episodes = "respect" then draws no
        window that runs from the slot before into this one)."""
        i = self.next_idx
        self.first_buffer[i] = 1 if first else 0
        self.observation_buffer[i] = np.array(observation, dtype=self.observation_buffer.dtype)
        self.action_buffer[i] = np.array(action, dtype=np.float32)
        self.continue_buffer[i] = np.array(continue_, dtype=np.float32)
        self.reward_buffer[i] = symlog_np(np.array(reward, dtype=np.float32))
        self._dirty.append(i)
        self.next_idx = (i + 1) % self.capacity
        if self.size < self.capacity:
            self.size += 1

    def load_arrays(self, frames, actions, rewards_symlog, continues, first=None):
        """Bulk fill (benchmarks / fixtures): rewards already symlog'ed; first: the per-slot flags (None: 0)."""
        n = len(frames)
        assert n <= self.capacity
        self.observation_buffer[:n] = frames
        self.action_buffer[:n] = actions.reshape(n, -1)
        self.reward_buffer[:n] = rewards_symlog.reshape(n, 1)
        self.continue_buffer[:n] = continues.reshape(n, 1)
        self.first_buffer[:n] = 0 if first is None else np.asarray(first).reshape(n) != 0
        self.size = max(self.size, n)
        self.next_idx = n % self.capacity
        self._dirty = list(range(n))

    def sample_start_indices(self, batch_size):
        """Window starts with the reference's RNG consumption (Buffer.py:33-48)."""
        if self.size < self.sequence_length:
            raise ValueError("Not enough data in buffer to sample a full sequence")
        valid = self.size - self.sequence_length + 1
        starts = np.random.randint(0, valid, size=batch_size)
        if self.size == self.capacity:
            out = []
            for s in starts:
                out.append(np.random.randint(0, valid) if s < self.next_idx < s + self.sequence_length else s)
            starts = np.array(out)
        return starts

    # ---- device mirror -------------------------------------------------------
    def _require_gpu(self):
        if not self.device.type == "cuda":
            raise RuntimeError("dreamer_amd: the replay device mirror needs a GPU device")

    def _mirror(self):
        self._require_gpu()
        if self._dev is None:
            self._dev = dict(
                frames=torch.zeros(self.observation_buffer.shape, dtype=torch.float32 if self.vector else torch.uint8,
                                   device=self.device),
                actions=torch.zeros(self.action_buffer.shape, device=self.device),
                rewards=torch.zeros(self.reward_buffer.shape, device=self.device),
                continues=torch.zeros(self.continue_buffer.shape, device=self.device))
            self._dirty = list(range(self.size))
        curious = self.replay != "uniform"
        if curious and "priority" not in self._dev:
            # every slot starts as new; a slot never written is not a valid start
            self._dev["priority"] = torch.full((self.capacity,), float(self.replay_p_new), device=self.device)
            self._dev["visits"] = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        respect = self.replay_episodes != "ignore"
        if respect and "first" not in self._dev:
            self._dev["first"] = torch.from_numpy(self.first_buffer).to(self.device)
            self._dev["span"] = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self._dev["n_valid"] = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._span_key = None
        if self._dirty:
            idx = np.unique(np.asarray(self._dirty, dtype=np.int64))
            runs = np.split(idx, np.where(np.diff(idx) != 1)[0] + 1)
            for r in runs:
                a, b = int(r[0]), int(r[-1]) + 1
                for k, host in (("frames", self.observation_buffer), ("actions", self.action_buffer),
                                ("rewards", self.reward_buffer), ("continues", self.continue_buffer)):
                    self._dev[k][a:b].copy_(torch.from_numpy(host[a:b]), non_blocking=False)
                if respect:
                    self._dev["first"][a:b].copy_(torch.from_numpy(self.first_buffer[a:b]), non_blocking=False)
                if curious:  # a written slot is a new window; windows that merely contain it keep theirs
                    self._dev["priority"][a:b] = float(self.replay_p_new)
                    self._dev["visits"][a:b] = 0
            self._dirty = []
            self._span_key = None
        if respect and self._span_key != (self.size, self.next_idx):
            # one span pass per refresh (new slots, or a moved write head), and one read-back of the count: the
            # draws themselves neither rescan nor sync
            m = self._dev
            ws = hip.workspace(self.device).get("replay_spans", L.query("dr_replay_spans_workspace_bytes",
                                                                        self.capacity))
            L.call("dr_replay_spans", self.capacity, self.size, self.next_idx, L.ptr(m["continues"]),
                   L.ptr(m["first"]), self.sequence_length, L.ptr(m["span"]), L.ptr(m["n_valid"]), L.ptr(ws),
                   ws.numel(), hip.stream())
            self._n_valid = int(m["n_valid"].item())
            self._span_key = (self.size, self.next_idx)
        return self._dev

    # ---- prioritised replay (replay = "curious") -----------------------------
    def _curious(self):
        if self.replay == "uniform":
            raise RuntimeError("dreamer_amd: prioritised sampling needs replay = 'curious'")
        return self._sampler()

    def _sampler(self):
        """(mirror, workspace) of the device sampler: replay = "curious", replay_episodes = "respect" or both."""
        respect = self.replay_episodes != "ignore"
        if self.replay == "uniform" and not respect:
            raise RuntimeError("dreamer_amd: device sampling needs replay = 'curious' or replay_episodes = 'respect'")
        check_replay(self.replay, self.replay_c, self.replay_beta, self.replay_alpha, self.replay_eps,
                     self.replay_p_new)
        check_replay_episodes(self.replay_episodes)
        self._require_gpu()
        if not valid_window_exists(self.size, self.capacity, self.next_idx, self.sequence_length):
            raise ValueError("Not enough data in buffer to sample a full sequence")
        m = self._mirror()
        if respect and self._n_valid == 0:  # data enough for a window, but every window holds a break
            raise ValueError("Not enough data in buffer to sample a full sequence")
        ws = hip.workspace(self.device).get("replay", L.query("dr_replay_sample_workspace_bytes", self.capacity))
        return m, ws

    def _respecting(self):
        if self.replay_episodes == "ignore":
            raise RuntimeError("dreamer_amd: window spans need replay_episodes = 'respect'")
        check_replay_episodes(self.replay_episodes)
        self._require_gpu()
        return self._mirror()

    def window_spans(self):
        """int32 device tensor (capacity,): span[i] slots from i on lie in one stream of data (0 for an unwritten
        slot); slot i is a valid start iff span[i] >= sequence_length (include/dreamer_hip.h).  The mirror's own
        tensor: read it, do not write it."""
        return self._respecting()["span"]

    def valid_start_count(self):
        """How many slots are valid starts (read back when the mirror last took in new data: no sync here)."""
        self._respecting()
        return self._n_valid

    def sample_eval_starts(self, batch_size):
        """Window starts for evaluation: the data distribution, whatever `replay` says.  replay_episodes =
        "ignore": exactly sample_start_indices (np.random).  "respect": an unweighted device draw among the valid
        starts from the ad-hoc generator (int64 device tensor)."""
        if self.replay_episodes == "ignore":
            return self.sample_start_indices(batch_size)
        return self._draw(batch_size, None, prioritised=False)[0]

    def p_floor(self):
        """What a stored priority that is non-finite or <= 0 counts as."""
        return float(self.replay_eps) ** float(self.replay_alpha)

    def sample_start_indices_device(self, batch_size, u=None):
        """Prioritised window starts drawn on the device: (starts int64 (B,),
        prob f32 (B,)), both device tensors; prob[b] = w / W of the start drawn.
        No np.random call and no sync: the uniforms are Philox draws on a
        stream id of the ad-hoc generator (u: explicit float64 uniforms (B,)
        on the device, for parity tests).  replay_episodes = "respect": only
        starts with span >= sequence_length are drawn, with the priorities of
        curious mode or, in uniform mode, every valid start alike."""
        return self._draw(batch_size, u, prioritised=self.replay != "uniform")

    def _draw(self, batch_size, u, prioritised):
        m, ws = self._sampler()
        B = int(batch_size)
        starts = torch.empty(B, dtype=torch.int64, device=self.device)
        prob = torch.empty(B, device=self.device)
        if u is not None:
            if u.dtype != torch.float64 or tuple(u.shape) != (B,):
                raise ValueError(f"u must be float64 of shape ({B},)")
            u = u.contiguous()
            rng, sid = None, 0
        else:
            nz = hip.adhoc(self.device).noise()
            rng, sid = nz.rng, nz.stream
        if self.replay_episodes == "ignore":
            L.call("dr_replay_sample", self.capacity, self.size, self.next_idx, self.sequence_length, B,
                   L.ptr(m["priority"]), self.p_floor(), L.ptr(u), rng, sid, L.ptr(starts), L.ptr(prob), L.ptr(ws),
                   ws.numel(), hip.stream())
        else:
            L.call("dr_replay_sample_spans", self.capacity, self.size, self.next_idx, self.sequence_length, B,
                   L.ptr(m["priority"]) if prioritised else None, self.p_floor(), L.ptr(m["span"]), L.ptr(u), rng,
                   sid, L.ptr(starts), L.ptr(prob), L.ptr(ws), ws.numel(), hip.stream())
        return starts, prob

    def update_priorities(self, starts_dev, scores_dev):
        """priority / visits after a world-model step on windows `starts_dev`
        (int64 (B,)) whose losses were `scores_dev` (f32 (B,)); no sync."""
        m, _ = self._curious()
        B = int(starts_dev.numel())
        if starts_dev.dtype != torch.int64 or scores_dev.dtype != torch.float32 or int(scores_dev.numel()) != B:
            raise ValueError("update_priorities takes int64 starts and float32 scores of one length")
        L.call("dr_replay_priority_update", self.capacity, B, L.ptr(starts_dev.contiguous()),
               L.ptr(scores_dev.contiguous()), float(self.replay_c), float(self.replay_beta),
               float(self.replay_alpha), float(self.replay_eps), float(self.replay_p_new), L.ptr(m["priority"]),
               L.ptr(m["visits"]), hip.stream())

    def sampling_probabilities(self):
        """f32 device tensor (capacity,): the probability that a draw of
        sample_start_indices_device returns each slot (0 for an invalid start)."""
        m, ws = self._sampler()
        prob = torch.empty(self.capacity, device=self.device)
        if self.replay_episodes == "ignore":
            L.call("dr_replay_probabilities", self.capacity, self.size, self.next_idx, self.sequence_length,
                   L.ptr(m["priority"]), self.p_floor(), L.ptr(prob), L.ptr(ws), ws.numel(), hip.stream())
        else:
            L.call("dr_replay_probabilities_spans", self.capacity, self.size, self.next_idx, self.sequence_length,
                   L.ptr(m["priority"]) if self.replay != "uniform" else None, self.p_floor(), L.ptr(m["span"]),
                   L.ptr(prob), L.ptr(ws), ws.numel(), hip.stream())
        return prob

    def device_key(self):
        m = self._mirror()
        return (m["frames"].data_ptr(), self.capacity)

    def frames_struct(self, starts_dev):
        """dr_frames reading the warm-start frames straight from the u8 ring
        (vector observations: the f32 ring, dr_dims.obs_dim)."""
        m = self._mirror()
        return L.dr_frames(L.ptr(m["frames"]), self.capacity, L.ptr(starts_dev), None, 0, 0, 0 if self.vector else 1)

    def gather_actions(self, starts_dev, out):
        """out[b][s][:] = action at slot (starts[b]+s) % capacity."""
        m = self._mirror()
        B, S, A = out.shape
        L.call("dr_replay_gather", self.capacity, B, S, 0, A, None, L.ptr(m["actions"]), L.ptr(m["rewards"]),
               L.ptr(m["continues"]), L.ptr(starts_dev), None, L.ptr(out), None, None, hip.stream())

    def sample_sequences(self, batch_size):
        """Buffer.sample_sequences (Buffer.py:32-63): float32 tensors on the
        buffer's device, obs holding 0..255."""
        starts = self.sample_start_indices(batch_size)
        S = self.sequence_length
        if self.device.type != "cuda":
            idx = (starts[:, None] + np.arange(S)[None, :]) % self.capacity
            f = lambda a: torch.tensor(a[idx], dtype=torch.float32, device=self.device)
            return (f(self.observation_buffer), f(self.action_buffer), f(self.reward_buffer),
                    f(self.continue_buffer), S)
        m = self._mirror()
        dev = self.device
        st = torch.as_tensor(starts, dtype=torch.int64).to(dev)
        if self.vector:  # f32 rows: a plain device gather
            idx = (st[:, None] + torch.arange(S, device=dev)[None, :]) % self.capacity
            return m["frames"][idx], m["actions"][idx], m["rewards"][idx], m["continues"][idx], S
        fe = int(np.prod(self.observation_buffer.shape[1:]))
        A = self.action_buffer.shape[1]
        obs = torch.empty(batch_size, S, *self.observation_buffer.shape[1:], device=dev)
        act = torch.empty(batch_size, S, A, device=dev)
        rew = torch.empty(batch_size, S, 1, device=dev)
        cont = torch.empty(batch_size, S, 1, device=dev)
        L.call("dr_replay_gather", self.capacity, batch_size, S, fe, A, L.ptr(m["frames"]), L.ptr(m["actions"]),
               L.ptr(m["rewards"]), L.ptr(m["continues"]), L.ptr(st), L.ptr(obs), L.ptr(act), L.ptr(rew),
               L.ptr(cont), hip.stream())
        return obs, act, rew, cont, S
