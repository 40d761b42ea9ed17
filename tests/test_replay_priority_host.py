"""Prioritised replay, the parts that need no GPU: the float64 reference's own
invariants, the valid-start set against what the reference's sampler
(oracle.replay_starts, Buffer.py:33-48) can and cannot return, the config
validation, the CPU-device error and the uniform-mode training-state keys."""
import numpy as np
import pytest
import torch

import replay_ref as RR
from formula import SMALL
from oracle import dreamer_oracle as O

# (cap, size, next_idx, S)
RINGS = [(64, 40, 40, 8), (64, 64, 20, 8), (64, 64, 3, 8), (64, 64, 0, 8), (64, 64, 63, 8), (64, 7, 7, 8),
         (64, 8, 8, 8)]

# "buffer" / top-level keys of Dreamer.training_state() as the parent commit wrote them
PARENT_STATE_KEYS = {"format", "model", "opt_actor", "opt_critic", "opt_wm", "S", "rng_engine", "rng_engine_counter",
                     "rng_adhoc", "rng_adhoc_counter", "np_rng", "torch_rng", "buffer", "seed"}
PARENT_BUFFER_KEYS = {"obs", "act", "rew", "cont", "next_idx", "size"}


@pytest.mark.parametrize("cap,size,next_idx,S", RINGS)
def test_reference_probabilities(cap, size, next_idx, S):
    from dreamer_amd.buffer import valid_starts, valid_window_exists
    ok = RR.valid_mask(cap, size, next_idx, S)
    assert np.array_equal(ok, RR.valid_mask_fast(cap, size, next_idx, S))
    assert np.array_equal(ok, valid_starts(size, cap, next_idx, S))
    assert valid_window_exists(size, cap, next_idx, S) == bool(ok.any())
    if not ok.any():
        return
    g = np.random.RandomState(3)
    pri = np.exp(g.uniform(np.log(0.04), np.log(1e5), cap)).astype(np.float32)
    pri[::7] = np.array([np.nan, 0.0, -1.0, np.inf], dtype=np.float32)[np.arange(len(pri[::7])) % 4]
    p = RR.probabilities(pri, size, next_idx, S, 0.01 ** 0.7)
    assert abs(p.sum() - 1.0) < 1e-12
    assert np.all(p[~ok] == 0.0) and np.all(p[ok] > 0.0)
    starts, prob, margin = RR.sample(pri, size, next_idx, S, 0.01 ** 0.7, g.uniform(size=4096))
    assert ok[starts].all() and np.allclose(prob, p[starts]) and np.all(margin >= 0.0)
    first, last = np.nonzero(ok)[0][[0, -1]]
    s2, _, _ = RR.sample(pri, size, next_idx, S, 0.01 ** 0.7, np.array([0.0, 1.0 - 2.0 ** -53]))
    assert s2[0] == first and s2[1] == last


def test_valid_window_exists_exhaustive():
    from dreamer_amd.buffer import valid_window_exists
    for cap in (1, 2, 5, 9):
        for S in (1, 2, 3, 5, 9, 12):
            for size in range(cap + 1):
                for nxt in range(cap):
                    assert valid_window_exists(size, cap, nxt, S) == bool(RR.valid_mask(cap, size, nxt, S).any()), \
                        (cap, S, size, nxt)


class _NoRedraw:
    """np.random.RandomState whose scalar draws (the reference's redraws of a
    straddling start) come back as -1: what is left are the first draws kept."""

    def __init__(self, seed):
        self.r = np.random.RandomState(seed)

    def randint(self, lo, hi, size=None):
        v = self.r.randint(lo, hi, size=size)
        return v if size is not None else -1


@pytest.mark.parametrize("cap,size,next_idx,S", RINGS[:5])
def test_valid_set_is_what_the_reference_keeps(cap, size, next_idx, S):
    """The starts oracle.replay_starts returns without a redraw, over 1e5 seeded
    draws, are exactly the valid set: the tail zone is never drawn, the
    straddle zone is always redrawn."""
    out = O.replay_starts(size, cap, next_idx, S, 100000, rng=_NoRedraw(7))
    kept = set(int(s) for s in np.unique(out) if s >= 0)
    assert kept == set(int(i) for i in np.nonzero(RR.valid_mask(cap, size, next_idx, S))[0])


def test_update_reference_order_independent():
    g = np.random.RandomState(5)
    starts = g.randint(0, 16, 64)
    scores = g.normal(size=64)
    scores[3], scores[9] = np.nan, np.inf
    p0, v0 = np.full(16, 1e5), np.zeros(16, dtype=np.int64)
    a = RR.update(p0, v0, starts, scores, 1e4, 0.7, 0.7, 0.01, 1e5)
    perm = g.permutation(64)
    b = RR.update(p0, v0, starts[perm], scores[perm], 1e4, 0.7, 0.7, 0.01, 1e5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[1].sum() == 64 and a[0][starts[3]] == 1e5 and a[0][starts[9]] == 1e5


@pytest.mark.parametrize("bad", [dict(replay="prioritised"), dict(replay="curious", replay_beta=0.0),
                                 dict(replay="curious", replay_beta=1.5), dict(replay="curious", replay_alpha=0.0),
                                 dict(replay="curious", replay_eps=0.0), dict(replay="curious", replay_c=-1.0),
                                 dict(replay="curious", replay_p_new=0.0), dict(replay_beta=float("nan"))])
def test_config_validation(bad):
    from dreamer_amd import Dreamer
    cfg = dict(SMALL)
    cfg.update(bad)
    with pytest.raises(ValueError):
        Dreamer(cfg, "cpu")


def test_config_defaults_and_keys():
    from dreamer_amd import Dreamer
    d = Dreamer(dict(SMALL), "cpu")
    b = d.buffer
    assert (b.replay, b.replay_c, b.replay_beta, b.replay_alpha, b.replay_eps, b.replay_p_new) == \
        ("uniform", 1e4, 0.7, 0.7, 0.01, 1e5)
    d = Dreamer(dict(SMALL, replay="curious", replay_beta=1.0, replay_c=0.0, replay_p_new=10.0), "cpu")
    assert (d.buffer.replay, d.buffer.replay_beta, d.buffer.replay_c, d.buffer.replay_p_new) == \
        ("curious", 1.0, 0.0, 10.0)


def test_cpu_buffer_in_curious_mode_raises():
    from dreamer_amd.buffer import Buffer
    b = Buffer(64, 8, 3, (32, 32), device="cpu")
    b.replay = "curious"
    for _ in range(16):
        b.add_to_buffer(np.zeros((3, 32, 32), np.uint8), np.zeros(3, np.float32), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="the replay device mirror needs a GPU device"):
        b._mirror()
    for call in (lambda: b.sample_start_indices_device(4), lambda: b.sampling_probabilities(),
                 lambda: b.update_priorities(torch.zeros(4, dtype=torch.int64), torch.zeros(4))):
        with pytest.raises(RuntimeError, match="the replay device mirror needs a GPU device"):
            call()
    assert b._dev is None
    # the uniform sampler is untouched by the mode
    np.random.seed(0)
    a = b.sample_start_indices(8)
    np.random.seed(0)
    assert np.array_equal(a, O.replay_starts(b.size, b.capacity, b.next_idx, 8, 8))


def test_uniform_mode_needs_the_mode_for_the_device_sampler():
    from dreamer_amd.buffer import Buffer
    b = Buffer(64, 8, 3, (32, 32), device="cpu")
    with pytest.raises(RuntimeError, match="replay = 'curious'"):
        b.sample_start_indices_device(4)


class _HostRng:
    def __init__(self):
        self.state, self.counter = torch.zeros(2, dtype=torch.int64), 0


def test_uniform_training_state_keys_unchanged(monkeypatch):
    """Uniform mode: training_state() has exactly the parent's keys (the two
    Philox generators are stood in for by host tensors: no GPU here)."""
    from dreamer_amd import Dreamer, hip
    monkeypatch.setattr(hip, "rng", lambda dev: _HostRng())
    monkeypatch.setattr(hip, "adhoc", lambda dev: _HostRng())
    d = Dreamer(dict(SMALL), "cpu")
    st = d.training_state()
    assert set(st) == PARENT_STATE_KEYS
    assert set(st["buffer"]) == PARENT_BUFFER_KEYS
    assert st["format"] == "dreamer_amd.training_state.v1"
    assert d.buffer._dev is None
