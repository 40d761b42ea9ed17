"""Episode-aware replay, the parts that need no GPU: the reference's own
invariants (tests/episodes_ref.py) on the rings the GPU test uses, the Buffer's
host API, the config validation, the untouched np.random consumption of ignore
mode and the header / binding agreement."""
import os
import re

import numpy as np
import pytest
import torch

import episodes_ref as ER
import replay_ref as RR
from conftest import REPO
from formula import SMALL
from oracle import dreamer_oracle as O

P_FLOOR = 0.01 ** 0.7
MARGIN = 1e-9
NEW_SYMBOLS = {"dr_replay_spans", "dr_replay_spans_workspace_bytes", "dr_replay_sample_spans",
               "dr_replay_probabilities_spans"}


@pytest.mark.parametrize("name", ER.NAMES)
def test_reference_spans(name):
    c = ER.case(name)
    cap, size, nxt, S = c["cap"], c["size"], c["next_idx"], c["S"]
    fast = ER.spans_fast(c["cont"], c["first"], size, nxt)
    if cap <= 10007:
        assert np.array_equal(fast, ER.spans(c["cont"], c["first"], size, nxt)), "loop per slot vs vectorised"
    old = RR.valid_mask_fast(cap, size, nxt, S)
    new = fast >= S
    assert not (new & ~old).any(), "span >= S must be a subset of the valid starts of prioritised replay"
    assert np.all(fast[size:] == 0) and np.all(fast[:size] >= 1)
    if name == "size_below_S":  # the old rule allows no start either: nothing to remove
        assert not old.any() and not new.any()
    elif name != ER.NAMES[0]:
        assert (old & ~new).sum() >= 1, "the breaks must remove a start the old rule allows"
    if name == "cap5000_one_break":
        assert fast[1] == 4500 and fast[0] == 1 and fast[4501] == 499
    # without breaks the rule is exactly the old one (first = None is all 0)
    plain = ER.case(name, breaks=False)
    for first in (plain["first"], None):
        assert np.array_equal(ER.spans_fast(plain["cont"], first, size, nxt) >= S, old)
    # a window drawn by the new rule: continue >= 0.5 before its last slot, no first flag after its first
    for i in np.nonzero(new)[0][:: max(1, int(new.sum()) // 200)]:
        assert np.all(c["cont"][i:i + S - 1] >= 0.5) and not c["first"][i + 1:i + S].any()


@pytest.mark.parametrize("cap,size,nxt", [(64, 64, 0), (64, 64, 1), (64, 64, 30), (64, 40, 40), (64, 8, 8),
                                          (1025, 1025, 0), (1025, 1025, 1), (1025, 1025, 600), (1025, 700, 700)])
def test_no_break_is_the_old_rule(cap, size, nxt):
    for S in (1, 2, 8, 16):
        sp = ER.spans_fast(np.ones(cap, np.float32), None, size, nxt)
        assert np.array_equal(sp, ER.spans(np.ones(cap, np.float32), None, size, nxt))
        assert np.array_equal(sp >= S, RR.valid_mask_fast(cap, size, nxt, S)), (cap, size, nxt, S)


@pytest.mark.parametrize("name", ER.DRAWABLE)
def test_reference_draws_and_left_out_cap(name):
    """The masked reference draws only valid starts, and on the GPU test's own
    priorities and uniforms at most B // 100 draws sit within 1e-9 of a
    running-sum boundary (the draws that test leaves out)."""
    c = ER.case(name)
    S, B = c["S"], c["B"]
    sp = ER.spans_fast(c["cont"], c["first"], c["size"], c["next_idx"])
    ok = sp >= S
    starts, prob, margin = ER.sample(c["pri"], sp, S, P_FLOOR, c["u"])
    left = int((margin < MARGIN).sum())
    print(f"{name}: {left} of {B} draws within {MARGIN} of a boundary (cap {B // 100})")
    assert left <= B // 100
    assert ok[starts].all()
    p = ER.probabilities(c["pri"], sp, S, P_FLOOR)
    assert abs(p.sum() - 1.0) < 1e-12 and np.all(p[~ok] == 0.0) and np.allclose(prob, p[starts])
    first, last = np.nonzero(ok)[0][[0, -1]]
    ends, _, _ = ER.sample(c["pri"], sp, S, P_FLOOR, np.array([0.0, 1.0 - 2.0 ** -53]))
    assert ends[0] == first and ends[1] == last
    # no priorities: exact integer sums, the start is the floor(u n)-th valid slot
    su, pu, _ = ER.sample(None, sp, S, P_FLOOR, c["u"])
    n = int(ok.sum())
    assert np.array_equal(su, np.nonzero(ok)[0][np.minimum(np.floor(c["u"] * n).astype(np.int64), n - 1)])
    assert np.all(pu == 1.0 / n)


def _frame():
    return np.zeros((3, 32, 32), np.uint8), np.zeros(3, np.float32)


def test_buffer_records_first():
    from dreamer_amd.buffer import Buffer
    b = Buffer(16, 4, 3, (32, 32), device="cpu")
    assert b.replay_episodes == "ignore" and b.first_buffer.dtype == np.uint8 and b.first_buffer.shape == (16,)
    f, a = _frame()
    b.add_to_buffer(f, a, 0.5, 1.0)  # the reference's four positional arguments
    b.add_to_buffer(f, a, 0.5, 1.0, first=True)
    b.add_to_buffer(f, a, 0.5, 1.0, True)
    b.add_to_buffer(f, a, 0.5, 0.0, first=False)
    assert b.first_buffer[:5].tolist() == [0, 1, 1, 0, 0] and b._dirty == [0, 1, 2, 3]
    for _ in range(13):  # wraps: slot 0 is overwritten with first = True
        b.add_to_buffer(f, a, 0.5, 1.0, first=True)
    assert b.next_idx == 1 and b.first_buffer[0] == 1 and b.first_buffer[1] == 1
    b.add_to_buffer(f, a, 0.5, 1.0)
    assert b.first_buffer[1] == 0, "a slot written without the flag loses the old one"
    n = 8
    args = (np.zeros((n, 3, 32, 32), np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.float32),
            np.ones(n, np.float32))
    b.load_arrays(*args, first=np.arange(n) % 3 == 0)
    assert b.first_buffer[:n].tolist() == [1, 0, 0, 1, 0, 0, 1, 0]
    b.load_arrays(*args)
    assert not b.first_buffer[:n].any()


def test_config_validation_and_default():
    from dreamer_amd import Dreamer
    assert Dreamer(dict(SMALL), "cpu").buffer.replay_episodes == "ignore"
    assert Dreamer(dict(SMALL, replay_episodes="respect"), "cpu").buffer.replay_episodes == "respect"
    d = Dreamer(dict(SMALL, replay_episodes="respect", replay="curious"), "cpu")
    assert (d.buffer.replay, d.buffer.replay_episodes) == ("curious", "respect")
    for bad in ("Respect", "reset", "", None, True):
        with pytest.raises(ValueError, match="replay_episodes"):
            Dreamer(dict(SMALL, replay_episodes=bad), "cpu")


def test_ignore_mode_draws_as_before():
    """Ignore mode: sample_start_indices and sample_eval_starts consume np.random
    as the reference formula does, first flags or not; no device state appears."""
    from dreamer_amd.buffer import Buffer
    b = Buffer(64, 8, 3, (32, 32), device="cpu")
    f, a = _frame()
    for t in range(64 + 20):
        b.add_to_buffer(f, a, 0.0, float(t % 9 != 0), first=t % 11 == 0)
    for draw in (b.sample_start_indices, b.sample_eval_starts):
        np.random.seed(3)
        got = draw(16)
        after = np.random.get_state()
        np.random.seed(3)
        want = O.replay_starts(b.size, b.capacity, b.next_idx, 8, 16)
        assert np.array_equal(got, want)
        ref = np.random.get_state()
        assert np.array_equal(after[1], ref[1]) and after[2] == ref[2]
    assert b._dev is None
    with pytest.raises(RuntimeError, match="replay_episodes = 'respect'"):
        b.window_spans()
    with pytest.raises(RuntimeError, match="replay_episodes = 'respect'"):
        b.valid_start_count()


def test_respect_mode_needs_a_gpu():
    from dreamer_amd.buffer import Buffer
    b = Buffer(64, 8, 3, (32, 32), device="cpu")
    b.replay_episodes = "respect"
    f, a = _frame()
    for _ in range(16):
        b.add_to_buffer(f, a, 0.0, 1.0)
    for call in (lambda: b.sample_start_indices_device(4), lambda: b.sampling_probabilities(),
                 lambda: b.sample_eval_starts(4), lambda: b.window_spans(), lambda: b.valid_start_count()):
        with pytest.raises(RuntimeError, match="the replay device mirror needs a GPU device"):
            call()
    with pytest.raises(RuntimeError, match="replay = 'curious'"):
        b.update_priorities(torch.zeros(4, dtype=torch.int64), torch.zeros(4))  # stays curious-only
    assert b._dev is None


def test_respect_refuses_data_parallelism():
    from dreamer_amd import Dreamer
    d = Dreamer(dict(SMALL, replay_episodes="respect"), "cpu")
    d.world = (0, 2, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_world_model()
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()


def test_header_declares_what_the_binding_binds():
    from dreamer_amd import _lib
    src = open(os.path.join(REPO, "include", "dreamer_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dr_[A-Za-z0-9_]+)\s*\(", src))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.EXPORTED)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    # the argument counts of the declarations and of the ctypes signatures agree
    for s in NEW_SYMBOLS:
        args = re.search(r"\b" + s + r"\s*\(([^)]*)\)", src).group(1)
        assert len(args.split(",")) == len(_lib._SIGS[s][1]), s
    assert _lib.query("dr_replay_spans_workspace_bytes", 1) >= 8
    assert _lib.query("dr_replay_spans_workspace_bytes", 131072) >= 128 * 2 * 4
    assert _lib.query("dr_replay_spans_workspace_bytes", 0) == 0
