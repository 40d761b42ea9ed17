"""Episode-aware replay on the GPU against the numpy reference
(tests/episodes_ref.py): the span pass, the masked draws with priorities, with
none and with Philox, Dreamer end to end, vector rollouts and resume.  Run on
the MI355X box: pytest -m gpu.

Tolerances.  Spans and the valid-start count are integers: exact.  With
priorities, starts are exact wherever the reference's margin to the nearest
running-sum boundary is >= 1e-9 of W (the kernel's float64 sums differ from
np.cumsum's only by their order, at most cap 2^-53 = 1.5e-11 relative at
cap = 131072), and at most B // 100 draws may sit closer (the reference alone
meets that cap: test_episodes_host.py).  Without priorities the sums are exact
integers: every start is exact, with no margin.  Probabilities are an f32
rounding of an f64 quotient: 1e-6 relative; without priorities the quotient is
1 / n_valid and the rounding is the reference's own."""
import numpy as np
import pytest
import torch
from scipy import stats

import episodes_ref as ER
import replay_ref as RR
from conftest import fixture_params, load_fixture
from formula import SMALL, replay_data

pytestmark = pytest.mark.gpu
P_MIN = 1e-4  # tests/test_gpu_noise.py
P_FLOOR = 0.01 ** 0.7
MARGIN = 1e-9


def _lib():
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    return L, hip


def _spans(gpu, cont, first, size, next_idx, S):
    """dr_replay_spans on bare arrays: (span int32 [cap], n_valid) as numpy / int."""
    L, hip = _lib()
    cap = len(cont)
    ct = torch.from_numpy(np.asarray(cont, dtype=np.float32)).to(gpu)
    fr = None if first is None else torch.from_numpy(np.asarray(first, dtype=np.uint8)).to(gpu)
    span = torch.full((cap,), -7, dtype=torch.int32, device=gpu)
    n = torch.full((1,), -7, dtype=torch.int64, device=gpu)
    ws = torch.empty(max(8, L.query("dr_replay_spans_workspace_bytes", cap)), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_spans", cap, size, next_idx, L.ptr(ct), L.ptr(fr), S, L.ptr(span), L.ptr(n), L.ptr(ws),
           ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return span.cpu().numpy(), int(n.item())


def _sample(gpu, pri, span, size, next_idx, S, u):
    """dr_replay_sample_spans with explicit uniforms (pri None: no priorities): (starts, prob) as numpy."""
    L, hip = _lib()
    cap, B = len(span), len(u)
    p = None if pri is None else torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(gpu)
    sp = torch.from_numpy(np.array(span, dtype=np.int32)).to(gpu)
    ud = torch.from_numpy(np.asarray(u, dtype=np.float64)).to(gpu)
    starts = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    prob = torch.full((B,), -1.0, device=gpu)
    ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_sample_spans", cap, size, next_idx, S, B, L.ptr(p), P_FLOOR, L.ptr(sp), L.ptr(ud), None, 0,
           L.ptr(starts), L.ptr(prob), L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return starts.cpu().numpy(), prob.cpu().numpy()


def _probabilities(gpu, pri, span, size, next_idx, S):
    L, hip = _lib()
    cap = len(span)
    p = None if pri is None else torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(gpu)
    sp = torch.from_numpy(np.array(span, dtype=np.int32)).to(gpu)
    out = torch.full((cap,), -1.0, device=gpu)
    ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_probabilities_spans", cap, size, next_idx, S, L.ptr(p), P_FLOOR, L.ptr(sp), L.ptr(out),
           L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


_REF = {}


def _ref(name):
    """The named case with its reference spans, computed once and shared."""
    if name not in _REF:
        c = ER.case(name)
        c["span"] = ER.spans_fast(c["cont"], c["first"], c["size"], c["next_idx"])
        c["span"].setflags(write=False)
        _REF[name] = c
    return _REF[name]


# ---- 1. spans ----------------------------------------------------------------
@pytest.mark.parametrize("name", ER.NAMES)
def test_spans(name, gpu):
    c = _ref(name)
    cap, size, nxt, S = c["cap"], c["size"], c["next_idx"], c["S"]
    span, n = _spans(gpu, c["cont"], c["first"], size, nxt, S)
    bad = np.nonzero(span != c["span"])[0]
    assert bad.size == 0, (bad[:8], span[bad[:8]], c["span"][bad[:8]])
    assert n == int((c["span"] >= S).sum())
    span2, n2 = _spans(gpu, c["cont"], c["first"], size, nxt, S)
    assert np.array_equal(span, span2) and n == n2
    # first = NULL is an all-zero first
    zero = np.zeros(cap, dtype=np.uint8)
    a, na = _spans(gpu, c["cont"], None, size, nxt, S)
    b, nb = _spans(gpu, c["cont"], zero, size, nxt, S)
    assert np.array_equal(a, b) and na == nb
    assert np.array_equal(a, ER.spans_fast(c["cont"], None, size, nxt))


def test_spans_n_valid_is_optional(gpu):
    L, hip = _lib()
    c = _ref("cap3000")
    ct = torch.from_numpy(c["cont"]).to(gpu)
    fr = torch.from_numpy(c["first"]).to(gpu)
    span = torch.zeros(c["cap"], dtype=torch.int32, device=gpu)
    ws = torch.empty(L.query("dr_replay_spans_workspace_bytes", c["cap"]), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_spans", c["cap"], c["size"], c["next_idx"], L.ptr(ct), L.ptr(fr), c["S"], L.ptr(span), None,
           L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    assert np.array_equal(span.cpu().numpy(), c["span"])
    with pytest.raises(L.HipError):  # a workspace one byte short
        L.call("dr_replay_spans", c["cap"], c["size"], c["next_idx"], L.ptr(ct), L.ptr(fr), c["S"], L.ptr(span), None,
               L.ptr(ws), ws.numel() - 1, hip.stream())
    with pytest.raises(L.HipError):  # next_idx outside the ring
        L.call("dr_replay_spans", c["cap"], c["size"], c["cap"], L.ptr(ct), L.ptr(fr), c["S"], L.ptr(span), None,
               L.ptr(ws), ws.numel(), hip.stream())


# ---- 2. no break: the bits of the unmasked entry points ------------------------
@pytest.mark.parametrize("name", ER.DRAWABLE)
def test_no_break_equals_unmasked_sampler(name, gpu):
    import test_gpu_replay_priority as TP
    c = ER.case(name, breaks=False)
    cap, size, nxt, S = c["cap"], c["size"], c["next_idx"], c["S"]
    span, _ = _spans(gpu, c["cont"], c["first"], size, nxt, S)
    s0, p0 = TP._sample(gpu, c["pri"], size, nxt, S, c["u"])
    s1, p1 = _sample(gpu, c["pri"], span, size, nxt, S, c["u"])
    assert np.array_equal(s0, s1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    q0 = TP._probabilities(gpu, c["pri"], size, nxt, S)
    q1 = _probabilities(gpu, c["pri"], span, size, nxt, S)
    assert np.array_equal(q0.view(np.uint32), q1.view(np.uint32))


# ---- 3. prioritised draws ------------------------------------------------------
@pytest.mark.parametrize("name", ER.DRAWABLE)
def test_prioritised_draws(name, gpu):
    c = _ref(name)
    size, nxt, S, B, u, pri = c["size"], c["next_idx"], c["S"], c["B"], c["u"], c["pri"]
    ref_s, ref_p, margin = ER.sample(pri, c["span"], S, P_FLOOR, u)
    keep = margin >= MARGIN
    print(f"{name}: {int((~keep).sum())} of {B} draws within {MARGIN} of a boundary (left out)")
    assert (~keep).sum() <= B // 100
    s, p = _sample(gpu, pri, c["span"], size, nxt, S, u)
    assert (c["span"][s] >= S).all(), "a start with span < S was drawn"
    assert np.array_equal(s[keep], ref_s[keep]), f"{int((s[keep] != ref_s[keep]).sum())} starts differ"
    rel = np.abs(p[keep] - ref_p[keep]) / ref_p[keep]
    print(f"{name}: prob worst relative error {rel.max():.3g}")
    assert rel.max() <= 1e-6
    first, last = np.nonzero(c["span"] >= S)[0][[0, -1]]
    se, _ = _sample(gpu, pri, c["span"], size, nxt, S, np.array([0.0, 1.0 - 2.0 ** -53]))
    assert se[0] == first and se[1] == last, (se, first, last)
    pr = _probabilities(gpu, pri, c["span"], size, nxt, S)
    ref = ER.probabilities(pri, c["span"], S, P_FLOOR)
    assert np.all(pr[ref == 0.0] == 0.0)
    assert (np.abs(pr - ref)[ref > 0] / ref[ref > 0]).max() <= 1e-6


# ---- 4. draws without priorities ------------------------------------------------
@pytest.mark.parametrize("name", ER.DRAWABLE)
def test_uniform_draws(name, gpu):
    c = _ref(name)
    size, nxt, S = c["size"], c["next_idx"], c["S"]
    ok = c["span"] >= S
    n = int(ok.sum())
    u = np.concatenate([c["u"], [0.0, 1.0 - 2.0 ** -53], np.arange(0, n, max(1, n // 64)) / n])  # on the boundaries too
    ref_s, ref_p, _ = ER.sample(None, c["span"], S, P_FLOOR, u)
    s, p = _sample(gpu, None, c["span"], size, nxt, S, u)
    assert np.array_equal(s, ref_s), f"{int((s != ref_s).sum())} starts differ"
    assert ok[s].all()
    assert np.all(p == np.float32(1.0 / n))
    pr = _probabilities(gpu, None, c["span"], size, nxt, S)
    assert np.all(pr[ok] == np.float32(1.0 / n)) and np.all(pr[~ok] == 0.0)


def test_no_valid_start(gpu):
    """size < S: the kernel answers start 0, prob 0; the Buffer refuses before any launch -- also where there is
    data for a window but every window holds a break."""
    from dreamer_amd.buffer import Buffer
    c = _ref("size_below_S")
    s, p = _sample(gpu, c["pri"], c["span"], c["size"], c["next_idx"], c["S"], c["u"][:16])
    assert np.all(s == 0) and np.all(p == 0.0)
    b = Buffer(64, 8, 3, (32, 32), device=gpu)
    b.replay_episodes = "respect"
    cont = np.ones(64, np.float32)
    cont[::4] = 0.0
    b.load_arrays(np.zeros((64, 3, 32, 32), np.uint8), np.zeros((64, 3), np.float32), np.zeros(64, np.float32), cont)
    assert b.valid_start_count() == 0 and int(b.window_spans().max()) == 4
    for call in (lambda: b.sample_start_indices_device(4), b.sampling_probabilities, lambda: b.sample_eval_starts(4)):
        with pytest.raises(ValueError, match="Not enough data in buffer to sample a full sequence"):
            call()


# ---- 5. Philox ----------------------------------------------------------------
def _buffer(gpu, c, replay="uniform"):
    """A respecting Buffer holding the case's ring."""
    from dreamer_amd.buffer import Buffer
    cap, n = c["cap"], c["size"]
    b = Buffer(cap, c["S"], 3, (32, 32), device=gpu)
    b.replay, b.replay_episodes = replay, "respect"
    b.load_arrays(np.zeros((n, 3, 32, 32), np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.float32),
                  c["cont"][:n], first=c["first"][:n])
    b.next_idx = c["next_idx"]
    return b


def test_philox_draws(gpu):
    _, hip = _lib()
    c = _ref("cap3000")
    b = _buffer(gpu, c)
    N = 65536
    ar = hip.adhoc(gpu)
    ar.reseed(0xE915)
    state, counter = ar.state.clone(), ar.counter
    before = np.random.get_state()
    s1, p1 = b.sample_start_indices_device(N)
    s2, _ = b.sample_start_indices_device(N)
    ar.state.copy_(state)
    ar.counter = counter
    s3, _ = b.sample_start_indices_device(N)
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2], "nothing is drawn from np.random"
    assert set(b._dev) == {"frames", "actions", "rewards", "continues", "first", "span", "n_valid"}
    assert torch.equal(s1, s3) and not torch.equal(s1, s2)
    assert np.array_equal(b.window_spans().cpu().numpy(), c["span"])
    ok = c["span"] >= c["S"]
    n = int(ok.sum())
    assert b.valid_start_count() == n
    s = s1.cpu().numpy()
    assert ok[s].all(), "a start with span < S was drawn"
    assert np.all(p1.cpu().numpy() == np.float32(1.0 / n))
    groups = np.array_split(np.nonzero(ok)[0], 64)  # 64 bins of (all but) equal count
    label = np.full(c["cap"], -1)
    for k, gr in enumerate(groups):
        label[gr] = k
    obs = np.bincount(label[s], minlength=64).astype(np.float64)
    exp = np.array([len(gr) for gr in groups], dtype=np.float64) * N / n
    chi = float(((obs - exp) ** 2 / exp).sum())
    p_chi = float(stats.chi2.sf(chi, 63))
    print(f"philox, no priorities: chi2 {chi:.1f} on 63 dof (p = {p_chi:.3g}), {n} valid starts of {c['cap']}")
    assert p_chi >= P_MIN, chi


# ---- 6. end to end ----------------------------------------------------------------
E2E = dict(buffer_size=256, batch_size=8, sequence_length=8, horizon=5, WM_epochs=3, AC_epochs=2)


def _dreamer(gpu, **kw):
    from dreamer_amd import Dreamer
    cfg = dict(SMALL)
    cfg.update(E2E)
    cfg.update(kw)
    torch.manual_seed(0)
    d = Dreamer(cfg, gpu)
    P = fixture_params("small", load_fixture("small_epoch"))
    d.load_state_dict({k: v.to(gpu) for k, v in P.items()})
    fr, ac, rw, _ = replay_data(256, (32, 32), 3, seed=11)
    cont, first = ER.broken_ring(np.random.RandomState(77), 256, 8)
    d.buffer.load_arrays(fr, ac, rw, cont, first=first)
    return d


def _check_windows(buf, starts, S):
    cont, first = buf.continue_buffer[:, 0], buf.first_buffer
    for i in np.asarray(starts).reshape(-1):
        assert i + S <= buf.capacity
        assert np.all(cont[i:i + S - 1] >= 0.5), f"window {i} holds a terminal before its last slot"
        assert not first[i + 1:i + S].any(), f"window {i} runs into a new stream"


@pytest.mark.parametrize("replay", ["uniform", "curious"])
def test_respect_end_to_end(replay, gpu):
    _, hip = _lib()
    d = _dreamer(gpu, replay=replay, replay_episodes="respect")
    buf, S = d.buffer, E2E["sequence_length"]
    hip.adhoc(gpu).reseed(0xC0FFEE)
    ref_span = ER.spans_fast(buf.continue_buffer[:, 0], buf.first_buffer, buf.size, buf.next_idx)
    old = int(RR.valid_mask_fast(256, buf.size, buf.next_idx, S).sum())
    assert 0 < (ref_span >= S).sum() < old, "the ring must have breaks for the check to mean something"
    log = []
    draw = buf.sample_start_indices_device

    def recording(batch_size, u=None):
        out = draw(batch_size, u)
        log.append(out[0].clone())
        return out

    buf.sample_start_indices_device = recording
    np_state = np.random.get_state()
    if replay == "curious":
        pri0 = buf._mirror()["priority"].clone()
    losses = d.train_world_model()
    n_wm = len(log)
    la, lc = d.train_Agent()
    buf.sample_start_indices_device = draw
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert np.array_equal(np_state[1], after[1]) and np_state[2] == after[2], "respect mode draws nothing from np.random"
    assert n_wm == E2E["WM_epochs"] and len(log) == n_wm + E2E["AC_epochs"]
    assert all(torch.isfinite(x) for x in losses) and np.isfinite(float(la)) and np.isfinite(float(lc))
    assert np.array_equal(buf.window_spans().cpu().numpy(), ref_span)
    assert buf.valid_start_count() == int((ref_span >= S).sum())
    for st in log:
        assert tuple(st.shape) == (E2E["batch_size"],)
        _check_windows(buf, st.cpu().numpy(), S)
    m = buf._mirror()
    if replay == "curious":
        seen = torch.cat(log[:n_wm]).unique()
        assert bool((m["priority"][seen] != pri0[seen]).all()), "the visited slots' priorities changed"
        assert int(m["visits"].sum()) == n_wm * E2E["batch_size"]
    else:
        assert "priority" not in m and d.world_model.last_window_scores is None

    # evaluation: unweighted device draws among the valid windows, random state left as found
    ev = []
    draw_eval = buf.sample_eval_starts

    def recording_eval(n):
        ev.append(draw_eval(n))
        return ev[-1]

    buf.sample_eval_starts = recording_eval
    ar = hip.adhoc(gpu)
    np_state, state, counter = np.random.get_state(), ar.state.clone(), ar.counter
    curves = d.evaluate_world_model(batches=2, context=3, horizon=4)
    buf.sample_eval_starts = draw_eval
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert np.array_equal(np_state[1], after[1]) and np_state[2] == after[2]
    assert torch.equal(ar.state, state) and ar.counter == counter
    assert len(ev) == 2 and all(e.is_cuda and e.dtype == torch.int64 for e in ev)
    for e in ev:
        _check_windows(buf, e.cpu().numpy(), S)
    assert curves


def test_ignore_mode_has_no_episode_state(gpu):
    """Key absent: no first or span tensor on the device, first flags in the data or not."""
    d = _dreamer(gpu)
    assert d.buffer.replay_episodes == "ignore" and d.buffer.first_buffer.any()
    np.random.seed(5)
    d.train_world_model()
    d.train_Agent()
    torch.cuda.synchronize()
    assert set(d.buffer._dev) == {"frames", "actions", "rewards", "continues"}
    assert set(d.training_state()["buffer"]) == {"obs", "act", "rew", "cont", "next_idx", "size"}
    with pytest.raises(RuntimeError, match="replay = 'curious'"):
        d.buffer.sample_start_indices_device(4)


# ---- 7. vector rollouts -------------------------------------------------------------
def test_rollout_policy_vec_marks_blocks(gpu):
    from test_gpu_act_batch import SeededEnv
    from test_gpu_act_batch import _dreamer as full_dreamer
    S, N = 8, 2
    d, _ = full_dreamer(gpu, formula=False, sequence_length=S, buffer_size=64, replay_episodes="respect")
    envs = [SeededEnv(space_seed=20 + e) for e in range(N)]
    d.seed = 47  # SeededEnv: episodes of 3 + seed % 7 steps, so the first two last 8 and 9: their blocks are whole
    d.rollout_policy_vec(envs, random_policy=True)
    d.rollout_policy_vec(envs, random_policy=True)
    d.act_check()
    buf = d.buffer
    assert buf.size == 2 * N * S
    want = np.zeros(64, dtype=np.uint8)
    want[np.arange(0, 2 * N * S, S)] = 1
    assert np.array_equal(buf.first_buffer, want), "the first slot of each block carries first, no other slot"
    span = buf.window_spans().cpu().numpy()
    assert np.array_equal(span, ER.spans_fast(buf.continue_buffer[:, 0], buf.first_buffer, buf.size, buf.next_idx))
    valid = np.nonzero(span >= S)[0]
    assert np.all(valid % S == 0), "blocks of exactly S: only block-aligned starts remain"
    assert buf.valid_start_count() == len(valid) >= 2
    cont = buf.continue_buffer[:2 * N * S, 0].reshape(2 * N, S)
    assert len(valid) == int((cont[:, :-1] >= 0.5).all(1).sum()), "a block with no done before its last step is valid"
    # one env: nothing is flagged (the continue = 0 of the previous slot marks the break)
    d1, _ = full_dreamer(gpu, formula=False, sequence_length=S, buffer_size=64, replay_episodes="respect")
    d1.rollout_policy_vec([SeededEnv(space_seed=20)], random_policy=True)
    d1.act_check()
    assert d1.buffer.size == S and not d1.buffer.first_buffer.any()


# ---- 8. resume ----------------------------------------------------------------
def test_resume_in_respect_mode(gpu, tmp_path):
    _, hip = _lib()
    d = _dreamer(gpu, replay="curious", replay_episodes="respect")
    hip.adhoc(gpu).reseed(0xBEEF)
    hip.rng(gpu).reseed(0xFEED)
    d.train_world_model()
    path = tmp_path / "state.pt"
    d.save_training_state(path)
    st = torch.load(path, weights_only=True)
    assert set(st["buffer"]) == {"obs", "act", "rew", "cont", "next_idx", "size", "priority", "visits", "first"}
    assert np.array_equal(st["buffer"]["first"].numpy(), d.buffer.first_buffer)
    want = [x.clone() for x in d.train_world_model()] + [x.clone() for x in d.train_Agent()]
    s_want, _ = d.buffer.sample_start_indices_device(8)
    d2 = _dreamer(gpu, replay="curious", replay_episodes="respect")
    d2.buffer.first_buffer[:] = 0  # what the file holds must come back
    d2.load_training_state(path)
    assert np.array_equal(d2.buffer.first_buffer, d.buffer.first_buffer)
    got = [x.clone() for x in d2.train_world_model()] + [x.clone() for x in d2.train_Agent()]
    s_got, _ = d2.buffer.sample_start_indices_device(8)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b), "the resumed run must continue bit for bit"
    assert torch.equal(s_want, s_got)
    assert torch.equal(d2.buffer.window_spans(), d.buffer.window_spans())
    # a state saved without first flags is refused
    plain = _dreamer(gpu, replay="curious")
    plain.save_training_state(tmp_path / "plain.pt")
    with pytest.raises(ValueError, match="first"):
        d2.load_training_state(tmp_path / "plain.pt")
