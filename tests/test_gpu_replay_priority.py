"""Prioritised ("curious") replay on the GPU against the float64 reference
(tests/replay_ref.py): the device sampler with explicit uniforms and with
Philox, the per-slot probabilities, the priority update, the per-window scores
of a world-model step and Dreamer end to end.  Run on the MI355X box:
pytest -m gpu.

Tolerances.  Starts are exact wherever the reference's margin to the nearest
running-sum boundary is >= 1e-9 of W: the kernel's float64 sums differ from
np.cumsum's only by their order, at most cap 2^-53 = 1.5e-11 relative at
cap = 131072 (60x below).  Probabilities are an f32 rounding of an f64
quotient: 1e-6 relative.  The updated priority is the float64 formula rounded
to f32 once: 1e-5 relative allows a few tens of f32 ulps.  Window scores hold
the step's own bound, 1e-4 max(1, |ref|) (test_wm_step_matches_reference)."""
import numpy as np
import pytest
import torch
from scipy import stats

import replay_ref as RR
from conftest import fixture_params, load_fixture
from formula import SMALL, replay_data
from gpu_helpers import build, cpu
from oracle import dreamer_oracle as O
from test_oracle_wm import window

pytestmark = pytest.mark.gpu
P_MIN = 1e-4  # tests/test_gpu_noise.py
P_FLOOR = 0.01 ** 0.7
MARGIN = 1e-9
CONSTS = (1e4, 0.7, 0.7, 0.01, 1e5)  # c, beta, alpha, eps, p_new


def _lib():
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    return L, hip


def _sample(gpu, pri, size, next_idx, S, u, p_floor=P_FLOOR):
    """dr_replay_sample on a bare priority array with explicit uniforms: (starts, prob) as numpy."""
    L, hip = _lib()
    cap, B = len(pri), len(u)
    p = torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(gpu)
    ud = torch.from_numpy(np.asarray(u, dtype=np.float64)).to(gpu)
    starts = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    prob = torch.full((B,), -1.0, device=gpu)
    ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_sample", cap, size, next_idx, S, B, L.ptr(p), p_floor, L.ptr(ud), None, 0, L.ptr(starts),
           L.ptr(prob), L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return starts.cpu().numpy(), prob.cpu().numpy()


def _log_uniform(g, n, lo, hi):
    return np.exp(g.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


def _dynamic_range_case(g, cap, next_idx, S, B):
    """One slot holds 1e5, the rest 0.01 .. 0.05; half the uniforms fall in the
    low-priority mass before the big slot, half in the mass after it."""
    pri = g.uniform(0.01, 0.05, cap).astype(np.float32)
    big = 50000
    pri[big] = 1e5
    C = np.cumsum(RR.weights(pri, cap, next_idx, S, P_FLOOR))
    lo_end, hi_start = C[big - 1] / C[-1], C[big] / C[-1]
    u = np.concatenate([g.uniform(0.0, lo_end, B // 2), hi_start + g.uniform(0.0, 1.0, B // 2) * (1.0 - hi_start)])
    return pri, u, big


# cap, size, next_idx, S, B, seed
SAMPLER_CASES = [(64, 40, 40, 8, 256, 1), (64, 64, 20, 8, 256, 2), (64, 64, 3, 8, 256, 3), (64, 64, 0, 8, 256, 4),
                 (10007, 10007, 5000, 16, 256, 5), (131072, 131072, 70000, 16, 4096, 6)]


@pytest.mark.parametrize("cap,size,next_idx,S,B,seed", SAMPLER_CASES, ids=[f"cap{c[0]}_next{c[2]}_size{c[1]}"
                                                                           for c in SAMPLER_CASES])
def test_sampler_explicit_uniforms(cap, size, next_idx, S, B, seed, gpu):
    g = np.random.RandomState(seed)
    if cap == 131072:
        pri, u, big = _dynamic_range_case(g, cap, next_idx, S, B)
    else:
        pri, u = _log_uniform(g, cap, 0.04, 1e5), g.uniform(size=B)
    ref_s, ref_p, margin = RR.sample(pri, size, next_idx, S, P_FLOOR, u)
    keep = margin >= MARGIN
    print(f"cap {cap}: {int((~keep).sum())} of {B} draws within {MARGIN} of a boundary (left out)")
    assert (~keep).sum() <= B // 100
    s, p = _sample(gpu, pri, size, next_idx, S, u)
    ok = RR.valid_mask_fast(cap, size, next_idx, S)
    assert ok[s].all(), "an invalid start was drawn"
    assert np.array_equal(s[keep], ref_s[keep]), f"{int((s[keep] != ref_s[keep]).sum())} starts differ"
    if cap == 131072:  # the low-priority mass on both sides of the big slot is reached
        assert (s[:B // 2] < big).all() and (s[B // 2:] > big).all()
    rel = np.abs(p[keep] - ref_p[keep]) / ref_p[keep]
    print(f"cap {cap}: prob worst relative error {rel.max():.3g}")
    assert rel.max() <= 1e-6
    s2, p2 = _sample(gpu, pri, size, next_idx, S, u)
    assert np.array_equal(s, s2) and np.array_equal(p.view(np.uint32), p2.view(np.uint32))
    # the ends of the unit interval: the first and the last valid slot
    first, last = np.nonzero(ok)[0][[0, -1]]
    se, _ = _sample(gpu, pri, size, next_idx, S, np.array([0.0, 1.0 - 2.0 ** -53]))
    assert se[0] == first and se[1] == last, (se, first, last)


def test_sampler_bad_stored_priorities_count_as_floor(gpu):
    """NaN / 0 / -1 / inf stored in valid slots weigh p_floor, in the draws and in prob."""
    g = np.random.RandomState(11)
    cap, size, next_idx, S, B = 3000, 3000, 1500, 8, 1024
    pri = _log_uniform(g, cap, 0.04, 10.0)
    bad = np.array([np.nan, 0.0, -1.0, np.inf], dtype=np.float32)
    where = g.choice(np.nonzero(RR.valid_mask_fast(cap, size, next_idx, S))[0], 400, replace=False)
    pri[where] = bad[np.arange(400) % 4]
    p_floor = 2.0  # large enough that the floored slots are drawn often
    u = g.uniform(size=B)
    ref_s, ref_p, margin = RR.sample(pri, size, next_idx, S, p_floor, u)
    keep = margin >= MARGIN
    s, p = _sample(gpu, pri, size, next_idx, S, u, p_floor=p_floor)
    assert (~keep).sum() <= B // 100
    assert np.array_equal(s[keep], ref_s[keep])
    hit = np.isin(s, where)
    assert hit.sum() > 50, "the floored slots must be drawn for the check to mean something"
    assert (np.abs(p[keep] - ref_p[keep]) / ref_p[keep]).max() <= 1e-6
    pr = _probabilities(gpu, pri, size, next_idx, S, p_floor)
    ref = RR.probabilities(pri, size, next_idx, S, p_floor)
    assert np.all(pr[ref == 0.0] == 0.0)
    assert (np.abs(pr - ref)[ref > 0] / ref[ref > 0]).max() <= 1e-6


def _probabilities(gpu, pri, size, next_idx, S, p_floor=P_FLOOR):
    L, hip = _lib()
    cap = len(pri)
    p = torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(gpu)
    out = torch.full((cap,), -1.0, device=gpu)
    ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=gpu)
    L.call("dr_replay_probabilities", cap, size, next_idx, S, L.ptr(p), p_floor, L.ptr(out), L.ptr(ws), ws.numel(),
           hip.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ring_buffer(gpu, cap, S, next_idx, pri):
    """A full curious-mode Buffer of `cap` slots with the given priorities and write head."""
    from dreamer_amd.buffer import Buffer
    b = Buffer(cap, S, 3, (32, 32), device=gpu)
    b.replay = "curious"
    b.load_arrays(np.zeros((cap, 3, 32, 32), np.uint8), np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32),
                  np.ones(cap, np.float32))
    b.next_idx = next_idx
    b._mirror()["priority"].copy_(torch.from_numpy(pri))
    return b


def test_sampler_philox(gpu):
    """2^18 Philox draws at cap = 256: chi-square of the counts against
    dr_replay_probabilities (cells with expectation < 5 pooled), no invalid
    start, a second call differs, the restored generator repeats the first."""
    _, hip = _lib()
    cap, S, next_idx, N = 256, 4, 100, 1 << 18
    pri = _log_uniform(np.random.RandomState(21), cap, 0.1, 100.0)
    b = _ring_buffer(gpu, cap, S, next_idx, pri)
    ar = hip.adhoc(gpu)
    ar.reseed(0x51CADA5)
    state, counter = ar.state.clone(), ar.counter
    prob = b.sampling_probabilities()
    s1, p1 = b.sample_start_indices_device(N)
    s2, _ = b.sample_start_indices_device(N)
    ar.state.copy_(state)
    ar.counter = counter
    s3, p3 = b.sample_start_indices_device(N)
    torch.cuda.synchronize()
    assert s1.dtype == torch.int64 and s1.is_cuda and p1.dtype == torch.float32 and p1.is_cuda
    assert torch.equal(s1, s3) and torch.equal(p1, p3), "the restored generator must repeat the draws"
    assert not torch.equal(s1, s2), "a second call must draw afresh"
    pr = prob.cpu().numpy().astype(np.float64)
    ref = RR.probabilities(pri, cap, next_idx, S, P_FLOOR)
    ok = RR.valid_mask_fast(cap, cap, next_idx, S)
    assert np.all(pr[~ok] == 0.0)
    assert (np.abs(pr - ref)[ok] / ref[ok]).max() <= 1e-6 and abs(pr.sum() - 1.0) <= 1e-6
    s = s1.cpu().numpy()
    assert ok[s].all(), "an invalid start was drawn"
    assert np.array_equal(p1.cpu().numpy(), prob.cpu().numpy()[s]), "prob[b] is the drawn slot's probability"
    counts = np.bincount(s, minlength=cap).astype(np.float64)
    exp = ref * N
    small = exp < 5
    o = np.concatenate([counts[~small & ok], [counts[small].sum()]]) if (small & ok).any() else counts[ok]
    e = np.concatenate([exp[~small & ok], [exp[small].sum()]]) if (small & ok).any() else exp[ok]
    chi = float(((o - e) ** 2 / e).sum())
    p_chi = float(stats.chi2.sf(chi, len(o) - 1))
    print(f"philox sampler: chi2 {chi:.1f} on {len(o) - 1} dof (p = {p_chi:.3g}); "
          f"probabilities span {ref[ok].min():.3g} .. {ref[ok].max():.3g}")
    assert ref[ok].max() / ref[ok].min() > 300, "the check needs priorities over three decades"
    assert p_chi > P_MIN, (chi, len(o) - 1)


def _update(gpu, pri, vis, starts, scores):
    L, hip = _lib()
    p = torch.from_numpy(pri.copy()).to(gpu)
    v = torch.from_numpy(vis.copy()).to(gpu)
    st = torch.from_numpy(np.asarray(starts, dtype=np.int64)).to(gpu)
    sc = torch.from_numpy(np.asarray(scores, dtype=np.float32)).to(gpu)
    L.call("dr_replay_priority_update", len(pri), len(starts), L.ptr(st), L.ptr(sc), *CONSTS, L.ptr(p), L.ptr(v),
           hip.stream())
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("B", [8, 256])
def test_priority_update(B, gpu):
    g = np.random.RandomState(31 + B)
    cap = 64
    pri = _log_uniform(g, cap, 0.04, 1e5)
    vis = g.randint(0, 6, cap).astype(np.int32)
    starts = g.randint(0, cap if B > 8 else 5, B)  # B = 8: five slots for eight rows
    scores = (g.normal(size=B) * 30.0).astype(np.float32)
    scores[:4] = np.array([np.nan, np.inf, -12.5, 0.0], dtype=np.float32)
    if B == 8:
        starts[:4] = [0, 1, 2, 2]  # the negative score shares a slot with the 0
    p, v = _update(gpu, pri, vis, starts, scores)
    rp, rv = RR.update(pri, vis, starts, scores, *CONSTS)
    assert np.array_equal(v.astype(np.int64), rv), "visit counts"
    assert v.sum() - vis.sum() == B
    rel = np.abs(p.astype(np.float64) - rp) / np.abs(rp)
    print(f"B = {B}: priority worst relative error {rel.max():.3g} (tolerance 1e-5)")
    assert rel.max() <= 1e-5
    assert p[starts[0]] == np.float32(1e5) and p[starts[1]] == np.float32(1e5), "a non-finite score gives p_new"
    untouched = np.setdiff1d(np.arange(cap), starts)
    assert np.array_equal(p[untouched].view(np.uint32), pri[untouched].view(np.uint32))
    assert np.array_equal(v[untouched], vis[untouched])
    perm = g.permutation(B)
    p2, v2 = _update(gpu, pri, vis, starts[perm], scores[perm])
    assert np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and np.array_equal(v, v2), "row order must not matter"


def _t(a, dev=None):
    t = torch.from_numpy(np.asarray(a).copy())
    return t if dev is None else t.to(dev)


def _wm_step(gpu, fx, scores):
    d, P = build("small", gpu, fx)
    wm = d.world_model
    obs, act, rew, cont, T = window(fx)
    wm.train_step_hip(obs.to(gpu), act.to(gpu), rew.to(gpu), cont.to(gpu), noise_q=_t(fx["q"], gpu), scores=scores)
    torch.cuda.synchronize()
    return d, P, (obs, act, rew, cont, T)


def test_window_scores(gpu):
    fx = load_fixture("small_wm")
    d, P, (obs, act, rew, cont, T) = _wm_step(gpu, fx, True)
    wm = d.world_model
    R, C = int(fx["cfg_rows"]), int(fx["cfg_cols"])
    betas = (wm.beta_pred, wm.beta_dyn, wm.beta_rep)
    with torch.no_grad():
        o = O.wm_losses(obs, act, rew, cont, P, _t(fx["q"]), R, C, T, betas=betas)
    ref, pred, _, msum = RR.window_scores(o, cont, T, betas)
    got = cpu(wm.last_window_scores).double().numpy()
    assert got.shape == (obs.shape[0],) and wm.last_window_scores.is_cuda
    err = np.abs(got - ref)
    print(f"window scores: worst |d| {err.max():.3g} at |ref| up to {np.abs(ref).max():.3g}")
    assert np.all(err <= 1e-4 * np.maximum(1.0, np.abs(ref))), (got, ref)
    # the windows' prediction terms add up to the step's loss_pred:
    # sum_b (sum_t m)_b pred_b / (sum m + 1e-5), from the reference's pred_b and
    # from the kernel's scores (beta_pred pred_b = L_b - (beta_dyn + beta_rep) kl_b)
    ls = cpu(wm.last_losses).double().numpy()
    _, _, klb, _ = RR.window_scores(o, cont, T, betas)
    pred_gpu = (got - (betas[1] + betas[2]) * klb) / betas[0]
    for what, pb in (("reference", pred), ("kernel", pred_gpu)):
        pooled = float((msum * pb).sum() / (msum.sum() + 1e-5))
        print(f"pooled loss_pred from the {what}'s windows {pooled:.8g} vs the step's {ls[1]:.8g}")
        assert abs(pooled - ls[1]) <= 1e-4 * max(1.0, abs(ls[1])), (what, pooled, ls[1])
    # scores=True changes nothing the step computes
    d0, _, _ = _wm_step(gpu, fx, False)
    wm0 = d0.world_model
    assert wm0.last_window_scores is None
    assert torch.equal(wm.last_losses, wm0.last_losses)
    for (k, a), (_, b) in zip(wm.named_parameters(), wm0.named_parameters()):
        assert torch.equal(a, b), k
    assert torch.equal(wm.optimiser.exp_avg, wm0.optimiser.exp_avg)
    assert torch.equal(wm.optimiser.exp_avg_sq, wm0.optimiser.exp_avg_sq)


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
    fr, ac, rw, ct = replay_data(256, (32, 32), 3, seed=11)
    d.buffer.load_arrays(fr, ac, rw, ct)
    return d


def test_curious_replay_end_to_end(gpu, tmp_path):
    _, hip = _lib()
    d = _dreamer(gpu, replay="curious")
    buf, B = d.buffer, E2E["batch_size"]
    hip.adhoc(gpu).reseed(0xC0FFEE)
    log = []
    update = buf.update_priorities

    def recording(starts, scores):
        log.append((starts.clone(), scores.clone()))
        update(starts, scores)

    buf.update_priorities = recording
    np_state = np.random.get_state()
    losses = d.train_world_model()
    buf.update_priorities = update
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(np_state[1:3], after[1:3])), "curious mode draws nothing from np.random"
    assert len(losses) == 3 and len(log) == 3 and all(torch.isfinite(x) for x in losses)
    m = buf._mirror()
    pri, vis = m["priority"].cpu().numpy(), m["visits"].cpu().numpy()
    assert vis.sum() == 3 * B
    rp, rv = np.full(256, 1e5), np.zeros(256, dtype=np.int64)
    ok = RR.valid_mask_fast(256, buf.size, buf.next_idx, 8)
    for st, sc in log:
        assert ok[st.cpu().numpy()].all() and sc.shape == (B,)
        rp, rv = RR.update(rp, rv, st.cpu().numpy(), sc.cpu().numpy(), *CONSTS)
    assert np.array_equal(vis.astype(np.int64), rv)
    seen = rv > 0
    assert (np.abs(pri[seen] - rp[seen]) / rp[seen]).max() <= 1e-5
    assert np.all(pri[~seen] == np.float32(1e5)), "unvisited slots still hold p_new"
    assert np.all(pri[seen] < 1e5), "a visited slot's priority has dropped"

    # one more transition resets exactly the slot it writes (the ring is full: slot 0)
    m["priority"][0], m["visits"][0] = 3.0, 2
    slot = buf.next_idx
    assert slot == 0
    before_p, before_v = m["priority"].clone(), m["visits"].clone()
    buf.add_to_buffer(np.zeros((3, 32, 32), np.uint8), np.zeros(3, np.float32), 0.5, 1.0)
    m = buf._mirror()
    assert float(m["priority"][slot]) == 1e5 and int(m["visits"][slot]) == 0
    assert torch.equal(m["priority"][1:], before_p[1:]) and torch.equal(m["visits"][1:], before_v[1:])

    # train_Agent draws from the same sampler and leaves priorities and visits alone
    before_p, before_v = m["priority"].clone(), m["visits"].clone()
    la, lc = d.train_Agent()
    torch.cuda.synchronize()
    assert np.isfinite(float(la)) and np.isfinite(float(lc))
    ok = RR.valid_mask_fast(256, buf.size, buf.next_idx, 8)
    assert ok[d.engine.starts.cpu().numpy()].all()
    assert torch.equal(m["priority"], before_p) and torch.equal(m["visits"], before_v)

    # resume: the per-slot state and the next draw
    path = tmp_path / "state.pt"
    d.save_training_state(path)
    st = torch.load(path, weights_only=True)
    assert st["format"] == "dreamer_amd.training_state.v1"
    assert set(st["buffer"]) == {"obs", "act", "rew", "cont", "next_idx", "size", "priority", "visits"}
    s_ref, _ = buf.sample_start_indices_device(B)
    d2 = _dreamer(gpu, replay="curious")
    d2.load_training_state(path)
    m2 = d2.buffer._mirror()
    assert torch.equal(m2["priority"], m["priority"]) and torch.equal(m2["visits"], m["visits"])
    s_got, _ = d2.buffer.sample_start_indices_device(B)
    assert torch.equal(s_ref, s_got)


def test_uniform_replay_untouched(gpu):
    """replay = "uniform": no priority tensors, and train_world_model consumes
    np.random exactly as the same number of sample_start_indices calls."""
    d = _dreamer(gpu)
    assert d.buffer.replay == "uniform"
    np.random.seed(5)
    d.train_world_model()
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert set(d.buffer._dev) == {"frames", "actions", "rewards", "continues"}
    assert d.world_model.last_window_scores is None
    np.random.seed(5)
    for _ in range(E2E["WM_epochs"]):
        d.buffer.sample_start_indices(E2E["batch_size"])
    want = np.random.get_state()
    assert np.array_equal(after[1], want[1]) and after[2] == want[2]
    st = d.training_state()
    assert set(st["buffer"]) == {"obs", "act", "rew", "cont", "next_idx", "size"}


def test_curious_refuses_data_parallelism(gpu):
    d = _dreamer(gpu, replay="curious")
    d.world = (0, 2, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_world_model()
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()
