"""The latent-disagreement ensemble on the MI355X (run on the GPU box: pytest -m gpu): the two row kernels alone through
dr_internal_disag_run, the composed forward / gradients / train_step against the float64 references of
tests/disag_ref.py on the inputs of tests/disag_cases.py, a deterministic learning run, and the public interface
(Dreamer with explore = "disagreement": train_Agent's rewards, train_world_model, graphs, pipelined epochs, resume,
novelty, data parallelism).

Launch geometry of the row kernels (read from the launchers in dreamer_amd/csrc/disag.hip; the derived bounds
(chain + tree depth + c) 2^-24 sum|terms| are formed from it in disag_ref.var_bound / mse_bounds):
  k_disag_var   a wave per row, 4 rows per 256-thread workgroup, ceil(M / 4) workgroups: a lane takes the columns j =
                lane, lane + 64, ... in ascending order -- per column the K members' deviations from member 0, their
                mean, the centred deviations scaled by a power of two, K squares, one division, one sqrt -- and adds the
                ceil(L / 64) stds; wave_sum (4 DPP levels + 3 adds); one division by L; lane 0 stores d and the reward
  k_disag_mse   a wave per (row, member), grid (ceil(M / 4), K): a lane stores (p - z) scale for its columns and adds
                ceil(L / 64) squares; wave_sum; lane 0 stores the row sum
  k_disag_loss  1 workgroup x 256 threads: per member a thread adds ceil(M / 256) row sums, wave_sum, thread 0 adds the
                four wave totals in order and divides by M L; the K losses are added in order and divided by K

Per row-kernel case: the hook returns 0; two runs on fresh buffers give identical bits; nothing outside an output and no
row >= M is written (NaN-poisoned buffers, compared bit for bit); every output within its derived bound of float64; and
bit for bit: d == 0.0 where the members agree (every K) and at K = 1, d >= 0, a gradient exactly 0 where p == z, a NaN /
Inf row non-finite in its own d and in no other, the loss sums finite exactly where float64's are."""
import ctypes
import os

import numpy as np
import pytest
import torch

import disag_cases as C
import disag_ref as R
from conftest import fixture_params, load_fixture
from formula import FULL, SMALL, formula_state_dict, replay_data

pytestmark = pytest.mark.gpu
ERRORS_FILE = os.environ.get("DISAG_ERRORS")
U = R.U


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_disag_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                  ctypes.c_int]
    return f


def _run(op, v, num, bufs, dev):
    """One call of the hook on fresh device copies of `bufs` (numpy arrays, None = NULL): (rc, message, the buffers back)."""
    from dreamer_amd import hip
    held = [None if b is None else torch.from_numpy(b.copy()).to(dev) for b in bufs]
    va = (ctypes.c_int * 16)(*v)
    na = (ctypes.c_double * 4)(*num)
    pa = (ctypes.c_void_p * 8)(*[None if t is None else t.data_ptr() for t in held])
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(op, va, na, pa, hip.stream(), msg, 256)
    torch.cuda.synchronize()
    return rc, msg.value.decode(), [None if t is None else t.cpu().numpy() for t in held]


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def _check_var(K, L, M, dev, fails):
    pred, z, kinds = C.row_case(K, L, M)
    buf, ks, ldp = C.padded_pred(pred)
    fin = np.array([k not in ("nan", "inf") for k in kinds])
    with np.errstate(invalid="ignore", over="ignore"):
        ref, tol = R.disagreement(pred.astype(np.float64)), R.var_bound(pred)
    tag = f"var K{K} L{L} M{M}"
    # d alone
    v = [K, M, L, ks, ldp, 0, 0, 0, 0]
    rc, msg, out = _run(R.DG_VAR, v, [0.0, 0.0], [buf, C.poison(M + 3), None], dev)
    assert rc == 0, f"{tag}: rc {rc}: {msg}"
    rc2, _, again = _run(R.DG_VAR, v, [0.0, 0.0], [buf, C.poison(M + 3), None], dev)
    assert rc2 == 0
    d = out[1]
    if not _same_bits(d, again[1]):
        fails.append(f"{tag}: d differs between two runs")
    if not C.is_poison(d[M:]).all():
        fails.append(f"{tag}: rows >= M written")
    if not _same_bits(out[0], buf):
        fails.append(f"{tag}: the predictions were written")
    d = d[:M].astype(np.float64)
    if np.isfinite(d[~fin]).any() or not np.isfinite(d[fin]).all():
        fails.append(f"{tag}: finiteness of d does not follow the rows ({d[~fin]}, {kinds})")
    if not np.all(np.abs(d - ref)[fin] <= tol[fin]):
        w = np.nanmax((np.abs(d - ref) / tol)[fin])
        fails.append(f"{tag}: d off by {w:.2f} of its bound")
    if not np.all(d[fin] >= 0.0):
        fails.append(f"{tag}: negative d")
    for r, kind in enumerate(kinds):
        if (kind == "equal" or K == 1) and fin[r] and not (d[r] == 0.0):
            fails.append(f"{tag}: row {r} ({kind}) d = {d[r]!r}, not exactly 0")
    worst = float(np.max((np.abs(d - ref) / tol)[fin])) if fin.any() else 0.0
    # the in-place reward update on a strided reward array (d not asked for)
    T1, skip, sb, st, n, at = C.reward_map(M)
    g = C.rng(4, K, L, M)
    rew = C.poison(n)
    r0 = g.standard_normal(M).astype(np.float32)
    for m, a in enumerate(at):
        if a >= 0:
            rew[a] = r0[m]
    e, s = C.REW_W
    rc, msg, out = _run(R.DG_VAR, [K, M, L, ks, ldp, T1, skip, sb, st], [e, s], [buf, None, rew], dev)
    assert rc == 0, f"{tag} reward: rc {rc}: {msg}"
    got = out[2]
    touched = np.zeros(n, dtype=bool)
    for m, a in enumerate(at):
        if a < 0:
            continue
        touched[a] = True
        if not fin[m]:
            if np.isfinite(got[a]):
                fails.append(f"{tag}: reward of the non-finite row {m} is finite")
            continue
        want = e * float(r0[m]) + s * ref[m]
        lim = abs(s) * tol[m] + 3 * U * (abs(e * float(r0[m])) + abs(s * ref[m]))  # two products and a sum, each rounded
        if not abs(float(got[a]) - want) <= lim:
            fails.append(f"{tag}: reward of row {m}: {got[a]!r} vs {want!r} (+- {lim:.3g})")
    if not C.is_poison(got[~touched]).all():
        fails.append(f"{tag}: rewards outside the mapping written")
    return worst


def _check_mse(K, L, M, dev, fails):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # (the NaN / Inf / 1e15 rows)
        return _check_mse_rows(K, L, M, dev, fails)


def _check_mse_rows(K, L, M, dev, fails):
    pred, z, kinds = C.row_case(K, L, M)
    buf, ks, ldp = C.padded_pred(pred)
    zb, ldz = C.padded_rows(z)
    tag = f"mse K{K} L{L} M{M}"
    bufs = [buf, zb, C.poison(K * M * L + 5), C.poison(K * M + 5), C.poison(1 + K + 3)]
    v = [K, M, L, ks, ldp, ldz]
    rc, msg, out = _run(R.DG_MSE, v, [], bufs, dev)
    assert rc == 0, f"{tag}: rc {rc}: {msg}"
    rc2, _, again = _run(R.DG_MSE, v, [], bufs, dev)
    assert rc2 == 0
    for i, name in ((2, "g"), (3, "row sums"), (4, "losses")):
        if not _same_bits(out[i], again[i]):
            fails.append(f"{tag}: {name} differ between two runs")
    if not (C.is_poison(out[2][K * M * L:]).all() and C.is_poison(out[3][K * M:]).all() and
            C.is_poison(out[4][1 + K:]).all()):
        fails.append(f"{tag}: written past an output")
    if not (_same_bits(out[0], buf) and _same_bits(out[1], zb)):
        fails.append(f"{tag}: an input was written")
    g = out[2][:K * M * L].reshape(K, M, L)
    ls = out[4][:1 + K].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g64 = R.mse_grad(pred.astype(np.float64), z.astype(np.float64))
        l64 = R.losses(pred.astype(np.float64), z.astype(np.float64))
        eg, el = R.mse_bounds(pred, z)
    ok = np.isfinite(g64)
    if np.isfinite(g[~ok]).any() or not np.isfinite(g[ok]).all():
        fails.append(f"{tag}: finiteness of g does not follow float64")
    if not np.all(np.abs(g.astype(np.float64) - g64)[ok] <= eg[ok]):
        fails.append(f"{tag}: g off by {np.max((np.abs(g - g64) / eg)[ok]):.2f} of its bound")
    if not np.all(g[pred == z[None]] == 0.0):
        fails.append(f"{tag}: g not exactly 0 where p == z")
    if not np.array_equal(np.isfinite(ls), np.isfinite(l64)):
        fails.append(f"{tag}: loss sums' finiteness {np.isfinite(ls)} vs float64's {np.isfinite(l64)}")
    okl = np.isfinite(l64)
    if not np.all(np.abs(ls - l64)[okl] <= el[okl]):
        fails.append(f"{tag}: losses off by {np.max((np.abs(ls - l64) / el)[okl]):.2f} of their bound")
    return float(np.max((np.abs(ls - l64) / el)[okl])) if okl.any() else 0.0


@pytest.mark.parametrize("K", C.ROW_K)
def test_row_kernels_match_float64(K, gpu):
    fails, wv, wm = [], 0.0, 0.0
    for L in C.ROW_L:
        for M in C.ROW_M:
            wv = max(wv, _check_var(K, L, M, gpu, fails))
            wm = max(wm, _check_mse(K, L, M, gpu, fails))
    print(f"K = {K}: d at most {wv:.3f} of its derived bound, the losses {wm:.3f} of theirs")
    assert not fails, f"{len(fails)} failures, first: " + " || ".join(fails[:6])


def test_hook_rejects_bad_descriptors(gpu):
    pred = np.zeros((2, 2, 4), dtype=np.float32)
    for v in ([0, 2, 4, 8, 4], [17, 2, 4, 8, 4], [2, 0, 4, 8, 4], [2, 2, 4, 8, 3], [2, 2, 4, 6, 4]):
        rc, msg, _ = _run(R.DG_VAR, v + [0, 0, 0, 0], [0.0, 0.0], [pred, C.poison(4), None], gpu)
        assert rc == 1001 and msg, (v, rc, msg)
    rc, msg, _ = _run(R.DG_VAR, [2, 2, 4, 8, 4, 0, 0, 0, 0], [0.0, 0.0], [pred, None, None], gpu)
    assert rc == 1001


# --------------------------------------------------------------------------------------------------------------------
# composed
# --------------------------------------------------------------------------------------------------------------------
def _module(c, dev, lr=C.TRAIN_LR):
    from dreamer_amd.networks import DisagreementEnsemble
    ex = DisagreementEnsemble(c["Hd"], c["L"], c["K"], c["W"], lr, (0.9, 0.999), 1e-5, seed=0, device=dev)
    ex.load_state_dict({k: torch.from_numpy(v).to(dev) for k, v in c["P"].items()})
    ex._ensure_flat()
    return ex


def _record(lines):
    for line in lines:
        print(line)
    if ERRORS_FILE:
        with open(ERRORS_FILE, "a") as f:
            f.write("\n".join(lines) + "\n")


def _measured(key, i, got, ref, f32, fails, lines):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    tol, scale = C.measured_tol(key, ref, f32)
    units = err / (U * scale) if scale > 0 else 0.0
    cap = "-" if f32 is None else f"{float(np.abs(f32.astype(np.float64) - ref).max()) / (U * scale):.3f}"
    lines.append(f"{key} | case {i} | err {units:.3f} x 2^-24 max abs ref | f32 numpy {cap} | "
                 f"asserted at {tol / (U * scale) if scale > 0 else 0.0:.3f}")
    if not err <= tol:
        fails.append(f"case {i}: {key} off by {units:.3f} x 2^-24 max abs ref (allowed {tol / (U * scale):.3f})")


@pytest.mark.parametrize("i", range(len(C.COMPOSED)))
def test_composed_forward_gradients_and_steps(i, gpu):
    c = C.composed_case(i)
    ref, f32 = c["ref"], c["f32"]
    ex = _module(c, gpu)
    h, z = torch.from_numpy(c["h"]).to(gpu), torch.from_numpy(c["z"]).to(gpu)
    fails, lines = [], []
    d, pred = ex.forward_rows(h, predictions=True)
    d2 = ex.disagreement(h.view(1, c["M"], c["Hd"]))
    assert tuple(d2.shape) == (1, c["M"]) and torch.equal(d2.view(-1), d)  # same bits with and without pred_out
    pred, d = pred.cpu().numpy(), d.cpu().numpy()
    # propagated bounds (disag_ref.forward_bounds), tightened by the measured figure
    for key, got, want, bound in (("pred", pred, ref["pred"], c["e_pred"]), ("d", d, ref["d"], c["e_d"])):
        err = np.abs(got.astype(np.float64) - want)
        if not np.all(err <= bound):
            fails.append(f"case {i}: {key} off by {float((err / bound).max()):.3g} of its propagated bound")
        lines.append(f"{key} | case {i} | at most {float((err / bound).max()):.3g} of its propagated bound")
        _measured(key, i, got, want, None, fails, lines)
    if c["K"] == 1:
        assert np.all(d == 0.0)
    assert np.all(d >= 0.0)
    ex.grads(h, z)
    torch.cuda.synchronize()
    ls = ex.last_losses.cpu().numpy()
    err = np.abs(ls.astype(np.float64) - ref["losses"])
    if not np.all(err <= c["e_loss"]):
        fails.append(f"case {i}: losses off by {float((err / c['e_loss']).max()):.3g} of their propagated bound")
    _measured("losses", i, ls, ref["losses"], None, fails, lines)
    for n in R.NAMES:
        _measured(f"grad.{n}", i, getattr(ex, n).grad.cpu().numpy(), ref["grads"][n], f32["grads"][n], fails, lines)
    # three train_steps from the case's weights
    ex.load_state_dict({k: torch.from_numpy(v).to(gpu) for k, v in c["P"].items()})
    hist = []
    for _ in range(C.TRAIN_STEPS):
        loss = ex.train_step(h, z)
        assert loss.dim() == 0 and loss.is_cuda
        hist.append(loss)
        assert int(ex.last_skip) == 0
    assert int(ex.optimiser.step_dev) == C.TRAIN_STEPS
    assert tuple(ex.last_losses.shape) == (1 + c["K"],)
    hist = [float(x) for x in hist]
    for a, b in zip(hist, ref["hist"]):
        assert abs(a - b) <= 1e-4 * abs(b), (hist, ref["hist"])
    for n in R.NAMES:
        _measured(f"trained.{n}", i, getattr(ex, n).detach().cpu().numpy(), ref["trained"][n], f32["trained"][n], fails,
                  lines)
    _record(lines)
    assert not fails, f"{len(fails)} failures, first: " + " || ".join(fails[:6])


def test_learning(gpu):
    """200 train_steps on 64 rows: the ensemble agrees where it was trained and not on the shifted held-out rows (the
    float64 reference ends at d(train) = 0.0141, d(held-out) = 0.264; disag_cases.LEARN_REF)."""
    P, h_train, h_held, z = C.learn_case()
    c = dict(K=C.LEARN["K"], W=C.LEARN["W"], Hd=C.LEARN["Hd"], L=C.LEARN["rows"] * C.LEARN["cols"], P=P)
    ex = _module(c, gpu, lr=C.LEARN["lr"])
    ht, hh, zz = (torch.from_numpy(x).to(gpu) for x in (h_train, h_held, z))
    first = ex.train_step(ht, zz)
    for _ in range(C.LEARN["steps"] - 1):
        last = ex.train_step(ht, zz)
    d_train, d_held = float(ex.disagreement(ht).mean()), float(ex.disagreement(hh).mean())
    print(f"d(train) {d_train:.6f} (float64 {C.LEARN_REF['d_train']:.6f}), d(held-out) {d_held:.6f} "
          f"({C.LEARN_REF['d_held']:.6f}), loss {float(first):.6f} -> {float(last):.6f}")
    assert int(ex.last_skip) == 0
    assert d_train < d_held
    assert float(last) < float(first)


# --------------------------------------------------------------------------------------------------------------------
# through the public interface (formula.SMALL, B = 16, the fixture's H and S, a filled ring)
# --------------------------------------------------------------------------------------------------------------------
B = 16


def _dreamer(dev, **over):
    """SMALL at B = 16 with the fixture's parameters (an exploring Dreamer keeps its fresh ensemble) and a filled ring."""
    from dreamer_amd import Dreamer
    from oracle import dreamer_oracle as O
    fx = load_fixture("small_epoch")
    cfg = dict(SMALL)
    cfg.update(batch_size=B, horizon=int(fx["cfg_H"]), sequence_length=int(fx["cfg_S"]),
               buffer_size=int(fx["buf_capacity"]))
    cfg.update(over)
    torch.manual_seed(0)
    d = Dreamer(cfg, dev)
    P = dict(fixture_params("small", fx))
    P.update({k: v.detach().cpu().clone() for k, v in d.state_dict().items() if k.startswith("explorer.")})
    d.load_state_dict({k: v.to(dev) for k, v in P.items()})
    n = cfg["buffer_size"]
    fr, ac, rw, ct = replay_data(n, (32, 32), 3, seed=3)
    d.buffer.load_arrays(fr, ac, O.symlog(torch.tensor(rw)).numpy(), ct)
    return d


ON = dict(explore="disagreement", explore_ensemble=3, explore_width=32)


def _noise(d, seed=5):
    R_, C_ = d.latent_state_dims
    S, H, A = d.sequence_length, d.horizon, d.action_dims
    g = torch.Generator().manual_seed(seed)
    return (torch.empty(S // 2, B * R_, C_).exponential_(generator=g).to(d.device),
            torch.randn(H, B, 1, A, generator=g).to(d.device),
            torch.empty(H, B * R_, C_).exponential_(generator=g).to(d.device))


def _epoch(d, noise, starts):
    """One train_Agent epoch with explicit noise, phase by phase as the engine runs it."""
    from dreamer_amd import hip
    from dreamer_amd.engine import ImaginationEngine
    eng = ImaginationEngine(d, use_graph=False)
    eng.rng.reseed(11)
    hip.adhoc(d.device).reseed(12)
    q_warm, eps, q = noise
    eng.starts.copy_(torch.from_numpy(starts))
    d.buffer.gather_actions(eng.starts, eng.act_win)
    eng.encode_and_warm(d.buffer.frames_struct(eng.starts), noise_q=q_warm)
    eng.imagine(eps=eps, q=q)
    head = eng.rewards.clone()
    eng.returns()
    eng.losses_and_grads()
    eng.optimise()
    torch.cuda.synchronize()
    ag = d.agent
    return dict(eng=eng, head=head.cpu(), rewards=eng.rewards.cpu(), R=eng.R.cpu(), hiddens=eng.hiddens.clone(),
                losses=ag.loss_buffer[0:2].cpu(), fa=ag.fa.flat.cpu(), fc=ag.fc.flat.cpu(), ft=ag.ft.flat.cpu(),
                S=ag.S_dev.cpu(), rng=(eng.rng.state.cpu(), eng.rng.counter, hip.adhoc(d.device).state.cpu(),
                                       hip.adhoc(d.device).counter))


def _starts(d, seed=21):
    np.random.seed(seed)
    return d.buffer.sample_start_indices(B)


def test_inert_at_weight_zero(gpu):
    off = _dreamer(gpu)
    on = _dreamer(gpu, explore_scale=0.0, explore_extrinsic=1.0, **ON)
    a = _epoch(off, _noise(off), _starts(off))
    b = _epoch(on, _noise(on), _starts(on))
    for k in ("rewards", "R", "losses", "fa", "fc", "ft", "S"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["losses"]).all()
    assert torch.equal(a["rng"][0], b["rng"][0]) and a["rng"][1] == b["rng"][1]
    assert torch.equal(a["rng"][2], b["rng"][2]) and a["rng"][3] == b["rng"][3]


def test_reward_relation(gpu):
    e, s = 0.5, 2.0
    off = _dreamer(gpu)
    on = _dreamer(gpu, explore_scale=s, explore_extrinsic=e, **ON)
    a = _epoch(off, _noise(off), _starts(off))
    b = _epoch(on, _noise(on), _starts(on))
    assert torch.equal(a["rewards"], a["head"]) and torch.equal(b["head"], a["rewards"])  # the head's own values
    d = on.disagreement(b["hiddens"])[:, 1:].cpu()
    assert tuple(d.shape) == tuple(a["rewards"].shape) and bool((d > 0).all())
    x, y = e * a["rewards"].double(), s * d.double()
    assert bool(((b["rewards"].double() - (x + y)).abs() <= 2.0 ** -23 * (x.abs() + y.abs())).all())
    assert not torch.equal(a["R"], b["R"])
    assert not torch.equal(a["fa"], b["fa"])
    assert torch.isfinite(b["losses"]).all()


@pytest.mark.parametrize("replay", ["uniform", "curious"])
def test_world_model_untouched(replay, gpu):
    from dreamer_amd import hip
    res = []
    for over in ({}, ON):
        d = _dreamer(gpu, replay=replay, WM_epochs=2, **over)
        np.random.seed(4)
        hip.adhoc(gpu).reseed(31)
        before = {k: v.detach().clone() for k, v in d.state_dict().items() if k.startswith("explorer.")}
        losses = d.train_world_model()
        torch.cuda.synchronize()
        wm, ar = d.world_model, hip.adhoc(gpu)
        res.append(([float(x) for x in losses], wm._flat.flat.cpu(), wm.optimiser.exp_avg.cpu(),
                    wm.optimiser.exp_avg_sq.cpu(), wm.optimiser.step_dev.cpu(), ar.state.cpu(), ar.counter,
                    np.random.get_state()[1].copy()))
        if over:
            assert all(not torch.equal(before[k], v) for k, v in d.state_dict().items()
                       if k.startswith("explorer.l")), "the ensemble's Linear parameters did not move"
            assert int(d.explorer.optimiser.step_dev) == 2 and int(d.explorer.last_skip) == 0
            assert torch.isfinite(d.explorer.last_losses).all()
    off, on = res
    assert off[0] == on[0] and np.isfinite(off[0]).all()
    for a, b in zip(off[1:6], on[1:6]):
        assert torch.equal(a, b)
    assert off[6] == on[6] and np.array_equal(off[7], on[7])


def test_graph_replay_equals_eager(gpu):
    from dreamer_amd.engine import ImaginationEngine
    res = []
    for use_graph in (False, True):
        d = _dreamer(gpu, **ON)
        eng = ImaginationEngine(d, use_graph=use_graph)
        eng.rng.reseed(77)
        np.random.seed(8)
        ls = []
        for _ in range(2):
            la, lc = eng.run(d.buffer.sample_start_indices(B))
            ls.append(torch.cat([la, lc]).clone())
        torch.cuda.synchronize()
        res.append((torch.stack(ls).cpu(), eng.rewards.cpu(), eng.R.cpu(), d.agent.fa.flat.cpu(), d.agent.fc.flat.cpu(),
                    d.agent.S_dev.cpu()))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_pipelined_epochs_equal_sequential(gpu, monkeypatch):
    """run_many's captured `returns` graph carries the intrinsic reward: AC_epochs = 2 pipelined = sequential, bit for
    bit (both in launch form, as tests/test_gpu_parity.py::test_pipelined_epochs_match_sequential)."""
    from dreamer_amd.engine import ImaginationEngine
    monkeypatch.setenv("DREAMER_PERSISTENT", "0")
    res = []
    for pipe in (False, True):
        d = _dreamer(gpu, AC_epochs=2, **ON)
        eng = ImaginationEngine(d)
        eng.rng.reseed(4321)
        np.random.seed(5)
        starts = [d.buffer.sample_start_indices(B) for _ in range(2)]
        if pipe:
            losses = eng.run_many(starts).cpu()
        else:
            losses = torch.stack([torch.cat(eng.run(st)).clone() for st in starts]).cpu()
        torch.cuda.synchronize()
        res.append((losses, eng.rewards.cpu(), d.agent.fa.flat.cpu(), d.agent.fc.flat.cpu(), d.agent.ft.flat.cpu(),
                    d.agent.S_dev.cpu(), eng.rng.state.cpu()))
    for a, b in zip(*res):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_persistent_kernels_still_run(gpu):
    """At the full widths (the only ones gpu_helpers.assert_persistent_ran's offsets describe) and B = 16 the scan, the
    unroll and the BPTT still run as the persistent kernels with exploration on; at SMALL the library's answer to
    dr_persistent_kernels is the same with and without it."""
    from dreamer_amd import Dreamer, _lib as L
    from dreamer_amd.engine import ImaginationEngine
    from conftest import state_layout
    from gpu_helpers import assert_persistent_ran
    cfg = dict(FULL)
    cfg.update(batch_size=B, sequence_length=16, horizon=6, buffer_size=64, explore="disagreement", explore_ensemble=2)
    torch.manual_seed(0)
    d = Dreamer(cfg, gpu)
    P = dict(formula_state_dict(dict(state_layout("full"))))
    P.update({k: v.detach().cpu().clone() for k, v in d.state_dict().items() if k.startswith("explorer.")})
    d.load_state_dict({k: v.to(gpu) for k, v in P.items()})
    fr, ac, rw, ct = replay_data(64, (64, 64), 3, seed=3)
    d.buffer.load_arrays(fr, ac, rw, ct)
    eng = ImaginationEngine(d)
    eng.rng.reseed(9)
    np.random.seed(2)
    la, lc = eng.run(d.buffer.sample_start_indices(B))
    torch.cuda.synchronize()
    assert np.isfinite(float(la)) and np.isfinite(float(lc))
    assert_persistent_ran(eng)
    small_on, small_off = ImaginationEngine(_dreamer(gpu, **ON)), ImaginationEngine(_dreamer(gpu))
    q = lambda e: L.query("dr_persistent_kernels", e.d, e.B, e.T, e.H)
    assert q(small_on) == q(small_off)


def test_resume(gpu, tmp_path):
    kw = dict(AC_epochs=1, WM_epochs=1, explore_scale=0.5, **ON)
    d = _dreamer(gpu, **kw)
    np.random.seed(1)
    d.train_world_model()
    d.train_Agent()
    path = tmp_path / "state.pt"
    d.save_training_state(path)

    def rounds(dr):
        out = []
        for _ in range(2):
            wm = float(dr.train_world_model()[0])
            la, lc = dr.train_Agent()
            out += [wm, float(la), float(lc), float(dr.explorer.last_losses[0])]
        torch.cuda.synchronize()
        o = dr.explorer.optimiser
        return out, {k: v.detach().cpu().clone() for k, v in dr.state_dict().items()}, \
            (o.exp_avg.cpu(), o.exp_avg_sq.cpu(), o.step_dev.cpu())

    ref = rounds(d)
    torch.manual_seed(123)
    np.random.seed(99)
    d2 = _dreamer(gpu, **dict(kw, seed=7))  # another ensemble initialisation: the state brings the weights
    d2.load_training_state(path)
    got = rounds(d2)
    assert got[0] == ref[0] and all(np.isfinite(ref[0])), (got[0], ref[0])
    assert any(k.startswith("explorer.") for k in ref[1])
    for k in ref[1]:
        assert torch.equal(got[1][k], ref[1][k]), k
    for a, b in zip(got[2], ref[2]):
        assert torch.equal(a, b)
    assert int(ref[2][2]) == 3
    st = torch.load(path, weights_only=True)
    assert st["format"] == "dreamer_amd.training_state.v1" and "opt_explorer" in st
    # a state saved without exploration has no ensemble optimiser state
    plain = _dreamer(gpu)
    assert "opt_explorer" not in plain.training_state()
    with pytest.raises(ValueError, match="exploration"):
        _dreamer(gpu, **kw).load_training_state(plain.training_state())


def test_novelty(gpu):
    from dreamer_amd import hip
    d = _dreamer(gpu, **ON)
    S = d.sequence_length
    np.random.seed(6)
    hip.adhoc(gpu).reseed(41)
    ar = hip.adhoc(gpu)
    before = (np.random.get_state()[1].copy(), torch.get_rng_state().clone(), ar.state.clone(), ar.counter,
              hip.rng(gpu).state.clone(), hip.rng(gpu).counter)
    starts = np.arange(B) * 2
    nov = d.novelty(starts=starts, length=S - 1)
    assert tuple(nov.shape) == (B, S - 1) and bool(torch.isfinite(nov).all()) and bool((nov >= 0).all())
    assert bool((nov > 0).any())
    sampled = d.novelty(batch_size=5)
    assert tuple(sampled.shape) == (5, S)
    ev = d.evaluate_novelty(batches=2, batch_size=4, length=3)
    assert len(ev["novelty"]) == 3 and np.isfinite(ev["mean"]) and ev["mean"] >= 0
    after = (np.random.get_state()[1], torch.get_rng_state(), ar.state, ar.counter, hip.rng(gpu).state,
             hip.rng(gpu).counter)
    assert np.array_equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(before[2], after[2]) and before[3] == after[3]
    assert torch.equal(before[4], after[4]) and before[5] == after[5]
    # the same windows through the public pieces: the filter on the ring's frames, then disagreement
    idx = (starts[:, None] + np.arange(S - 1)[None, :]) % d.buffer.capacity
    obs = torch.from_numpy(d.buffer.observation_buffer[idx]).to(gpu).float()
    act = torch.from_numpy(d.buffer.action_buffer[idx]).to(gpu)
    hid = d.world_model.observe_sequence(obs, act)[1]  # (draws the ad-hoc stream id novelty's filter drew)
    assert torch.equal(d.disagreement(hid), nov)
    with pytest.raises(ValueError):
        d.novelty(starts=starts, length=S + 1)
    with pytest.raises(RuntimeError, match="explore"):
        _dreamer(gpu).novelty(starts=starts)


def test_data_parallel_raises(gpu):
    from dreamer_amd.engine import ImaginationEngine
    d = _dreamer(gpu, **ON)
    with pytest.raises(ValueError, match="data parallelism"):
        ImaginationEngine(d, world=(0, 1, None))
    d.world = (0, 1, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_world_model()
