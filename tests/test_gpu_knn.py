"""The fused k-nearest-neighbour search and the particle-entropy reward on the MI355X (run on the GPU box: pytest -m
gpu): the kernels through dr_internal_knn_run against the float64 references of tests/knn_ref.py on the cases of
tests/knn_cases.py, the C entry points, and the public interface (Dreamer with explore = "entropy").

Launch geometry (read from dreamer_amd/csrc/knn.hip; the bounds of knn_ref are formed from it):
  k_knn_tile     256 threads, grid (ceil(Mq / 128), splits): 128 query rows x a contiguous range of 128-row bank tiles,
                 columns staged 16 at a time, zero past D.  Per pair ONE v_mfma_f32_16x16x4_f32 accumulator: the dot
                 product is the k-ascending fmaf chain from 0 (D roundings); both norms are the same chain on the VALU
                 from the same staged values; then (|x|^2 + |y|^2) - 2 x.y: one rounded sum, an exact doubling, one
                 rounded difference, clamped at 0.  Gram bound G_mj = (D + c) 2^-24 (|x|^2 + |y|^2 + 2 sum |x_i||y_i|)
                 with c = 3: the two roundings after the chains and one for the second-order terms.
  k_knn_merge    a wave per query row: the splits' lists merged by (d2, index); per chosen pair a lane adds the
                 ceil(D / 64) squares (x - y)^2 of its columns in ascending order, wave_sum (4 DPP levels + 3 adds):
                 direct bound (ceil(D / 64) + 10) 2^-24 d2; rank sort by (recomputed d2, index)
  k_knn_entropy  a thread per row: k_m square roots added in slot order, one division, log1pf, the reward rewrite

Per case: rc == 0; two runs on fresh buffers give identical bits; nothing outside an output and no row >= Mq is written,
no input is written (NaN-padded rows, poisoned outputs, compared bit for bit); integer-valued inputs give the
reference's indices and distances exactly; random inputs meet the contract of knn_cases.check_contract in every row."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_cases as C
import knn_ref as R

pytestmark = pytest.mark.gpu
U = R.U
ERRORS_FILE = os.environ.get("KNN_ERRORS")


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_knn_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                  ctypes.c_int]
    return f


def _run(op, v, num, bufs, dev):
    """One call of the hook on fresh device copies of `bufs` (numpy arrays, None = NULL): (rc, message, buffers back)."""
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


def _planned(Mq, Nb):
    out = ctypes.c_int(0)
    va = (ctypes.c_int * 16)(Mq, Nb)
    pa = (ctypes.c_void_p * 8)(ctypes.addressof(out))
    assert _hook()(R.KN_PLAN, va, None, pa, None, None, 0) == 0
    return out.value


def _knn(q, bank, k, qg, bg, dev, split=0, fails=None, tag="", pads=(3, 5)):
    """dr_knn through the hook on padded / poisoned buffers: (d2 [Mq][k], idx [Mq][k]); the write checks go to fails."""
    Mq, D = q.shape
    Nb = bank.shape[0]
    qb, ldq = C.padded_rows(q, pad=pads[0])
    bb, ldb = C.padded_rows(bank, pad=pads[1])
    ws_bytes = 64 * Mq * k * 8 + 2 * Mq * k * 4 + 4096  # any split count up to 64
    ws = np.zeros(ws_bytes // 4, dtype=np.float32)
    bufs = [qb, qg, bb, bg, C.poison(Mq * k + 5), C.poison(Mq * k + 5).view(np.int32), ws]
    rc, msg, out = _run(R.KN_KNN, [D, k, Mq, Nb, ldq, ldb, split], [float(ws_bytes)], bufs, dev)
    assert rc == 0, f"{tag}: rc {rc}: {msg}"
    if fails is not None:
        if not (C.is_poison(out[4][Mq * k:]).all() and C.is_poison(out[5][Mq * k:].view(np.float32)).all()):
            fails.append(f"{tag}: written past an output")
        if not (_same_bits(out[0], qb) and _same_bits(out[2], bb)):
            fails.append(f"{tag}: an input was written")
    return out[4][:Mq * k].reshape(Mq, k), out[5][:Mq * k].reshape(Mq, k)


def _record(lines):
    for line in lines:
        print(line)
    if ERRORS_FILE:
        with open(ERRORS_FILE, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("i", range(len(C.CASES)))
def test_cases_match_float64(i, gpu):
    D, (Mq, Nb), k, kind = C.CASES[i]
    tag = f"case {i} D{D} Mq{Mq} Nb{Nb} k{k} {kind}"
    fails = []
    # integer-valued inputs: exact
    c = C.reference(i, "ints")
    d2, idx = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu, fails=fails, tag=tag)
    d2b, idxb = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu)
    if not (_same_bits(d2, d2b) and np.array_equal(idx, idxb)):
        fails.append(f"{tag}: two runs differ")
    if not np.array_equal(idx, c["idx"]):
        bad = int(np.argmax((idx != c["idx"]).any(axis=1)))
        fails.append(f"{tag}: integer inputs: row {bad} indices {idx[bad]} vs {c['idx'][bad]}")
    if not _same_bits(d2, c["d2"].astype(np.float32)):
        fails.append(f"{tag}: integer inputs: distances are not the exact ones")
    # random inputs: the contract, every row
    c = C.reference(i, "rand")
    d2, idx = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu, fails=fails, tag=tag)
    d2b, idxb = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu)
    if not (_same_bits(d2, d2b) and np.array_equal(idx, idxb)):
        fails.append(f"{tag}: two runs differ (random inputs)")
    f, w_direct, w_sel = C.check_contract(c, d2, idx)
    fails += [f"{tag}: {x}" for x in f]
    if kind == "self" and (idx == np.arange(Mq)[:, None]).any():
        fails.append(f"{tag}: a row returned itself")
    if kind == "dream" and ((idx // C.DREAM_T == (np.arange(Mq) // C.DREAM_T)[:, None]) & (idx >= 0)).any():
        fails.append(f"{tag}: a row of the same dream returned")
    # a bank row that is bit-identical to the query: exactly 0
    same = (c["T"] == 0.0) & c["el"]
    for m in range(Mq):
        n0 = int(min(same[m].sum(), k))
        if not np.all(d2[m, :n0] == 0.0):
            fails.append(f"{tag}: row {m}: {n0} identical bank rows, distances {d2[m, :n0]}")
    _record([f"knn | {tag} | reported d2 at most {w_direct:.3f} of the direct bound | selection slack used "
             f"{max(w_sel, 0.0):.3f} of 2 max G | splits {_planned(Mq, Nb)}"])
    assert not fails, f"{len(fails)} failures, first: " + " || ".join(fails[:6])


def test_non_finite_rows(gpu):
    """A NaN / Inf bank row is never returned and changes no other result, bit for bit against the same case with the
    rows removed and the indices remapped; a NaN query row is NaN / -1 in its own slots only."""
    for i in (4, 8):
        D, (Mq, Nb), k, kind = C.CASES[i]
        c = C.reference(i, "rand")
        q, bank = c["q"].copy(), c["bank"].copy()
        qg, bg = (None, None) if c["qg"] is None else (c["qg"].copy(), c["bg"].copy())
        bad = [5, Nb // 2, Nb - 1]
        if kind == "self":  # the queries stay what they were: only the bank copies are poisoned
            pass
        bank[bad[0], D // 2] = np.nan
        bank[bad[1], 0] = np.inf
        bank[bad[2], D - 1] = -np.inf
        d2, idx = _knn(q, bank, k, qg, bg, gpu)
        assert not np.isin(idx, bad).any()
        keep = np.setdiff1d(np.arange(Nb), bad)
        d2r, idxr = _knn(q, bank[keep], k, qg, None if bg is None else bg[keep], gpu)
        back = np.where(idxr >= 0, keep[np.maximum(idxr, 0)], -1)
        assert _same_bits(d2, d2r) and np.array_equal(idx, back)
        # a NaN query row
        q2 = q.copy()
        q2[Mq // 2, D - 1] = np.nan
        q2[0, 0] = np.inf
        d2n, idxn = _knn(q2, bank, k, qg, bg, gpu)
        rows = np.array([0, Mq // 2])
        assert np.isnan(d2n[rows]).all() and (idxn[rows] == -1).all()
        others = np.setdiff1d(np.arange(Mq), rows)
        assert _same_bits(d2n[others], d2[others]) and np.array_equal(idxn[others], idx[others])


def test_batch_independence(gpu):
    """A query's outputs are the same bits alone, in a batch of 65, in the whole batch, and with the bank split forced
    to 1, 2 and the planner's count."""
    for i in (9, 8):
        D, (Mq, Nb), k, kind = C.CASES[i]
        c = C.reference(i, "rand")
        assert _planned(Mq, Nb) > 2
        full = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu)
        for split in (1, 2, _planned(Mq, Nb), 64):
            got = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu, split=split)
            assert _same_bits(got[0], full[0]) and np.array_equal(got[1], full[1]), (i, split)
        # rows at strides that are multiples of 4: at D = 600, 64, 4 the float4-fetch form of the tile kernel runs
        for j in (i, 10, 2):
            cj = C.reference(j, "rand")
            a = _knn(cj["q"], cj["bank"], cj["k"], cj["qg"], cj["bg"], gpu)
            for pads in ((0, 0), (4, 8)):
                b = _knn(cj["q"], cj["bank"], cj["k"], cj["qg"], cj["bg"], gpu, pads=pads)
                assert _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), (j, pads)
        for rows in (slice(Mq - 1, Mq), slice(Mq - 66, Mq - 1)):
            qg = None if c["qg"] is None else c["qg"][rows]
            got = _knn(c["q"][rows], c["bank"], k, qg, c["bg"], gpu)
            assert _same_bits(got[0], full[0][rows]) and np.array_equal(got[1], full[1][rows]), (i, rows)


def test_entropy_row_kernel(gpu):
    """e within its derived bound of float64, exactly 0 for all-duplicate neighbours, 0 at k_m = 0, NaN for a NaN row;
    the strided reward rewrite in k_disag_var's form (rew_skip, rew_T = 0, untouched elements bit-equal)."""
    worst = 0.0
    for M, k, D in ((1, 1, 5), (5, 3, 64), (20, 12, 600), (257, 32, 65), (300, 12, 600)):
        g = C.rng(3, M, k)
        d2 = (g.random((M, k)) * D * 0.5).astype(np.float32)
        d2.sort(axis=1)
        idx = g.integers(0, 1000, size=(M, k)).astype(np.int32)
        if M > 4:
            d2[1] = 0.0                       # all neighbours identical to the row
            d2[2, k // 2:], idx[2, k // 2:] = np.inf, -1   # fewer eligible than k
            d2[3], idx[3] = np.inf, -1        # none eligible
            d2[4], idx[4] = np.nan, -1        # a non-finite query row
        ref = R.entropy(d2.astype(np.float64), idx)
        tol = R.entropy_bound(d2.astype(np.float64), idx, D)
        fin = np.isfinite(ref)
        T1, skip, sb, st, n, at = C.reward_map(M)
        rew = C.poison(n)
        r0 = g.standard_normal(M).astype(np.float32)
        for m, a in enumerate(at):
            if a >= 0:
                rew[a] = r0[m]
        e_w, s_w = C.REW_W
        bufs = [d2, idx, C.poison(M + 3), rew]
        rc, msg, out = _run(R.KN_ENT, [k, M, T1, skip, sb, st], [e_w, s_w], bufs, gpu)
        assert rc == 0, msg
        rc, msg, again = _run(R.KN_ENT, [k, M, T1, skip, sb, st], [e_w, s_w], bufs, gpu)
        assert _same_bits(out[2], again[2]) and _same_bits(out[3], again[3])
        e = out[2]
        assert C.is_poison(e[M:]).all() and _same_bits(out[0], d2) and np.array_equal(out[1], idx)
        e = e[:M].astype(np.float64)
        assert np.array_equal(np.isfinite(e), fin)
        assert np.all(np.abs(e - ref)[fin] <= tol[fin]), float((np.abs(e - ref)[fin] / np.maximum(tol[fin], 1e-300)).max())
        nz = fin & (tol > 0)
        if nz.any():
            worst = max(worst, float((np.abs(e - ref)[nz] / tol[nz]).max()))
        if M > 4:
            assert e[1] == 0.0 and e[3] == 0.0 and np.isnan(e[4])
        got = out[3]
        touched = np.zeros(n, dtype=bool)
        for m, a in enumerate(at):
            if a < 0:
                continue
            touched[a] = True
            if not fin[m]:
                assert not np.isfinite(got[a])
                continue
            # the kernel's own e in the kernel's own form: two products and one sum, each rounded
            want = np.float32(np.float32(e_w) * r0[m]) + np.float32(np.float32(s_w) * out[2][m])
            assert got[a] == np.float32(want), (m, got[a], want)
        assert C.is_poison(got[~touched]).all()
        # ent alone and rew alone give the same bits
        rc, _, o2 = _run(R.KN_ENT, [k, M, T1, skip, sb, st], [e_w, s_w], [d2, idx, None, rew], gpu)
        assert rc == 0 and _same_bits(o2[3], got)
    _record([f"entropy row kernel | at most {worst:.3f} of its derived bound"])


def test_entry_points(gpu):
    """dr_knn and dr_state_entropy_fwd through ctypes: the hook's bits, the reward on a strided array, and the error
    codes (k out of range, D < 1, Mq or Nb < 1, a null pointer, too small a workspace)."""
    from dreamer_amd import _lib as L, hip
    i = 7
    D, (Mq, Nb), k, kind = C.CASES[i]
    c = C.reference(i, "rand")
    want = _knn(c["q"], c["bank"], k, c["qg"], c["bg"], gpu)
    q, bank = torch.from_numpy(c["q"]).to(gpu), torch.from_numpy(c["bank"]).to(gpu)
    qg, bg = torch.from_numpy(c["qg"]).to(gpu), torch.from_numpy(c["bg"]).to(gpu)
    nbytes = L.query("dr_knn_workspace_bytes", Mq, Nb, D, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    d2 = torch.empty(Mq, k, device=gpu)
    idx = torch.empty(Mq, k, dtype=torch.int32, device=gpu)
    args = (D, k, Mq, L.ptr(q), D, L.ptr(qg), Nb, L.ptr(bank), D, L.ptr(bg))
    L.call("dr_knn", *args, L.ptr(d2), L.ptr(idx), L.ptr(ws), nbytes, hip.stream())
    assert _same_bits(d2.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])
    ent = torch.empty(Mq, device=gpu)
    rew = torch.ones(Mq, device=gpu)
    L.call("dr_state_entropy_fwd", *args, None, None, L.ptr(ent), L.ptr(rew), 0, 0, 0, 1, 0.5, 2.0, L.ptr(ws), nbytes,
           hip.stream())
    e64 = R.entropy(want[0].astype(np.float64), want[1])
    assert np.all(np.abs(ent.cpu().numpy() - e64) <= R.entropy_bound(want[0].astype(np.float64), want[1], D))
    assert torch.equal(rew, 0.5 * torch.ones_like(rew) + 2.0 * ent)
    tail = (L.ptr(d2), L.ptr(idx), L.ptr(ws), nbytes, hip.stream())
    for bad in ((D, 0) + args[2:], (D, 33) + args[2:], (0,) + args[1:], args[:2] + (0,) + args[3:],
                args[:6] + (0,) + args[7:], args[:3] + (None,) + args[4:], args[:7] + (None,) + args[8:]):
        with pytest.raises(L.HipError) as ei:
            L.call("dr_knn", *bad, *tail)
        assert ei.value.code == L.DR_E_INVALID
    with pytest.raises(L.HipError) as ei:
        L.call("dr_knn", *args, L.ptr(d2), L.ptr(idx), L.ptr(ws), nbytes - 1, hip.stream())
    assert ei.value.code == L.DR_E_WORKSPACE
    with pytest.raises(L.HipError):
        L.call("dr_knn", *args, None, L.ptr(idx), L.ptr(ws), nbytes, hip.stream())
    assert L.query("dr_knn_workspace_bytes", Mq, Nb, D, 33) == 0


# --------------------------------------------------------------------------------------------------------------------
# through the public interface (formula.SMALL, B = 16, the fixture's H and S, a filled ring: the disagreement tests'
# Dreamer, noise and phase-by-phase epoch)
# --------------------------------------------------------------------------------------------------------------------
from test_gpu_disag import B, _dreamer, _epoch, _noise, _starts  # noqa: E402

ON = dict(explore="entropy", explore_knn=5)


def _ref_reward(hiddens, k, exclude, H):
    """float64 entropy reward [B][H] of the engine's hiddens [B][H + 1][Hd], its bound, the reference's indices.
    The bound: knn_ref.entropy_bound on the reference's selection, plus what the Gram-form selection may move: a
    returned row's true d2 lies within 2 max_j G_mj of the true k-th, so a slot's distance, and with it the mean,
    moves by at most sqrt(kth + 2 G) - sqrt(max(kth - 2 G, 0)) (d log1p <= 1)."""
    h = hiddens.cpu().numpy().reshape(-1, hiddens.shape[-1])
    row = np.arange(h.shape[0], dtype=np.int32)
    g = row // (H + 1) if exclude == "dream" else row
    T = R.dist2(h, h)
    d2, idx = R.knn(h, h, k, g, g, d2=T)
    assert (idx >= 0).all()
    G2 = 2.0 * np.where(R.eligible(h, h, g, g), R.gram_bound(h, h), 0.0).max(axis=1)
    kth = d2[:, -1]
    sel = np.sqrt(kth + G2) - np.sqrt(np.maximum(kth - G2, 0.0))
    e, tol = R.entropy(d2, idx), R.entropy_bound(d2, idx, h.shape[1]) + sel
    return e.reshape(-1, H + 1)[:, 1:], tol.reshape(-1, H + 1)[:, 1:], idx


@pytest.mark.parametrize("exclude", ["self", "dream"])
def test_reward_relation(exclude, gpu):
    e, s = 0.5, 2.0
    off = _dreamer(gpu)
    on = _dreamer(gpu, explore_scale=s, explore_extrinsic=e, explore_knn_exclude=exclude, **ON)
    a = _epoch(off, _noise(off), _starts(off))
    b = _epoch(on, _noise(on), _starts(on))
    assert torch.equal(a["rewards"], a["head"]) and torch.equal(b["head"], a["rewards"])  # the head's own values
    assert torch.equal(a["hiddens"], b["hiddens"])
    H = on.horizon
    ent, tol, idx = _ref_reward(b["hiddens"], ON["explore_knn"], exclude, H)
    assert (ent > 0).all()
    if exclude == "dream":
        rows = np.arange(idx.shape[0])[:, None]
        assert not ((idx // (H + 1) == rows // (H + 1)) & (idx >= 0)).any()
    x, y = e * a["rewards"].double().numpy(), s * ent
    # e within its bound (_ref_reward), then two products and one sum, each rounded
    lim = s * tol + 3 * U * (np.abs(x) + np.abs(y))
    err = np.abs(b["rewards"].double().numpy() - (x + y))
    print(f"entropy rewards ({exclude}): at most {float((err / lim).max()):.3f} of the bound")
    assert np.all(err <= lim)
    # the public read-out on the same states, bit for bit the reward's e where the exclusion is "self"
    if exclude == "self":
        se = on.state_entropy(b["hiddens"])[:, 1:].cpu()
        assert torch.equal(b["rewards"], (e * a["rewards"] + s * se))
    assert not torch.equal(a["R"], b["R"]) and not torch.equal(a["fa"], b["fa"])
    assert torch.isfinite(b["losses"]).all()


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


def test_world_model_untouched_and_nothing_added(gpu):
    from dreamer_amd import hip
    res = []
    for over in ({}, ON):
        d = _dreamer(gpu, WM_epochs=2, **over)
        np.random.seed(4)
        hip.adhoc(gpu).reseed(31)
        hip.rng(gpu).reseed(32)
        losses = d.train_world_model()
        torch.cuda.synchronize()
        wm, ar, er = d.world_model, hip.adhoc(gpu), hip.rng(gpu)
        res.append(([float(x) for x in losses], wm._flat.flat.cpu(), wm.optimiser.exp_avg.cpu(),
                    wm.optimiser.exp_avg_sq.cpu(), wm.optimiser.step_dev.cpu(), ar.state.cpu(), er.state.cpu(),
                    ar.counter, er.counter, np.random.get_state()[1].copy(), list(d.state_dict()),
                    sorted(d.training_state())))
        assert not hasattr(d, "explorer")
    off, on = res
    assert off[0] == on[0] and np.isfinite(off[0]).all()
    for a, b in zip(off[1:7], on[1:7]):
        assert torch.equal(a, b)
    assert off[7:9] == on[7:9] and np.array_equal(off[9], on[9])
    assert off[10] == on[10] and off[11] == on[11]


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
            out += [wm, float(la), float(lc)]
        torch.cuda.synchronize()
        return out, {k: v.detach().cpu().clone() for k, v in dr.state_dict().items()}

    ref = rounds(d)
    torch.manual_seed(123)
    np.random.seed(99)
    d2 = _dreamer(gpu, **dict(kw, seed=7))
    d2.load_training_state(path)
    got = rounds(d2)
    assert got[0] == ref[0] and all(np.isfinite(ref[0])), (got[0], ref[0])
    for k in ref[1]:
        assert torch.equal(got[1][k], ref[1][k]), k
    st = torch.load(path, weights_only=True)
    plain = _dreamer(gpu).training_state()
    assert sorted(st) == sorted(plain) and "opt_explorer" not in st
    # a state saved without exploration loads into an entropy Dreamer (and back): there is nothing to miss
    _dreamer(gpu, **kw).load_training_state(plain)
    _dreamer(gpu).load_training_state(st)


def test_novelty_and_knn_read_outs(gpu):
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
    assert tuple(nov.shape) == (B, S - 1) and bool(torch.isfinite(nov).all())
    # the filter starts every window from the zero state: B > k bit-identical rows, whose reward is exactly 0
    assert bool((nov[:, 0] == 0).all()) and bool((nov[:, 1:] > 0).all())
    assert tuple(d.novelty(batch_size=5).shape) == (5, S)
    ev = d.evaluate_novelty(batches=2, batch_size=4, length=3)
    assert len(ev["novelty"]) == 3 and np.isfinite(ev["mean"]) and ev["mean"] > 0
    after = (np.random.get_state()[1], torch.get_rng_state(), ar.state, ar.counter, hip.rng(gpu).state,
             hip.rng(gpu).counter)
    assert np.array_equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(before[2], after[2]) and before[3] == after[3]
    assert torch.equal(before[4], after[4]) and before[5] == after[5]
    idx = (starts[:, None] + np.arange(S - 1)[None, :]) % d.buffer.capacity
    obs = torch.from_numpy(d.buffer.observation_buffer[idx]).to(gpu).float()
    act = torch.from_numpy(d.buffer.action_buffer[idx]).to(gpu)
    hid = d.world_model.observe_sequence(obs, act)[1]
    assert torch.equal(d.state_entropy(hid), nov)
    with pytest.raises(ValueError):
        d.novelty(starts=starts, length=S + 1)
    with pytest.raises(RuntimeError, match="explore"):
        d.disagreement(hid)
    # Dreamer.knn in "none" mode, against the float64 reference (the rows are far apart against the Gram bound)
    plain = _dreamer(gpu)
    with pytest.raises(RuntimeError, match="explore"):
        plain.novelty(starts=starts)
    c = C.reference(8, "rand")
    q, bank = torch.from_numpy(c["q"]).to(gpu), torch.from_numpy(c["bank"]).to(gpu)
    dist, nn = plain.knn(q.view(3, 43, -1), bank, k=c["k"])
    assert tuple(dist.shape) == (3, 43, c["k"]) and nn.dtype == torch.int32
    f, _, _ = C.check_contract(c, (dist.view(-1, c["k"]) ** 2).cpu().numpy(), nn.view(-1, c["k"]).cpu().numpy())
    assert not [x for x in f if "direct-form" not in x], f[:3]  # (the squared square root is a rounding off d2)
    assert np.all(np.abs(dist.view(-1, c["k"]).cpu().numpy() - np.sqrt(c["T"][np.arange(129)[:, None], nn.view(-1, c["k"]).cpu().numpy()]))
                  <= 1e-6 * (1 + dist.view(-1, c["k"]).cpu().numpy()))
    own, own_i = plain.knn(bank)  # among themselves: k = explore_knn's default, never the row itself
    assert tuple(own.shape) == (257, 12) and not (own_i.cpu() == torch.arange(257)[:, None]).any()
    se = plain.state_entropy(bank, k=12)
    assert torch.equal(se, torch.log1p(own.mean(dim=1))) or torch.allclose(se, torch.log1p(own.mean(dim=1)), rtol=1e-6)
    with pytest.raises(ValueError):
        plain.knn(q, bank[:, :5])


def test_data_parallel_raises(gpu):
    from dreamer_amd.engine import ImaginationEngine
    d = _dreamer(gpu, **ON)
    with pytest.raises(ValueError, match="data parallelism"):
        ImaginationEngine(d, world=(0, 1, None))
    d.world = (0, 1, None)
    with pytest.raises(ValueError, match="data parallelism"):
        d.train_Agent()
