"""tests/step_ops_ref.py and tests/step_ops_cases.py without a GPU.

The references agree with oracle.dreamer_oracle (gru / gru_manual, sample_onehot, actor_act) on ordinary inputs to
float32 rounding, and the actor head's closed-form backward with float64 autograd on unsaturated inputs, so a wrong
reference cannot fail a right kernel or pass a wrong one.  The inputs of tests/test_gpu_step_ops.py are sensitive:
each mutation of step_ops_ref.MUTATIONS moves at least one element of one output by at least 100 of that output's
tolerances (so every measured bound sits below a hundredth of the smallest mutation effect).  The comparison itself
catches a stray write, an unwritten element and a wrong value; the sampler's cases leave out at most 1% of their
groups; the hook refuses what it documents, by error code, before anything is launched."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import step_ops_cases as C
import step_ops_ref as R
from oracle import dreamer_oracle as O

U = R.U
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dreamer_amd", "libdreamer_hip.so")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _near(got, want, units, scale=None, what=""):
    """|got - want| <= units 2^-24 scale (scale: max |want| by default): the oracle's float32 rounding."""
    got, want = got.double(), want.double()
    sc = float(want.abs().max()) if scale is None else scale
    err = float((got - want).abs().max())
    assert err <= units * U * sc, (what, err, units * U * sc)


# ----------------------------------------------------------------------------
# the references against the oracle
# ----------------------------------------------------------------------------
def test_gru_matches_oracle():
    g = _gen(1)
    B, Rr, Cc, A, Hd = 6, 4, 5, 3, 24
    z = F.one_hot(torch.randint(0, Cc, (B, Rr), generator=g), Cc).float()
    a, h = torch.randn(B, A, generator=g), torch.randn(B, Hd, generator=g)
    w_ih, w_hh = torch.randn(3 * Hd, Rr * Cc + A, generator=g) * 0.3, torch.randn(3 * Hd, Hd, generator=g) * 0.2
    b_ih, b_hh = torch.randn(3 * Hd, generator=g) * 0.3, torch.randn(3 * Hd, generator=g) * 0.3
    r = R.gru(z, a, h, w_ih.t().contiguous(), b_ih, w_hh, b_hh)
    x = torch.cat([z.reshape(B, -1), a], 1)
    _near(r["hout"], O.gru_manual(x, h, w_ih, w_hh, b_ih, b_hh), 64, scale=1.0, what="gru_manual")
    P = {O.WM + "sequence_model.GRU.weight_ih": w_ih, O.WM + "sequence_model.GRU.weight_hh": w_hh,
         O.WM + "sequence_model.GRU.bias_ih": b_ih, O.WM + "sequence_model.GRU.bias_hh": b_hh}
    _near(r["hout"], O.gru(z.unsqueeze(1), h.unsqueeze(1), a.unsqueeze(1), P).squeeze(1), 64, scale=1.0, what="gru_cell")
    # the saves are gru_cell's own intermediates
    gi, gh = F.linear(x, w_ih, b_ih), F.linear(h, w_hh, b_hh)
    _near(r["sr"], torch.sigmoid(gi[:, :Hd] + gh[:, :Hd]), 64, scale=1.0, what="r")
    _near(r["su"], torch.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd]), 64, scale=1.0, what="u")
    _near(r["sghn"], gh[:, 2 * Hd:], 64, what="gh_n")
    _near(r["sn"], torch.tanh(gi[:, 2 * Hd:] + r["sr"].float() * gh[:, 2 * Hd:]), 64, scale=1.0, what="n")
    r0 = R.gru(z, a, None, w_ih.t().contiguous(), b_ih, w_hh, b_hh)
    _near(r0["hout"], O.gru_manual(x, torch.zeros(B, Hd), w_ih, w_hh, b_ih, b_hh), 64, scale=1.0, what="h == NULL")
    gg = R.gru_gates(gi.double(), gh.double(), h.double())
    _near(gg["hout"], O.gru_manual(x, h, w_ih, w_hh, b_ih, b_hh), 64, scale=1.0, what="gru_gates")


def test_zgather_add_is_the_latent_part_of_a_linear():
    g = _gen(2)
    M, Rr, Cc, N = 5, 4, 6, 12
    z = F.one_hot(torch.randint(0, Cc, (M, Rr), generator=g), Cc).float()
    w, base = torch.randn(N, Rr * Cc, generator=g), torch.randn(M, N, generator=g)
    _near(R.zgather_add(z, w.t().contiguous(), base)["out"], base + F.linear(z.reshape(M, -1), w), 32, what="out")


def test_sampler_matches_oracle():
    g = _gen(3)
    M, Rr, Cc = 7, 3, 5
    logits = torch.randn(M, Rr, Cc, generator=g) * 2
    q = torch.empty(2, M * Rr, Cc).exponential_(generator=g)
    for step in (0, 1):
        z, idx, probs = O.sample_onehot(logits, q[step], Cc)
        r = R.sample(logits, q, step)
        assert torch.equal(r["win"], idx)
        _near(r["pu"], probs, 8, scale=1.0, what="unimixed probabilities")
        zr = F.one_hot(r["win"], Cc).float() * R.ste_value(r["p"].float(), Cc)
        _near(zr, z, 4, scale=1.0, what="straight-through latent")
        assert float(r["margin"].min()) > C.MARGIN


def test_actor_head_matches_oracle():
    g = _gen(4)
    B, Hd, Rr, Cc, A, Hn = 6, 10, 2, 4, 3, 16
    P = {}
    for name, (o, i) in (("base_net.0", (Hn, Hd + Rr * Cc)), ("base_net.3", (Hn, Hn)), ("mu_head", (A, Hn)), ("log_sig_head", (A, Hn))):
        P[O.AG + f"actor.{name}.weight"] = torch.randn(o, i, generator=g) * 0.5
        P[O.AG + f"actor.{name}.bias"] = torch.randn(o, generator=g) * 0.5
    for name in ("base_net.1", "base_net.4"):
        P[O.AG + f"actor.{name}.weight"], P[O.AG + f"actor.{name}.bias"] = torch.ones(Hn), torch.zeros(Hn)
    P[O.AG + "actor.log_sig_head.weight"] *= 4  # some rows beyond the clamp
    h, z = torch.randn(B, 1, Hd, generator=g), F.one_hot(torch.randint(0, Cc, (B, 1, Rr), generator=g), Cc).float()
    eps = torch.randn(B, 1, A, generator=g)
    st = torch.cat([h, z.flatten(2)], -1)
    x = F.silu(O._ln(O._lin(st, P, O.AG + "actor.base_net.0"), P, O.AG + "actor.base_net.1"))
    x = F.silu(O._ln(O._lin(x, P, O.AG + "actor.base_net.3"), P, O.AG + "actor.base_net.4"))
    mu_raw, ls_raw = O._lin(x, P, O.AG + "actor.mu_head").squeeze(1), O._lin(x, P, O.AG + "actor.log_sig_head").squeeze(1)
    assert bool((ls_raw > 2).any()) and bool((ls_raw < -5).any())
    for det in (0, 1):
        a, mu, sigma = O.actor_act(h, z, P, None if det else eps)
        r = R.actor_head(mu_raw, ls_raw, eps.squeeze(1), det)
        _near(r["a"], a.squeeze(1), 16, scale=1.0 + float(mu_raw.abs().max()), what="a")
        _near(r["sigma"], sigma.squeeze(1), 8, what="sigma")
        assert torch.equal(r["mu"], mu.squeeze(1).double())


def test_actor_head_backward_matches_float64_autograd():
    """On unsaturated inputs with ls off the clamp's edges; a is the float64 tanh itself, so 1 - a^2 = 1 - tanh^2."""
    g = _gen(5)
    M, A, N = 9, 3, 7
    mu = torch.randn(M, A, generator=g, dtype=torch.float64).requires_grad_(True)
    ls = (torch.randn(M, A, generator=g, dtype=torch.float64) * 4 - 1.5).requires_grad_(True)
    eps, g_a = torch.randn(M, A, generator=g, dtype=torch.float64), torch.randn(M, A, generator=g, dtype=torch.float64)
    g_mu_l, g_sig_l = torch.randn(M, A, generator=g, dtype=torch.float64), torch.randn(M, A, generator=g, dtype=torch.float64)
    wt = torch.randn(N, 2 * A, generator=g, dtype=torch.float64)
    sigma = F.softplus(torch.clamp(ls, -5.0, 2.0)) + R.E3
    a = torch.tanh(mu + eps * sigma)
    loss = (a * g_a).sum() + (mu * g_mu_l).sum() + (sigma * g_sig_l).sum()
    gm, gl = torch.autograd.grad(loss, [mu, ls])
    r = R.actor_head_bwd_x(g_a, g_mu_l, g_sig_l, a.detach(), ls.detach(), eps, wt)
    assert bool((ls.detach() > 2).any()) and bool((ls.detach() < -5).any())
    assert torch.allclose(r["g_heads"], torch.cat([gm, gl], 1), rtol=1e-12, atol=1e-14)
    assert torch.allclose(r["gx"], torch.cat([gm, gl], 1) @ wt.t(), rtol=1e-12, atol=1e-14)
    # the clamp is closed at both ends, like torch.clamp's gradient
    e = torch.tensor([[-5.0, 2.0, C.nextf(-5.0, False), C.nextf(2.0, True)]], dtype=torch.float64).requires_grad_(True)
    ge, = torch.autograd.grad(F.softplus(torch.clamp(e, -5.0, 2.0)).sum(), e)
    one = torch.ones(1, 4)
    re = R.actor_head_bwd_x(None, None, one, None, e.detach(), None, torch.zeros(1, 8))
    assert torch.allclose(re["g_heads"][:, 4:], ge, rtol=1e-14, atol=0) and bool((ge[0, :2] > 0).all()) and bool((ge[0, 2:] == 0).all())
    # every optional input is a zero
    z = torch.zeros(M, A)
    full = R.actor_head_bwd_x(z, z, g_sig_l.float(), a.detach().float(), ls.detach().float(), eps.float(), wt.float())
    none = R.actor_head_bwd_x(None, None, g_sig_l.float(), None, ls.detach().float(), None, wt.float())
    assert torch.equal(full["g_heads"], none["g_heads"])


def test_onehot_index_and_bf16():
    z = torch.tensor([[[0.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.25, 0.0, 0.5], [-0.0, 0.0, -2.0], [float("nan"), 0.0, 0.0]]])
    idx, zval = R.onehot_index(z)
    assert idx.tolist() == [[0, 1, -1, 2, 0]]
    assert zval[0, :4].tolist() == [0.0, 1.5, 0.0, -2.0] and bool(torch.isnan(zval[0, 4]))
    y = torch.randn(4096, generator=_gen(6))
    assert torch.equal(R.bf16_bits(y), y.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF)
    assert not torch.equal(R.bf16_bits(y, "gru_bf16_truncate"), R.bf16_bits(y))


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def _live(op):
    return [c for c in C.cases_by_op()[op] if not c.refuse]


def test_shapes_the_cases_cover():
    by = C.cases_by_op()
    assert sorted(by) == sorted(R.OP_NAMES)
    gru = _live("gru")
    fused = [c for c in gru if not (c.slots[15] is not None and c.v[0] >= 128)]
    split = [c for c in gru if c.slots[15] is not None and c.v[0] >= 128]
    assert {(c.v[0], c.v[1]) for c in fused} >= {(b, h) for b in C.GRU_FUSED_B for h in C.GRU_FUSED_HD} | {(1, 644), (17, 644), (130, 36), (127, 36)}
    assert {(c.v[0], c.v[1]) for c in split} >= {(b, h) for b in C.GRU_SPLIT_B for h in C.GRU_SPLIT_HD}
    assert any(c.v[0] == 127 and c.slots[15] is not None for c in fused) and any(c.v[0] == 130 and c.slots[15] is None for c in fused)
    assert {C.gru_tiles(c.v[0], c.v[1], False) for c in fused} >= {1, 7, 8, 9, 17}
    assert {c.v[4] for c in fused} == {1, 3, 8} and {tuple(c.v[2:4]) for c in fused} == {(4, 3), (12, 8), (32, 33)}
    for cs in (fused, split):
        assert {c.slots[4] is None for c in cs} == {True, False}       # h
        assert {c.slots[10] is None for c in cs} == {True, False}      # hout16
        assert {c.slots[11] is None for c in cs} == {True, False}      # the saves
        assert {c.label.split("-", 1)[1] for c in cs} >= {"dense-one", "dense-several", "dense-all", "gates", "nan-row"}
    for c in gru:  # no dense marker without the latent rows behind it
        assert c.slots[2] is not None or bool((c.slots[0] >= 0).all()), c
    assert {(c.v[0], c.v[1]) for c in _live("zgather_add")} >= {(m, n) for m in C.ZG_M for n in C.ZG_N}
    assert {c.v[2] for c in _live("zgather_add")} == {4, 12, 32}
    assert {c.label for c in by["zgather_add"] if c.refuse} == {
        "refuse-N6", "refuse-ldw", "refuse-ldb", "refuse-ldo", "refuse-R33", "refuse-misaligned-wt", "refuse-misaligned-base",
        "refuse-misaligned-out"}
    assert {(c.v[0] * c.v[1], c.v[2]) for c in _live("onehot_index")} == {(m * r, k) for m, r in C.ONEHOT_MR for k in C.ONEHOT_C}
    assert {c.v[0] * c.v[1] for c in _live("gru_fwd")} == {1, 255, 256, 257, 1000}
    for Cc in C.SAMPLE_C:
        W = C.pow2_ge(Cc)
        th = {c.v[0] * c.v[1] * W for c in _live("sample") if c.v[2] == Cc}
        assert any(t < 256 or t % 256 for t in th) and any(t > 256 for t in th) and 256 in th or W == 1 and 256 in th, (Cc, th)
    assert {c.v[6] for c in _live("sample")} == {0, 2}
    assert {c.slots[3] is None for c in _live("sample")} == {True, False} and {c.slots[4] is None for c in _live("sample")} == {True, False}
    assert {c.v[2] for c in by["sample"] if c.refuse} == {0, 65}
    ah = _live("actor_head")
    assert {c.v[1] for c in ah} == {1, 3, 8} and {c.v[8] for c in ah} == {0, 1}
    assert {c.v[0] * c.v[1] for c in ah} >= {255, 256, 257, 258, 264}
    for slot in (3, 4, 5, 6):
        assert any(c.slots[slot] is None for c in ah)
    bw = _live("actor_head_bwd_x")
    assert {(c.v[0], c.v[2]) for c in bw} == {(m, n) for m in (1, 15, 16, 17, 33) for n in C.BWD_N}
    assert {c.v[1] for c in bw} == {1, 3, 8}
    assert {tuple(c.slots[i] is None for i in range(3)) for c in bw} == {(False,) * 3, (True, False, False), (False, True, False), (False, False, True)}
    assert [c.v[1] for c in by["actor_head_bwd_x"] if c.refuse] == [9]
    assert {c.v[0] for c in _live("mean")} == set(C.MEAN_N)
    assert {tuple(c.v) for c in _live("transpose")} == {(r, k) for r in C.T_SIZES for k in C.T_SIZES}
    assert {c.v[0] for c in by["transpose_multi"]} >= {10, 11} and {c.v[0] for c in by["copy2d_multi"]} >= {4, 5}
    assert {c.label for c in by["copy2d"]} == {f[0] for f in C.COPY_FORMS}
    assert any(c.v[0] == 4 * (2048 * 256 + 3) for c in by["fill"]) and any(isinstance(c.slots[0], C.Shift) for c in by["fill"])
    assert {c.v[2] for c in _live("vec_gather")} == {1, 5, 64} and len([c for c in by["vec_gather"] if c.refuse]) == 5
    for op, cs in by.items():  # a leading dimension wider than the logical width in at least one case per op
        if op in ("mean", "fill", "transpose", "onehot_index", "vec_gather"):  # no leading dimension on the output side
            continue
        assert any(any(isinstance(s, C.Out) and len(s.shape) == 2 and s.region[1] != slice(None) for s in c.outs()) for c in cs), op
    for op in R.OP_NAMES:
        print(f"{op}: {len(by[op])} cases ({len([c for c in by[op] if c.refuse])} refusals)")


def test_sampler_leaves_out_at_most_one_percent():
    n = 0
    for case in _live("sample"):
        M, Rr, Cc, step = case.v[0], case.v[1], case.v[2], case.v[6]
        logits = case.slots[0][:M, :Rr * Cc].reshape(M, Rr, Cc)
        q = case.slots[1].reshape(step + 1, M * Rr, Cc)
        r = R.sample(logits, q, step)
        left = float((r["margin"] < C.MARGIN).double().mean())
        assert left <= C.MAX_LEFT_OUT, (case, left)
        n += int((r["margin"] < C.MARGIN).sum())
    print(f"{n} groups left out of the idx comparison")


def _emulate(case):
    """The reference written into the buffers as the op would write it."""
    w, bufs = case.wants(), {}
    for o in case.outs():
        b = o.make()
        if o.name in w:
            ref = w[o.name].ref.reshape(b[o.region].shape)
            b[o.region] = ref.to(b.dtype)
        bufs[o.name] = b
    return bufs


def test_the_reference_in_the_buffers_passes_and_breaks_are_caught():
    for op in R.OP_NAMES:
        for case in _live(op)[:4]:
            # (the bit-exact claims are the device's: they are made of its own float32 outputs)
            fails = [f for f in C.compare(case, _emulate(case)) if "exactly" not in f and "bit for bit" not in f
                     and "is not" not in f and "the g_a path" not in f and "changes under" not in f]
            assert fails == [], (case, fails)
    case = next(c for c in _live("gru") if c.label == "fused-B17-Hd36")
    bufs = _emulate(case)
    bufs["hout"][17, 0] = 1.0    # a row >= B
    assert any("hout" in f and "outside the output" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["sr"][3, 35] = C.poison(1)[0]
    assert any("sr" in f and "unwritten" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["hout"][0, 36] = 0.0    # a column past Hd, inside ldo
    assert any("hout" in f and "outside the output" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["sn"][2, 7] += 1e-3
    assert any("sn" in f and "beyond tolerance" in f for f in C.compare(case, bufs))
    ws = next(c for c in _live("gru") if c.label == "fused-B127-ws")
    bufs = _emulate(ws)
    bufs["gh_ws"][0] = 0.0       # the fused form must leave the scratch alone
    assert any("gh_ws" in f and "must not be" in f for f in C.compare(ws, bufs))
    ref = next(c for c in C.cases_by_op()["mean"] if c.refuse)
    bufs = {o.name: o.make() for o in ref.outs()}
    assert C.untouched(ref, bufs) == []
    bufs["out"][1] = 0.0
    assert C.untouched(ref, bufs) != []


def test_measured_table_is_complete():
    """Every output compared at a measured bound has its entry: no bound is made up while the suite runs."""
    keys = {w.key for cs in C.cases_by_op().values() for c in cs if not c.refuse for w in c.wants().values() if w.key}
    assert keys == set(C.MEASURED), (sorted(keys - set(C.MEASURED)), sorted(set(C.MEASURED) - keys))


# the mutations of an output that is an exact function of the device's own other outputs (Case.given)
GIVEN_MUTANTS = ("gru_bf16_truncate", "sample_no_unimix", "sample_q_step0")


@pytest.mark.parametrize("mut", sorted(R.MUTATIONS))
def test_inputs_see_the_mutation(mut):
    """The mutated reference differs from the reference by >= 100 tolerances on at least one element of one output of
    one case of the GPU test (a NaN or infinite difference is not counted as seen)."""
    best, where = 0.0, None
    for case in _live(R.MUTATIONS[mut]):
        w0, w1 = case.wants(), case.ref(mut)
        for k, a in w0.items():
            if k in case.given and mut not in GIVEN_MUTANTS:
                continue  # an exact output sees any change: the mutation must show in an output with a tolerance
            d = (w1[k].ref - a.ref).abs()
            d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
            ratio = torch.where(d > 0, d / a.tol.clamp(min=1e-300), torch.zeros_like(d))
            if ratio.numel() and float(ratio.max()) > best:
                best, where = float(ratio.max()), (case, k)
        if best >= 1e6:
            break
    print(f"{mut}: {best:.3g} tolerances at {where}")
    assert best >= 100.0, (mut, best, where)


# ----------------------------------------------------------------------------
# the hook's refusals (no GPU: nothing is launched)
# ----------------------------------------------------------------------------
def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_step_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                  ctypes.c_int]
    return f


def _refused(op, v, ptrs=True, num=True):
    va = (ctypes.c_int * 64)(*v) if v is not None else None
    na = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0) if num else None
    pa = (ctypes.c_void_p * 32)() if ptrs else None  # every pointer NULL: a call that got past the checks would fault
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(op, va, na, pa, None, msg, 256)
    assert rc == C.DR_E_INVALID and msg.value, (op, v, rc, msg.value)
    return msg.value.decode()


@pytest.mark.skipif(not os.path.exists(LIB), reason="the library is not built")
def test_hook_refuses_what_it_documents():
    from dreamer_amd import _lib
    assert C.DR_E_INVALID == _lib.DR_E_INVALID
    assert "null descriptor" in _refused(R.GRU, None)
    assert "null descriptor" in _refused(R.GRU, [1] * 10, ptrs=False)
    assert "unknown op" in _refused(len(R.OP_NAMES), [1, 1, 1])
    assert "unknown op" in _refused(-1, [1, 1, 1])
    assert "null operand" in _refused(R.GRU, [4, 8, 4, 3, 1, 12, 1, 8, 8, 0])
    assert "stride" in _refused(R.GRU, [4, 8, 4, 3, 1, 11, 1, 8, 8, 0])
    assert "positive" in _refused(R.GRU, [0, 8, 4, 3, 1, 12, 1, 8, 8, 0])
    assert "null operand" in _refused(R.ONEHOT_INDEX, [2, 4, 3, 12])
    assert "stride" in _refused(R.ONEHOT_INDEX, [2, 4, 3, 11])
    assert "null operand" in _refused(R.ZGATHER_ADD, [3, 8, 4, 3, 12, 8, 8, 8])
    assert "null operand" in _refused(R.GRU_FWD, [2, 8, 8, 8])
    assert "stride" in _refused(R.GRU_FWD, [2, 8, 8, 7])
    for Cc in (0, 65, -1, 128):
        assert "[1,64]" in _refused(R.SAMPLE, [2, 3, Cc, 1000, 1000, 1000, 0])
    assert "null operand" in _refused(R.SAMPLE, [2, 3, 8, 24, 24, 24, 0])
    assert "stride" in _refused(R.SAMPLE, [2, 3, 8, 23, 24, 24, 0])
    assert "step" in _refused(R.SAMPLE, [2, 3, 8, 24, 24, 24, -1])
    assert "null operand" in _refused(R.ACTOR_HEAD, [2, 3, 3, 3, 3, 3, 3, 0, 0])
    assert "stride" in _refused(R.ACTOR_HEAD, [2, 3, 2, 3, 3, 3, 3, 0, 0])
    for A in (0, 9, -1):
        assert "actions" in _refused(R.ACTOR_HEAD_BWD_X, [4, A, 64, 9, 9, 9, 9, 18, 64])
    assert "N >= 1" in _refused(R.ACTOR_HEAD_BWD_X, [4, 3, 0, 3, 3, 3, 3, 6, 0])
    assert "null operand" in _refused(R.ACTOR_HEAD_BWD_X, [4, 3, 64, 3, 3, 3, 3, 6, 64])
    assert "stride" in _refused(R.ACTOR_HEAD_BWD_X, [4, 3, 64, 3, 3, 3, 3, 5, 64])
    assert "null operand" in _refused(R.SIGMOID, [4, 1, 1])
    for n in (0, -5):
        assert "positive" in _refused(R.MEAN, [n])
    assert "null operand" in _refused(R.MEAN, [4])
    for rows, cols in ((0, 4), (4, 0), (-1, 4)):
        assert "positive" in _refused(R.TRANSPOSE, [rows, cols])
    assert "null operand" in _refused(R.TRANSPOSE, [4, 4])
    assert "at most" in _refused(R.TRANSPOSE_MULTI, [11] + [2, 2, 2] * 11)
    assert "null operand" in _refused(R.TRANSPOSE_MULTI, [2] + [2, 2, 2] * 2)
    assert "at most" in _refused(R.COPY2D_MULTI, [5] + [4, 4, 4, 2] * 5)
    assert "pitch" in _refused(R.COPY2D_MULTI, [1, 3, 4, 4, 2])
    assert "null operand" in _refused(R.COPY2D, [4, 4, 4, 2])
    assert "null operand" in _refused(R.FILL, [4])
    assert "num" in _refused(R.FILL, [4], num=False)
    assert "null operand" in _refused(R.VEC_GATHER, [12, 3, 5, 7, 0, 0, 0])
