"""tests/gemm_ref.py on the CPU: the float64 reference against plain torch on tiny shapes, field by field; the integer
pass's exactness claim; the sampler tie guard on the reference alone; the left-out list; the misalignment nibbles."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R
import test_gemm_plan_host as H
from test_gemm_plan_host import ACC, G_NN, G_NT, G_TN, LNBWD, LNSILU, PLAIN, STEBWD, prob

CASES = H._cases()
RUN = sorted(n for n in CASES if R.left_out(n) is None)


def raw(p, name):
    """A matrix read out of its store element by element: independent of Buf.view's strides."""
    b = p.buf[name]
    s = b.store.double()
    return torch.tensor([[float(s[b.off + r * b.ld + c]) for c in range(b.cols)] for r in range(b.rows)],
                        dtype=torch.float64).reshape(b.rows, b.cols)


def one(case, fields=None, mode="rand", seed=1):
    probs = R.materialise(case, mode, seed, fields)
    return probs[0], R.reference(case[0], case[1], probs)[0]


def test_nt_every_epilogue_field():
    fl = H.A2 | H.BIAS | H.ADDEND | ACC
    case = (G_NT, PLAIN, [prob(5, 7, 6, fl, lda=5, lda2=3, ksA=4, ldb=9, ldy=6)])
    for act in (0, 1, 2):
        p, e = one(case, [dict(alpha=-2.0, act=act, addend=11, nsplitY=4, ldy2=5)])
        a = torch.cat([raw(p, "A"), raw(p, "A2")], 1)
        assert a.shape == (5, 6) and p.buf["W"].ld == 9 and p.buf["addend"].ld == 11 and p.buf["Y2"].ld == 5
        v = -2.0 * a @ raw(p, "W").t() + raw(p, "bias") + raw(p, "addend")
        v = [v, F.silu(v), torch.sigmoid(v)][act] + torch.cat([raw(p, "Y"), raw(p, "Y2")], 1)
        assert torch.equal(e["Y"], v[:, :4]) and torch.equal(e["Y2"], v[:, 4:])
        ab = 2.0 * a.abs() @ raw(p, "W").abs().t() + raw(p, "bias").abs() + raw(p, "addend").abs()
        assert torch.allclose(e["abs"], ab + torch.cat([raw(p, "Y"), raw(p, "Y2")], 1).abs(), rtol=1e-15, atol=0)


def test_nn_w2_both_ways_and_tn():
    p, e = one((G_NN, PLAIN, [prob(3, 6, 8, H.W2, ldb=7)]), [dict(ksplitB=5, ldb2=10)])
    assert torch.equal(e["Y"], raw(p, "A") @ torch.cat([raw(p, "W"), raw(p, "W2")], 0))
    assert raw(p, "W").shape == (5, 6) and raw(p, "W2").shape == (3, 6)
    p, e = one((G_NN, PLAIN, [prob(3, 6, 8, H.W2, ldb=7)]), [dict(nsplitB=2, ldb2=4)])
    assert torch.equal(e["Y"], raw(p, "A") @ torch.cat([raw(p, "W"), raw(p, "W2")], 1))
    assert raw(p, "W").shape == (8, 2) and raw(p, "W2").shape == (8, 4)
    p, e = one((G_TN, PLAIN, [prob(3, 6, 8, lda=4, ldb=7)]))
    assert raw(p, "A").shape == (8, 3) and torch.equal(e["Y"], raw(p, "A").t() @ raw(p, "W"))


def test_out_conv_is_the_nchw_permutation():
    p, e = one((G_NN, PLAIN, [prob(6, 5, 4, H.OUT_CONV, ldb=5)]), [dict(ohow=3)])
    y = raw(p, "A") @ raw(p, "W")
    for m in range(6):
        for n in range(5):
            assert e["Y"][(m // 3) * 5 + n, m % 3] == y[m, n]  # Y[frame][n][pixel]
    assert p.buf["Y"].rows == 10 and p.buf["Y"].cols == 3


def test_lnsilu_is_layernorm_then_silu():
    p, e = one((G_NT, LNSILU, [prob(4, 3, 8, H.LN | H.AOUT | H.BIAS)]))
    ln = torch.nn.LayerNorm(8, eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(raw(p, "ln_g")[0]); ln.bias.copy_(raw(p, "ln_b")[0])
        a = torch.nn.SiLU()(ln(raw(p, "A")))
    assert torch.allclose(e["a_out"], a, rtol=1e-13, atol=1e-15)
    assert torch.allclose(e["Y"], a @ raw(p, "W").t() + raw(p, "bias"), rtol=1e-13, atol=1e-15)


def test_lnbwd_matches_the_closed_form():
    """ops.hip k_ln_silu_bwd: dy = gx s (1 + y (1 - s)), g_pre = rstd (dxh - mean(dxh) - xh mean(dxh xh))."""
    p, e = one((G_NT, LNBWD, [prob(4, 3, 8, H.LN | H.PRE | H.AOUT)]), [dict(sv=True)])
    pre, gx, gm, bt = raw(p, "pre"), raw(p, "A"), raw(p, "ln_g")[0], raw(p, "ln_b")[0]
    mean, var = pre.mean(1, keepdim=True), pre.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-5)
    xh = (pre - mean) * rstd
    y = xh * gm + bt
    s = torch.sigmoid(y)
    dy = gx * s * (1 + y * (1 - s))
    dxh = dy * gm
    g_pre = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    for name, want in (("a_out", g_pre), ("sv_gy", dy), ("sv_xh", xh), ("Y", g_pre @ raw(p, "W").t())):
        assert torch.allclose(e[name], want, rtol=1e-11, atol=1e-13), name


def test_stebwd_matches_the_closed_form():
    """ops.hip k_softmax_ste_bwd: a = s (0.99 g - sum_group(0.99 g s))."""
    p, e = one((G_NT, STEBWD, [prob(3, 2, 8, H.PRE, C=4)]))
    s, g = raw(p, "pre").reshape(3, 2, 4), raw(p, "A").reshape(3, 2, 4)
    assert torch.allclose(s.sum(-1), torch.ones(3, 2, dtype=torch.float64), atol=1e-6)
    a = (s * (0.99 * g - (0.99 * g * s).sum(-1, keepdim=True))).reshape(3, 8)
    assert torch.allclose(e["Y"], a @ raw(p, "W").t(), rtol=1e-5, atol=1e-7)  # (the f32 softmax rows sum to 1 +- 1e-7)


def test_gru_epilogue_matches_gru_cell_autograd():
    """One row through torch.gru_cell itself: W_ih = I, so the input is the gate pre-activations; W_hh = 0 and
    b_hh = (0, 0, hn), so the hidden side is the saved hn and h reaches h' directly alone, as in the epilogue."""
    Hd = 3
    p, e = one((G_NT, PLAIN, [prob(1, 5, 6, ACC)]), [dict(gru=Hd)])
    gen = p.gen
    x = torch.cat([gen["pr"], gen["pu"], gen["in"]], 1).clone().requires_grad_(True)
    b_hh = torch.cat([torch.zeros(2 * Hd, dtype=torch.float64), gen["hn"][0]]).requires_grad_(True)
    h = gen["h"].clone().requires_grad_(True)
    eye, zero = torch.eye(3 * Hd, dtype=torch.float64), torch.zeros(3 * Hd, dtype=torch.float64)
    h1 = torch.gru_cell(x, h, eye, torch.zeros(3 * Hd, Hd, dtype=torch.float64), zero, b_hh)
    (h1 * e["Y"][:, :Hd]).sum().backward()
    assert torch.allclose(e["gb_gi"], x.grad, rtol=1e-12, atol=1e-14)
    assert torch.allclose(e["gb_gh"][:, :2 * Hd], x.grad[:, :2 * Hd], rtol=1e-12, atol=1e-14)
    assert torch.allclose(e["gb_gh"][0, 2 * Hd:], b_hh.grad[2 * Hd:], rtol=1e-12, atol=1e-14)
    assert torch.allclose(e["gb_ho"], raw(p, "gb_ho") + h.grad, rtol=1e-12, atol=1e-14)
    r, u = torch.sigmoid(gen["pr"]), torch.sigmoid(gen["pu"])
    assert torch.allclose(raw(p, "gb_r"), r, atol=1e-7) and torch.allclose(raw(p, "gb_u"), u, atol=1e-7)
    assert torch.allclose(raw(p, "gb_n"), torch.tanh(gen["in"] + r * gen["hn"]), atol=1e-7)
    assert torch.equal(raw(p, "gb_ghn"), gen["hn"]) and torch.equal(raw(p, "gb_h"), gen["h"])


def test_sampler_and_actor_epilogues():
    p, e = one((G_NT, PLAIN, [prob(3, 8, 5, H.BIAS, epi=R.SAMPLE, C=4, R=2)]))
    lg = (raw(p, "A") @ raw(p, "W").t() + raw(p, "bias")).reshape(3, 2, 4)
    pm = 0.99 * torch.softmax(lg, -1) + 0.01 / 4
    assert torch.equal(e["idx"], (pm / pm.sum(-1, keepdim=True) / raw(p, "q").reshape(3, 2, 4)).argmax(-1))
    assert torch.allclose(e["soft"].reshape(3, 2, 4), torch.softmax(lg, -1)) and bool((raw(p, "q") > 0).all())
    assert torch.equal(e["z_out"].reshape(3, 2, 4).argmax(-1), e["idx"]) and float(e["z_out"].sum()) == 6
    p, e = one((G_NT, PLAIN, [prob(3, 4, 5, H.BIAS, epi=R.ACTOR, na=2)]))
    y = raw(p, "A") @ raw(p, "W").t() + raw(p, "bias")
    sg = torch.log1p(torch.exp(y[:, 2:].clamp(-5, 2))) + 1e-3
    assert torch.allclose(e["sig"], sg) and torch.equal(e["mu"], y[:, :2])
    assert torch.allclose(e["act"], torch.tanh(y[:, :2] + raw(p, "eps") * sg))


def test_bf16_rounding_is_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -3.0], dtype=torch.float64)
    assert R.bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0, -3.0]


def _all_problem_lists():
    import test_gpu_gemm_routes as T
    for n in RUN:
        yield n, CASES[n], R.table_fields(n, CASES[n])
    for fam in T.FAMILY_SHAPES:
        for fld in T.FIELDS:
            case, f, _ = T.field_case(fam, fld)
            yield f"{fam} {fld}", case, f


def test_integer_pass_is_exact_in_f32_and_bf16():
    """|operand| <= 3, |alpha| <= 2: every partial sum of alpha * sum_k a b is an integer (or a half) below
    2 * 9 * K, far under 2^24, so f32 adds it exactly in any order; with bias, addend and Y0 the same.  -3 .. 3 are
    exact in bf16, so the bf16 routes and plane 0 of the split (remaining planes zero) compute the same integers."""
    ints = torch.arange(-3, 4, dtype=torch.float64)
    assert torch.equal(R.bf16(ints), ints)
    for name, case, f in _all_problem_lists():
        for v, fl in zip(case[2], f or [{}] * len(case[2])):
            assert 2 * (9 * v[2] + 9) < 2 ** 24 / 2, name  # halves (alpha = 0.5) need one bit more
            assert abs(fl.get("alpha", 1.0)) in (1.0, 0.5, 2.0)
    # and on a case: the float64 reference of the integer inputs holds only multiples of 1/2 under 2^23
    p, e = one(CASES["maxM 127"], mode="int")
    assert torch.equal(e["Y"], e["Y"].round()) and float(e["Y"].abs().max()) < 2 ** 23
    assert torch.equal(e["Y"].float().double(), e["Y"])


def test_the_two_passes_catch_the_bugs_they_are_for():
    """A bias applied once per split and a k term lost in one column's tail, simulated on the reference: the integer
    pass sees both in every affected element, the random pass's derived bound in some."""
    case = (G_NT, PLAIN, [prob(256, 200, 1620, H.BIAS)])
    for mode in ("int", "rand"):
        p, e = one(case, mode=mode)
        a, w, bias = p.buf["A"].f64(), p.buf["W"].f64(), p.buf["bias"].f64()
        per_split = e["Y"] + 3 * bias
        tail = e["Y"].clone()
        tail[:, -1] -= a[:, -1] * w[-1, -1]
        for got, hit in ((per_split, (bias != 0).expand(256, 200)), (tail, (e["Y"] != tail))):
            if mode == "int":
                assert torch.equal((got.float() != e["Y"].float()), hit) and bool(hit.any())
            else:
                assert bool(((got - e["Y"]).abs() > R.f32_bound(1620, e["abs"], e["Y"])).any())


SAMPLER_CASES =[n for n in RUN if any((v[11] >> 8) & 3 == R.SAMPLE for v in CASES[n][2])]


@pytest.mark.parametrize("name", SAMPLER_CASES)
def test_tie_guard_cap_holds_on_the_reference_alone(name):
    """Draws whose top two scores lie within 1e-4 relative are exempt from the index comparison (the rule of
    gpu_helpers.flip_report); at the seeds the GPU test uses they stay under 1e-3 of a case's draws."""
    case = CASES[name]
    probs = R.materialise(case, "rand", 0, R.table_fields(name, case))
    for p, e in zip(probs, R.reference(case[0], case[1], probs)):
        close = int((e["margin"] < 1e-4).sum())
        assert close <= 1e-3 * e["margin"].numel(), (name, close, e["margin"].numel())


def test_left_out_list_matches_the_table():
    assert sorted(n for n in CASES if R.left_out(n)) == R.LEFT_OUT
    assert len(RUN) + len(R.LEFT_OUT) == len(CASES) == len(H.EXPECT)
    for n in RUN:  # what runs stays small: at most 10256 rows, 2052 columns (the widest mlp3 layer), K 3840
        for v in CASES[n][2]:
            assert v[0] <= 10256 and v[1] <= 2052 and v[2] <= 3840, n


@pytest.mark.parametrize("name", RUN)
def test_materialiser_honours_strides_and_nibbles(name):
    case = CASES[name]
    probs = R.materialise(case, "int", 0, R.table_fields(name, case))
    for p, v in zip(probs, case[2]):
        for slot in R.SLOTS:
            if slot in p.buf:
                b = p.buf[slot]
                assert R.pointer(b, b.store) % 16 == p.nib(slot), (name, slot)
                assert b.store.numel() >= b.off + b.rows * b.ld + R.GUARD
        assert p.buf["A"].ld == v[3] and p.buf["W"].ld == v[6]
        if not v[11] & H.OUT_CONV:
            assert p.buf["Y"].ld == v[7]
        if "a_out" in p.buf:
            assert p.buf["a_out"].ld == v[16]
        y = p.buf["Y"]
        assert y.untouched(y.store) and not y.untouched(y.store + 0 * y.store)  # SENT is a NaN: arithmetic loses it
    steps, err = H.plan_steps(*case)
    assert err is None and R.route_of(steps, case[2]) == H.route(*case) == H.EXPECT[name]
