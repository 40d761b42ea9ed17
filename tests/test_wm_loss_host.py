"""tests/wm_loss_ref.py and tests/wm_loss_cases.py without a GPU.

The references agree with oracle.dreamer_oracle (wm_losses on the small fixture, _cat_kl, twohot, gru_manual, _ln,
sample_onehot) on ordinary inputs to float32 rounding, so a wrong reference cannot fail a right kernel or pass a wrong
one.  The inputs of tests/test_gpu_wm_loss.py are sensitive: each mutation of wm_loss_ref.MUTATIONS moves at least one
element of one output by at least 100 of that output's tolerances (so every measured bound sits below a hundredth of
the smallest mutation effect).  The comparison itself catches a stray write, an unwritten element and a wrong value.
The hook refuses what it documents, by error code, before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import primitives_ref as PR
import wm_loss_cases as C
import wm_loss_ref as R
from conftest import fixture_params, load_fixture
from oracle import dreamer_oracle as O
from test_oracle_wm import window

U = R.U


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
def test_loss_construction_matches_oracle_on_the_small_fixture():
    """stats -> final on the oracle's own per-row terms reproduces its losses; prep its denominator."""
    fx = load_fixture("small_wm")
    P = fixture_params("small", fx)
    obs, act, rew, cont, T = window(fx)
    Rr, Cc = int(fx["cfg_rows"]), int(fx["cfg_cols"])
    with torch.no_grad():
        o = O.wm_losses(obs, act, rew, cont, P, torch.from_numpy(fx["q"].copy()), Rr, Cc, T)
    B = cont.shape[0]
    tm = lambda x: x.transpose(0, 1).reshape((T - 1) * B, *x.shape[2:])  # batch-first -> rows m = t B + b
    mask = tm(cont[:, :T - 1]).reshape(-1)
    prior, post = tm(o["prior"]).reshape(-1, Rr, Cc), tm(o["post"]).reshape(-1, Rr, Cc)
    kl_grp = R.kl_fwd(prior, post)["kl_grp"]
    _near(kl_grp.sum(-1), tm(O._cat_kl(o["post"], o["prior"]).sum(-1)), 64, what="row KL")
    s = R.stats(-tm(o["obs_ll"]).reshape(-1, 1), tm(o["rew_ll"]).reshape(-1), tm(o["cont_ll"]).reshape(-1), kl_grp, mask)
    s5 = torch.cat([R.prep(mask, 1.0)["stats0"], s["stats"]])
    f = R.final(s5.float(), B * (T - 1), (1.0, 0.5, 0.1))
    for i, k in enumerate(("total", "loss_pred", "kl_dyn", "kl_rep")):
        _near(f["losses"][i], o[k], 64, what=k)
    assert float(o["kl_dyn"]) < 1.0 and float(f["scal1"]) == 0.0 and float(f["scal2"]) == 0.0 and f["skip"] == 0
    _near(R.prep(mask, 1.0)["scal0"], mask.sum() + 1e-5, 2, what="denominator")


def test_kl_gradients_match_oracle_autograd():
    """The oracle's loss construction (WorldModel.py:175-189 as wm_losses writes it) on random logits with the clamp
    open: d total / d prior and d total / d post in float32 against final's factors and kl_bwd."""
    g = _gen(1)
    M1, Rr, Cc = 12, 4, 6
    prior = (torch.randn(M1, Rr, Cc, generator=g) * 2).requires_grad_(True)
    post = (torch.randn(M1, Rr, Cc, generator=g) * 2).requires_grad_(True)
    mask = (torch.rand(M1, generator=g) > 0.3).float()
    kl_dyn = torch.mean(O._cat_kl(post.detach(), prior).sum(-1) * mask)
    kl_rep = torch.mean(O._cat_kl(post, prior.detach()).sum(-1) * mask)
    one = torch.tensor(1.0)
    total = 0.5 * torch.max(one, kl_dyn) + 0.1 * torch.max(one, kl_rep)
    assert float(kl_dyn.detach()) > 1.0
    gq, gp = torch.autograd.grad(total, [prior, post])
    kl_grp = R.kl_fwd(prior.detach(), post.detach())["kl_grp"]
    s5 = torch.tensor([float(mask.sum()), 0.0, 0.0, 0.0, float((kl_grp.sum(-1) * mask).sum())])
    f = R.final(s5, M1, (1.0, 0.5, 0.1))
    scal = torch.tensor([0.0, float(f["scal1"]), float(f["scal2"])])
    r = R.kl_bwd(prior.detach(), post.detach(), mask, scal)
    _near(r["g_prior"], gq, 32, what="g_prior")
    _near(r["g_post"], gp, 32, what="g_post")


def test_free_bit_factor_is_torchs_max_gradient():
    """1 / 0.5 / 0 for KL >, ==, < 1 (k_wm_final's documented convention)."""
    for s4, wk in ((46.0, 1.0), (45.0, 0.5), (44.0, 0.0)):
        f = R.final(torch.tensor([40.0, 1.0, 1.0, 1.0, s4]), 45, (1.0, 0.5, 0.1))
        assert float(f["scal1"]) == float(np.float32(0.5)) * wk / 45 and float(f["scal2"]) == float(np.float32(0.1)) * wk / 45


def test_heads_match_oracle():
    g = _gen(2)
    M1, nb = 40, 255
    b = torch.linspace(-20, 20, nb)
    rlog, clog = torch.randn(M1, nb, generator=g) * 2, torch.randn(M1, generator=g) * 2
    rew, cont = torch.randn(M1, generator=g) * 3, (torch.rand(M1, generator=g) > 0.3).float()
    coef = torch.rand(M1, generator=g)
    x, xc = rlog.clone().requires_grad_(True), clog.clone().requires_grad_(True)
    rew_ll = torch.sum(O.twohot(rew.unsqueeze(-1), b) * F.log_softmax(x, -1), -1)
    cont_ll = F.binary_cross_entropy_with_logits(xc, cont, reduction="none")
    gx, gxc = torch.autograd.grad((coef * (cont_ll - rew_ll)).sum(), [x, xc])
    r = R.heads(rlog, clog, rew, cont, b, coef)
    # the oracle's two-hot weight is (v - b_lo) / step in float32: about ulp(20) / step of error (test_primitives_ref)
    w_err = 4 * 20 / (40 / 254)
    _near(r["rew_row"], rew_ll.detach(), w_err * 8 + 600, what="rew_row")
    _near(r["cont_row"], cont_ll.detach(), 16, what="cont_row")
    _near(r["g_rew"], gx, w_err + 16, scale=1.0, what="g_rew")
    _near(r["g_cont"], gxc, 16, scale=1.0, what="g_cont")
    _near(PR.twohot(rew, b), O.twohot(rew.unsqueeze(-1), b), w_err, scale=1.0, what="two-hot")


def test_gru_backward_matches_oracle_autograd():
    g = _gen(3)
    Hd = 37
    x = torch.randn(1, 3 * Hd, generator=g).requires_grad_(True)
    bhh = torch.randn(3 * Hd, generator=g).requires_grad_(True)
    h = torch.randn(1, Hd, generator=g).requires_grad_(True)
    hp = O.gru_manual(x, h, torch.eye(3 * Hd), torch.zeros(3 * Hd, Hd), torch.zeros(3 * Hd), bhh)
    g_hp = torch.randn(1, Hd, generator=g)
    g_gi, g_gh, g_h = torch.autograd.grad((hp * g_hp).sum(), [x, bhh, h])
    i_r, i_z, i_n = x.detach().chunk(3, -1)
    h_r, h_z, h_n = bhh.detach().reshape(1, -1).chunk(3, -1)
    sr, su = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    sn = torch.tanh(i_n + sr * h_n)
    prev = torch.randn(1, Hd, generator=g)
    r = R.gru_bwd(g_hp, h.detach(), sr, su, sn, h_n, prev, 1)
    # the saved gates are float32: 1 - n^2 and (1 - r) r carry their rounding, relative to the gradient's size
    _near(r["g_gi"], g_gi, 64, what="g_gi")
    _near(r["g_gh"], g_gh.reshape(1, -1), 64, what="g_gh")
    _near(r["gh_out"], g_h + prev, 16, what="gh_out")
    r0 = R.gru_bwd(g_hp, None, sr, su, sn, h_n, prev, 0)
    assert torch.allclose(r0["gh_out"], g_hp.double() * su.double(), rtol=1e-12, atol=0)  # h == NULL, no accumulate


def test_ln_silu_backward_matches_oracle_autograd():
    g = _gen(4)
    M, K = 5, 77
    P = {"n.weight": 1 + 0.2 * torch.randn(K, generator=g), "n.bias": 0.1 * torch.randn(K, generator=g)}
    pre = (torch.randn(M, K, generator=g) * 1.5 + 0.3).requires_grad_(True)
    gx = torch.randn(M, K, generator=g)
    y = O._ln(pre, P, "n")
    y.retain_grad()
    (F.silu(y) * gx).sum().backward()
    r = R.ln_silu_bwd(gx, pre.detach(), P["n.weight"], P["n.bias"])
    _near(r["g_pre"], pre.grad, 256, what="g_pre")
    _near(r["gy"], y.grad, 16, what="gy")
    _near(r["xhat"], (y.detach() - P["n.bias"]) / P["n.weight"], 64, what="xhat")


def test_ste_backward_matches_oracle_autograd():
    g = _gen(5)
    M, Rr, Cc = 6, 3, 5
    logits = (torch.randn(M, Rr, Cc, generator=g) * 2).requires_grad_(True)
    q = torch.empty(M * Rr, Cc).exponential_(generator=g)
    z, _, _ = O.sample_onehot(logits, q, Cc)
    gz = torch.randn(M, Rr, Cc, generator=g)
    gl, = torch.autograd.grad((z * gz).sum(), logits)
    soft = torch.softmax(logits.detach(), -1)
    _near(R.ste_bwd(gz, soft)["gl"], gl, 32, what="gl")
    extra = torch.randn(M, Rr, Cc, generator=g)
    assert torch.equal(R.ste_bwd(gz, soft, extra)["gl"], R.ste_bwd(gz, soft)["gl"] + extra.double())


def test_bf16_rne():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, 0.0, 1e-40], dtype=torch.float32)
    want = x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(R.bf16_rne(x), want)
    y = torch.randn(4096, generator=_gen(6))
    assert torch.equal(R.bf16_rne(y), y.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF)


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def test_shapes_the_cases_cover():
    by = C.cases_by_op()
    assert sorted(by) == sorted(R.OP_NAMES)
    for op in ("kl_fwd", "kl_bwd", "ste_bwd_add", "softmax_ste_bwd"):
        seen = {tuple(c.v[1:3]) for c in by[op]}
        assert seen == set(C.GROUPED_RC), op
        for Rr, Cc in C.GROUPED_RC:
            ms = {c.v[0] for c in by[op] if tuple(c.v[1:3]) == (Rr, Cc)}
            assert {1, 15} <= ms
            W = C.pow2_ge(Cc)
            # a last workgroup that is partly valid, wherever R W leaves room for one
            assert any((m * Rr * W) % 256 for m in ms) or (Rr * W) % 256 == 0, (op, Rr, Cc)
    assert {(c.v[1], c.v[0]) for c in by["heads"]} == {(nb, m) for nb in C.HEADS_NB for m in C.HEADS_M1}
    assert {c.v[0] for c in by["prep"]} == set(C.SUM_M1)
    assert {(c.v[0], c.v[2], c.v[1]) for c in by["stats"]} == {(m, p, r) for m in C.SUM_M1 for p in (1, 4) for r in (1, 32)}
    assert {(c.v[0], c.v[1]) for c in by["window_scores"]} == {(1, 1), (4, 5), (5, 64), (3, 65), (2, 130)}
    assert {(c.v[1], c.v[0]) for c in by["vec_mse"]} == {(d, m) for d in (1, 63, 64, 65, 200) for m in (1, 5)}
    assert {(c.v[0], c.v[1], c.slots[1] is None, c.v[5]) for c in by["gru_bwd"]} == {
        (b, h, noh, a) for b, h in ((1, 1), (3, 85), (2, 128), (1, 257), (5, 600)) for noh in (False, True) for a in (0, 1)}
    ln = by["ln_silu_bwd"]
    assert {(c.v[1], c.v[0]) for c in ln} == {(k, m) for k in (1, 63, 64, 65, 600, 1024, 1025, 1600) for m in (1, 4, 5)}
    for K in (1, 63, 64, 65, 600, 1024, 1025, 1600):  # every K with and without gy / xhat, and with and without g_pre16
        assert {c.slots[5] is None for c in ln if c.v[1] == K} == {True, False}
        assert {c.slots[7] is None for c in ln if c.v[1] == K} == {True, False}
    cs = by["colsum_multi"]
    assert {c.v[0] for c in cs if c.v[1] > 1} == set(C.CS_M) and all(c.v[3:18:3] == list(C.CS_N) for c in cs if c.v[1] > 1)
    assert any(c.v[2] == 1 for c in cs) and any(c.v[2] == 0 for c in cs)
    n = sum(len(v) for v in by.values())
    print(f"{n} cases")


def _emulate(case):
    """The reference written into the buffers as the op would write it."""
    w, bufs = case.wants(), {}
    for o in case.outs():
        b = o.make()
        if o.name in w:
            ref = w[o.name].ref.reshape(b[o.region].shape)
            b[o.region] = ref.to(b.dtype)
        elif o.name == "g_pre16":
            b[o.region] = R.bf16_rne(w["g_pre"].ref.float()).to(torch.int16).reshape(b[o.region].shape)
        bufs[o.name] = b
    return bufs


def test_the_reference_in_the_buffers_passes_and_breaks_are_caught():
    by = C.cases_by_op()
    for op in ("gather", "prep", "stats", "final", "vec_mse", "window_scores", "colsum_multi", "gru_bwd", "ln_silu_bwd"):
        for case in by[op][:6]:
            # (the bit-exact claims are the device's: float64 autograd leaves 1e-17 where the kernels give 0)
            fails = [f for f in C.compare(case, _emulate(case)) if "exactly" not in f]
            assert fails == [], (case, fails)
    case = next(c for c in by["ln_silu_bwd"] if c.v[0] == 4 and c.v[1] == 65 and c.slots[5] is not None)
    bufs = _emulate(case)
    bufs["g_pre"][4, 0] = 1.0   # a row >= M
    assert any("outside the output" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["gy"][0, 65] = 0.0     # a column past K, inside ld
    assert any("gy" in f and "outside the output" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["xhat"][3, 64] = C.poison(1)[0]
    assert any("xhat" in f and "unwritten" in f for f in C.compare(case, bufs))
    bufs = _emulate(case)
    bufs["g_pre"][2, 7] += 1e-3 * bufs["g_pre"][2].abs().max()
    assert any("g_pre" in f and "beyond tolerance" in f for f in C.compare(case, bufs))
    nogy = next(c for c in by["final"] if c.label == "no-skip-pointer")
    assert all(o.name != "skip" for o in nogy.outs())


def test_measured_table_is_complete():
    """Every output compared at a measured bound has its entry: no bound is made up while the suite runs."""
    keys = {w.key for cs in C.cases_by_op().values() for c in cs for w in c.wants().values() if w.key}
    assert keys == set(C.MEASURED), (sorted(keys - set(C.MEASURED)), sorted(set(C.MEASURED) - keys))


@pytest.mark.parametrize("mut", sorted(R.MUTATIONS))
def test_inputs_see_the_mutation(mut):
    """The mutated reference differs from the reference by >= 100 tolerances on at least one element of one output of
    one case of the GPU test (a NaN or infinite difference is not counted as seen)."""
    best, where = 0.0, None
    for case in C.cases_by_op()[R.MUTATIONS[mut]]:
        w0, w1 = case.wants(), case.ref(mut)
        for k, a in w0.items():
            d = (w1[k].ref - a.ref).abs()
            d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
            ratio = torch.where(d > 0, d / a.tol.clamp(min=1e-300), torch.zeros_like(d))
            if ratio.numel() and float(ratio.max()) > best:
                best, where = float(ratio.max()), (case, k)
    print(f"{mut}: {best:.3g} tolerances at {where}")
    assert best >= 100.0, (mut, best, where)


# ----------------------------------------------------------------------------
# the hook's refusals (no GPU: nothing is launched)
# ----------------------------------------------------------------------------
def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_wm_loss_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                  ctypes.c_int]
    return f


def _refused(op, v, ptrs=True, num=True):
    from dreamer_amd import _lib
    va = (ctypes.c_int * 32)(*v) if v is not None else None
    na = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0) if num else None
    pa = (ctypes.c_void_p * 32)() if ptrs else None  # every pointer NULL: a call that got past the checks would fault
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(op, va, na, pa, None, msg, 256)
    assert rc == _lib.DR_E_INVALID and msg.value, (op, v, rc, msg.value)
    return msg.value.decode()


def test_hook_refuses_what_it_documents():
    assert "null descriptor" in _refused(R.KL_FWD, None)
    assert "null descriptor" in _refused(R.KL_FWD, [1, 1, 8], ptrs=False)
    assert "unknown op" in _refused(len(R.OP_NAMES), [1, 1, 1])
    assert "unknown op" in _refused(-1, [1, 1, 1])
    for op in (R.KL_FWD, R.KL_BWD, R.STE_BWD_ADD, R.SOFTMAX_STE_BWD):
        for Cc in (0, 65, -1, 128):
            assert "[1,64]" in _refused(op, [2, 3, Cc, 1000, 1000, 1000, 1000])
        assert "null operand" in _refused(op, [2, 3, 8, 24, 24, 24, 24])
        assert "positive" in _refused(op, [0, 3, 8, 24, 24, 24, 24])
    assert "stride" in _refused(R.STE_BWD_ADD, [2, 3, 8, 23, 24, 24, 24])
    assert "stride" in _refused(R.SOFTMAX_STE_BWD, [2, 3, 8, 24, 23])
    assert "stride" in _refused(R.GRU_BWD, [2, 8, 7, 8, 8, 0])
    assert "stride" in _refused(R.LN_SILU_BWD, [2, 8, 8, 8, 7])
    assert "at least 2" in _refused(R.HEADS, [4, 1])
    assert "scalars" in _refused(R.FINAL, [45], num=False)
    assert "jobs" in _refused(R.COLSUM_MULTI, [4, 9, 0])
    assert "one job" in _refused(R.COLSUM_MULTI, [4, 2, 1])
    assert "null operand" in _refused(R.HEADS, [4, 8])
