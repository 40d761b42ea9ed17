"""Every pinned GEMM route (tests/test_gemm_plan_host.py) run on the GPU through dr_internal_gemm_run and compared
with float64 (tests/gemm_ref.py), plus the epilogue fields of GemmArgs one at a time on each NT plain family.

Per case, in this order: the route the hook ran equals the pinned string; the integer pass is bit-exact (AM_PLAIN:
operands in [-3, 3], every partial sum exact in f32 in any order, exact in bf16 too); the random pass is within the
bound -- derived for the exact-f32 families and, on bf16-rounded operands, for the bf16 routes (gemm_ref.f32_bound),
the project's 1e-4 |ref| + 1e-5 max|ref| where none is derived (three-plane split3, the fast-SiLU prologues, act != 0,
the backward prologues); everything outside the written regions still holds the sentinel."""
import ctypes
import os

import pytest
import torch

import gemm_ref as R
import test_gemm_plan_host as H
from test_gemm_plan_host import ACC, BF16, G_NN, G_NT, G_TN, LNBWD, PLAIN, prob

pytestmark = pytest.mark.gpu

CASES = H._cases()
RUN = sorted(n for n in CASES if R.left_out(n) is None)
# where a measuring run appends the observed errors of the routes without a derived bound (profiles/gemm_routes_errors.txt)
ERRORS_FILE = os.environ.get("GEMM_ROUTES_ERRORS")


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_gemm_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    return f


def run(case, probs, dev):
    """The batch through the hook: (steps, None) or (None, (code, message)), and the device stores back on the CPU."""
    from dreamer_amd import hip
    lay, amode, plist = case
    n = len(probs)
    dstore = [{k: b.store.to(dev) for k, b in p.buf.items()} for p in probs]
    ptrs = (ctypes.c_void_p * (15 * max(n, 1)))()
    num = (ctypes.c_double * (R.GX_COUNT * max(n, 1)))()
    xp = (ctypes.c_void_p * (R.GP_COUNT * max(n, 1)))()
    for i, p in enumerate(probs):
        for s, name in enumerate(R.SLOTS):
            if name in p.buf:
                ptrs[15 * i + s] = R.pointer(p.buf[name], dstore[i][name])
                assert ptrs[15 * i + s] % 16 == p.nib(name)
        for s, name in enumerate(R.GP):
            if name in p.buf:
                xp[R.GP_COUNT * i + s] = R.pointer(p.buf[name], dstore[i][name])
        num[R.GX_COUNT * i:R.GX_COUNT * (i + 1)] = p.numbers()
    flat = [v for p in plist for v in p] or [0]
    arr = (ctypes.c_int * len(flat))(*flat)
    out = (ctypes.c_int * (H.STEP_INTS * 10))()
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(lay, amode, len(plist), arr, ptrs, num, xp, hip.stream(), out, 10, msg, 256)
    torch.cuda.synchronize()
    got = [{k: t.cpu() for k, t in d.items()} for d in dstore]
    if rc < 0:
        return None, (-rc, msg.value.decode()), got
    return [list(out[H.STEP_INTS * k:H.STEP_INTS * (k + 1)]) for k in range(rc)], None, got


def main_step(steps, i):
    """The step that computes problem i's product."""
    return [s for s in steps if s[12] >> i & 1 and s[0] not in (H.F_LN_ROWS, H.F_FINISH)][0]


def rounded_routes(steps, n):
    """Per problem: does its product run on bf16-rounded operands (k_gemm_tile_b16, one-plane k_gemm_wks3)?"""
    return [main_step(steps, i)[0] == H.F_TILE_B16 or (main_step(steps, i)[0] == H.F_WKS3 and bool(main_step(steps, i)[10]))
            for i in range(n)]


def derived(step, amode, p):
    """Is the f32 dot-product bound derivable for this problem's route?"""
    three_plane = step[0] == H.F_S3_TALL or (step[0] == H.F_WKS3 and not step[10])
    return amode == PLAIN and not three_plane and not p.num.get("act", 0) and not p.num.get("gb_Hd", 0)


def check_sentinels(probs, got, steps, what):
    for i, p in enumerate(probs):
        for name, b in p.buf.items():
            if not b.out or name in ("wsplit", "A16"):
                continue
            if name == "ws":
                st = main_step(steps, i)
                if st[20] or (st[18] <= 1 and st[0] != H.F_S3_TALL):  # withheld, or no split-K: never written
                    assert bool((got[i]["ws"].view(torch.int32) == R.SENT).all()), f"{what}: p{i} scratch written"
            assert b.untouched(got[i][name]), f"{what}: p{i} {name} written outside its [{b.rows}, {b.cols}] region"


def _report(what, route, name, err, bound_f32):
    line = f"{what} | p {name} | max err {err:.3e} | derived f32 bound there {bound_f32:.3e} | {route}"
    print(line)
    if ERRORS_FILE:
        with open(ERRORS_FILE, "a") as f:
            f.write(line + "\n")


def check_case(what, case, fields, dev, expect_route=None, seed=0):
    lay, amode, plist = case
    # integer pass: bit-exact (the forward product on plain operands)
    int_ok = amode == PLAIN and not any((f or {}).get("act") for f in (fields or [{}] * len(plist)))
    steps0 = None
    if int_ok:
        probs = R.materialise(case, "int", seed, fields)
        steps0, err, got = run(case, probs, dev)
        assert err is None, f"{what}: {err}"
        if expect_route is not None:
            assert R.route_of(steps0, plist) == expect_route
        ref = R.reference(lay, amode, probs)
        for i, p in enumerate(probs):
            for name in ("Y", "Y2"):
                if name in ref[i]:
                    g, r = p.buf[name].view(got[i][name]), ref[i][name].float()
                    bad = (g != r) | g.isnan()
                    if bool(bad.any()):
                        rows, cols = bad.nonzero()[:, 0], bad.nonzero()[:, 1]
                        m, n = int(rows[0]), int(cols[0])
                        raise AssertionError(
                            f"{what}: integer pass p{i} {name}: {int(bad.sum())} of {bad.numel()} wrong, rows "
                            f"{int(rows.min())}..{int(rows.max())}, columns {int(cols.min())}..{int(cols.max())}; "
                            f"first ({m}, {n}): got {float(g[m, n])}, expected {float(r[m, n])}")
        check_sentinels(probs, got, steps0, what + " (integer pass)")
    # random pass
    probs = R.materialise(case, "rand", seed, fields)
    steps, err, got = run(case, probs, dev)
    assert err is None, f"{what}: {err}"
    route = R.route_of(steps, plist)
    if expect_route is not None:
        assert route == expect_route
    assert steps0 is None or steps0 == steps
    rnd = rounded_routes(steps, len(probs))
    ref = R.reference(lay, amode, probs, rnd)
    for i, p in enumerate(probs):
        st, e = main_step(steps, i), ref[i]
        tight = derived(st, amode, p)
        n1 = e["Y"].shape[1]
        for name, r in e.items():
            if name in ("abs", "margin", "idx", "z_out", "zval") or name not in p.buf:
                continue
            g = p.buf[name].view(got[i][name]).double()
            d = (g - r).abs()
            assert not bool(g.isnan().any()), f"{what}: p{i} {name} holds NaN / unwritten elements"
            fb = None
            if name in ("Y", "Y2"):
                ab = e["abs"] if p.flags & H.OUT_CONV else (e["abs"][:, :n1] if name == "Y" else e["abs"][:, n1:])
                fb = R.f32_bound(p.K, ab, r)
            bound = fb if (tight and fb is not None) else R.loose_bound(r)
            if not tight and fb is not None and d.numel():
                k = int(d.argmax())
                _report(what, route, f"{i} {name}", float(d.max()), float(fb.flatten()[k]))
            bad = d > bound
            assert not bool(bad.any()), (f"{what}: p{i} {name}: {int(bad.sum())} of {bad.numel()} out of bound, max "
                                         f"|d| {float(d.max()):.3e}, worst d / bound {float((d / bound.clamp_min(1e-300)).max()):.3g}")
        if p.epi == R.SAMPLE:
            C, Rg = p.v[8], p.v[9]
            gi = p.buf["idx"].view(got[i]["idx"]).view(torch.int32).long()
            flips = gi != e["idx"]
            assert not bool((flips & (e["margin"] >= 1e-4)).any()), f"{what}: p{i} sampled indices differ off a tie"
            assert int(flips.sum()) <= 1e-3 * flips.numel(), f"{what}: p{i} {int(flips.sum())} guarded draws"
            z = p.buf["z_out"].view(got[i]["z_out"]).double().reshape(p.M, Rg, C)
            assert bool(((z - torch.nn.functional.one_hot(gi, C).double()).abs() <= 2.0 ** -22).all()), f"{what}: p{i} z_out"
            zv = p.buf["zval"].view(got[i]["zval"]).double()
            assert bool(((zv - 1).abs() <= 2.0 ** -22).all()), f"{what}: p{i} zval_out"
    check_sentinels(probs, got, steps, what)
    return steps, probs, got


@pytest.mark.parametrize("name", RUN)
def test_pinned_route_runs_and_matches_float64(name, gpu):
    check_case(name, CASES[name], R.table_fields(name, CASES[name]), gpu, expect_route=H.EXPECT[name])


def test_left_out_cases_are_exactly_the_named_ones():
    assert sorted(n for n in CASES if R.left_out(n)) == R.LEFT_OUT


def test_refused_batches_return_the_pinned_error_and_launch_nothing(gpu):
    """The `err ...` cases: every pointer slot aims into one sentinel store, which no launch may touch."""
    from dreamer_amd import hip
    store = torch.empty(1 << 18, dtype=torch.int32, device=gpu).fill_(R.SENT)
    for name in (n for n in R.LEFT_OUT if n.startswith("err ")):
        lay, amode, plist = CASES[name]
        n = max(len(plist), 1)
        ptrs = (ctypes.c_void_p * (15 * n))()
        for i, v in enumerate(plist):
            for s, slot in enumerate(R.SLOTS):
                k = R.NIBBLE.get(slot)
                ptrs[15 * i + s] = store.data_ptr() + 4096 + (0 if k is None else (v[14 + k // 8] >> (4 * (k % 8))) & 15)
        flat = [v for p in plist for v in p] or [0]
        out = (ctypes.c_int * (H.STEP_INTS * 10))()
        msg = ctypes.create_string_buffer(256)
        rc = _hook()(lay, amode, len(plist), (ctypes.c_int * len(flat))(*flat), ptrs, None, None, hip.stream(), out, 10,
                     msg, 256)
        torch.cuda.synchronize()
        assert f"E {-rc} {msg.value.decode()}" == H.EXPECT[name], name
        assert bool((store == R.SENT).all()), name


def test_a16_rows_give_the_same_bits(gpu):
    """k_gemm_wks3<1>: A read as the producer's bf16 rows or rounded on load -- `bitwise the same products`."""
    lay, amode, plist = CASES["planes bf16 a16"]
    ys = []
    for fl in (0, H.A16):
        pl = [list(v) for v in plist]
        for v in pl:
            v[11] = (v[11] & ~H.A16) | fl
        probs = R.materialise((lay, amode, pl), "rand", 3)
        steps, err, got = run((lay, amode, pl), probs, gpu)
        assert err is None and steps[0][0] == H.F_WKS3 and steps[0][11] == bool(fl), (err, steps)
        ys.append([p.buf["Y"].view(got[i]["Y"]) for i, p in enumerate(probs)])
    for a, b in zip(*ys):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# epilogue fields, one at a time and all together, on one shape per NT plain family just past a tile boundary
# ---------------------------------------------------------------------------
FAMILY_SHAPES = {
    # family: (M, N, K, ldy, kwargs of prob(), the family of the main step)
    "skinny16": (17, 17, 64, 20, {}, H.F_SKINNY),
    "skinny64": (65, 2049, 64, 2052, {}, H.F_SKINNY),
    "tile32 splitk": (129, 705, 1620, 708, dict(ws=4 * 129 * 705), H.F_TILE),
    "tile64 splitk": (513, 193, 1624, 196, dict(ws=4 * 513 * 193), H.F_TILE),
    "wk": (129, 705, 1024, 708, {}, H.F_WK),
    "wks3": (129, 33, 200, 36, dict(np_=64), H.F_WKS3),
    "tile_b16": (129, 705, 1024, 708, dict(flags=BF16), H.F_TILE_B16),
    "s3_tall": (1025, 132, 200, 136, dict(np_=256), H.F_S3_TALL),
    "legacy": (65, 33, 64, 33, dict(flags=H.OUT_CONV), H.F_LEGACY),
}
FIELDS = {
    "none": {}, "alpha": dict(alpha=-2.0), "act1": dict(act=1), "act2": dict(act=2), "addend": dict(addend=True),
    "accumulate": dict(acc=True), "Y2": dict(y2=True),
    "all": dict(alpha=0.5, act=1, addend=True, acc=True, y2=True),
}
S3_REFUSES = ("alpha", "act2", "addend", "all")  # s3_tall_ok: alpha == 1, act <= 1, no addend


def field_case(family, field):
    M, N, K, ldy, kw, fam = FAMILY_SHAPES[family]
    kw, f, o = dict(kw), {}, FIELDS[field]
    fl = kw.pop("flags", 0) | H.BIAS | (H.ADDEND if o.get("addend") else 0) | (ACC if o.get("acc") else 0)
    if fl & H.OUT_CONV:
        f["ohow"] = 13
    if "alpha" in o:
        f["alpha"] = o["alpha"]
    if "act" in o:
        f["act"] = o["act"]
    if o.get("addend"):
        f["addend"] = N + 5
    if o.get("y2") and not fl & H.OUT_CONV:  # (out_conv has no second output)
        f["nsplitY"], f["ldy2"] = 16, N - 16 + 4
    return (G_NT, PLAIN, [prob(M, N, K, fl, ldy=ldy, **kw)]), [f], fam


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("family", sorted(FAMILY_SHAPES))
def test_epilogue_field_on_each_family(family, field, gpu):
    case, f, fam = field_case(family, field)
    steps, probs, got = check_case(f"{family} {field}", case, f, gpu, seed=5)
    got_fam = main_step(steps, 0)[0]
    if family == "s3_tall" and field in S3_REFUSES:
        assert got_fam != H.F_S3_TALL  # the planner moves the batch to a family that handles the field
    else:
        assert got_fam == fam, H._kernel(main_step(steps, 0))
    if "splitk" in family:
        assert steps[-1][0] == H.F_FINISH and steps[0][18] > 1


def test_nn_second_weight_segment(gpu):
    """W2 by rows (k >= ksplitB) and by columns (n >= nsplitB), on the skinny NN kernel and on the NN tile kernel."""
    for M, N, K, ws in ((256, 200, 64, 0), (512, 512, 512, 4 * 512 * 512)):
        for f in (dict(ksplitB=K // 2 + 4, ldb2=N + 4), dict(nsplitB=N // 2 + 4, ldb2=N)):
            case = (G_NN, PLAIN, [prob(M, N, K, H.W2 | H.BIAS, ldb=N, ws=ws)])
            check_case(f"nn W2 {M} {f}", case, [f], gpu, seed=7)


def test_tn_batch_of_four_with_and_without_scratch(gpu):
    for ws in (0, 4 * 200 * 200):
        case = (G_TN, PLAIN, [prob(200 - 4 * i, 200, 3840, lda=200, ldb=200, ws=ws) for i in range(4)])
        steps, _, _ = check_case(f"tn x4 ws{ws}", case, None, gpu, seed=9)
        assert (steps[-1][0] == H.F_FINISH) == bool(ws)


@pytest.mark.parametrize("M,N,K,Hd,tile", [(256, 600, 200, 600, 48), (17, 40, 64, 24, 16)])
def test_gru_backward_epilogue(M, N, K, Hd, tile, gpu):
    """GruBwdEpi on the final accumulated value, behind the LayerNorm-backward prologue (the BPTT's last GEMM)."""
    case = (G_NT, LNBWD, [prob(M, N, K, H.LN | H.PRE | H.AOUT | ACC)])
    steps, _, _ = check_case(f"gru epilogue {M} {N}", case, [dict(gru=Hd, sv=True)], gpu, seed=11)
    assert steps[0][0] == H.F_SKINNY and (steps[0][1], steps[0][2]) == (16, tile)
