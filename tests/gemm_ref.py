"""The generic GEMM (csrc/gemm.hip) against float64: the case builder and the reference of
tests/test_gpu_gemm_routes.py.  Everything here runs on the CPU (tests/test_gemm_routes_host.py).

materialise() turns a problem list of the form of test_gemm_plan_host._cases() (17 ints per problem) into seeded CPU
tensors, every one a logical matrix at its leading dimension inside a larger store: inputs padded with a large finite
value, outputs prefilled with a NaN bit pattern (SENT), so that a kernel that reads padding as data or writes outside
its region shows.  reference() is the comment at the top of gemm.h in float64,

    Y (+)= act(alpha * opA @ opB + bias + addend)

with the A-modes as plain torch: LayerNorm + SiLU, and the backward prologues and the GRU epilogue as float64
autograd."""
import math

import torch
import torch.nn.functional as F

from test_gemm_plan_host import (A2, A16, ACC, ADDEND, AOUT, BF16, BIAS, G_NN, G_NT, G_TN, INT_MAX, LN, LNBWD, LNSILU,
                                 OUT_CONV, PLAIN, PLANES, PRE, STEBWD, W2, WS)

SAMPLE, ACTOR = 1, 2
SENT = 0x7FA5C3E1  # a quiet NaN no kernel computes: outputs and scratch before the run
PAD_IN = 7777.0    # input padding: finite, far off every operand
GUARD = 64         # floats of store either side of every matrix (a multiple of 4: the pointer keeps its nibble)
# dr_internal_gemm_run's extras, in the hook's order (gemm.hip GX_* / GP_*)
GX = ("alpha act ldy2 nsplitY ksplitB nsplitB ld_add ld_pre ld_sv ld_soft ld_mu ld_sig ld_act gb_ldh gb_ldo gb_Hd ohow "
      "unimix det step ldb2").split()
GP = "Y2 sv_gy sv_xh soft idx zval q eps mu sig act gb_h gb_r gb_u gb_n gb_ghn gb_gi gb_gh gb_ho".split()
GX_COUNT = GP_COUNT = 24
SLOTS = "A A2 W Y ln_g ln_b a_out pre ws wsplit A16 W2 addend bias z_out".split()
# misalignment nibble of a slot: its position in mis0 (0-7) / mis1 (8-11)
NIBBLE = dict(A=0, A2=1, W=2, Y=3, ln_g=4, ln_b=5, a_out=6, pre=7, wsplit=8, A16=9, bias=10, z_out=11)


class Buf:
    """A [rows, cols] matrix at row stride ld, GUARD + mis / 4 floats into a 1-D float32 store that ends GUARD floats
    past the last full row.  out: prefilled with SENT (then `init`, the values a += finds, in the matrix itself)."""

    def __init__(self, rows, cols, ld, mis=0, out=False, init=None, floats=None):
        assert mis % 4 == 0 and ld >= 0 and (ld >= cols or rows <= 1)
        self.rows, self.cols, self.ld, self.mis, self.out = rows, cols, ld, mis, out
        self.off = GUARD + mis // 4
        n = rows * ld if floats is None else floats
        self.store = torch.empty(self.off + n + GUARD, dtype=torch.float32)
        if out:
            self.store.view(torch.int32).fill_(SENT)
        else:
            self.store.fill_(PAD_IN)
        if init is not None:
            self.view().copy_(init)

    def view(self, store=None):
        s = self.store if store is None else store
        return s.as_strided((self.rows, self.cols), (self.ld, 1), self.off)

    def f64(self):
        return self.view().double()

    def untouched(self, store):
        """The store after a run, the matrix itself blanked: all SENT where nothing wrote outside it."""
        s = store.clone()
        self.view(s).view(torch.int32).fill_(SENT)
        return bool((s.view(torch.int32) == SENT).all())


class Problem:
    def __init__(self, v):
        self.v = list(v)
        self.M, self.N, self.K = v[0], v[1], v[2]
        self.flags = v[11]
        self.epi = (v[11] >> 8) & 3
        self.buf = {}   # name -> Buf (SLOTS and GP names)
        self.num = {}   # GX name -> value
        self.gen = {}   # float64 tensors behind derived inputs (the GRU saves' pre-activations)

    def nib(self, name):
        k = NIBBLE.get(name)
        return 0 if k is None else (self.v[14 + k // 8] >> (4 * (k % 8))) & 15

    def numbers(self):
        return [float(self.num.get(k, 0)) for k in GX] + [0.0] * (GX_COUNT - len(GX))


def _draw(g, shape, mode, scale=1.0):
    if mode == "int":
        return torch.randint(-3, 4, shape, generator=g).float()
    return (torch.randn(shape, generator=g) * scale).float()


def materialise(case, mode="rand", seed=0, fields=None):
    """(lay, amode, [17 ints, ...]) -> [Problem, ...] with seeded contents.  mode: "int" (operands, bias, addend and
    the initial Y small integers in [-3, 3]) or "rand" (A = randn, W = randn / sqrt(K)).  fields: per problem, a dict
    of what the 17 ints do not carry -- alpha, act, addend=ld_add, nsplitY (with ldy2), ksplitB | nsplitB (with the W2
    flag), ohow (out_conv), gru=Hd, sv=True (AM_LNBWD's saves), ld_pre."""
    lay, amode, probs = case
    g = torch.Generator().manual_seed(1000003 * seed + 17)
    out = []
    for i, v in enumerate(probs):
        p = Problem(v)
        f = dict((fields or [{}] * len(probs))[i])
        M, N, K, lda, lda2, ksA, ldb, ldy, C, R, na, fl = v[:12]
        ws_floats, np_, ld_aout = v[12], v[13], v[16]
        wscale = 1.0 / math.sqrt(max(K, 1))
        b = p.buf
        # A: [M][K] (NT, NN; a second K segment in A2) or [K][M] (TN)
        if lay == G_TN:
            b["A"] = Buf(K, M, lda, p.nib("A"), init=_draw(g, (K, M), mode))
        else:
            k1 = min(K, ksA) if fl & A2 else K
            b["A"] = Buf(M, k1, lda, p.nib("A"), init=_draw(g, (M, k1), mode))
            if fl & A2:
                b["A2"] = Buf(M, K - k1, lda2, p.nib("A2"), init=_draw(g, (M, K - k1), mode))
        # B: [N][K] (NT) or [K][N] (NN, TN; W2 past ksplitB rows or nsplitB columns)
        ksB, nsB = f.get("ksplitB", INT_MAX), f.get("nsplitB", INT_MAX)
        if lay == G_NT:
            b["W"] = Buf(N, K, ldb, p.nib("W"), init=_draw(g, (N, K), mode, wscale))
        else:
            kw, nw = min(K, ksB), min(N, nsB)
            b["W"] = Buf(kw, nw, ldb, p.nib("W"), init=_draw(g, (kw, nw), mode, wscale))
            if fl & W2:
                ldb2 = f.get("ldb2", ldb)
                shape = (K - kw, N) if ksB < K else (K, N - nw)
                b["W2"] = Buf(shape[0], shape[1], ldb2, init=_draw(g, shape, mode, wscale))
                p.num["ldb2"] = ldb2
        p.num["ksplitB"], p.num["nsplitB"] = ksB, nsB
        if fl & LN:
            b["ln_g"] = Buf(1, K, K, p.nib("ln_g"), init=1 + 0.1 * torch.randn(K, generator=g))
            b["ln_b"] = Buf(1, K, K, p.nib("ln_b"), init=0.1 * torch.randn(K, generator=g))
        if fl & PRE:
            ld_pre = f.get("ld_pre", lda)
            pre = _draw(g, (M, K), "rand")
            if amode == STEBWD:  # the softmax rows of the forward pass
                pre = torch.softmax(pre.double().reshape(M, K // C, C), -1).reshape(M, K).float()
            b["pre"] = Buf(M, K, ld_pre, p.nib("pre"), init=pre)
            p.num["ld_pre"] = ld_pre
        if fl & BIAS:
            b["bias"] = Buf(1, N, N, p.nib("bias"), init=_draw(g, (N,), mode, 0.5))
        if fl & ADDEND:
            ld_add = f.get("addend", ldy)
            b["addend"] = Buf(M, N, ld_add, init=_draw(g, (M, N), mode, 0.5))
            p.num["ld_add"] = ld_add
        # Y (and Y2 past nsplitY): out_conv stores NCHW [frame][N][oh * ow], frame = m / (oh * ow)
        nsY = f.get("nsplitY", INT_MAX)
        n1 = min(N, nsY)
        y0 = (lambda r, c: _draw(g, (r, c), mode, 0.5)) if fl & ACC else (lambda r, c: None)
        if fl & OUT_CONV:
            hw = f["ohow"]
            assert M % hw == 0
            b["Y"] = Buf(M // hw * N, hw, hw, p.nib("Y"), out=True, init=y0(M // hw * N, hw))
            p.num["ohow"] = hw
        else:
            b["Y"] = Buf(M, n1, ldy, p.nib("Y"), out=True, init=y0(M, n1))
        if nsY < N:
            ldy2 = f.get("ldy2", N - nsY)
            b["Y2"] = Buf(M, N - nsY, ldy2, out=True, init=y0(M, N - nsY))
            p.num["ldy2"] = ldy2
        p.num["nsplitY"] = nsY
        p.num["alpha"], p.num["act"] = f.get("alpha", 1.0), f.get("act", 0)
        if fl & AOUT:
            b["a_out"] = Buf(M, K, ld_aout, p.nib("a_out"), out=True)
        if f.get("sv"):
            ld_sv = K + 4
            b["sv_gy"], b["sv_xh"] = Buf(M, K, ld_sv, out=True), Buf(M, K, ld_sv, out=True)
            p.num["ld_sv"] = ld_sv
        if fl & WS:
            b["ws"] = Buf(1, ws_floats, ws_floats, out=True)
        if fl & PLANES:
            b["wsplit"] = Buf(1, 0, 0, p.nib("wsplit"), out=True, floats=(K + 31) // 32 * 3 * np_ * 16)
        if fl & A16:
            b["A16"] = Buf(1, 0, 0, p.nib("A16"), out=True, floats=(M * lda + 1) // 2)
        if p.epi == SAMPLE:
            b["z_out"] = Buf(M, N, ldy, p.nib("z_out"), out=True)
            b["soft"] = Buf(M, N, N + 4, out=True)
            b["idx"], b["zval"] = Buf(M, R, R, out=True), Buf(M, R, R, out=True)
            u = torch.rand((M, N), generator=g, dtype=torch.float64).clamp_min(1e-12)
            b["q"] = Buf(M, N, N, init=(-torch.log(u)).float().clamp_min(1e-6))
            p.num["ld_soft"], p.num["unimix"] = N + 4, 0.01 / C
        if p.epi == ACTOR:
            for k in ("mu", "sig", "act"):
                b[k] = Buf(M, na, na + 1, out=True)
                p.num["ld_" + k] = na + 1
            b["eps"] = Buf(M, na, na, init=torch.randn((M, na), generator=g))
        Hd = f.get("gru", 0)
        if Hd:  # the GRU forward's saves from seeded pre-activations; dL/dh (+=) and h at strides of their own
            pa = {k: torch.randn((M, Hd), generator=g, dtype=torch.float64) for k in ("pr", "pu", "in", "hn", "h")}
            pa = {k: t.float().double() for k, t in pa.items()}
            r, u = torch.sigmoid(pa["pr"]), torch.sigmoid(pa["pu"])
            n = torch.tanh(pa["in"] + r * pa["hn"])
            p.gen = pa
            for k, t in (("gb_r", r), ("gb_u", u), ("gb_n", n), ("gb_ghn", pa["hn"])):
                b[k] = Buf(M, Hd, Hd, init=t.float())
            b["gb_h"] = Buf(M, Hd, Hd + 4, init=pa["h"].float())
            b["gb_gi"], b["gb_gh"] = Buf(M, 3 * Hd, 3 * Hd, out=True), Buf(M, 3 * Hd, 3 * Hd, out=True)
            b["gb_ho"] = Buf(M, Hd, Hd + 8, out=True, init=_draw(g, (M, Hd), "rand"))
            p.num.update(gb_Hd=Hd, gb_ldh=Hd + 4, gb_ldo=Hd + 8)
        out.append(p)
    return out


def pointer(buf, store):
    """The address handed to the hook for `buf` living in `store` (the CPU store or its device copy)."""
    assert store.data_ptr() % 16 == 0
    return store.data_ptr() + 4 * buf.off


def route_of(steps, plist):
    """test_gemm_plan_host.route()'s string from steps already planned (the run hook returns the plan it ran)."""
    import test_gemm_plan_host as H
    ln_pre = any(s[0] == H.F_LN_ROWS for s in steps)
    out = []
    for s in steps:
        fam, mask = s[0], s[12]
        gx, gy, gz, block, lds, splits, npack, no_ws = s[13:21]
        idx = [i for i in range(4) if mask >> i & 1]
        if fam == H.F_S3_TALL:
            p = plist[idx[0]]
            out.append(f"s3_tall p{idx[0]} part{p[12] if p[11] & WS else 0}")
            continue
        ints = {H.F_SKINNY: [npack], H.F_TILE: [splits, npack], H.F_TILE_B16: [splits], H.F_WK: [1, npack],
                H.F_WKS3: [npack], H.F_FINISH: [splits]}.get(fam, [])
        toks = [H._kernel(s), f"g{gx},{gy},{gz}", f"b{block}", f"l{lds}"] + [f"i{v}" for v in ints]
        if fam != H.F_LN_ROWS:
            toks += [f"p{i}a{7 if ln_pre else 1}w{int(bool(plist[i][11] & WS) and not no_ws)}" for i in idx]
        else:
            toks.append(f"p{idx[0]}")
        out.append(" ".join(toks))
    return " ; ".join(out) if out else "-"


# ---------------------------------------------------------------------------
# which cases of the pinned table run on the GPU, and which are left out by name
# ---------------------------------------------------------------------------
def left_out(name):
    """Why a case of test_gemm_plan_host._cases() is not run on the GPU, or None."""
    if name.startswith("err "):
        return "error"  # the message is pinned on the host; the run hook returns it and launches nothing
    if name.startswith("offsets ") or name.startswith("tall_ln rows "):
        return "operands span more than 256 MB"
    if name.startswith("legacy conv") or name == "legacy x2 at":
        return "AM_CONV / AM_CONV_SRC: geometry not in the 17 ints (the encoder tests)"
    return None


LEFT_OUT = sorted(
    ["err count 0", "err count 5", "err negative", "err sampler C3", "err actor N", "err epi M4097", "err epi NN",
     "err lnbwd K1028", "err lnbwd K260 rows64", "err lnbwd pre off", "err stebwd rows64", "err stebwd C24",
     "err lnbwd offsets", "err amode",
     "offsets below", "offsets at", "offsets W at", "offsets tile below", "offsets tile at",
     "tall_ln rows 2^31 lda", "tall_ln rows 2^31 ld_aout", "tall_ln rows below 2^31",
     "legacy conv below", "legacy conv at", "legacy conv_src below", "legacy conv_src at", "legacy x2 at"])


def table_fields(name, case):
    """What a pinned case needs beyond its 17 ints: out_conv's image size, and AM_LNBWD's saves on one case."""
    lay, amode, plist = case
    f = [{} for _ in plist]
    for i, v in enumerate(plist):
        if v[11] & OUT_CONV:
            f[i]["ohow"] = 64
    if name == "lnbwd B256 N200 K200":
        f[0]["sv"] = True
    return f


def bf16(x):
    """Rounded to bfloat16 (round to nearest even), back in float64."""
    return x.float().bfloat16().double()


def _ln(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5) if x.shape[-1] else x


def op_a(p, lay, amode):
    """opA [M][K] in float64 and the prologue's side outputs (a_out, sv_gy, sv_xh)."""
    b, side = p.buf, {}
    if lay == G_TN:
        return b["A"].f64().t(), side
    a = b["A"].f64() if "A2" not in b else torch.cat([b["A"].f64(), b["A2"].f64()], 1)
    if amode == LNSILU:
        a = F.silu(_ln(a, b["ln_g"].f64()[0], b["ln_b"].f64()[0]))
        side["a_out"] = a
    elif amode == LNBWD:  # d/d(pre) of SiLU(LN(pre)) given gx = the A argument
        pre = b["pre"].f64().requires_grad_(True)
        gm, bt = b["ln_g"].f64()[0], b["ln_b"].f64()[0]
        xh = F.layer_norm(pre, (p.K,), None, None, 1e-5)
        y = (xh * gm + bt).requires_grad_(True)
        y.retain_grad()
        (F.silu(y) * a).sum().backward()
        side.update(a_out=pre.grad, sv_gy=y.grad, sv_xh=xh.detach())
        a = pre.grad
    elif amode == STEBWD:  # autograd through the straight-through sample z = onehot + p - p.detach()
        C = p.v[8]
        s = b["pre"].f64().reshape(p.M, p.K // C, C)
        logits = torch.log(s).requires_grad_(True)
        pm = 0.99 * torch.softmax(logits, -1) + 0.01 / C
        z = pm - pm.detach()  # the one-hot term carries no gradient
        (z * a.reshape(s.shape)).sum().backward()
        a = logits.grad.reshape(p.M, p.K)
    return a.detach(), side


def op_b(p, lay):
    b = p.buf
    if lay == G_NT:
        return b["W"].f64().t()
    w = b["W"].f64()
    if "W2" in b:
        w = torch.cat([w, b["W2"].f64()], 0 if p.num["ksplitB"] < p.K else 1)
    return w


def reference(lay, amode, probs, rounded=None):
    """Per problem, a dict of float64 expectations keyed like Problem.buf -- Y, Y2, a_out, sv_gy, sv_xh, the fused
    row epilogues' soft / idx / z_out / zval / mu / sig / act (and `margin`, the relative gap of the reference's top
    two sampler scores per group), the GRU epilogue's gb_gi / gb_gh / gb_ho -- plus `abs`, (|alpha| |opA| @ |opB| +
    |bias| + |addend| + |Y0|) for the f32 bound, laid out like Y | Y2.  rounded[i]: operands rounded to bf16 first."""
    res = []
    for i, p in enumerate(probs):
        b, fl = p.buf, p.flags
        a, exp = op_a(p, lay, amode)
        w = op_b(p, lay)
        if rounded and rounded[i]:
            a, w = bf16(a), bf16(w)
        alpha = p.num.get("alpha", 1.0)
        v = alpha * (a @ w)
        ab = abs(alpha) * (a.abs() @ w.abs())
        if "bias" in b:
            v, ab = v + b["bias"].f64(), ab + b["bias"].f64().abs()
        if "addend" in b:
            v, ab = v + b["addend"].f64(), ab + b["addend"].f64().abs()
        act = p.num.get("act", 0)
        v = F.silu(v) if act == 1 else torch.sigmoid(v) if act == 2 else v
        if fl & OUT_CONV:
            hw = p.num["ohow"]
            perm = lambda t: t.reshape(p.M // hw, hw, p.N).permute(0, 2, 1).reshape(-1, hw)
            v, ab = perm(v), perm(ab)
            if fl & ACC:
                v, ab = v + b["Y"].f64(), ab + b["Y"].f64().abs()
            exp["Y"] = v
        else:
            n1 = min(p.N, p.num.get("nsplitY", INT_MAX))
            if fl & ACC:
                y0 = b["Y"].f64() if n1 == p.N else torch.cat([b["Y"].f64(), b["Y2"].f64()], 1)
                v, ab = v + y0, ab + y0.abs()
            exp["Y"] = v[:, :n1]
            if n1 < p.N:
                exp["Y2"] = v[:, n1:]
        exp["abs"] = ab
        if p.epi == SAMPLE:
            C, R = p.v[8], p.v[9]
            lg = v.reshape(p.M, R, C)
            soft = torch.softmax(lg, -1)
            pu = 0.99 * soft + p.num["unimix"]
            score = pu / pu.sum(-1, keepdim=True) / b["q"].f64().reshape(p.M, R, C)
            idx = score.argmax(-1)
            top = score.topk(2, -1).values if C > 1 else torch.stack([score[..., 0], score[..., 0] * 0], -1)
            exp.update(soft=soft.reshape(p.M, -1), idx=idx, z_out=F.one_hot(idx, C).double().reshape(p.M, -1),
                       zval=torch.ones(p.M, R, dtype=torch.float64), margin=(top[..., 0] - top[..., 1]) / top[..., 0])
        if p.epi == ACTOR:
            na = p.v[10]
            mu, lr = v[:, :na], v[:, na:]
            sg = F.softplus(lr.clamp(-5.0, 2.0)) + 1e-3
            exp.update(mu=mu, sig=sg, act=torch.tanh(mu + b["eps"].f64() * sg))
        Hd = int(p.num.get("gb_Hd", 0))
        if Hd:  # gru_cell backward on the final value of the first Hd columns (h' = (1 - u) n + u h)
            t = {k: x.clone().requires_grad_(True) for k, x in p.gen.items()}
            r, u = torch.sigmoid(t["pr"]), torch.sigmoid(t["pu"])
            n = torch.tanh(t["in"] + r * t["hn"])
            (((1 - u) * n + u * t["h"]) * v[:, :Hd].detach()).sum().backward()
            exp["gb_gi"] = torch.cat([t["pr"].grad, t["pu"].grad, t["in"].grad], 1)
            exp["gb_gh"] = torch.cat([t["pr"].grad, t["pu"].grad, t["hn"].grad], 1)
            exp["gb_ho"] = b["gb_ho"].f64() + t["h"].grad
        res.append(exp)
    return res


def f32_bound(K, absprod, ref):
    """An f32 dot product of K terms plus the epilogue's adds, summed in any order, against float64:
    |got - ref| <= 2 (K + 4) 2^-24 (|A| @ |B| + |bias| + |addend| + |Y0|) + 2^-23 |ref|."""
    return 2.0 * (K + 4) * 2.0 ** -24 * absprod + 2.0 ** -23 * ref.abs()


def loose_bound(ref):
    """The project's own bound where none is derived (test_mlp3_shape_sweep): 1e-4 |ref| + 1e-5 max|ref|."""
    return 1e-4 * ref.abs() + 1e-5 * (float(ref.abs().max()) if ref.numel() else 0.0)
