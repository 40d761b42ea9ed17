"""The convolution family (csrc/conv.hip, conv_split.hip, conv_glds.hip, wmconv.hip) against float64: the reference,
the case table and the materialiser of tests/test_gpu_conv_routes.py.  Everything here runs on the CPU
(tests/test_conv_routes_host.py).

reference(): the formulas of csrc/conv.h written out in float64 -- the k4 s2 p1 conv with its epilogues, the
upsampling conv (ConvTranspose2d, or a Conv2d's data gradient), its last-layer tanh-MSE form, the weight gradient and
the channel sums.  The one-term forms (terms = 1) are the same formulas on RNE-bf16-rounded operands.

materialise(): every operand of a case carved from ONE float32 store, each with GUARD floats either side and a
chosen address nibble; inputs and their guards hold PAD_IN, outputs, scratch and their guards the NaN pattern SENT.  A
stray read shows as a value far off, a stray write lands inside the store and shows as a changed guard.

FORMS: every kernel instantiation a dispatcher of the family can launch, enumerated from the ladders
(op_conv_nhwc_ex, op_conv_split3_ex / op_conv_glds_s3, op_convT_nhwc, op_convT_split3 / op_convT_glds_s3,
op_convT_out3, op_conv_wgrad, op_wgrad_split3, op_chan_sum, op_chan_sum_final), as the string the launch helper
notes (DR_CONV_NOTE).  TABLE: form -> cases; route() restates the dispatchers on the host, so that a table case
that would not reach its form fails here, without a GPU.

Left out on purpose: the bf16-storage encoder kernels and the fused conv1 + conv2 kernels (op_conv_bf16,
op_conv1_bf16, op_enc12_*, op_conv_s1_bf16, op_conv_glds_bf16): tests/test_gpu_bf16.py and
tests/test_gpu_enc12_schedule.py compare them with an emulation at their only shapes."""
import torch

from gemm_ref import GUARD, PAD_IN, SENT, bf16, f32_bound, loose_bound

# dr_internal_conv_run's descriptor (conv_hook.hip CV_*, COP_*, CF_*, CP_*)
CV = ("op n ca cb h w epi nchw terms lda ldb ldc tstride cbo silu_in silu_out lo_silu flags acc ws_floats "
      "cin_raw").split()
CONV, CONV_S3, CONVT, CONVT_S3, OUT3, WGRAD, WGRAD_S3, CHAN, CHAN_FINAL = range(9)
F_BIAS, F_PRE, F_CSUM, F_OUT2, F_TARGET, F_COEF, F_PART, F_BPART, F_BIAS_OUT, F_NO_REPACK, F_WS = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
CP = "in w wr bias out pre csum out2 target coef part bpart ws hi bias_out".split()
FWD, DSILU = 0, 1                      # CONV_EPI_*
CT_BIAS, CT_DSILU, CT_TANH_MSE = 0, 1, 2
O3_TY, O3_TX = 8, 32                   # op_convT_out3's tile of low-resolution pixels


class Case:
    """One call of the hook.  h, w: the conv's input frame; the upsampling conv's and the weight gradient's
    low-resolution frame.  nib: operand name -> address nibble in bytes (a multiple of 4)."""
    DEFAULTS = dict(epi=0, nchw=0, terms=3, lda=0, ldb=0, ldc=0, tstride=4, cbo=0, silu_in=0, silu_out=0, lo_silu=0,
                    acc=0, cin_raw=0, scale=1.0, save_pre=False, csum=False, out2=False, loss=True, bpart=False,
                    bias_out=False, no_repack=False)

    def __init__(self, op, n, ca, cb, h, w, nib=None, **kw):
        self.op, self.n, self.ca, self.cb, self.h, self.w = op, n, ca, cb, h, w
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.pop(k, v))
        assert not kw, kw
        self.nib = dict(nib or {})
        self.lda = self.lda or ca
        self.ldb = self.ldb or cb
        self.cbo = self.cbo or cb
        if op in (CONVT, CONVT_S3):
            self.ldc = self.ldc or cb
        elif op == OUT3:
            self.ldc = 4 if self.loss else 3

    def __repr__(self):
        extra = {k: getattr(self, k) for k, v in self.DEFAULTS.items() if getattr(self, k) != v and k != "ldc"}
        return f"op{self.op} n{self.n} {self.ca}->{self.cb} {self.h}x{self.w} {extra} nib{self.nib}"

    @property
    def one_term(self):
        return self.terms == 1 and self.op in (CONV_S3, CONVT_S3, WGRAD_S3)

    @property
    def three_plane(self):
        return self.terms == 3 and self.op in (CONV_S3, CONVT_S3, WGRAD_S3)


# ---------------------------------------------------------------------------
# the float64 formulas (csrc/conv.h)
# ---------------------------------------------------------------------------
def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    """SiLU'(x) = s (1 + x (1 - s)), s = sigmoid(x)."""
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def conv_acc(x, w):
    """k4 s2 p1 conv: acc[f][oy][ox][co] = sum_{ci, ky, kx} x[f][2 oy - 1 + ky][2 ox - 1 + kx][ci] w[co][ci][ky][kx],
    taps outside the frame reading 0.  x NHWC, w Conv2d layout [co][ci][4][4]."""
    n, ih, iw, ci = x.shape
    oh, ow = ih // 2, iw // 2
    xp = torch.zeros(n, ih + 2, iw + 2, ci, dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    acc = torch.zeros(n, oh, ow, w.shape[0], dtype=x.dtype)
    for ky in range(4):
        for kx in range(4):  # input row 2 oy - 1 + ky is row 2 oy + ky of the padded frame
            acc += xp[:, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2, :] @ w[:, :, ky, kx].t()
    return acc


def up_acc(x, wt):
    """Upsampling k4 s2 p1: out[f][Y][X][co] = sum over ci and the (y, ky), (x, kx) with Y = 2 y - 1 + ky,
    X = 2 x - 1 + kx of x[f][y][x][ci] wt[ci][co][ky][kx].  x NHWC, wt [cin][cout][4][4]: a ConvTranspose2d
    weight, or a Conv2d weight [co][ci][4][4] read as [cin = co][cout = ci] (the Conv2d's input gradient)."""
    n, h, w, ci = x.shape
    op = torch.zeros(n, 2 * h + 2, 2 * w + 2, wt.shape[1], dtype=x.dtype)
    for ky in range(4):
        for kx in range(4):  # output row 2 y - 1 + ky is row 2 y + ky of the padded output
            op[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2, :] += x @ wt[:, :, ky, kx]
    return op[:, 1:-1, 1:-1].contiguous()


def wgrad_acc(lo, hi):
    """sum_{f, y, x} lo[f][y][x][a] hi[f][2 y - 1 + ky][2 x - 1 + kx][b] -> [a][b][4][4], rows / columns of hi
    outside the frame reading 0."""
    n, h, w, ca = lo.shape
    hp = torch.zeros(n, 2 * h + 2, 2 * w + 2, hi.shape[3], dtype=lo.dtype)
    hp[:, 1:-1, 1:-1] = hi
    dw = torch.zeros(ca, hi.shape[3], 4, 4, dtype=lo.dtype)
    for ky in range(4):
        for kx in range(4):
            dw[:, :, ky, kx] = torch.einsum("fyxa,fyxb->ab", lo, hp[:, ky:ky + 2 * h:2, kx:kx + 2 * w:2, :])
    return dw


def out3_parts(h, w):
    return (h // O3_TY) * ((w + O3_TX - 1) // O3_TX)


class Check:
    """One expected output.  kind: "lin" (linear in the operands: bit-exact in the integer pass, f32_bound in the
    random pass -- loose_bound for the three-plane split, whose observed error is reported beside the f32 bound),
    "loose" (behind SiLU, SiLU' or tanh: loose_bound), "rel" (1e-4 relative: the tanh-MSE per-frame sums), "sum"
    (sums of a loose output: `bound` given).  reduce: applied to the output before it is compared (partial sums are
    compared after summing over the parts: the partition is internal)."""

    def __init__(self, name, ref, kind, absprod=None, reduce=None, bound=None):
        self.name, self.ref, self.kind, self.absprod, self.reduce, self.bound = name, ref, kind, absprod, reduce, bound


def _sum_bound(elem_ref, dims):
    """Bound of a sum of loose-bound outputs summed in f32 in any order: the elementwise loose bounds add up, plus
    the f32 summation error of N terms, 2 (N + 4) 2^-24 sum|x|."""
    N = 1
    for d in dims:
        N *= elem_ref.shape[d]
    return loose_bound(elem_ref).sum(dims) + 2.0 * (N + 4) * 2.0 ** -24 * elem_ref.abs().sum(dims)


def reference(c, t, fault=None):
    """t: name -> float64 logical operands (materialise().f64).  Returns (checks, K): K the true term count of the
    linear outputs' dot products.  fault: a deliberate break of the formula (tests/test_conv_routes_host.py)."""
    rnd = bf16 if c.one_term else (lambda v: v)
    out = []
    if c.op in (CONV, CONV_S3):
        x, w = rnd(t["in"]), rnd(t["w"])
        if c.cin_raw:  # op_conv_repack_pad: the weight's channels past cin_raw are zero
            w = torch.cat([w, torch.zeros(c.cb, c.ca - c.cin_raw, 4, 4, dtype=w.dtype)], 1)
        if fault == "drop_ky0":
            w = w.clone()
            w[:, :, 0] = 0
        acc, ab = conv_acc(x, w), conv_acc(x.abs(), w.abs())
        K = 16 * c.ca
        nchw = (lambda v: v.permute(0, 3, 1, 2).contiguous()) if c.nchw else (lambda v: v)
        if c.epi == FWD:
            pre = acc + t["bias"]
            if c.save_pre:
                out.append(Check("pre", pre, "lin", ab + t["bias"].abs()))
            out.append(Check("out", nchw(silu(pre)), "loose"))
        else:
            o = acc * dsilu(t["pre"])
            out.append(Check("out", o, "loose"))
            if c.csum:
                out.append(Check("csum", o.sum((0, 1, 2)), "sum", reduce=lambda g: g.sum(0),
                                 bound=_sum_bound(o, (0, 1, 2))))
        return out, K
    if c.op in (CONVT, CONVT_S3):
        x = t["in"]
        x = rnd(silu(x) if c.silu_in else x)
        wt = rnd(t["w"])
        acc, ab = up_acc(x, wt), up_acc(x.abs(), wt.abs())
        K = 4 * c.ca
        pad = lambda v: torch.cat([v, torch.zeros(*v.shape[:3], c.ldc - c.cb, dtype=v.dtype)], 3)
        if c.epi == CT_BIAS:
            pre = acc + t["bias"]
            lin = not c.silu_in and not c.silu_out
            out.append(Check("out", pad(silu(pre) if c.silu_out else pre), "lin" if lin else "loose",
                             pad(ab + t["bias"].abs()) if lin else None))
            if c.out2:
                out.append(Check("out2", pad(silu(pre)), "loose"))
        else:
            out.append(Check("out", acc * dsilu(t["pre"]), "loose"))
        return out, K
    if c.op == OUT3:
        x = silu(t["in"]) if c.silu_in else t["in"]
        mu = torch.tanh(up_acc(x, t["w"]) + t["bias"])
        if not c.loss:
            return [Check("out", mu.permute(0, 3, 1, 2).contiguous(), "loose")], 4 * c.ca
        err = mu - t["target"][..., :3]
        g = t["coef"].reshape(-1, 1, 1, 1) * err * (1 - mu * mu)
        out.append(Check("out", torch.cat([g, torch.zeros(*g.shape[:3], 1, dtype=g.dtype)], 3), "loose"))
        out.append(Check("part", (err * err).sum((1, 2, 3)), "rel", reduce=lambda p: p.sum(1)))
        if c.bpart:
            out.append(Check("bpart", g.sum((1, 2)), "sum", reduce=lambda p: p.sum(1), bound=_sum_bound(g, (1, 2))))
        return out, 4 * c.ca
    if c.op in (WGRAD, WGRAD_S3):
        lo = t["lo"]
        lo = rnd(silu(lo) if c.lo_silu else lo)
        hi = rnd(t["hi"])
        dw, ab = wgrad_acc(lo, hi), wgrad_acc(lo.abs(), hi.abs())
        K = c.n * c.h * c.w
        d0 = t["dw"] if c.acc else torch.zeros(c.ca, c.cbo, 4, 4, dtype=dw.dtype)
        kind = "loose" if c.lo_silu else "lin"
        out.append(Check("dw", c.scale * dw[:, :c.cbo] + d0, kind, abs(c.scale) * ab[:, :c.cbo] + d0.abs()))
        if c.bias_out:  # hi's channel cbo is a pad of ones: tap (1, 1) reads pixel (2 y, 2 x), always inside
            b0 = t["bias_out"] if c.acc else torch.zeros(c.ca, dtype=dw.dtype)
            s, sa = lo.sum((0, 1, 2)), lo.abs().sum((0, 1, 2))
            out.append(Check("bias_out", c.scale * s + b0, kind, abs(c.scale) * sa + b0.abs()))
        return out, K
    if c.op in (CHAN, CHAN_FINAL):
        x = t["in"]
        o0 = t["out"] if c.acc else torch.zeros(c.ca, dtype=x.dtype)
        return [Check("out", x.sum(0) + o0, "lin", x.abs().sum(0) + o0.abs())], c.n
    raise ValueError(c.op)


# ---------------------------------------------------------------------------
# the materialiser: one store, guards, nibbles
# ---------------------------------------------------------------------------
class Region:
    def __init__(self, name, shape, strides, kind, off, span):
        self.name, self.shape, self.strides, self.kind, self.off, self.span = name, shape, strides, kind, off, span

    def view(self, store):
        return store.as_strided(self.shape, self.strides, self.off)


def _contig(shape):
    st, k = [], 1
    for s in reversed(shape):
        st.append(k)
        k *= s
    return tuple(reversed(st))


def layout(c, ws_need):
    """[(name, shape, strides or None, kind, floats or None)]: kind "in" / "out" / "io" (an output that += finds
    initialised) / "scratch" (written, content not compared: repacked weights, workspace)."""
    n, ca, cb, h, w = c.n, c.ca, c.cb, c.h, c.w
    L = []
    if c.op in (CONV, CONV_S3):
        oh, ow = h // 2, w // 2
        L.append(("in", (n, h, w, ca), None, "in", None))
        L.append(("w", (cb, c.cin_raw or ca, 4, 4), None, "in", None))
        L.append(("wr", None, None, "scratch", cb * 16 * ca if c.op == CONV else (3 * 16 * ca * cb + 1) // 2))
        if c.epi == FWD:
            L.append(("bias", (cb,), None, "in", None))
        L.append(("out", (n, cb, oh, ow) if c.nchw else (n, oh, ow, cb), None, "out", None))
        if c.epi == DSILU:
            L.append(("pre", (n, oh, ow, cb), None, "in", None))
        elif c.save_pre:
            L.append(("pre", (n, oh, ow, cb), None, "out", None))
        if c.csum:
            L.append(("csum", ((n * oh * ow + 127) // 128, cb), None, "out", None))
    elif c.op in (CONVT, CONVT_S3, OUT3):
        L.append(("in", (n, h, w, ca), None, "in", None))
        L.append(("w", (ca, cb, 4, 4), None, "in", None))
        wr = 48 * ca if c.op == OUT3 else 16 * ca * cb if c.op == CONVT else (3 * 16 * ca * cb + 1) // 2
        L.append(("wr", None, None, "scratch", wr))
        if c.op == OUT3 or c.epi == CT_BIAS:
            L.append(("bias", (cb,), None, "in", None))
        if c.op == OUT3 and not c.loss:
            L.append(("out", (n, 3, 2 * h, 2 * w), None, "out", None))
        else:
            L.append(("out", (n, 2 * h, 2 * w, c.ldc), None, "out", None))
        if c.op != OUT3 and c.out2:
            L.append(("out2", (n, 2 * h, 2 * w, c.ldc), None, "out", None))
        if c.op != OUT3 and c.epi == CT_DSILU:
            L.append(("pre", (n, 2 * h, 2 * w, cb), None, "in", None))
        if c.op == OUT3 and c.loss:
            ts = c.tstride
            L.append(("target", (n, 2 * h, 2 * w, ts), None, "in", None))
            L.append(("coef", (n,), None, "in", None))
            L.append(("part", (n, out3_parts(h, w)), None, "out", None))
            if c.bpart:
                L.append(("bpart", (n, out3_parts(h, w), 3), None, "out", None))
    elif c.op in (WGRAD, WGRAD_S3):
        L.append(("lo", (n, h, w, ca), (h * w * c.lda, w * c.lda, c.lda, 1), "in", n * h * w * c.lda))
        L.append(("hi", (n, 2 * h, 2 * w, cb), (4 * h * w * c.ldb, 2 * w * c.ldb, c.ldb, 1), "in", 4 * n * h * w * c.ldb))
        L.append(("dw", (ca, c.cbo, 4, 4), None, "io" if c.acc else "out", None))
        L.append(("ws", None, None, "scratch", ws_need))
        if c.bias_out:
            L.append(("bias_out", (ca,), None, "io" if c.acc else "out", None))
    elif c.op == CHAN:
        L.append(("in", (n, ca), (c.lda, 1), "in", n * c.lda))
        L.append(("out", (ca,), None, "io" if c.acc else "out", None))
        L.append(("ws", None, None, "scratch", ws_need))
    elif c.op == CHAN_FINAL:
        L.append(("in", (n, ca), None, "in", None))
        L.append(("out", (ca,), None, "io" if c.acc else "out", None))
    return L


class Mat:
    """The store of a case: .store (float32, CPU), .regions name -> Region, .f64 name -> float64 logical inputs."""

    def __init__(self, c, regions, store):
        self.case, self.regions, self.store = c, regions, store
        self.initial = store.clone()
        self.f64 = {k: r.view(store).double() for k, r in regions.items() if r.kind in ("in", "io") and r.shape}

    def pointer(self, name, base):
        return base + 4 * self.regions[name].off

    def ints(self):
        c, fl = self.case, 0
        has = self.regions.__contains__
        for name, bit in (("bias", F_BIAS), ("pre", F_PRE), ("csum", F_CSUM), ("out2", F_OUT2), ("target", F_TARGET),
                          ("coef", F_COEF), ("part", F_PART), ("bpart", F_BPART), ("bias_out", F_BIAS_OUT), ("ws", F_WS)):
            fl |= bit if has(name) else 0
        fl |= F_NO_REPACK if c.no_repack else 0
        ws = self.regions["ws"].span if has("ws") else 0
        d = dict(op=c.op, n=c.n, ca=c.ca, cb=c.cb, h=c.h, w=c.w, epi=c.epi, nchw=c.nchw, terms=c.terms, lda=c.lda,
                 ldb=c.ldb, ldc=c.ldc, tstride=c.tstride, cbo=c.cbo, silu_in=c.silu_in, silu_out=c.silu_out,
                 lo_silu=c.lo_silu, flags=fl, acc=c.acc, ws_floats=ws, cin_raw=c.cin_raw)
        return [int(d[k]) for k in CV]

    def slots(self, base):
        """CP_* pointers: the weight-gradient and channel-sum ops take their first operand in CP_IN, dW in CP_OUT."""
        alias = {"in": "lo" if self.case.op in (WGRAD, WGRAD_S3) else "in",
                 "out": "dw" if self.case.op in (WGRAD, WGRAD_S3) else "out"}
        return [self.pointer(alias.get(k, k), base) if alias.get(k, k) in self.regions else 0 for k in CP]


def materialise(c, mode, seed=0, ws_need=0):
    """mode "int": operands, bias and the initial dW integers in [-3, 3]; "rand": activations randn, weights randn /
    sqrt(terms of a dot product).  The tensors of the non-linear side (pre-activations, targets, coef) are random in
    both modes."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * c.op + c.n + 31 * c.ca + 17 * c.cb + (mode == "int"))
    regions, off = {}, 0
    for name, shape, strides, kind, floats in layout(c, ws_need):
        nib = c.nib.get(name, 0)
        assert nib % 4 == 0 and 0 <= nib < 16
        start = off + GUARD
        start += (nib // 4 - start) % 4
        strides = strides or (_contig(shape) if shape else None)
        span = floats if floats is not None else 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        regions[name] = Region(name, shape, strides, kind, start, span)
        off = start + span + GUARD
    store = torch.empty(off + 4, dtype=torch.float32)
    store.view(torch.int32).fill_(SENT)
    draw = (lambda *s: torch.randint(-3, 4, s, generator=g).float()) if mode == "int" else (
        lambda *s: torch.randn(*s, generator=g))
    rn = lambda *s: torch.randn(*s, generator=g)
    for name, r in regions.items():
        if r.kind == "in":
            store[r.off - GUARD:r.off + r.span + GUARD] = PAD_IN
        if r.kind not in ("in", "io"):
            continue
        v = r.view(store)
        if name in ("in", "lo", "hi"):
            v.copy_(draw(*r.shape))
        elif name == "w":
            k = 16 * c.ca if c.op in (CONV, CONV_S3) else 4 * c.ca
            v.copy_(draw(*r.shape) if mode == "int" else rn(*r.shape) / k ** 0.5)
        elif name == "bias":
            v.copy_(draw(*r.shape) if mode == "int" else 0.5 * rn(*r.shape))
        elif name in ("dw", "bias_out", "out"):
            v.copy_(draw(*r.shape) if mode == "int" else 0.5 * rn(*r.shape))
        elif name == "pre":
            v.copy_(rn(*r.shape))
        elif name == "target":
            v.copy_(torch.rand(*r.shape, generator=g) - 0.5)
        elif name == "coef":
            v.copy_((0.5 + torch.rand(*r.shape, generator=g)) / (c.n * 12 * c.h * c.w))
    if c.bias_out:  # conv1's shape: hi's channel cbo is op_frames_nhwc4's pad of ones
        regions["hi"].view(store)[..., c.cbo] = 1.0
    return Mat(c, regions, store)


def compare(c, m, final, mode, report=None):
    """The checks of one pass on the store a run left (`final`, CPU float32): the outputs against reference(), then
    the sentinels.  Returns a list of failure strings (empty: the pass is good).  report(name, err, f32 bound): called
    for the outputs without a derived bound."""
    fails = []
    checks, K = reference(c, m.f64)
    fbits, ibits = final.view(torch.int32), m.initial.view(torch.int32)
    for ck in checks:
        r = m.regions[ck.name]
        got = r.view(final).double()
        raw = r.view(fbits)
        if bool((raw == SENT).any()) or bool(got.isnan().any()):
            fails.append(f"{ck.name}: {int(((raw == SENT) | got.isnan()).sum())} of {got.numel()} elements unwritten / NaN")
            continue
        if ck.reduce is not None:
            got = ck.reduce(got)
        ref = ck.ref
        d = (got - ref).abs()
        if mode == "int":
            if ck.kind == "lin" and bool((got.float() != ref.float()).any()):
                bad = got.float() != ref.float()
                i = bad.reshape(-1).nonzero()[0]
                fails.append(f"{ck.name}: integer pass: {int(bad.sum())} of {bad.numel()} wrong, first at flat index "
                             f"{int(i)}: got {float(got.reshape(-1)[i])}, expected {float(ref.reshape(-1)[i])}")
            continue
        if ck.kind == "lin" and not c.three_plane:
            bound = f32_bound(K, ck.absprod, ref)
        elif ck.kind == "rel":
            bound = 1e-4 * ref.abs()
        elif ck.kind == "sum":
            bound = ck.bound
        else:
            bound = loose_bound(ref)
            if report is not None and d.numel():
                k = int(d.argmax())
                fb = float(f32_bound(K, ck.absprod, ref).reshape(-1)[k]) if ck.absprod is not None else float("nan")
                report(ck.name, float(d.max()), fb)
        bad = d > bound
        if bool(bad.any()):
            fails.append(f"{ck.name}: {int(bad.sum())} of {bad.numel()} out of bound, max |d| {float(d.max()):.3e}, "
                         f"worst d / bound {float((d / bound.clamp_min(1e-300)).max()):.3g}")
    # sentinels: only output and scratch elements may differ from the store before the run
    may = torch.zeros(final.numel(), dtype=torch.bool)
    for r in m.regions.values():
        if r.kind == "scratch":
            may[r.off:r.off + r.span] = True
        elif r.kind in ("out", "io"):
            r.view(may).fill_(True)
    moved = (fbits != ibits) & ~may
    if bool(moved.any()):
        i = int(moved.nonzero()[0])
        near = min(m.regions.values(), key=lambda r: min(abs(i - r.off), abs(i - (r.off + r.span))))
        fails.append(f"{int(moved.sum())} floats outside the outputs written, first at store[{i}] (by `{near.name}` "
                     f"[{near.off}, {near.off + near.span}))")
    return fails


def emulate(c, m, fault=None):
    """A stand-in for the GPU on the CPU: the reference's outputs rounded to float32 into a copy of the store, with an
    optional deliberate break (tests/test_conv_routes_host.py: each break must fail compare()).  Breaks: "drop_ky0"
    (the conv loses its ky = 0 taps), "ragged_row" (a ragged tile masks one row too many: the last valid pixel row is
    never stored), "cb_for_cbo" (the weight-gradient reduction strides dW's rows by cb where cbo belongs)."""
    final = m.store.clone()
    checks, _ = reference(c, m.f64, fault=fault)
    for ck in checks:
        r = m.regions[ck.name]
        v = r.view(final)
        if ck.reduce is not None:  # partial sums: everything in part 0, zeros elsewhere
            v.zero_()
            (v[0] if ck.name == "csum" else v[:, 0]).copy_(ck.ref.float())
        elif fault == "cb_for_cbo" and ck.name == "dw":
            val = ck.ref.float()
            for a in range(c.ca):
                final[r.off + a * c.cb * 16:r.off + a * c.cb * 16 + c.cbo * 16] = val[a].reshape(-1)
        else:
            v.copy_(ck.ref.float())
            if fault == "ragged_row" and ck.name == "out" and not c.nchw:
                v.reshape(-1, v.shape[-1])[-1].view(torch.int32).fill_(SENT)
    return final


# ---------------------------------------------------------------------------
# the dispatchers restated on the host: which form a case reaches (None: refused)
# ---------------------------------------------------------------------------
def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def _al(c, *names):
    return all(c.nib.get(k, 0) == 0 for k in names)


def conv_split3_supported(n, cin, ih, iw, cout):
    return (cin in (32, 64, 128, 256) and cout % 64 == 0 and ih % 2 == 0 and iw % 2 == 0
            and ((ih // 2) * (iw // 2)) % 4 == 0 and n * ih * iw * cin < (1 << 31) - (1 << 20))


def convT_cls_supported(n, cin, h, w, cout):
    return cin == 64 and cout == 32 and n > 0 and h % 8 == 0 and w % 16 == 0


def route(c):
    """The form op_* launches for the case, from the dispatch ladders; None where the op refuses."""
    n, ca, cb, h, w = c.n, c.ca, c.cb, c.h, c.w
    lay = "nchw" if c.nchw else "nhwc"
    if c.op == CONV:
        epi = "dsilu" if c.epi == DSILU else "fwd"
        if c.csum and (c.epi != DSILU or c.nchw):
            return None
        if ca == 4 and c.epi == FWD and not c.nchw and cb % 32 == 0:
            return "k_conv1_direct"
        if c.epi == DSILU and c.nchw:
            return None
        if ca == 4 and c.epi == DSILU and cb % 32 == 0 and _al(c, "in", "wr", "pre", "out"):
            return "k_conv4_direct_dsilu"
        if ca not in (4, 8, 16, 32, 64, 128, 256) or cb % 4:
            return None
        if cb <= 16:
            return f"k_conv_nhwc<128,16,{ca},{lay},{epi}>"
        if c.nchw:
            return f"k_conv_nhwc<128,64,{ca},nchw,fwd>"
        return f"k_conv_nhwc<128,{64 if cb % 64 == 0 else 32},{ca},nhwc,{epi}>"
    if c.op == CONV_S3:
        epi = "dsilu" if c.epi == DSILU else "fwd"
        if not conv_split3_supported(n, ca, h, w, cb) or c.terms not in (1, 3) or (c.epi == DSILU and c.nchw):
            return None
        if c.terms == 3:
            if not _al(c, "in", "wr", "out", "bias", "pre"):
                return None
            return f"k_conv_glds_s3<{ca},{lay},{128 if cb % 128 == 0 else 64},{epi}>"
        return f"k_conv_s1<256,{128 if cb % 128 == 0 else 64},{ca},{lay},{epi}>"
    if c.op == CONVT:
        if ca not in (8, 16, 32, 64, 128, 256) or c.ldc < cb or (c.epi == CT_DSILU and c.ldc != cb):
            return None
        bn = 16 if cb <= 16 else 64 if cb % 64 == 0 else 32
        return f"k_convT_nhwc<128,{bn},{ca},{'dsilu' if c.epi == CT_DSILU else 'bias'},{'silu_in' if c.silu_in else 'plain'}>"
    if c.op == CONVT_S3:
        epi = "dsilu" if c.epi == CT_DSILU else "bias"
        cls = convT_cls_supported(n, ca, h, w, cb)
        ok = cls or (ca in (32, 64, 128, 256) and cb > 0 and cb % (32 if c.terms == 1 else 64) == 0)
        if not ok or c.terms not in (1, 3) or c.silu_in or c.ldc != cb:
            return None
        if cls:
            if _al(c, "in", "out", "out2", "pre", "bias"):
                return f"k_convT_cls<{epi},{c.terms}>"
            if c.terms == 3:
                return None
        if c.terms == 3:
            if cb % 64 or not _al(c, "in", "out", "out2", "bias", "pre", "wr"):
                return None
            return f"k_conv_glds_s3<{ca},nhwc,{128 if cb % 128 == 0 else 64},{epi},up>"
        if ca not in (32, 64, 128, 256):
            return None
        return f"k_convT_s1<256,{128 if cb % 128 == 0 else 64 if cb % 64 == 0 else 32},{ca},{epi}>"
    if c.op == OUT3:
        if cb != 3 or h % O3_TY or ca not in (8, 16, 32, 64) or (c.loss and c.tstride < 3):
            return None
        return f"k_convT_out3<{ca},{'loss' if c.loss else 'mu'}>"
    if c.op == WGRAD:
        if (c.bias_out and c.cbo >= cb) or ca % 4 or cb % 4 or c.lda % 4 or c.ldb % 4 or c.lda < ca or c.ldb < cb:
            return None
        return f"k_conv_wgrad<{32 if ca <= 32 else 64 if ca <= 64 else 128}>"
    if c.op == WGRAD_S3:
        ok = (ca in (64, 128, 256) or (c.terms == 1 and ca == 32)) and cb % 8 == 0 and cb >= 8 and _pow2(h) and _pow2(w)
        if not ok or c.lda % 4 or c.ldb % 4 or c.lda < ca or c.ldb < cb or not _al(c, "lo", "hi"):
            return None
        bm, N = (128 if ca >= 128 else 64 if ca >= 64 else 32), 16 * cb
        if c.terms == 1:
            bn = (512 if N % 512 == 0 else 256 if N % 256 == 0 else 128) if bm == 64 else (256 if N % 256 == 0 else 128)
            return f"k_wgrad_s1<{bm},{bn}>"
        bn = 128 if bm == 128 else 256 if N % 256 == 0 else 128
        return f"k_wgrad_split3_db<{bm},{bn},32>"
    if c.op == CHAN:
        if not 0 < ca <= 256 or n <= 0 or c.lda < ca:
            return None
        vec = c.lda % 4 == 0 and _al(c, "in") and c.lda >= (ca + 3) // 4 * 4
        return "k_chan_sum_part4" if vec else "k_chan_sum_part"
    if c.op == CHAN_FINAL:
        return "k_chan_sum_final"
    raise ValueError(c.op)


# ---------------------------------------------------------------------------
# FORMS: the instantiations the ladders can launch
# ---------------------------------------------------------------------------
def _forms():
    f = ["k_conv1_direct", "k_conv4_direct_dsilu"]
    for C in (4, 8, 16, 32, 64, 128, 256):        # DR_CONV_CASE (op_conv_nhwc_ex)
        for bn, lay, epi in ((16, "nchw", "fwd"), (16, "nhwc", "fwd"), (16, "nhwc", "dsilu"), (64, "nchw", "fwd"),
                             (64, "nhwc", "fwd"), (64, "nhwc", "dsilu"), (32, "nhwc", "fwd"), (32, "nhwc", "dsilu")):
            if (C, bn, lay, epi) == (4, 64, "nhwc", "fwd"):
                continue  # cin 4, cout % 64 == 0, forward, NHWC: k_conv1_direct takes every such problem first
            f.append(f"k_conv_nhwc<128,{bn},{C},{lay},{epi}>")
    for C in (32, 64, 128, 256):
        for bn in (128, 64):
            for lay, epi in (("nhwc", "dsilu"), ("nchw", "fwd"), ("nhwc", "fwd")):
                f.append(f"k_conv_glds_s3<{C},{lay},{bn},{epi}>")    # DR_GL (op_conv_glds_s3)
                f.append(f"k_conv_s1<256,{bn},{C},{lay},{epi}>")     # DR_S1F (op_conv_split3_ex, one term)
            for epi in ("bias", "dsilu"):
                f.append(f"k_conv_glds_s3<{C},nhwc,{bn},{epi},up>")  # DR_GT (op_convT_glds_s3)
        for bn in (128, 64, 32):
            for epi in ("bias", "dsilu"):
                f.append(f"k_convT_s1<256,{bn},{C},{epi}>")          # DR_T1L (op_convT_split3, one term)
    for epi in ("bias", "dsilu"):
        for terms in (1, 3):
            f.append(f"k_convT_cls<{epi},{terms}>")                  # launch_convT_cls
    for C in (8, 16, 32, 64, 128, 256):           # convT_cin (op_convT_nhwc)
        for bn in (16, 64, 32):
            for epi in ("bias", "dsilu"):
                for si in ("plain", "silu_in"):
                    f.append(f"k_convT_nhwc<128,{bn},{C},{epi},{si}>")
    for C in (8, 16, 32, 64):                     # DR_O3
        f += [f"k_convT_out3<{C},loss>", f"k_convT_out3<{C},mu>"]
    f += [f"k_conv_wgrad<{bm}>" for bm in (32, 64, 128)]
    f += [f"k_wgrad_s1<{bm},{bn}>" for bm, bn in ((64, 512), (128, 256), (64, 256), (32, 256), (128, 128), (64, 128),
                                                  (32, 128))]                                     # DR_W3L
    f += [f"k_wgrad_split3_db<{bm},{bn},32>" for bm, bn in ((128, 128), (64, 256), (64, 128))]     # DR_W3D
    f += ["k_chan_sum_part4", "k_chan_sum_part", "k_chan_sum_final"]
    return f


FORMS = _forms()


# ---------------------------------------------------------------------------
# TABLE: form -> cases.  Geometries: borders dominate (a 1 x 1 / 1 x 4 / 2 x 2 low-resolution grid, one frame, or
# the smallest the form admits); several frames in one tile with a ragged tail (4 x 8, n = 3, non-square); one tile
# of the form's own BM plus a few rows (n = 33 / 65 / 129 at 2 x 2).
# ---------------------------------------------------------------------------
def _table():
    T = {}
    add = lambda c: T.setdefault(route(c), []).append(c)
    mis = dict(nib={"in": 4})
    # ---- op_conv_nhwc_ex: k_conv_nhwc (BM 128), k_conv1_direct, k_conv4_direct_dsilu ----
    for C in (4, 8, 16, 32, 64, 128, 256):
        raw = 3 if C == 4 else 0
        for co16, co64, co32 in ((8, 64, 32), (16, 192, 96)):
            geo = ((1, 2, 2), (3, 8, 16), (33, 4, 4)) if co16 == 8 else ((1, 2, 8), (3, 8, 16), (1, 4, 4))
            for gi, (n, ih, iw) in enumerate(geo):
                sp = gi != 0
                add(Case(CONV, n, C, co16, ih, iw, nchw=1, cin_raw=raw, save_pre=sp))
                add(Case(CONV, n, C, co16, ih, iw, cin_raw=raw, save_pre=gi != 1))
                add(Case(CONV, n, C, co16, ih, iw, epi=DSILU, cin_raw=raw, csum=sp))
                add(Case(CONV, n, C, co64, ih, iw, nchw=1, cin_raw=raw, save_pre=sp))
                add(Case(CONV, n, C, co32, ih, iw, nchw=1, cin_raw=raw))
                # cin 4 with cout % 32 == 0: the direct kernels, or (dsilu, an operand off 16 bytes) the ladder
                add(Case(CONV, n, C, co64, ih, iw, cin_raw=raw, save_pre=sp))
                add(Case(CONV, n, C, co32, ih, iw, cin_raw=raw, save_pre=gi != 1))
                add(Case(CONV, n, C, co64, ih, iw, epi=DSILU, cin_raw=raw, csum=sp))
                add(Case(CONV, n, C, co32, ih, iw, epi=DSILU, cin_raw=raw, csum=not sp))
                if C == 4:
                    add(Case(CONV, n, 4, 20 if co16 == 8 else 36, ih, iw, cin_raw=3, save_pre=sp))
                    add(Case(CONV, n, 4, co64, ih, iw, epi=DSILU, cin_raw=3, csum=sp, **mis))
                    add(Case(CONV, n, 4, co32, ih, iw, epi=DSILU, cin_raw=3, **mis))
        # a feature grid no float4 tiles (1 x 3: a 16 x 48 frame's last layer) on the NCHW forms
        add(Case(CONV, 2, C, 8, 2, 6, nchw=1, cin_raw=raw, save_pre=True))
        add(Case(CONV, 2, C, 64, 2, 6, nchw=1, cin_raw=raw))
    # ---- six-product and one-term convs: oh ow % 4 == 0, tiles of 8 RW = 256 (BN 128) / 512 (BN 64; k_conv_s1: 256) ----
    for C in (32, 64, 128, 256):
        for co, big in ((128, 65), (64, 129), (192, 129)):
            for terms in (3, 1):
                nb = big if terms == 3 else 65
                for gi, (n, ih, iw) in enumerate(((1, 2, 8), (3, 8, 16), (nb, 4, 4))):
                    if co == 192 and gi == 2:
                        continue
                    add(Case(CONV_S3, n, C, co, ih, iw, terms=terms, save_pre=gi != 0))
                    add(Case(CONV_S3, n, C, co, ih, iw, terms=terms, nchw=1, save_pre=gi != 1))
                    add(Case(CONV_S3, n, C, co, ih, iw, terms=terms, epi=DSILU))
    # ---- op_convT_nhwc: k_convT_nhwc (BM 128 low-resolution pixels) ----
    for C in (8, 16, 32, 64, 128, 256):
        for co16, co64, co32 in ((8, 64, 32), (16, 192, 40)):
            geo = ((1, 1, 1), (3, 4, 8), (33, 2, 2)) if co16 == 8 else ((1, 1, 4), (1, 2, 2))
            for gi, (n, h, w) in enumerate(geo):
                for si in (0, 1):
                    for co in (co16, co64, co32):
                        # ldc > cout where the last column tile has room for the extra channels (cout 8 and 40)
                        ldc = co + 4 if co in (8, 40) and gi == 1 else 0
                        add(Case(CONVT, n, C, co, h, w, silu_in=si, out2=gi == 1, silu_out=int(gi == 2), ldc=ldc))
                        add(Case(CONVT, n, C, co, h, w, silu_in=si, epi=CT_DSILU))
    # ---- op_convT_split3: the all-class kernel (64 -> 32, 8 x 16 anchor tiles), LDS-DMA (terms 3), k_convT_s1 ----
    for terms in (3, 1):
        for n, h, w in ((1, 8, 16), (3, 8, 16), (2, 8, 32)):
            add(Case(CONVT_S3, n, 64, 32, h, w, terms=terms, out2=n == 3, silu_out=int(n == 2)))
            add(Case(CONVT_S3, n, 64, 32, h, w, terms=terms, epi=CT_DSILU))
    for C in (32, 64, 128, 256):
        for co, big in ((128, 65), (64, 129), (192, 129), (32, 65), (96, 65)):
            for terms in (3, 1):
                if terms == 3 and co % 64:
                    continue
                nb = big if terms == 3 else 65
                for gi, (n, h, w) in enumerate(((1, 1, 1), (3, 4, 8), (nb, 2, 2))):
                    if co in (192, 96) and gi == 2:
                        continue
                    add(Case(CONVT_S3, n, C, co, h, w, terms=terms, out2=gi == 1, silu_out=int(gi == 2)))
                    add(Case(CONVT_S3, n, C, co, h, w, terms=terms, epi=CT_DSILU))
    # ---- op_convT_out3: h % 8 == 0, tiles of 8 x 32 low-resolution pixels ----
    for C in (8, 16, 32, 64):
        for gi, (n, h, w) in enumerate(((1, 8, 1), (3, 8, 4), (2, 8, 33), (1, 16, 4))):
            add(Case(OUT3, n, C, 3, h, w, tstride=4 if gi % 2 == 0 else 3, bpart=gi != 0, silu_in=int(gi == 1)))
            add(Case(OUT3, n, C, 3, h, w, loss=False, silu_in=int(gi == 2)))
    # ---- op_conv_wgrad: the tile runs along K = n h w (chunks of 32) ----
    kgeo = ((1, 2, 2), (3, 2, 2), (5, 4, 4), (7, 4, 8), (3, 1, 1))
    for ca, cb in ((8, 4), (32, 8), (48, 16), (64, 32), (96, 8), (128, 16), (256, 8)):
        for gi, (n, h, w) in enumerate(kgeo):
            if cb == 4:  # conv1's shape: three channels and the pad of ones
                add(Case(WGRAD, n, ca, 4, h, w, cbo=3, bias_out=True, acc=gi % 2, scale=0.5 if gi % 2 else 1.0))
            else:
                add(Case(WGRAD, n, ca, cb, h, w, lda=ca + 4 * (gi % 2), ldb=cb + 8 * (gi == 2), cbo=cb - (gi == 3),
                         lo_silu=int(gi == 4), acc=int(gi in (1, 3)), scale=(1.0, 2.0, 0.25, 0.5, 1.0)[gi]))
    # ---- op_wgrad_split3: chunks of 64, power-of-two frames, 8-pixel staging units that span rows and frames ----
    k3 = ((1, 2, 2), (3, 2, 2), (5, 4, 4), (9, 4, 4), (3, 1, 1))
    for ca, cb in ((32, 8), (32, 16), (64, 8), (64, 16), (64, 32), (128, 8), (128, 16), (256, 16), (256, 8)):
        for terms in (1, 3):
            if terms == 3 and ca == 32:
                continue
            for gi, (n, h, w) in enumerate(k3):
                add(Case(WGRAD_S3, n, ca, cb, h, w, terms=terms, lda=ca + 4 * (gi % 2), ldb=cb + 8 * (gi == 2),
                         cbo=cb - (gi == 3), acc=int(gi in (1, 3)), scale=(1.0, 2.0, 0.25, 0.5, 1.0)[gi]))
    # ---- channel sums ----
    for rows, C, ldx, acc in ((1000, 3, 4, 0), (5000, 32, 32, 1), (50, 256, 256, 0), (1, 8, 12, 0), (33, 5, 8, 1)):
        add(Case(CHAN, rows, C, 0, 1, 1, lda=ldx, acc=acc))
    for rows, C, ldx, acc, nib in ((1000, 3, 3, 0, 0), (700, 5, 5, 1, 0), (300, 32, 32, 0, 4), (1, 7, 9, 0, 0)):
        add(Case(CHAN, rows, C, 0, 1, 1, lda=ldx, acc=acc, nib={"in": nib}))
    for nb, C, acc in ((1, 3, 0), (300, 64, 1), (256, 1, 0), (17, 256, 1)):
        add(Case(CHAN_FINAL, nb, C, 0, 1, 1, acc=acc))
    return T


TABLE = _table()

# refusals: DR_E_INVALID and nothing launched (the hook skips the repack for these)
REFUSALS = {
    "conv cin 24": Case(CONV, 2, 24, 32, 8, 8, no_repack=True),
    "convT cin 24": Case(CONVT, 2, 24, 32, 4, 4, no_repack=True),
    "out3 cin 128": Case(OUT3, 1, 128, 3, 8, 8, no_repack=True),
    "six-product conv, in off 16 bytes": Case(CONV_S3, 3, 64, 64, 8, 16, nib={"in": 4}, no_repack=True),
    "six-product upsampling conv, in off 16 bytes": Case(CONVT_S3, 3, 64, 64, 4, 8, nib={"in": 8}, no_repack=True),
    "six-product all-class kernel, out off 16 bytes": Case(CONVT_S3, 1, 64, 32, 8, 16, nib={"out": 4}, no_repack=True),
    "out3 h % 8": Case(OUT3, 1, 16, 3, 4, 8, no_repack=True),
    "wgrad_split3 w not a power of two": Case(WGRAD_S3, 2, 64, 8, 4, 6),
    "csum with NCHW": Case(CONV, 2, 8, 16, 8, 8, epi=DSILU, nchw=1, csum=True, no_repack=True),
}
