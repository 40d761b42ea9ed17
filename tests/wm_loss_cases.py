"""The inputs, expected outputs and tolerances of tests/test_gpu_wm_loss.py, shared with tests/test_wm_loss_host.py
(which checks, without a GPU, that these very inputs tell every mutation of wm_loss_ref.MUTATIONS from the reference).

A Case is one call of dr_internal_wm_loss_run: the op, its ints and doubles, the pointer slots (an input buffer, an
output buffer description, or None) and ref(mut) -> {output: Want}.  Input buffers carry NaN in their padding (columns
past the logical width, a guard row): a kernel that reads it shows.  Output buffers are filled with a NaN of a payload
no arithmetic produces (POISON): what must stay unwritten is compared bit for bit.

Tolerances.  A Want holds either `tol`, a derived bound (sums: (longest chain + tree depth + c) 2^-24 sum|terms|, the
chain counted from the launcher's geometry, cited where it is formed; copies and three-rounding products: a few 2^-24 of
the value), or `key` and `scale`: the output goes through expf / logf / tanhf or a cancelling chain of products, the
device library's error is not derived, and the bound is 4 x MEASURED[key] x 2^-24 x scale, MEASURED being the largest
error of that output over all its cases on the first MI355X run (profiles/wm_loss_errors.txt).  `scale` is the
output's own size: max |ref| over the row, or where a row mixes magnitudes the size of the terms the value is made of
(stated per op below)."""
import math
import os

import torch

import primitives_ref as PR
import wm_loss_ref as R

U = R.U
F32 = torch.float32
F64 = torch.float64
POISON = 0x7FE5A5A5  # a quiet NaN with a payload
NAN = float("nan")
INF = float("inf")

# largest |got - ref| / (2^-24 scale) per output over every case of its op, first MI355X run
# (profiles/wm_loss_errors.txt); the asserted bound is 4 x this
MEASURED = {
    "kl_fwd.kl_grp": 8.470, "kl_bwd.g_prior": 2.809, "kl_bwd.g_post": 1.025,
    "heads.rew_row": 2.359, "heads.cont_row": 1.675, "heads.g_rew": 3.971, "heads.g_cont": 1.762,
    "ste_bwd_add.gl": 3.936, "softmax_ste_bwd.gl": 3.936,
    "gru_bwd.g_gi": 0.282, "gru_bwd.g_gh": 0.257,
    "ln_silu_bwd.g_pre": 3.406, "ln_silu_bwd.gy": 2.043, "ln_silu_bwd.xhat": 1.972,
}
MEASURING = bool(os.environ.get("WM_LOSS_ERRORS"))


def bound(key):
    """Asserted units of 2^-24 x scale for a measured output (2^100 while the table is being measured)."""
    if key not in MEASURED and MEASURING:
        return 2.0 ** 100
    return 4.0 * MEASURED[key]


def poison(*shape, dtype="f32"):
    if dtype == "i32":
        return torch.full(shape, -7, dtype=torch.int32)
    if dtype == "u16":
        return torch.full(shape, -1, dtype=torch.int16)
    return torch.full(shape, POISON, dtype=torch.int32).view(F32)


def is_poison(t):
    if t.dtype == torch.int32:
        return t == -7
    if t.dtype == torch.int16:
        return t == -1
    return t.view(torch.int32) == POISON


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *s, scale=1.0):
    return (torch.randn(*s, generator=g) * scale).to(F32)


def padded(x, ld=None, guard=1):
    """x [M, N] (or [N]) in the corner of a NaN buffer [M + guard][ld]."""
    if x.dim() == 1:
        b = torch.full((x.numel() + guard,), NAN)
        b[:x.numel()] = x
        return b
    M, N = x.shape
    b = torch.full((M + guard, N if ld is None else ld), NAN)
    b[:M, :N] = x
    return b


class Out:
    """An output buffer: `shape` elements (dtype f32 / i32 / u16), of which the op writes `region` (slices; default
    all of it); `init`: the region's contents before the call (in / out operands), else POISON like the rest."""

    def __init__(self, name, shape, region=None, init=None, dtype="f32"):
        self.name, self.shape, self.dtype = name, tuple(shape), dtype
        self.region = region if region is not None else tuple(slice(None) for _ in self.shape)
        self.init = init

    def make(self):
        b = poison(*self.shape, dtype=self.dtype)
        if self.init is not None:
            b[self.region] = self.init
        return b


class Want:
    def __init__(self, ref, tol=None, key=None, scale=None, nan_ok=None):
        self.ref = ref.to(F64)
        self.key = key
        self.scale = None if scale is None else torch.as_tensor(scale, dtype=F64).expand_as(self.ref)
        self._tol = None if tol is None else torch.as_tensor(tol, dtype=F64).expand_as(self.ref)
        self.nan_ok = nan_ok  # elements that may be NaN instead of ref (a NaN input's row)
        assert (tol is None) != (key is None)
        if key is not None and scale is None:
            self.scale = row_scale(self.ref)

    @property
    def tol(self):
        return self._tol if self._tol is not None else bound(self.key) * U * self.scale


def row_scale(ref):
    """max |ref| over each row (dim 0) of a >= 2-D output, over all of a 1-D one; non-finite values left out."""
    a = torch.where(torch.isfinite(ref), ref.abs(), torch.zeros_like(ref))
    if ref.dim() >= 2:
        m = a.reshape(a.shape[0], -1).max(1).values
        return m.reshape(-1, *([1] * (ref.dim() - 1))).expand_as(ref)
    return (a.max() if a.numel() else a.sum()).expand_as(ref)


class Case:
    def __init__(self, op, label, v, num, slots, ref, checks=()):
        self.op, self.label, self.v, self.num, self.slots, self.ref, self.checks = op, label, v, num, slots, ref, checks
        self._wants = None

    def wants(self):
        """ref() of the unmutated reference, computed once."""
        if self._wants is None:
            self._wants = self.ref()
        return self._wants

    @property
    def name(self):
        return R.OP_NAMES[self.op]

    def outs(self):
        return [s for s in self.slots if isinstance(s, Out)]

    def __repr__(self):
        return f"{self.name}[{self.label}]"


def _cdiv(a, b):
    return -(-a // b)


def pow2_ge(c):
    w = 1
    while w < c:
        w <<= 1
    return w


# ----------------------------------------------------------------------------
# gather
# ----------------------------------------------------------------------------
def gather_cases():
    out = []
    for B, T, A, pad in ((1, 1, 1, 0), (3, 4, 2, 3), (70, 5, 3, 1)):  # 350 rows: two workgroups, the last partly valid
        g = gen(B)
        S = T + pad  # the replay windows are longer than the horizon
        act, rew, cont = randn(g, B, S, A), randn(g, B, S), (torch.rand(B, S, generator=g) > 0.3).float()
        v = [B, T, A, S * A, A, S, 1]

        def ref(mut=None, act=act, rew=rew, cont=cont, T=T):
            r = R.gather(act[:, :T], rew[:, :T], cont[:, :T])
            return {k: Want(x, tol=0.0) for k, x in r.items()}
        slots = [act.reshape(-1), rew.reshape(-1), cont.reshape(-1),
                 Out("act_tm", (B * T + 1, A), (slice(0, B * T), slice(None))),
                 Out("rew_tm", (B * T + 1,), (slice(0, B * T),)), Out("cont_tm", (B * T + 1,), (slice(0, B * T),))]
        out.append(Case(R.GATHER, f"B{B}-T{T}-A{A}", v, [], slots, ref))
    return out


# ----------------------------------------------------------------------------
# prep: k_wm_masksum (1 x 256 threads: chain ceil(M1 / 256), tree depth 8) then k_wm_coef
# ----------------------------------------------------------------------------
SUM_M1 = (1, 255, 256, 257, 600)


def prep_cases():
    out = []
    for M1 in SUM_M1:
        for kind in ("local", "allreduced", "masked", "fraction"):
            g = gen(M1)
            cont = (torch.rand(M1, generator=g) > 0.3).float()
            cont[0] = 1.0
            stats0 = None
            if kind == "allreduced":  # mask.sum() over four ranks, written over the local sum
                stats0 = float(cont.sum()) * 4 - 3
            elif kind == "masked":
                cont.zero_()
            elif kind == "fraction":  # continues need not be 0 / 1: a small mask sum
                cont = cont * 0.01 / max(M1 // 8, 1)
            beta = 0.75

            def ref(mut=None, cont=cont, stats0=stats0, M1=M1, beta=beta):
                r = R.prep(cont, beta, stats0, mut)
                chain = _cdiv(M1, 256) + 8 + 1
                s_tol = 0.0 if stats0 is not None else chain * U * float(cont.double().abs().sum())
                # scal[0]: the sum's error and one addition; coef: that, the product and the division
                rel = (s_tol / float(r["scal0"]) if float(r["scal0"]) > 0 else 0.0)
                return dict(stats=Want(r["stats0"], tol=s_tol),
                            scal=Want(r["scal0"], tol=s_tol + 1.5 * U * r["scal0"].abs()),
                            coef_row=Want(r["coef_row"], tol=(4 * U + rel) * r["coef_row"].abs()),
                            coef_obs=Want(r["coef_obs"], tol=(4 * U + rel) * r["coef_obs"].abs()))
            slots = [padded(cont), Out("stats", (8,), (slice(0, 1),)), Out("scal", (8,), (slice(0, 1),)),
                     Out("coef_row", (M1 + 2,), (slice(0, M1),)), Out("coef_obs", (M1 + 2,), (slice(0, M1),))]
            out.append(Case(R.PREP, f"M{M1}-{kind}", [M1, 1 if stats0 is not None else 0],
                            [beta, stats0 if stats0 is not None else 0.0], slots, ref))
    return out


# ----------------------------------------------------------------------------
# grouped kernels: one latent group on W = pow2 >= C lanes, 256-thread workgroups
# ----------------------------------------------------------------------------
GROUPED_RC = ((3, 1), (2, 2), (5, 3), (3, 24), (8, 8), (32, 32), (2, 33), (1, 64))


def grouped_m1(R_, C):
    """1, 15, and an M1 whose last workgroup is partly valid (M1 R W no multiple of 256) where one exists."""
    W = pow2_ge(C)
    ms = [1, 15]
    for m in (7, 3, 5, 2):
        if (m * R_ * W) % 256:
            ms.append(m)
            break
    return ms


def quant(x, q=64.0):
    return torch.round(x * q) / q


def kl_inputs(M1, R_, C, seed):
    """Random logits (multiples of 2^-6, so that adding 1e4 to a group is exact) and the needles, each in group 0 of
    its own row where M1 allows: 0 identical post and prior; 1-4 one logit at +-80 in post / prior; 5 = row 6 + 1e4 on
    every logit of the group; 7 mask 0 on a row with KL ~ 160 (post +80, prior -80 on one class)."""
    g = gen(seed)
    prior, post = quant(randn(g, M1, R_, C, scale=2.0)), quant(randn(g, M1, R_, C, scale=2.0))
    cont = (torch.rand(M1, generator=g) > 0.3).float()
    post[0, 0] = prior[0, 0]
    cont[0] = 1.0
    if M1 >= 8:
        post[1, 0, 0], post[2, 0, C - 1] = 80.0, -80.0
        prior[3, 0, 0], prior[4, 0, C - 1] = 80.0, -80.0
        post[5, 0], prior[5, 0] = post[6, 0] + 1e4, prior[6, 0] + 1e4
        post[7, 0, 0], prior[7, 0, 0] = 80.0, -80.0
        cont[1:7] = 1.0
        cont[7] = 0.0
    return prior, post, cont


def kl_term_sizes(prior, post):
    """(p, size): softmax(post) and the size of what lp - lq is made of per class, |x - max| and log sum exp(x - max)
    on both sides and the difference itself -- the scale of the KL (sum p size) and of its gradients."""
    xp, xq = f64(post), f64(prior)
    dp, dq = xp - xp.max(-1, keepdim=True).values, xq - xq.max(-1, keepdim=True).values
    lsp, lsq = torch.logsumexp(dp, -1, keepdim=True), torch.logsumexp(dq, -1, keepdim=True)
    return torch.softmax(xp, -1), dp.abs() + dq.abs() + lsp + lsq + ((dp - lsp) - (dq - lsq)).abs()


def kl_cases():
    fwd, bwd = [], []
    for R_, C in GROUPED_RC:
        for M1 in grouped_m1(R_, C):
            prior, post, cont = kl_inputs(M1, R_, C, 100 * R_ + C + M1)
            # the factors k_wm_final leaves: beta_dyn wk / rows, beta_rep wk / rows with the clamp open
            scal = torch.tensor([NAN, 0.5 / (M1 + 3), 0.1 / (M1 + 3), NAN, NAN, NAN, NAN, NAN])

            def ref_f(mut=None, prior=prior, post=post):
                p, size = kl_term_sizes(prior, post)
                return dict(kl_grp=Want(R.kl_fwd(prior, post)["kl_grp"], key="kl_fwd.kl_grp", scale=(p * size).sum(-1)))

            def ref_b(mut=None, prior=prior, post=post, cont=cont, scal=scal):
                r = R.kl_bwd(prior, post, cont, scal, mut)
                p, size = kl_term_sizes(prior, post)
                m = f64(cont).reshape(-1, 1, 1)
                # g_prior = cd (q - p): cd times a probability difference; g_post = cr p (lp - lq - KL)
                return dict(g_prior=Want(r["g_prior"], key="kl_bwd.g_prior", scale=float(scal[1]) * m),
                            g_post=Want(r["g_post"], key="kl_bwd.g_post",
                                        scale=float(scal[2]) * m * (p * (size + (p * size).sum(-1, keepdim=True))).max(-1, keepdim=True).values))

            def chk_f(o, M1=M1, C=C):
                f = []
                if float(o["kl_grp"][0, 0]) != 0.0:
                    f.append(f"identical post and prior: KL {float(o['kl_grp'][0, 0])!r}, not exactly 0")
                if M1 >= 8 and not torch.equal(o["kl_grp"][5, :1].view(torch.int32), o["kl_grp"][6, :1].view(torch.int32)):
                    f.append("KL changes under a constant offset of 1e4 on the group's logits")
                if bool(torch.isnan(o["kl_grp"]).any()):
                    f.append("NaN in kl_grp")
                return f

            def chk_b(o, M1=M1):
                f = []
                for k in ("g_prior", "g_post"):
                    if bool((o[k][0, 0] != 0).any()):
                        f.append(f"identical post and prior: {k} not exactly 0")
                    if M1 >= 8:
                        if bool((o[k][7] != 0).any()):
                            f.append(f"{k} not exactly 0 on the masked row")
                        if not torch.equal(o[k][5, 0].view(torch.int32), o[k][6, 0].view(torch.int32)):
                            f.append(f"{k} changes under a constant offset of 1e4")
                    if bool(torch.isnan(o[k]).any()):
                        f.append(f"NaN in {k}")
                return f
            lab = f"R{R_}-C{C}-M{M1}"
            fwd.append(Case(R.KL_FWD, lab, [M1, R_, C], [],
                            [padded(prior.reshape(-1)), padded(post.reshape(-1)),
                             Out("kl_grp", (M1 + 1, R_), (slice(0, M1), slice(None)))], ref_f, [chk_f]))
            bwd.append(Case(R.KL_BWD, lab, [M1, R_, C], [],
                            [padded(prior.reshape(-1)), padded(post.reshape(-1)), padded(cont), scal,
                             Out("g_prior", (M1 + 1, R_, C), (slice(0, M1), slice(None), slice(None))),
                             Out("g_post", (M1 + 1, R_, C), (slice(0, M1), slice(None), slice(None)))], ref_b, [chk_b]))
    return fwd, bwd


def ste_cases():
    add, plain = [], []
    for R_, C in GROUPED_RC:
        for M in grouped_m1(R_, C):
            g = gen(7 * R_ + C + M)
            L = R_ * C
            gz = randn(g, M, R_, C)
            soft = torch.softmax(randn(g, M, R_, C, scale=2.0), -1)
            extra = randn(g, M, R_, C, scale=0.1)
            for with_extra in (True, False):
                def ref(mut=None, gz=gz, soft=soft, ex=extra if with_extra else None):
                    # scale: the row's largest soft |0.99 gz| (the products the value is made of) and |extra|
                    sc = (f64(soft) * f64(gz).abs()).reshape(gz.shape[0], -1).max(1).values.reshape(-1, 1, 1) \
                        + (0 if ex is None else f64(ex).abs())
                    return dict(gl=Want(R.ste_bwd(gz, soft, ex, mut)["gl"], key="ste_bwd_add.gl", scale=sc))
                ld = (L + 3, L + 5, L + 1, L + 7)
                slots = [padded(gz.reshape(M, L), ld[0]), padded(soft.reshape(M, L), ld[1]),
                         padded(extra.reshape(M, L), ld[2]) if with_extra else None,
                         Out("gl", (M + 1, ld[3]), (slice(0, M), slice(0, L)))]
                add.append(Case(R.STE_BWD_ADD, f"R{R_}-C{C}-M{M}-{'extra' if with_extra else 'plain'}",
                                [M, R_, C, *ld], [], slots, lambda mut=None, r=ref: _reshape2(r(mut))))

            def ref_s(mut=None, gz=gz, soft=soft):
                sc = (f64(soft) * f64(gz).abs()).reshape(gz.shape[0], -1).max(1).values.reshape(-1, 1, 1)
                return _reshape2(dict(gl=Want(R.ste_bwd(gz, soft, None, mut)["gl"], key="softmax_ste_bwd.gl", scale=sc)))
            plain.append(Case(R.SOFTMAX_STE_BWD, f"R{R_}-C{C}-M{M}", [M, R_, C, L + 2, L + 4], [],
                              [padded(gz.reshape(M, L), L + 2), padded(soft.reshape(M, L), L + 4),
                               Out("gl", (M + 1, L), (slice(0, M), slice(None)))], ref_s))
    return add, plain


f64 = R.f64


def _reshape2(wants):
    """[M, R, C] wants as the [M, R C] rows the buffers hold."""
    out = {}
    for k, w in wants.items():
        M = w.ref.shape[0]
        n = Want(w.ref.reshape(M, -1), key=w.key, scale=w.scale.reshape(M, -1))
        out[k] = n
    return out


# ----------------------------------------------------------------------------
# heads: one wave per row, four rows per workgroup, 64-lane loops over nb
# ----------------------------------------------------------------------------
HEADS_NB = (2, 63, 64, 65, 255)
HEADS_M1 = (1, 4, 5, 259)
CLOG_NEEDLES = [(x, y) for x in (-100.0, -20.0, 0.0, 20.0, 100.0) for y in (0.0, 1.0, 0.3)]


def buckets_of(kind, nb):
    if kind == "model":    # RewardPredictor.buckets_rew: uniform in symlog space
        return torch.linspace(-20.0, 20.0, nb)
    if kind == "symexp":   # ... and as rewards: symexp spacing, gaps from 0.04 to 30
        return PR.symexp(torch.linspace(-5.0, 5.0, nb)).to(F32)
    return torch.linspace(-1e-4, 1e-4, nb)  # "narrow": gaps down to 8e-7, where the two-hot weight's 1e-8 counts


def reward_needles(b, neighbours_first):
    nb = b.numel()
    up = torch.nextafter(b, torch.full_like(b, INF))
    dn = torch.nextafter(b, torch.full_like(b, -INF))
    ends = [0, nb - 1, nb - 2] if nb > 2 else [0, 1]
    special = [INF, -INF, float(b[-1]) * 2 + 1, float(b[0]) * 2 - 1, NAN]
    for k in ends:
        special += [float(b[k]), float(up[k]), float(dn[k])]
    on = [float(x) for x in b]
    nbr = [float(x) for pair in zip(up, dn) for x in pair]
    return special + (nbr + on if neighbours_first else on + nbr)


def heads_cases():
    out = []
    i = 0
    for nb in HEADS_NB:
        for M1 in HEADS_M1:
            for kind in (("model", "symexp", "narrow") if M1 == 259 else (("model", "symexp", "narrow")[i % 3],)):
                i += 1
                g = gen(1000 * nb + M1 + len(kind))
                b = buckets_of(kind, nb)
                rew = randn(g, M1) * float(b[-1] - b[0]) / 4
                nd = reward_needles(b, neighbours_first=(kind == "symexp"))
                # the NaN needle goes to row 4 (or nowhere): M1 <= 4 keeps every loss finite
                nd = [x for x in nd if x == x]
                k = min(M1, len(nd))
                rew[:k] = torch.tensor(nd[:k])
                nan_row = 4 if M1 > 4 else None
                if nan_row is not None:
                    rew[nan_row] = NAN
                rlog, clog = randn(g, M1, nb, scale=3.0), randn(g, M1, scale=2.0)
                cont = (torch.rand(M1, generator=g) > 0.3).float()
                for r_, (x, y) in enumerate(CLOG_NEEDLES):
                    if 5 + r_ < M1:
                        clog[5 + r_], cont[5 + r_] = x, y
                coef = torch.rand(M1, generator=g) + 0.1
                if M1 > 19:  # a zero factor on rows with extreme logits (continue logit 100; reward logits +-80)
                    coef[19], coef[20] = 0.0, 0.0
                    rlog[20, 0], rlog[20, nb - 1] = 80.0, -80.0

                def ref(mut=None, rlog=rlog, clog=clog, rew=rew, cont=cont, b=b, coef=coef, nan_row=nan_row):
                    r = R.heads(rlog, clog, rew, cont, b, coef, mut)
                    c = f64(coef)
                    g_rew, nan_ok = r["g_rew"], None
                    if nan_row is not None:  # the row's gradient: NaN on the two-hot's two buckets, right elsewhere
                        g_rew = g_rew.clone()
                        g_rew[nan_row] = c[nan_row] * torch.softmax(f64(rlog[nan_row]), -1)
                        nan_ok = torch.zeros_like(g_rew, dtype=torch.bool)
                        nan_ok[nan_row] = True
                    # scales: log-softmax is lse - x, the BCE (1 - y) x + softplus(-x): the terms' sizes; the
                    # gradients are coef times a probability difference
                    return dict(
                        rew_row=Want(r["rew_row"], key="heads.rew_row", scale=f64(rlog).abs().max(-1).values + r["rew_row"].abs().nan_to_num(0.0)),
                        cont_row=Want(r["cont_row"], key="heads.cont_row", scale=f64(clog).abs() + 1.0),
                        g_rew=Want(g_rew, key="heads.g_rew", scale=c.reshape(-1, 1), nan_ok=nan_ok),
                        g_cont=Want(r["g_cont"], key="heads.g_cont", scale=c))

                def chk(o, nan_row=nan_row, M1=M1):
                    f = []
                    if nan_row is not None:
                        if not math.isnan(float(o["rew_row"][nan_row])):
                            f.append("NaN reward: the row loss is not NaN")
                        if not bool(torch.isnan(o["g_rew"][nan_row]).any()):
                            f.append("NaN reward: no NaN in the row's gradient")
                    keep = [r_ for r_ in range(M1) if r_ != nan_row]
                    for k_ in ("rew_row", "cont_row", "g_rew", "g_cont"):  # the continue head does not read the reward
                        rows_ = keep if k_ in ("rew_row", "g_rew") else list(range(M1))
                        if bool(torch.isnan(o[k_][rows_]).any()):
                            f.append(f"NaN in {k_} outside the NaN reward's own outputs")
                    if M1 > 20:
                        for r_ in (19, 20):
                            if bool((o["g_rew"][r_] != 0).any()) or float(o["g_cont"][r_]) != 0.0:
                                f.append(f"coef_row 0 on row {r_}: a gradient that is not exactly 0")
                    return f
                slots = [padded(rlog.reshape(-1)), padded(clog), padded(rew), padded(cont), b.clone(), padded(coef),
                         Out("rew_row", (M1 + 4,), (slice(0, M1),)), Out("cont_row", (M1 + 4,), (slice(0, M1),)),
                         Out("g_rew", (M1 + 4, nb), (slice(0, M1), slice(None))), Out("g_cont", (M1 + 4,), (slice(0, M1),))]
                out.append(Case(R.HEADS, f"nb{nb}-M{M1}-{kind}", [M1, nb], [], slots, ref, [chk]))
    return out


# ----------------------------------------------------------------------------
# stats: 1 x 256 threads, chain ceil(M1 / 256) rows a thread, each row's parts / groups added first, tree depth 8
# ----------------------------------------------------------------------------
def loss_rows(g, M1, R_, nparts, masked=False):
    obs = torch.rand(M1, nparts, generator=g) * 50
    rew, cont_row = -torch.rand(M1, generator=g) * 6, torch.rand(M1, generator=g) * 2
    kl = torch.rand(M1, R_, generator=g) * 0.2
    cont = (torch.rand(M1, generator=g) > 0.3).float()
    if masked:
        cont.zero_()
    if M1 >= 3:  # a masked row whose terms are huge
        cont[2] = 0.0
        obs[2], rew[2], cont_row[2], kl[2] = 1e30, -1e30, 1e30, 1e30
    return obs, rew, cont_row, kl, cont


def stats_cases():
    out = []
    for M1 in SUM_M1:
        for nparts in (1, 4):
            for R_ in (1, 32):
                for masked in ((False, True) if (nparts, R_) == (4, 32) else (False,)):
                    g = gen(M1 * 7 + nparts + R_)
                    obs, rew, cont_row, kl, cont = loss_rows(g, M1, R_, nparts, masked)

                    def ref(mut=None, a=(obs, rew, cont_row, kl, cont), M1=M1, nparts=nparts, R_=R_):
                        s = R.stats(*a)["stats"]
                        sabs = R.stats_terms(a[0].abs(), a[1].abs(), a[2].abs(), a[3].abs(), a[4]).sum(-1)
                        inner = torch.tensor([nparts, 1, 1, R_], dtype=F64)  # the row's own additions and its product
                        return dict(stats=Want(s, tol=(_cdiv(M1, 256) + 8 + inner + 1) * U * sabs))
                    slots = [padded(obs.reshape(-1)), padded(rew), padded(cont_row), padded(kl.reshape(-1)), padded(cont),
                             Out("stats", (8,), (slice(1, 5),))]
                    out.append(Case(R.STATS, f"M{M1}-p{nparts}-R{R_}{'-masked' if masked else ''}", [M1, R_, nparts],
                                    [], slots, ref))
    return out


# ----------------------------------------------------------------------------
# final: one thread
# ----------------------------------------------------------------------------
BETAS = (1.0, 0.5, 0.1)


def final_cases():
    out = []
    up = lambda x: float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(INF)))
    dn = lambda x: float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(-INF)))
    base = [40.0, 500.0, -30.0, 8.0, 60.0]
    table = [("open", base, 45, True), ("tie", base[:4] + [45.0], 45, True), ("tie-up", base[:4] + [up(45.0)], 45, True),
             ("tie-down", base[:4] + [dn(45.0)], 45, True), ("shut", base[:4] + [20.0], 45, True),
             # four ranks: the sums are global, rows_global = 4 x 45 is not this rank's row count
             ("global-rows", [160.0, 2100.0, -110.0, 30.0, 300.0], 180, True), ("global-tie", base[:4] + [180.0], 180, True),
             ("all-masked", [0.0, 0.0, 0.0, 0.0, 0.0], 45, True),
             ("all-masked-residue", [0.0, 1e-3, -2e-3, 5e-4, 0.0], 45, True),  # the 1e-5 alone is the denominator
             ("fraction-mask", [0.25, 3.0, -0.5, 0.1, 0.3], 45, True),
             ("no-skip-pointer", base, 45, False)]
    for i in range(5):
        for nm, bad in (("nan", NAN), ("inf", INF), ("-inf", -INF)):
            s = list(base)
            s[i] = bad
            table.append((f"{nm}-in-stats{i}", s, 45, True))
    for label, s5, rows, with_skip in table:
        st = torch.tensor(s5 + [NAN] * 3, dtype=F32)
        finite = all(math.isfinite(x) for x in s5)

        def ref(mut=None, st=st, rows=rows, finite=finite, with_skip=with_skip):
            r = R.final(st[:5], rows, BETAS, mut)
            s = f64(st)
            d = float(s[0]) + 1e-5
            # pred: two additions, the denominator's, the division; kl: the division; total: three products, two sums
            # (a non-finite sum: the non-finite losses compare as such, the finite ones keep their bounds)
            pabs = float(s[1].abs() + s[2].abs() + s[3].abs()) / abs(d)
            kl = float(r["losses"][2])
            tabs = BETAS[0] * pabs + (BETAS[1] + BETAS[2]) * max(1.0, kl)
            ltol = torch.tensor([4.5 * U * pabs * BETAS[0] + 6 * U * tabs, 4.5 * U * pabs, 1.5 * U * abs(kl), 1.5 * U * abs(kl)])
            w = dict(losses=Want(r["losses"], tol=torch.nan_to_num(ltol, nan=0.0, posinf=0.0)))
            sc = torch.cat([r["scal1"], r["scal2"]])
            # a NaN KL: the comparisons of the free-bit factor are all false on the device, torch propagates the NaN;
            # the step is skipped either way and the factors are only required to be written
            w["scal"] = Want(sc, tol=INF if math.isnan(kl) else 2.5 * U * sc.abs())
            if with_skip:
                w["skip"] = Want(torch.tensor([float(r["skip"])]), tol=0.0)
            return w
        slots = [st, Out("scal", (8,), (slice(1, 3),)), Out("losses", (6,), (slice(0, 4),)),
                 Out("skip", (2,), (slice(0, 1),), dtype="i32") if with_skip else None]
        out.append(Case(R.FINAL, label, [rows], list(BETAS), slots, ref))
    return out


# ----------------------------------------------------------------------------
# window scores: one wave per window, lane t over the steps (chain ceil(T1 / 64), tree depth 6)
# ----------------------------------------------------------------------------
def window_cases():
    out = []
    for B, T1 in ((1, 1), (4, 5), (5, 64), (3, 65), (2, 130)):
        g = gen(B * 131 + T1)
        R_, nparts = 3, 2
        obs, rew, cont_row, kl, cont = loss_rows(g, T1 * B, R_, nparts)
        if B > 1:  # a window that is masked throughout: denominator 1e-5
            cont.reshape(T1, B)[:, 1] = 0.0

        def ref(mut=None, a=(obs, rew, cont_row, kl, cont), B=B, T1=T1, R_=R_, nparts=nparts):
            s = R.window_scores(*a, B, BETAS)["scores"]
            t = R.stats_terms(a[0].abs(), a[1].abs(), a[2].abs(), a[3].abs(), a[4]).reshape(4, T1, B)
            den = f64(a[4]).reshape(T1, B).sum(0) + 1e-5
            c = _cdiv(T1, 64) + 6
            tol = (c + nparts + 6) * U * BETAS[0] * (t[0] + t[1] + t[2]).sum(0) / den \
                + (c + R_ + 4) * U * (BETAS[1] + BETAS[2]) * t[3].sum(0) / T1
            return dict(scores=Want(s, tol=tol))

        def chk(o, B=B):
            return ["a window masked throughout does not score exactly 0"] if B > 1 and float(o["scores"][1]) != 0.0 else []
        slots = [padded(obs.reshape(-1)), padded(rew), padded(cont_row), padded(kl.reshape(-1)), padded(cont),
                 Out("scores", (B + 4,), (slice(0, B),))]
        out.append(Case(R.WINDOW_SCORES, f"B{B}-T{T1}", [B, T1, R_, nparts], list(BETAS), slots, ref, [chk]))
    return out


# ----------------------------------------------------------------------------
# vec_mse: one wave per row (chain ceil(D / 64), tree depth 6)
# ----------------------------------------------------------------------------
def vec_mse_cases():
    out = []
    for D in (1, 63, 64, 65, 200):
        for M1 in (1, 5):
            g = gen(D * 3 + M1)
            mu, x, coef = randn(g, M1, D), randn(g, M1, D), torch.rand(M1, generator=g) * 0.1
            coef[0] = 0.0 if M1 > 1 else coef[0]

            def ref(mut=None, mu=mu, x=x, coef=coef, D=D):
                r = R.vec_mse(mu, x, coef)
                # part: the difference and the square (3 roundings), the chain, the tree; g: difference and product
                return dict(part=Want(r["part"], tol=(_cdiv(D, 64) + 6 + 3) * U * r["part"]),
                            g=Want(r["g"], tol=2.5 * U * (f64(coef).reshape(-1, 1) * (f64(mu).abs() + f64(x).abs()))))
            slots = [padded(mu.reshape(-1)), padded(x.reshape(-1)), padded(coef),
                     Out("g", (M1 + 4, D), (slice(0, M1), slice(None))), Out("part", (M1 + 4,), (slice(0, M1),))]
            out.append(Case(R.VEC_MSE, f"D{D}-M{M1}", [M1, D], [], slots, ref))
    return out


# ----------------------------------------------------------------------------
# GRU gates backward: one thread per element, 256-thread workgroups
# ----------------------------------------------------------------------------
def gru_cases():
    out = []
    for B, Hd in ((1, 1), (3, 85), (2, 128), (1, 257), (5, 600)):
        for with_h in (False, True):
            for acc in (0, 1):
                g = gen(B * 1000 + Hd + 2 * with_h + acc)
                sr, su = torch.sigmoid(randn(g, B, Hd, scale=2.0)), torch.sigmoid(randn(g, B, Hd, scale=2.0))
                sn, hn = torch.tanh(randn(g, B, Hd, scale=2.0)), randn(g, B, Hd)
                if Hd >= 8:  # saved gates exactly 0 and exactly 1, n = +-1
                    sr[0, 0], sr[0, 1], su[0, 2], su[0, 3], sn[0, 4], sn[0, 5] = 0.0, 1.0, 0.0, 1.0, 1.0, -1.0
                    sr[-1, -1], su[-1, -1], sn[-1, -1] = 1.0, 0.0, -1.0
                g_hp, h, prev = randn(g, B, Hd), randn(g, B, Hd), randn(g, B, Hd)
                ld = (Hd + 3, Hd + 5, Hd + 2)

                def ref(mut=None, a=(g_hp, h if with_h else None, sr, su, sn, hn, prev, acc)):
                    r = R.gru_bwd(*a, mut=mut)
                    # scale: |g_hp| times the sizes of what multiplies it (|h| + 1 into the update gate, |hn| + 1)
                    sc = f64(a[0]).abs().max(-1, keepdim=True).values * (1.0 + f64(a[5]).abs().max(-1, keepdim=True).values
                                                                        + (0 if a[1] is None else f64(a[1]).abs().max(-1, keepdim=True).values))
                    return dict(g_gi=Want(r["g_gi"], key="gru_bwd.g_gi", scale=sc), g_gh=Want(r["g_gh"], key="gru_bwd.g_gh", scale=sc),
                                # the direct path: one product, one addition
                                gh_out=Want(r["gh_out"], tol=2.5 * U * (f64(a[0]).abs() + (f64(a[6]).abs() if a[7] else 0))))
                slots = [padded(g_hp, ld[0]), padded(h, ld[1]) if with_h else None, padded(sr.reshape(-1)), padded(su.reshape(-1)),
                         padded(sn.reshape(-1)), padded(hn.reshape(-1)),
                         Out("g_gi", (B + 1, 3 * Hd), (slice(0, B), slice(None))), Out("g_gh", (B + 1, 3 * Hd), (slice(0, B), slice(None))),
                         Out("gh_out", (B + 1, ld[2]), (slice(0, B), slice(0, Hd)), init=prev)]
                out.append(Case(R.GRU_BWD, f"B{B}-H{Hd}-{'h' if with_h else 'noh'}-acc{acc}", [B, Hd, ld[0], ld[1], ld[2], acc],
                                [], slots, ref))
    return out


# ----------------------------------------------------------------------------
# LayerNorm + SiLU backward: one wave per row, registers for K <= 1024, streaming beyond
# ----------------------------------------------------------------------------
def ln_cases():
    out = []
    i = 0
    for K in (1, 63, 64, 65, 600, 1024, 1025, 1600):
        for M in (1, 4, 5):
            for with_gy, with_16 in (((True, True), (False, False)) if i % 2 else ((True, False), (False, True))):
                g = gen(K * 10 + M)
                pre, gx = randn(g, M, K, scale=1.5) + 0.3, randn(g, M, K)
                gamma, beta = 1.0 + 0.2 * randn(g, K), 0.1 * randn(g, K)
                if K > 2:
                    gamma[0], gamma[K // 2] = 0.0, 0.0
                if M >= 4:
                    pre[1] = 0.5                # a constant row: variance 0, rstd = 1 / sqrt(1e-5); sum and mean exact
                    pre[2, K // 3] = pre[2].abs().max() * 1e4  # one element 1e4 times the rest
                ld = (K + 3, K + 1, K + 2)

                def ref(mut=None, a=(gx, pre, gamma, beta)):
                    r = R.ln_silu_bwd(*a, mut=mut)
                    w = dict(g_pre=Want(r["g_pre"], key="ln_silu_bwd.g_pre", scale=_ln_scale(a, r)))
                    w["gy"] = Want(r["gy"], key="ln_silu_bwd.gy", scale=f64(a[0]).abs().max(-1, keepdim=True).values)
                    w["xhat"] = Want(r["xhat"], key="ln_silu_bwd.xhat")
                    return w

                def pick(mut=None, ref=ref, with_gy=with_gy):
                    w = ref(mut)
                    return w if with_gy else {"g_pre": w["g_pre"]}

                def chk(o, with_16=with_16):
                    if not with_16:
                        return []
                    want = R.bf16_rne(o["g_pre"])
                    got = o["g_pre16"].to(torch.int32) & 0xFFFF
                    return [] if torch.equal(want, got) else [f"g_pre16 is not the bf16 RNE of g_pre at {int((want != got).sum())} elements"]
                slots = [padded(gx, ld[0]), padded(pre, ld[1]), padded(gamma), padded(beta),
                         Out("g_pre", (M + 4, ld[2]), (slice(0, M), slice(0, K))),
                         Out("gy", (M + 4, ld[2]), (slice(0, M), slice(0, K))) if with_gy else None,
                         Out("xhat", (M + 4, ld[2]), (slice(0, M), slice(0, K))) if with_gy else None,
                         Out("g_pre16", (M + 4, ld[2]), (slice(0, M), slice(0, K)), dtype="u16") if with_16 else None]
                out.append(Case(R.LN_SILU_BWD, f"K{K}-M{M}-{'gy' if with_gy else 'nogy'}-{'bf16' if with_16 else 'f32'}",
                                [M, K, *ld], [], slots, pick, [chk]))
            i += 1
    return out


def _ln_scale(a, r):
    """g_pre = rstd (gxh - mean(gxh) - xhat mean(gxh xhat)): the size of its terms, rstd max |gy gamma| (1 + max xhat^2)."""
    gx, pre, gamma, beta = (f64(t) for t in a)
    var = pre.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    gxh = (r["gy"] * gamma).abs().max(-1, keepdim=True).values
    return rstd * gxh * (1.0 + (r["xhat"] ** 2).max(-1, keepdim=True).values)


# ----------------------------------------------------------------------------
# column sums: 16-column slabs, 64 row groups (chain ceil(M / 64), 8 rows unrolled), tree 8 + 8
# ----------------------------------------------------------------------------
CS_M = (1, 63, 64, 65, 511, 512, 513, 1030)
CS_N = (1, 15, 16, 17, 200)


def colsum_cases():
    out = []
    for M in CS_M:  # five jobs of different N in one launch, Y on every other one
        g = gen(M)
        v, slots, jobs = [M, len(CS_N), 0], [], []
        for j, N in enumerate(CS_N):
            X, Y = randn(g, M, N), randn(g, M, N) if (j + M) % 2 else None
            jobs.append((X, Y))
            v += [N, N + 3, N + 1]
            slots += [padded(X, N + 3), None if Y is None else padded(Y, N + 1), Out(f"out{j}", (N + 2,), (slice(0, N),))]

        def ref(mut=None, jobs=jobs, M=M):
            w = {}
            for j, (X, Y) in enumerate(jobs):
                r = R.colsum(X, Y)
                w[f"out{j}"] = Want(r["out"], tol=(_cdiv(M, 64) + 16 + 2) * U * r["abs"])
            return w
        out.append(Case(R.COLSUM_MULTI, f"M{M}-multi", v, [], slots, ref))
    for M, N, with_y in ((1, 1, False), (65, 17, True), (513, 16, False), (1030, 200, True)):  # out += (op_colsum)
        g = gen(M + N)
        X, Y, prev = randn(g, M, N), randn(g, M, N) if with_y else None, randn(g, N, scale=5.0)

        def ref(mut=None, X=X, Y=Y, prev=prev, M=M):
            r = R.colsum(X, Y, prev)
            return dict(out0=Want(r["out"], tol=(_cdiv(M, 64) + 16 + 3) * U * (r["abs"] + f64(prev).abs())))
        slots = [padded(X, N + 3), None if Y is None else padded(Y, N + 1), Out("out0", (N + 2,), (slice(0, N),), init=prev)]
        out.append(Case(R.COLSUM_MULTI, f"M{M}-N{N}-accumulate", [M, 1, 1, N, N + 3, N + 1], [], slots, ref))
    return out


def all_cases():
    klf, klb = kl_cases()
    add, plain = ste_cases()
    return (gather_cases() + prep_cases() + klf + heads_cases() + stats_cases() + final_cases() + klb + add
            + vec_mse_cases() + window_cases() + gru_cases() + ln_cases() + plain + colsum_cases())


_CACHE = {}


def cases_by_op():
    """{op name: [Case]} (built once: the references are computed once per session and shared)."""
    if not _CACHE:
        for c in all_cases():
            _CACHE.setdefault(c.name, []).append(c)
    return _CACHE


# ----------------------------------------------------------------------------
# the comparison both test files use
# ----------------------------------------------------------------------------
def compare(case, bufs, wants=None, report=None):
    """bufs: {output name: the whole buffer after the call}.  Returns the failures: an element outside the region or
    unwritten inside it that is no longer POISON, a written element that still is, a value off its reference by more
    than its tolerance (no element left out), a failed exactness check.  report(key, kind, x): kind "measured": the
    largest error of the output in units of 2^-24 x scale; "derived": as a fraction of its derived bound."""
    fails = []
    wants = case.wants() if wants is None else wants
    region = {}
    for o in case.outs():
        b = bufs[o.name]
        keep = torch.ones(o.shape, dtype=torch.bool)
        keep[o.region] = False
        if not bool(is_poison(b)[keep].all()):
            fails.append(f"{o.name}: {int((~is_poison(b)[keep]).sum())} elements outside the output changed")
        r = b[o.region]
        region[o.name] = r
        if o.name not in wants:
            if o.name == "g_pre16":
                if bool(is_poison(r).any()):
                    fails.append("g_pre16: unwritten elements")
                continue
            if not bool(is_poison(r).all()):  # an output this call must not write (the unused outputs of a mode)
                fails.append(f"{o.name}: written, and must not be")
            continue
        w = wants[o.name]
        if o.init is None and bool(is_poison(r).any()):
            fails.append(f"{o.name}: {int(is_poison(r).sum())} unwritten elements")
            continue
        got = r.to(F64)
        ref = w.ref.reshape(got.shape)
        tol = w.tol.reshape(got.shape)
        assert not bool(torch.isnan(tol).any()), (case, o.name)
        both_nan = torch.isnan(ref) & torch.isnan(got)
        same_inf = torch.isinf(ref) & (ref == got)
        err = torch.where(both_nan | same_inf, torch.zeros_like(got), (got - ref).abs())
        if w.nan_ok is not None:
            err = torch.where(w.nan_ok.reshape(got.shape) & torch.isnan(got), torch.zeros_like(err), err)
        bad = ~(err <= tol)  # a NaN where none belongs fails
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{o.name}: {int(bad.sum())} of {bad.numel()} beyond tolerance, first at {i}: got "
                         f"{float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} tol {float(tol.reshape(-1)[i]):.3e}")
        if report and w.key:
            sc = w.scale.reshape(got.shape)
            ok = (sc > 0) & torch.isfinite(err)
            units = float((err[ok] / (U * sc[ok])).max()) if bool(ok.any()) else 0.0
            report(w.key, "measured", units)
        elif report:  # a derived bound: the largest error as a fraction of it (0 where the bound is 0: exact)
            ok = (tol > 0) & torch.isfinite(tol) & torch.isfinite(err)
            report(f"{case.name}.{o.name}", "derived", float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0)
    for chk in case.checks:
        fails += chk(region)
    return fails
