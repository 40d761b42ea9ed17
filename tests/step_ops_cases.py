"""The inputs, expected outputs and tolerances of tests/test_gpu_step_ops.py, shared with tests/test_step_ops_host.py
(which checks, without a GPU, that these very inputs tell every mutation of step_ops_ref.MUTATIONS from the reference).

A Case is one call of dr_internal_step_run, built like the cases of wm_loss_cases.py (whose Out, Want, Case, padded,
poison and row_scale it reuses): inputs carry NaN in their padding columns and a guard row, outputs are POISON-filled,
and every leading dimension is wider than the logical width in at least one case per op.  Besides: a `refuse` case
must come back DR_E_INVALID with a message and every output still POISON; `twin` = (key, rows): the first `rows` rows
of every output have the same bits in all cases of one key (a row's result must not depend on the tile it lands in,
g_heads not on N); the outputs named in `given` are exact functions of the device's own other outputs (hout16 of
hout, the sampler's z of its soft) and are compared by the case's checks, their Want serving the host test.

Tolerances.  Exact outputs: tol 0.  Sums: a derived bound (chain + tree + c) 2^-24 sum|terms|, the chain read from the
launcher's geometry (module doc of test_gpu_step_ops.py); the split GRU's hidden product: gemm_ref.f32_bound, the bound
the GEMM route tests hold that route to.  Outputs that go through expf / tanhf / log1pf: 4 x MEASURED[key] x 2^-24 x
scale, MEASURED being the largest error of that output over all its cases on the first MI355X run
(profiles/step_ops_errors.txt), with the scale per op:
  gru, gru_fwd   r, u: max(1, S) of their gate, S = sum|terms| of the pre-activation (gi and gh with their biases);
                 n: max(1, S_n); h' = (h - n) u + n: (|h| + 1) max(1, S_u) + max(1, S_n)
  sample         soft: p (1 + |x - max x|) (the subtraction's rounding scales with the distance from the maximum)
  actor_head     sigma: its own size; a: 1 + |mu| + |eps sigma|
  actor_head_bwd_x   g_heads: |g_mu_l| + |g_a| for g_mu, |g_sig_l| + |g_a eps| for g_ls (0 outside the clamp: exact)
  sigmoid        its own size, and not below 2^-102 (bound x 2^-126: 1 / (1 + expf(100)) is 1 / inf = 0 in float32
                 where float64 has 3.7e-44, below float32's normal range)"""
import math
import os

import torch

import gemm_ref
import step_ops_ref as R
import wm_loss_cases as W
from wm_loss_cases import Out, gen, is_poison, padded, poison, pow2_ge, quant, randn, row_scale  # noqa: F401

U = R.U
F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
f64 = R.f64
DR_E_INVALID = 1001  # include/dreamer_hip.h

# largest |got - ref| / (2^-24 scale) per output over every case of its op, first MI355X run
# (profiles/step_ops_errors.txt); the asserted bound is 4 x this
MEASURED = {
    "gru.h": 0.529,
    "gru.n": 1.164,
    "gru.r": 0.846,
    "gru.u": 0.907,
    "gru_fwd.h": 0.601,
    "gru_fwd.n": 1.614,
    "gru_fwd.r": 1.089,
    "gru_fwd.u": 0.996,
    "sample.soft": 2.111,
    "actor_head.a": 0.761,
    "actor_head.sigma": 2.658,
    "actor_head_bwd_x.g_heads": 1.550,
    "sigmoid.out": 1.793,
}
MEASURING = bool(os.environ.get("STEP_OPS_ERRORS"))


def bound(key):
    """Asserted units of 2^-24 x scale for a measured output (open only while the table is being measured)."""
    if key not in MEASURED and MEASURING:
        return 2.0 ** 100
    return 4.0 * MEASURED[key]


class Want(W.Want):
    @property
    def tol(self):
        return self._tol if self._tol is not None else bound(self.key) * U * self.scale


class Shift:
    """A slot handed to the hook `off` floats into its buffer (a pointer that is not 16-byte aligned)."""

    def __init__(self, slot, off=1):
        self.slot, self.off = slot, off


class Case(W.Case):
    def __init__(self, op, label, v, num, slots, ref, checks=(), refuse=None, twin=None, given=()):
        super().__init__(op, label, v, num, slots, ref, checks)
        self.refuse, self.twin, self.given = refuse, twin, tuple(given)

    @property
    def name(self):
        return R.OP_NAMES[self.op]

    def outs(self):
        s = [x.slot if isinstance(x, Shift) else x for x in self.slots]
        return [x for x in s if isinstance(x, Out)]


def _cdiv(a, b):
    return -(-a // b)


def _clean(x):
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == F32 else t


def _f32(x):
    return float(torch.tensor(x, dtype=F32))


def nextf(x, up):
    return float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(INF if up else -INF, dtype=F32)))


# ----------------------------------------------------------------------------
# latent rows
# ----------------------------------------------------------------------------
def latent(g, B, R_, C, dense="none", zero=False):
    """[B][R][C]: per group one class at the sampler's straight-through value (1 + pu) - pu (off 1 by an ulp or not
    at all), negative in some groups, no class at all in others; dense groups (two classes, or all of them) where
    `dense` says: "one" the last group of every other row, "several" every third group, "all" every group."""
    z = torch.zeros(B, R_, C)
    if zero:
        return z
    k = torch.randint(0, C, (B, R_), generator=g)
    pu = torch.rand(B, R_, generator=g) * 0.98 + 0.01
    val = (1.0 + pu) - pu
    soft = torch.rand(B, R_, C, generator=g) + 0.05
    for b in range(B):
        for u in range(R_):
            is_dense = C >= 2 and (dense == "all" or (dense == "several" and u % 3 == 0) or
                                   (dense == "one" and u == R_ - 1 and b % 2 == 0))
            if is_dense:
                if (b + u) % 2:
                    z[b, u] = soft[b, u] / soft[b, u].sum()
                else:
                    z[b, u, int(k[b, u])] = soft[b, u, 0]
                    z[b, u, (int(k[b, u]) + 1) % C] = -soft[b, u, 1]
            elif (b + u) % 11 == 5:
                pass  # no class
            else:
                z[b, u, int(k[b, u])] = -val[b, u] if (b + u) % 7 == 3 else val[b, u]
    return z


def index_of(z):
    idx, zval = R.onehot_index(z)
    return idx.to(torch.int32).contiguous(), zval.contiguous()


# ----------------------------------------------------------------------------
# gru: k_gru_fused (16 rows x 16 units per workgroup) and, with gh_ws at B >= 128, GEMM + k_gru_gates (8 x 32)
# ----------------------------------------------------------------------------
GRU_CFG = {  # Hd -> A, (R, C), h given, saves, hout16 (the same at every B: B = 17 / 33 and 129 / 136 are twins)
    4: (1, (4, 3), True, True, True), 20: (3, (12, 8), False, False, False), 36: (8, (32, 33), True, True, False),
    64: (3, (4, 3), True, False, True), 100: (8, (12, 8), False, True, True), 644: (1, (4, 3), True, True, True),
    268: (3, (4, 3), True, True, False),
}
SPLIT_CFG = {32: (1, (4, 3), True, True, True), 36: (3, (12, 8), False, False, False), 100: (8, (32, 33), True, True, False)}
GRU_FUSED_B = (1, 15, 16, 17, 33)
GRU_FUSED_HD = (4, 20, 36, 64, 100)
GRU_SPLIT_B = (128, 129, 135, 136)
GRU_SPLIT_HD = (32, 36, 100)


def gru_tiles(B, Hd, split):
    return _cdiv(Hd, 32) * _cdiv(B, 8) if split else _cdiv(Hd, 16) * _cdiv(B, 16)


def gru_case(label, B, Hd, A, RC, h_on, saves, h16, ws=False, ready=0, dense="none", special=None, z_given=None,
             Bgen=None, seed=None, twin=None, refuse=None, ldh_add=4):
    R_, C = RC
    L = R_ * C
    Bgen = max(B, Bgen or B)
    g = gen(1000 + Hd if seed is None else seed)
    z = latent(g, Bgen, R_, C, dense)[:B].contiguous()
    a = randn(g, Bgen, A)[:B].contiguous()
    h = randn(g, Bgen, Hd)[:B].contiguous()
    wt, b_ih = randn(g, L + A, 3 * Hd, scale=0.5), randn(g, 3 * Hd, scale=0.3)
    w_hh, b_hh = randn(g, 3 * Hd, Hd, scale=1.0 / math.sqrt(Hd)), randn(g, 3 * Hd, scale=0.3)
    if special == "gates":  # pre-activations forced through b_ih, the unit's weights and b_hh zeroed
        for t, j, x in ((1, 0, -100.0), (1, 1, 100.0), (1, 2, 30.0), (2, 3, 30.0), (2, 4, -100.0), (0, 5, -100.0),
                        (0, 6, 100.0)):
            c = t * Hd + j
            wt[:, c], w_hh[c], b_hh[c], b_ih[c] = 0.0, 0.0, 0.0, x
    if special == "nan":
        h[2, 5] = NAN
    idx, zval = index_of(z)
    any_dense = bool((idx < 0).any())
    if z_given is None:
        z_given = any_dense or Hd % 8 == 4
    assert z_given or not any_dense  # idx = -1 with a NULL z would be an out-of-bounds read, not a test
    split = ws and B >= 128
    ldz, lda, ldh, ldo = L + 3, A + 1, Hd + ldh_add, Hd + 8
    hh = h if h_on else None

    def ref(mut=None):
        r = R.gru(z, a, hh, wt, b_ih, w_hh, b_hh, mut)
        one = torch.ones_like(r["abs_r"])
        s_r, s_u, s_n = (torch.maximum(one, _clean(r[k])) for k in ("abs_r", "abs_u", "abs_n"))
        nanrow = torch.isnan(r["hout"])
        w = dict(hout=Want(r["hout"], key="gru.h", scale=torch.where(nanrow, 0 * one, (_clean(r["habs"]) + 1) * s_u + s_n)))
        if h16:
            w["hout16"] = Want(R.bf16_bits(_clean(r["hout"]).float(), mut), tol=0.0)
        if saves:
            if hh is None:
                tghn = 0.0 * one  # b_hh itself
            elif split:
                tghn = gemm_ref.f32_bound(Hd, _clean(r["abs_ghn"]), _clean(r["sghn"]))
            else:  # a wave's chain of kw products, three additions of the four waves' partial sums, the bias
                tghn = (_cdiv(Hd, 64) * 16 + 4 + 2) * U * _clean(r["abs_ghn"])
            w.update(sr=Want(r["sr"], key="gru.r", scale=torch.where(nanrow, 0 * one, s_r)),
                     su=Want(r["su"], key="gru.u", scale=torch.where(nanrow, 0 * one, s_u)),
                     sn=Want(r["sn"], key="gru.n", scale=torch.where(nanrow, 0 * one, s_n)),
                     sghn=Want(r["sghn"], tol=tghn))
        if split and hh is not None and not ready:
            w["gh_ws"] = Want(r["gh"].reshape(-1), tol=gemm_ref.f32_bound(Hd, _clean(r["gh_abs"]), _clean(r["gh"])).reshape(-1))
        return w

    def chk(o):
        f = []
        ho = o["hout"]
        if h16:
            ok = ~torch.isnan(ho)
            got = o["hout16"].to(torch.int32) & 0xFFFF
            if not torch.equal(got[ok], R.bf16_bits(ho.contiguous())[ok]):
                f.append("hout16 is not the bf16 round-to-nearest-even of hout")
        if special == "nan":
            nan = torch.isnan(ho)
            if not bool(nan[2].all()) or bool(nan[torch.arange(B) != 2].any()):
                f.append("a NaN in row 2 of h: row 2 of h' must be NaN and no other row")
        if special == "gates":
            n, u, r = o["sn"], o["su"], o["sr"]
            hv = h if h_on else torch.zeros(B, Hd)
            claims = (("u at -100 is 0", bool((u[:, 0] == 0).all())), ("h' at u = 0 is n", torch.equal(_bits(ho[:, 0]), _bits(n[:, 0]))),
                      ("u at +100 is 1", bool((u[:, 1] == 1).all())), ("u at +30 is 1", bool((u[:, 2] == 1).all())),
                      ("h' at u = 1 is (h - n) + n", torch.equal(_bits(ho[:, 1:3]), _bits((hv[:, 1:3] - n[:, 1:3]) + n[:, 1:3]))),
                      ("n at +30 is 1", bool((n[:, 3] == 1).all())), ("n at -100 is -1", bool((n[:, 4] == -1).all())),
                      ("r at -100 is 0", bool((r[:, 5] == 0).all())), ("r at +100 is 1", bool((r[:, 6] == 1).all())))
            f += [f"saturated gate: {c} does not hold exactly" for c, ok in claims if not ok]
        return f
    v = [B, Hd, R_, C, A, ldz, lda, ldh, ldo, ready]
    sv = lambda n: Out(n, (B + 1, Hd), (slice(0, B), slice(None))) if saves else None  # noqa: E731
    slots = [idx.reshape(-1), zval.reshape(-1), padded(z.reshape(B, L), ldz) if z_given else None, padded(a, lda),
             padded(h, ldh) if h_on else None, wt.reshape(-1), b_ih, w_hh.reshape(-1), b_hh,
             Out("hout", (B + 1, ldo), (slice(0, B), slice(0, Hd))),
             Out("hout16", (B + 1, ldo), (slice(0, B), slice(0, Hd)), dtype="u16") if h16 else None,
             sv("sr"), sv("su"), sv("sn"), sv("sghn"),
             Out("gh_ws", (B * 3 * Hd + 4,), (slice(0, B * 3 * Hd),)) if ws else None]
    return Case(R.GRU, label, v, [], slots, ref, [chk], refuse=refuse, twin=twin, given=("hout16",))


def gru_cases():
    out = []
    for Hd in GRU_FUSED_HD:
        A, RC, h_on, saves, h16 = GRU_CFG[Hd]
        for B in GRU_FUSED_B:
            hb = h_on if B >= 16 else not h_on  # h NULL and non-NULL at every Hd
            out.append(gru_case(f"fused-B{B}-Hd{Hd}", B, Hd, A, RC, hb, saves, h16, Bgen=33,
                                twin=(f"fused-Hd{Hd}", 17) if B in (17, 33) else None))
    for B, Hd in ((1, 644), (17, 644), (3, 268)):  # kw = 176 > 160: a second GRU_PRE round; 17 x 1 tiles
        A, RC, h_on, saves, h16 = GRU_CFG[Hd]
        out.append(gru_case(f"fused-B{B}-Hd{Hd}", B, Hd, A, RC, h_on, saves, h16))
    A, RC, h_on, saves, h16 = GRU_CFG[36]
    out.append(gru_case("fused-B130-no-ws", 130, 36, A, RC, h_on, saves, h16, Bgen=136, seed=2036))
    out.append(gru_case("fused-B127-ws", 127, 36, A, RC, h_on, saves, h16, ws=True, Bgen=136, seed=2036))
    for Hd in GRU_SPLIT_HD:
        A, RC, h_on, saves, h16 = SPLIT_CFG[Hd]
        for B in GRU_SPLIT_B:
            out.append(gru_case(f"split-B{B}-Hd{Hd}", B, Hd, A, RC, h_on, saves, h16, ws=True, Bgen=136, seed=2000 + Hd,
                                twin=(f"split-Hd{Hd}", 129) if B in (129, 136) else None))
    for form, B, ws in (("fused", 17, False), ("split", 129, True)):
        for dense in ("one", "several", "all"):
            out.append(gru_case(f"{form}-dense-{dense}", B, 36, 3, (12, 8), True, True, True, ws=ws, dense=dense, seed=77))
        out.append(gru_case(f"{form}-gates", B, 36, 3, (4, 3), True, True, True, ws=ws, special="gates", seed=78))
        out.append(gru_case(f"{form}-gates-h-null", B, 36, 3, (4, 3), False, True, False, ws=ws, special="gates", seed=79))
        out.append(gru_case(f"{form}-nan-row", B, 36, 1, (4, 3), True, True, True, ws=ws, special="nan", seed=80))
    # refusals (op_gru_fused's documented limits)
    out.append(gru_case("refuse-R3", 5, 36, 1, (3, 4), True, True, True, refuse="R % 4"))
    out.append(gru_case("refuse-Hd6", 5, 6, 1, (4, 3), True, True, True, refuse="Hd % 4", ldh_add=2))
    out.append(gru_case("refuse-A9", 5, 36, 9, (4, 3), True, True, True, refuse="A <= 8"))
    out.append(gru_case("refuse-ldh", 5, 36, 1, (4, 3), True, True, True, refuse="aligned", ldh_add=3))
    return out


def with_ready(case, gh_ws):
    """The same call with gh_ready = 1 on the gh_ws (the whole buffer) a gh_ready = 0 call left."""
    v = list(case.v)
    v[9] = 1
    slots = list(case.slots)
    slots[15] = gh_ws
    return Case(case.op, case.label + "-ready", v, case.num, slots, case.ref, case.checks, given=case.given)


# ----------------------------------------------------------------------------
# onehot_index: a thread per (row, group), 256-thread workgroups
# ----------------------------------------------------------------------------
ONEHOT_MR = ((1, 4), (15, 17), (16, 16), (257, 1))
ONEHOT_C = (1, 3, 32, 33)


def onehot_cases():
    out = []
    for M, R_ in ONEHOT_MR:
        for C in ONEHOT_C:
            g = gen(M + C)
            z = torch.zeros(M, R_, C)
            kind = torch.randint(0, 8, (M, R_), generator=g)
            k = torch.randint(0, C, (M, R_), generator=g)
            for m in range(M):
                for u in range(R_):
                    t, c = int(kind[m, u]) if M * R_ > 8 else (m * R_ + u) % 8, int(k[m, u])
                    if t == 1:
                        z[m, u, c] = 1.0
                    elif t == 2:
                        z[m, u, c] = _f32(1.0 + 2.0 ** -23)
                    elif t == 3:
                        z[m, u, c] = -0.75
                    elif t == 4:
                        z[m, u, c] = NAN
                    elif t == 5:  # two or more (C = 1: one)
                        z[m, u, c], z[m, u, (c + 1) % C] = 0.25, 0.5
                    elif t == 6:  # -0.0 counts as zero
                        z[m, u, c] = -0.0
                    elif t == 7:  # one class beside a -0.0
                        z[m, u, c], z[m, u, (c + 1) % C] = -0.0, 2.0
            L, ldz = R_ * C, R_ * C + 5

            def ref(mut=None, z=z):
                idx, zval = R.onehot_index(z)
                return dict(idx=Want(idx.reshape(-1), tol=0.0), zval=Want(zval.reshape(-1), tol=0.0))
            slots = [padded(z.reshape(M, L), ldz), Out("idx", (M * R_ + 3,), (slice(0, M * R_),), dtype="i32"),
                     Out("zval", (M * R_ + 3,), (slice(0, M * R_),))]
            out.append(Case(R.ONEHOT_INDEX, f"M{M}-R{R_}-C{C}", [M, R_, C, ldz], [], slots, ref))
    z = torch.zeros(2, 4, 3)
    out.append(Case(R.ONEHOT_INDEX, "refuse-C0", [2, 4, 0, 12], [],
                    [padded(z.reshape(2, 12)), Out("idx", (11,), dtype="i32"), Out("zval", (11,))], None, refuse="C >= 1"))
    return out


# ----------------------------------------------------------------------------
# zgather_add: 4 rows x (64 threads x 4 columns) per workgroup
# ----------------------------------------------------------------------------
ZG_M = (1, 3, 4, 5, 9)
ZG_N = (4, 252, 256, 260, 516)
ZG_RC = ((4, 3), (12, 8), (32, 33))


def zg_case(label, M, N, RC, dense="none", zero=False, refuse=None, ld_add=(4, 8, 4), shift=None, seed=0):
    R_, C = RC
    L = R_ * C
    g = gen(3000 + seed + M * 7 + N)
    z = latent(g, M, R_, C, dense, zero=zero)
    idx, zval = index_of(z)
    ldz, ldw, ldb, ldo = L + 3, N + ld_add[0], N + ld_add[1], N + ld_add[2]
    wt, base = randn(g, L, N, scale=0.5), randn(g, M, N)
    nd = int((idx < 0).sum(-1).max())

    def ref(mut=None):
        r = R.zgather_add(z, wt, base, mut)
        # R gathered products (+ C per dense group) in one fma chain, then base + v
        return dict(out=Want(r["out"], tol=(R_ + nd * C + 2) * U * (r["abs"] + f64(base).abs())))

    def chk(o):
        if zero and not torch.equal(_bits(o["out"]), _bits(base)):
            return ["all zval 0: out is not base bit for bit"]
        return []
    sh = lambda name, s: Shift(s) if shift == name else s  # noqa: E731
    slots = [idx.reshape(-1), zval.reshape(-1), padded(z.reshape(M, L), ldz), sh("wt", padded(wt, ldw)),
             sh("base", padded(base, ldb)), sh("out", Out("out", (M + 1, ldo), (slice(0, M), slice(0, N))))]
    return Case(R.ZGATHER_ADD, label, [M, N, R_, C, ldz, ldw, ldb, ldo], [], slots, ref, [chk], refuse=refuse)


def zgather_cases():
    out = []
    for i, M in enumerate(ZG_M):
        for j, N in enumerate(ZG_N):
            RC = ZG_RC[(i + j) % 3]
            dense = ("none", "one", "several", "all")[(i + 2 * j) % 4]
            out.append(zg_case(f"M{M}-N{N}-R{RC[0]}-{dense}", M, N, RC, dense))
    out.append(zg_case("M5-N260-all-zero", 5, 260, (12, 8), zero=True))
    out.append(zg_case("refuse-N6", 3, 6, (4, 3), refuse="zgather_add"))
    out.append(zg_case("refuse-ldw", 3, 8, (4, 3), refuse="zgather_add", ld_add=(2, 8, 4)))
    out.append(zg_case("refuse-ldb", 3, 8, (4, 3), refuse="zgather_add", ld_add=(4, 6, 4)))
    out.append(zg_case("refuse-ldo", 3, 8, (4, 3), refuse="zgather_add", ld_add=(4, 8, 5)))
    out.append(zg_case("refuse-R33", 3, 8, (33, 2), refuse="zgather_add"))
    for name in ("wt", "base", "out"):
        out.append(zg_case(f"refuse-misaligned-{name}", 3, 8, (4, 3), refuse="zgather_add", shift=name))
    return out


# ----------------------------------------------------------------------------
# gru_fwd: a thread per element
# ----------------------------------------------------------------------------
GRU_FWD_BH = ((1, 1), (3, 85), (2, 128), (1, 257), (5, 200))


def gru_fwd_cases():
    out = []
    for B, Hd in GRU_FWD_BH:
        for h_on in (True, False):
            for saves in (True, False):
                g = gen(B * Hd + h_on + 2 * saves)
                gi, gh, h = randn(g, B, 3 * Hd, scale=2.0), randn(g, B, 3 * Hd, scale=2.0), randn(g, B, Hd)
                ldh, ldo = Hd + 3, Hd + 2

                def ref(mut=None, gi=gi, gh=gh, h=h, h_on=h_on, saves=saves):
                    r = R.gru_gates(f64(gi), f64(gh), f64(h) if h_on else None, mut, f64(gi).abs(), f64(gh).abs())
                    one = torch.ones_like(r["abs_r"])
                    s_r, s_u, s_n = (torch.maximum(one, r[k]) for k in ("abs_r", "abs_u", "abs_n"))
                    w = dict(hout=Want(r["hout"], key="gru_fwd.h", scale=(r["habs"] + 1) * s_u + s_n))
                    if saves:
                        w.update(sr=Want(r["sr"], key="gru_fwd.r", scale=s_r), su=Want(r["su"], key="gru_fwd.u", scale=s_u),
                                 sn=Want(r["sn"], key="gru_fwd.n", scale=s_n), sghn=Want(r["sghn"], tol=0.0))
                    return w
                sv = lambda n, B=B, Hd=Hd, saves=saves: Out(n, (B + 1, Hd), (slice(0, B), slice(None))) if saves else None  # noqa: E731
                slots = [padded(gi), padded(gh), padded(h, ldh) if h_on else None,
                         Out("hout", (B + 1, ldo), (slice(0, B), slice(0, Hd))), sv("sr"), sv("su"), sv("sn"), sv("sghn")]
                out.append(Case(R.GRU_FWD, f"B{B}-Hd{Hd}-h{int(h_on)}-s{int(saves)}", [B, Hd, ldh, ldo], [], slots, ref))
    return out


# ----------------------------------------------------------------------------
# sample: a latent group on W = pow2 >= C lanes, 256 / W groups per workgroup
# ----------------------------------------------------------------------------
SAMPLE_C = (1, 2, 3, 5, 31, 33, 63, 64)
MARGIN = 1e-5      # a group whose best and second-best score are relatively closer is left out of the idx comparison
MAX_LEFT_OUT = 0.01


def sample_case(M, R_, C, step, with_idx, with_soft, seed, refuse=None):
    g = gen(seed)
    L, G = R_ * max(C, 1), M * R_
    Cc = max(C, 1)
    logits = quant(randn(g, M, R_, Cc, scale=2.0))
    if G >= 2:  # group 0 = group 1 + 1e4: the same distribution
        logits.view(G, Cc)[0] = logits.view(G, Cc)[1] + 1e4
    if G >= 3 and Cc >= 2:  # all but one class at -inf
        keep = float(logits.view(G, Cc)[2, Cc // 2])
        logits.view(G, Cc)[2] = -INF
        logits.view(G, Cc)[2, Cc // 2] = keep
    steps = step + 1
    q = torch.rand(steps, G, Cc, generator=g) * 0.95 + 0.05
    ldl, ldz, lds = L + 1, L + 2, L + 3
    memo = {}

    def base():
        if "r" not in memo:
            memo["r"] = R.sample(logits, q, step)
        return memo["r"]

    def ref(mut=None):
        r = R.sample(logits, q, step, mut) if mut else base()
        x = f64(logits)
        d = _clean((x - x.max(-1, keepdim=True).values).abs())
        close = base()["margin"] < MARGIN
        p32 = r["p"].float()
        val = (1.0 + p32) - p32 if mut == "sample_no_unimix" else R.ste_value(p32, Cc)
        zref = torch.nn.functional.one_hot(r["win"], Cc).to(F32) * val
        w = dict(z=Want(zref.reshape(M, L), tol=0.0))
        if with_soft:
            w["soft"] = Want(r["p"].reshape(M, L), key="sample.soft", scale=(r["p"] * (1 + d) + 1e-30).reshape(M, L))
        if with_idx:
            w["idx"] = Want(r["win"].reshape(-1), tol=torch.where(close, float(Cc), 0.0).reshape(-1))
        return w

    def chk(o):
        f, r = [], base()
        sure = (r["margin"] >= MARGIN).reshape(-1)
        hot = torch.nn.functional.one_hot(r["win"], Cc).bool().reshape(G, Cc)
        z = o["z"].reshape(G, Cc)
        if bool((z[sure][~hot[sure]] != 0).any()):
            f.append("z is not exactly 0 off the winner")
        zw = z[hot]
        if with_soft:
            want = R.ste_value(o["soft"].reshape(G, Cc), Cc)[hot]
            if not torch.equal(_bits(zw[sure]), _bits(want[sure])):
                f.append("z at the winner is not (1 + pu) - pu of the device's own soft")
            s = o["soft"].reshape(G, Cc)
            if G >= 2 and not torch.equal(_bits(s[0]), _bits(s[1])):
                f.append("soft changes under a constant offset of 1e4")
            if G >= 3 and Cc >= 2 and not torch.equal(s[2], torch.nn.functional.one_hot(torch.tensor(Cc // 2), Cc).to(F32)):
                f.append("-inf on all but one class: soft is not exactly one-hot")
        elif bool(((zw[sure].double() - 1.0).abs() > 2.0 ** -23).any()):
            f.append("z at the winner is not within 2^-23 of 1")
        return f
    if refuse is None:
        left = float((base()["margin"] < MARGIN).double().mean())
        assert left <= MAX_LEFT_OUT, (M, R_, C, left)
    slots = [padded(logits.reshape(M, L), ldl), q.reshape(-1), Out("z", (M + 1, ldz), (slice(0, M), slice(0, L))),
             Out("idx", (G + 2,), (slice(0, G),), dtype="i32") if with_idx else None,
             Out("soft", (M + 1, lds), (slice(0, M), slice(0, L))) if with_soft else None]
    lab = f"M{M}-R{R_}-C{C}-step{step}" + ("" if with_idx else "-noidx") + ("" if with_soft else "-nosoft")
    return Case(R.SAMPLE, ("refuse-" if refuse else "") + lab, [M, R_, C, ldl, ldz, lds, step], [], slots, ref, [chk],
                refuse=refuse, given=("z",))


def sample_cases():
    out = []
    for i, C in enumerate(SAMPLE_C):
        W_ = pow2_ge(C)
        per = 256 // W_  # groups per workgroup: M R W on both sides of 256
        for G in sorted({max(1, per - 1), per, per + 1}):
            out.append(sample_case(G, 1, C, 0, True, True, 10 * C + G))
        out.append(sample_case(5, 3, C, 2, i % 2 == 0, i % 4 < 2, 500 + C))
        out.append(sample_case(3, 4, C, 2 * (i % 2), i % 2 == 1, i % 4 >= 2, 600 + C))
    out.append(sample_case(2, 3, 0, 0, True, True, 1, refuse="[1,64]"))
    out.append(sample_case(2, 3, 65, 0, True, True, 2, refuse="[1,64]"))
    return out


# ----------------------------------------------------------------------------
# actor_head: a thread per (row, action)
# ----------------------------------------------------------------------------
LS_EDGES = (-5.0, nextf(-5.0, False), nextf(-5.0, True), 2.0, nextf(2.0, False), nextf(2.0, True), INF, -INF, 0.0)
HEAD_MA = ((1, 1), (255, 1), (256, 1), (257, 1), (85, 3), (86, 3), (32, 8), (33, 8), (2, 3))


def actor_head_cases():
    out = []
    n = 0
    for M, A in HEAD_MA:
        for det in (0, 1):
            g = gen(M * A + det)
            step = n % 2
            mu, ls, eps = randn(g, M, A, scale=1.5), randn(g, M, A, scale=2.0), randn(g, step + 1, M, A)
            for i, e in enumerate(LS_EDGES):
                if i < M * A:
                    ls.view(-1)[i] = e
            if M * A >= 12:  # mu + eps sigma = +-20: tanh saturates to exactly +-1
                mu.view(-1)[10], mu.view(-1)[11] = 20.0, -20.0
                eps[:, :, :].view(step + 1, -1)[:, 10:12] = 0.0
            null = (None, "a", "mu", "sigma", "eps_save")[n % 5]
            n += 1
            ldm, ldl, lda, ldmu, lds = A + 1, A + 2, A + 3, A + 1, A + 2

            def ref(mut=None, mu=mu, ls=ls, eps=eps, det=det, step=step, null=null):
                r = R.actor_head(mu, ls, eps[step], det, mut)
                w = dict(a=Want(r["a"], key="actor_head.a", scale=1.0 + r["pre_abs"]), mu=Want(r["mu"], tol=0.0),
                         sigma=Want(r["sigma"], key="actor_head.sigma", scale=r["sigma"].abs()))
                if not det:
                    w["eps_save"] = Want(eps[step].reshape(-1), tol=0.0)
                w.pop(null, None)
                return w

            def chk(o, M=M, A=A, det=det):
                if "a" in o and M * A >= 12:
                    av = o["a"].reshape(-1)
                    if float(av[10]) != 1.0 or float(av[11]) != -1.0:
                        return ["tanh at +-20 is not exactly +-1"]
                return []
            o2 = lambda name, ld, M=M, A=A, null=null: None if null == name else Out(name, (M + 1, ld), (slice(0, M), slice(0, A)))  # noqa: E731
            slots = [padded(mu, ldm), padded(ls, ldl), None if det and n % 3 == 0 else eps.reshape(-1), o2("a", lda),
                     o2("mu", ldmu), o2("sigma", lds),
                     None if null == "eps_save" else Out("eps_save", (M * A + 1,), (slice(0, M * A),))]
            out.append(Case(R.ACTOR_HEAD, f"M{M}-A{A}-det{det}-step{step}" + (f"-no-{null}" if null else ""),
                            [M, A, ldm, ldl, lda, ldmu, lds, step, det], [], slots, ref, [chk]))
    return out


# ----------------------------------------------------------------------------
# actor_head_bwd_x: 16 rows x 64 columns per workgroup, the column-block 0 stores g_heads
# ----------------------------------------------------------------------------
BWD_M = {1: (3, "all"), 15: (8, "no-g_a"), 16: (1, "no-g_mu_l"), 17: (8, "no-g_sig_l"), 33: (3, "all")}  # M -> A, inputs
BWD_N = (1, 63, 64, 65, 130)


def bwd_case(M, A, N, variant, refuse=None):
    g = gen(40 + M)  # the same rows at every N
    g_a, g_mu_l, g_sig_l = randn(g, M, A), randn(g, M, A), randn(g, M, A)
    a, ls, eps = torch.tanh(randn(g, M, A, scale=1.5)), randn(g, M, A, scale=2.0), randn(g, M, A)
    for i, e in enumerate(LS_EDGES):
        if i < M:
            ls[i, i % A] = e
    sat = M >= 12
    if sat:
        a[10, 0], a[11, A - 1] = 1.0, -1.0
    gw = gen(4000 + N + A)
    wt = randn(gw, N, 2 * A)
    if variant == "no-g_a":
        g_a = None
    elif variant == "no-g_mu_l":
        g_mu_l = None
    elif variant == "no-g_sig_l":
        g_sig_l = None
    ldga, ldgl, lda, ldl, ldh, ldx = A + 1, A + 2, A + 3, A + 1, 2 * A + 1, N + 3

    def ref(mut=None):
        r = R.actor_head_bwd_x(g_a, g_mu_l, g_sig_l, a, ls, eps, wt, mut)
        wh = Want(r["g_heads"], key="actor_head_bwd_x.g_heads", scale=r["heads_abs"])
        # 2 A products in one fma chain on the kernel's own g_heads, which carry their own tolerance
        tgx = (2 * A + 2) * U * (r["g_heads"].abs() @ r["W_abs"].t()) + wh.tol @ r["W_abs"].t()
        return dict(g_heads=wh, gx=Want(r["gx"], tol=tgx))

    def chk(o):
        f = []
        if sat and g_a is not None:
            for m, k in ((10, 0), (11, A - 1)):
                want = torch.zeros(()) if g_mu_l is None else g_mu_l[m, k]
                if not torch.equal(_bits(o["g_heads"][m, k].reshape(1)), _bits(want.reshape(1))):
                    f.append(f"a = +-1 exactly: the g_a path adds to g_mu at ({m}, {k})")
        return f
    pd = lambda x, ld: None if x is None else padded(x, ld)  # noqa: E731
    slots = [pd(g_a, ldga), pd(g_mu_l, ldgl), pd(g_sig_l, ldgl), pd(a, lda) if g_a is not None or M % 2 else None,
             padded(ls, ldl), padded(eps.reshape(-1)) if g_a is not None or M % 2 else None,
             Out("g_heads", (M + 1, ldh), (slice(0, M), slice(0, 2 * A))), padded(wt),
             Out("gx", (M + 1, ldx), (slice(0, M), slice(0, N)))]
    return Case(R.ACTOR_HEAD_BWD_X, ("refuse-" if refuse else "") + f"M{M}-A{A}-N{N}-{variant}",
                [M, A, N, ldga, ldgl, lda, ldl, ldh, ldx], [], slots, ref, [chk], refuse=refuse,
                twin=None if refuse else (f"bwd-M{M}-A{A}-{variant}", M))


def bwd_cases():
    out = [bwd_case(M, A, N, variant) for M, (A, variant) in BWD_M.items() for N in BWD_N]
    out += [bwd_case(16, 3, 65, "no-g_a"), bwd_case(15, 1, 64, "no-g_sig_l"), bwd_case(17, 3, 130, "no-g_mu_l")]
    out.append(bwd_case(5, 9, 64, "all", refuse="actions"))
    return out


# ----------------------------------------------------------------------------
# sigmoid, mean
# ----------------------------------------------------------------------------
def sigmoid_cases():
    out = []
    for M, ldx, os_ in ((1, 1, 1), (255, 3, 1), (256, 1, 3), (257, 5, 2)):
        g = gen(M)
        x = randn(g, M, scale=3.0)
        for i, e in enumerate((0.0, 100.0, -100.0, INF, -INF)):
            if i < M:
                x[i] = e
        xb = torch.full((M + 1, ldx), NAN)
        xb[:M, 0] = x

        def ref(mut=None, x=x, M=M):
            s = R.sigmoid(x).reshape(M, 1)
            return dict(out=Want(s, key="sigmoid.out", scale=torch.clamp(s.abs(), min=2.0 ** -102)))

        def chk(o, x=x, M=M):
            want = {0.0: 0.5, 100.0: 1.0, INF: 1.0, -INF: 0.0}
            bad = [e for i, e in enumerate((0.0, 100.0, -100.0, INF, -INF)) if i < M and e in want
                   and float(o["out"][i, 0]) != want[e]]
            return [f"sigmoid({e}) is not exactly {want[e]}" for e in bad]
        out.append(Case(R.SIGMOID, f"M{M}-ldx{ldx}-os{os_}", [M, ldx, os_], [],
                        [xb, Out("out", (M + 1, os_), (slice(0, M), slice(0, 1)))], ref, [chk]))
    return out


MEAN_N = (1, 1023, 1024, 1025, 3840)


def mean_cases():
    out = []
    for n in MEAN_N:
        x = randn(gen(n), n) + 0.25

        def ref(mut=None, x=x, n=n):
            r = R.mean(x, mut)
            # a thread adds ceil(n / 1024) elements, an LDS tree of depth 10, the division
            return dict(out=Want(r["out"], tol=(_cdiv(n, 1024) + 10 + 2) * U * r["abs"]))
        out.append(Case(R.MEAN, f"n{n}", [n], [], [padded(x), Out("out", (2,), (slice(0, 1),))], ref))
    out.append(Case(R.MEAN, "refuse-n0", [0], [], [padded(randn(gen(1), 4)), Out("out", (2,))], None, refuse="positive"))
    return out


# ----------------------------------------------------------------------------
# transpose, copy2d, fill, vec_gather: exact
# ----------------------------------------------------------------------------
T_SIZES = (1, 31, 32, 33, 65)


def transpose_cases():
    out = []
    for rows in T_SIZES:
        for cols in T_SIZES:
            x = randn(gen(rows * 100 + cols), rows, cols)

            def ref(mut=None, x=x):
                return dict(out=Want(R.transpose(x), tol=0.0))
            out.append(Case(R.TRANSPOSE, f"{rows}x{cols}", [rows, cols], [],
                            [padded(x.reshape(-1)), Out("out", (cols + 1, rows), (slice(0, cols), slice(None)))], ref))
    for rows, cols in ((0, 5), (5, 0)):
        out.append(Case(R.TRANSPOSE, f"refuse-{rows}x{cols}", [rows, cols], [],
                        [padded(randn(gen(1), 8)), Out("out", (6, 5))], None, refuse="positive"))
    return out


def transpose_multi_case(label, sizes, refuse=None):
    v, slots, xs = [len(sizes)], [], []
    for j, (rows, cols, pad) in enumerate(sizes):
        x = randn(gen(j * 1000 + rows * 10 + cols), rows, cols)
        xs.append((x, rows + pad))
        v += [rows, cols, rows + pad]
        slots += [padded(x.reshape(-1)), Out(f"out{j}", (cols + 1, rows + pad), (slice(0, cols), slice(0, rows)))]

    def ref(mut=None):
        w = {}
        for j, (x, ldo) in enumerate(xs):
            t = R.transpose(x)
            if mut == "transpose_ignores_ldo":
                flat = torch.zeros(t.shape[0] * ldo, dtype=F64)
                flat[:t.numel()] = t.reshape(-1)
                t = flat.reshape(t.shape[0], ldo)[:, :t.shape[1]]
            w[f"out{j}"] = Want(t, tol=0.0)
        return w
    return Case(R.TRANSPOSE_MULTI, label, v, [], slots, ref, refuse=refuse)


def transpose_multi_cases():
    # the grid is the largest job's (65 x 65: 3 x 3 workgroups): the others' surplus workgroups must write nothing
    ten = [(65, 65, 3), (1, 1, 1), (31, 33, 2), (33, 31, 0), (32, 32, 4), (1, 65, 5), (65, 1, 1), (2, 3, 7), (33, 65, 1),
           (64, 2, 2)]
    return [transpose_multi_case("ten-mixed", ten), transpose_multi_case("one", [(33, 32, 3)]),
            transpose_multi_case("three", [(5, 70, 1), (70, 5, 2), (32, 32, 0)]),
            transpose_multi_case("refuse-eleven", ten + [(2, 2, 0)], refuse="at most")]


def copy_job(j, rows, width, dp, sp, doff=0, soff=0):
    """(v ints, [dst slot, src slot], source matrix).  An offset of one float moves the matrix one column right in
    its buffer (the pointer then is not 16-byte aligned)."""
    x = randn(gen(j * 31 + rows + width), max(rows, 1), width)[:rows]
    src = torch.full((rows + 1, sp), NAN)
    assert soff + width <= sp and doff + width <= dp
    src[:rows, soff:soff + width] = x
    dst = Out(f"dst{j}", (rows + 1, dp), (slice(0, rows), slice(doff, doff + width)))
    return [dp, sp, width, rows], [Shift(dst, doff) if doff else dst, Shift(src, soff) if soff else src], x


COPY_FORMS = (  # label, rows, width, dp, sp, doff, soff
    ("v4", 5, 8, 12, 16, 0, 0), ("v4-1x4", 1, 4, 4, 4, 0, 0),
    ("scalar-dst-offset", 5, 8, 12, 16, 1, 0), ("scalar-src-offset", 5, 8, 12, 16, 0, 1),
    ("scalar-width", 5, 7, 12, 16, 0, 0), ("scalar-dp", 5, 8, 13, 16, 0, 0), ("scalar-sp", 5, 8, 12, 15, 0, 0),
    ("v4-grid-stride", 2052, 1024, 1028, 1024, 0, 0), ("scalar-grid-stride", 514, 1023, 1023, 1025, 0, 0),
)


def copy2d_cases():
    out = []
    for j, (label, rows, width, dp, sp, doff, soff) in enumerate(COPY_FORMS):
        v, slots, x = copy_job(0, rows, width, dp, sp, doff, soff)

        def ref(mut=None, x=x):
            return dict(dst0=Want(x, tol=0.0))
        out.append(Case(R.COPY2D, label, v, [], slots, ref))
    return out


def copy2d_multi_case(label, jobs, refuse=None):
    v, slots, xs = [len(jobs)], [], []
    for j, job in enumerate(jobs):
        vj, sj, x = copy_job(j, *job)
        v += vj
        slots += sj
        xs.append(x)

    def ref(mut=None):
        return {f"dst{j}": Want(x, tol=0.0) for j, x in enumerate(xs) if x.shape[0] > 0}
    return Case(R.COPY2D_MULTI, label, v, [], slots, ref, refuse=refuse)


def copy2d_multi_cases():
    four = [(5, 8, 12, 16), (0, 8, 8, 8), (70, 7, 9, 7), (3, 300, 304, 300, 1, 0)]  # float4, no rows, two scalar forms
    return [copy2d_multi_case("four-one-empty", four), copy2d_multi_case("one-v4", [(33, 64, 64, 68)]),
            copy2d_multi_case("two-sizes", [(600, 1024, 1024, 1024), (1, 1, 1, 1)]),
            copy2d_multi_case("refuse-five", four + [(2, 4, 4, 4)], refuse="at most")]


FILL_N = (1, 7, 1023, 1024, 4 * (2048 * 256 + 3))


def fill_cases():
    out = []
    for n, off in [(n, 0) for n in FILL_N] + [(1024, 1), (8, 3)]:
        val = -2.5 if off else 0.0 if n == 1024 else 3.25

        def ref(mut=None, n=n, val=val):
            return dict(x=Want(torch.full((n,), val), tol=0.0))
        o = Out("x", (n + off + 5,), (slice(off, off + n),))
        out.append(Case(R.FILL, f"n{n}-off{off}", [n], [val], [Shift(o, off) if off else o], ref))
    return out


def vec_gather_cases():
    out = []
    for D in (1, 5, 64):
        nb, T, t0, cap = 3, 4, 2, 7
        n = nb * T
        g = gen(D)
        ring = randn(g, cap, D)
        starts = torch.tensor([5, 6, 0], dtype=torch.int64)  # start + t0 + t runs past the ring's end and wraps
        st, sb = D + 2, (T + t0) * (D + 2) + 3
        obs = torch.full((nb, sb), NAN)
        for b in range(nb):
            for t in range(T + t0):
                obs[b, t * st:t * st + D] = randn(g, D)

        def ref_ring(mut=None, D=D, ring=ring, starts=starts):
            return dict(X=Want(R.vec_gather(n, nb, D, ring=ring, ring_cap=cap, starts=starts, t0=t0), tol=0.0))

        def ref_obs(mut=None, D=D, obs=obs, sb=sb, st=st):
            return dict(X=Want(R.vec_gather(n, nb, D, obs=obs, stride_b=sb, stride_t=st, t0=t0), tol=0.0))
        X = lambda: Out("X", (n + 1, D), (slice(0, n), slice(None)))  # noqa: E731
        out.append(Case(R.VEC_GATHER, f"ring-D{D}", [n, nb, D, cap, 0, 0, t0], [], [padded(ring.reshape(-1)), starts, None, X()], ref_ring))
        out.append(Case(R.VEC_GATHER, f"obs-D{D}", [n, nb, D, 0, sb, st, t0], [], [None, None, obs.reshape(-1), X()], ref_obs))
    ring, starts = randn(gen(9), 7, 5), torch.tensor([5, 6, 0], dtype=torch.int64)
    X = lambda: Out("X", (13, 5))  # noqa: E731
    for label, v, slots in (("D0", [12, 3, 0, 7, 0, 0, 0], [ring.reshape(-1), starts, None, X()]),
                            ("nb0", [12, 0, 5, 7, 0, 0, 0], [ring.reshape(-1), starts, None, X()]),
                            ("no-source", [12, 3, 5, 7, 0, 0, 0], [None, None, None, X()]),
                            ("ring-no-starts", [12, 3, 5, 7, 0, 0, 0], [ring.reshape(-1), None, None, X()]),
                            ("ring-cap0", [12, 3, 5, 0, 0, 0, 0], [ring.reshape(-1), starts, None, X()])):
        out.append(Case(R.VEC_GATHER, "refuse-" + label, v, [], slots, None, refuse="bad source"))
    return out


def all_cases():
    return (gru_cases() + onehot_cases() + zgather_cases() + gru_fwd_cases() + sample_cases() + actor_head_cases()
            + bwd_cases() + sigmoid_cases() + mean_cases() + transpose_cases() + transpose_multi_cases() + copy2d_cases()
            + copy2d_multi_cases() + fill_cases() + vec_gather_cases())


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
def _num(t):
    """An output region as float64 (u16 patterns as 0 .. 65535)."""
    return (t.to(torch.int32) & 0xFFFF).to(F64) if t.dtype == torch.int16 else t.to(F64)


def untouched(case, bufs):
    """A refused call: every output buffer is still POISON."""
    return [f"{o.name}: written by a refused call" for o in case.outs() if not bool(is_poison(bufs[o.name]).all())]


def compare(case, bufs, wants=None, report=None):
    """bufs: {output name: the whole buffer after the call}.  Returns the failures: an element outside the region or
    of an output the call must not write that is no longer POISON, a written element that still is, a value off its
    reference by more than its tolerance (no element left out; the `given` outputs are left to the checks), a failed
    exactness check.  report(key, kind, x): kind "measured": the largest error of the output in units of 2^-24 x
    scale; "derived": as a fraction of its derived bound."""
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
        if o.name not in wants:
            if not bool(is_poison(r).all()):  # an output this call must not write
                fails.append(f"{o.name}: written, and must not be")
            continue
        region[o.name] = r
        w = wants[o.name]
        if bool(is_poison(r).any()):
            fails.append(f"{o.name}: {int(is_poison(r).sum())} unwritten elements")
            continue
        if o.name in case.given:
            continue
        got = _num(r)
        ref = w.ref.reshape(got.shape)
        tol = w.tol.reshape(got.shape)
        assert not bool(torch.isnan(tol).any()), (case, o.name)
        both_nan = torch.isnan(ref) & torch.isnan(got)
        same_inf = torch.isinf(ref) & (ref == got)
        err = torch.where(both_nan | same_inf, torch.zeros_like(got), (got - ref).abs())
        bad = ~(err <= tol)  # a NaN where none belongs fails
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{o.name}: {int(bad.sum())} of {bad.numel()} beyond tolerance, first at {i}: got "
                         f"{float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} tol {float(tol.reshape(-1)[i]):.3e}")
        if report and w.key:
            sc = w.scale.reshape(got.shape)
            ok = (sc > 0) & torch.isfinite(err)
            report(w.key, "measured", float((err[ok] / (U * sc[ok])).max()) if bool(ok.any()) else 0.0)
        elif report:  # a derived bound: the largest error as a fraction of it (0 where the bound is 0: exact)
            ok = (tol > 0) & torch.isfinite(tol) & torch.isfinite(err)
            report(f"{case.name}.{o.name}", "derived", float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0)
    if not fails:
        for chk in case.checks:
            fails += chk(region)
    return fails
