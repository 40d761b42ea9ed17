"""The value-learning and gradient-norm primitives of dreamer_amd/csrc/ops.hip
held, one entry point at a time, to the float64 references of
tests/primitives_ref.py (run on the MI355X box: pytest -m gpu).

  dr_sqnorm, dr_sqnorm_multi, dr_clip_stats   squared-norm reductions, skip flag
  dr_nonfinite                                non-finite guard
  dr_lambda_returns                           Agent.py:156-172
  dr_bucket_value                             symexp E[bucket]
  dr_critic_loss_bwd (+ dr_critic_fwd)        two-hot cross-entropy and its backward
  dr_actor_loss_grad                          Agent.py:105-125

The whole-epoch tests see these kernels only through averaged losses on
well-behaved data; here the inputs sit on the edges: the last n % 4 elements
and every workgroup's chunk boundary of a reduction, returns exactly on a
bucket and beyond the bucket range, actions of exactly +-1, an episode end in
the middle of a return.  The kernels read the float32 inputs given here; the
references read the same float32 values and continue in float64.

Launch geometry (read from ops.hip, used for needle positions and summation
bounds):
  dr_sqnorm        1 workgroup x 1024 threads; float4 loop of stride 1024 over
                   n / 4 float4 when the pointer is 16-byte aligned (else a
                   scalar loop of stride 1024 over everything), the n % 4 tail
                   by scalar loads; LDS tree; acc += total.
  dr_sqnorm_multi  blocks = clamp(ceil(n4 / 4096), 1, 512), contiguous chunks of
                   ceil(n4 / blocks) float4, 256 threads each; a second kernel
                   (1 x 256) adds the partials and the tail; acc += total.
                   Misaligned pointer or no scratch: dr_sqnorm.
  dr_clip_stats    per buffer blocks = clamp(ceil(n4 / 2048), 1, 256), chunks of
                   ceil(n4 / blocks) float4, 256 threads; the last workgroup to
                   arrive adds the partials and the tails; sq[w] = total.

Summation bound (random data): |got - sum x^2| <= (L + log2(threads) + serial
+ 4) * 2^-24 * sum x^2, L the longest chain one thread adds, serial the
additions of the second stage (its chain and its tree), 4 = the square, the
two-level combine of the four float4 lanes and the final add.

NaN returns are not fed to the two-hot target anywhere below: fminf / fmaxf
and torch.clamp differ on NaN, and the non-finite skip handles NaN upstream.
"""
import math

import numpy as np
import pytest
import torch

import primitives_ref as PR

pytestmark = pytest.mark.gpu

U = PR.U
F32_MAX = 3.4e38
DENORMAL = 1e-40


def _api():
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    return L, hip.stream()


def _cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------
# 1. squared norms
# ----------------------------------------------------------------------------
def _multi_geometry(n):
    n4 = n // 4
    nb = min(max(_cdiv(n4, 4096), 1), 512)
    return n4, nb, _cdiv(n4, nb)


def _clip_geometry(n):
    n4 = n // 4
    nb = min(max(_cdiv(n4, 2048), 1), 256)
    return n4, nb, _cdiv(n4, nb)


def _positions(n, n4=None, blocks=1, chunk=None, extra=()):
    """Needle positions: 0, n - 1, the n % 4 tail, 4 (n / 4) - 1, and the first
    element of the first / last element of the last float4 of every block's chunk."""
    n4 = n // 4 if n4 is None else n4
    chunk = n4 if chunk is None else chunk
    ps = {0, n - 1, 4 * n4 - 1, *range(4 * n4, n), *extra}
    for b in range(blocks):
        b0, b1 = b * chunk, min((b + 1) * chunk, n4)
        if b0 < b1:
            ps |= {4 * b0, 4 * b0 + 3, 4 * (b1 - 1), 4 * b1 - 1}
    return sorted(p for p in ps if 0 <= p < n)


def _buffer(n, dev, offset):
    """n zeros, 16-byte aligned (offset 0) or one float past alignment."""
    buf = torch.zeros(n + 8, device=dev)
    x = buf[offset:offset + n]
    assert x.data_ptr() % 16 == 4 * offset
    return x


def _needles(x, positions, launch, out):
    """For each position: x = 0 except x[p] = 3, launch(x, out[i]).  One sync."""
    for i, p in enumerate(positions):
        x[p:p + 1].fill_(3.0)
        launch(x, out[i])
        x[p:p + 1].zero_()
    torch.cuda.synchronize()
    return out.cpu()


# 1023 * 4 + 1: one float4 short of a full pass of the 1024 threads; 4096 and 4103: one pass exactly, and a
# second pass (n4 = 1025) with a 3-element tail
SQ_SIZES = [1, 3, 4, 5, 1023 * 4 + 1, 4096, 4103]
# positions where the 1024-thread loops wrap (float4 loop and the scalar loop of a misaligned pointer)
SQ_WRAP = (1023, 1024, 4 * 1023 + 3, 4 * 1024)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SQ_SIZES)
def test_sqnorm_needle(gpu, n, offset):
    """One 3.0 anywhere gives exactly 9.0, added to the accumulator's 5.0."""
    L, st = _api()
    x = _buffer(n, gpu, offset)
    pos = _positions(n, extra=SQ_WRAP)
    out = torch.full((len(pos),), 5.0, device=gpu)
    got = _needles(x, pos, lambda g, o: L.call("dr_sqnorm", n, L.ptr(g), L.ptr(o), st), out)
    bad = [(p, float(v)) for p, v in zip(pos, got) if float(v) != 14.0]
    assert not bad, f"n={n}: (position, result) {bad[:8]}"


MULTI_SIZES = SQ_SIZES + [4 * 4096, 4 * 4097, 4 * 512 * 4096, 4 * (512 * 4096 + 1), 4 * 512 * 4096 + 7]


@pytest.mark.parametrize("n", MULTI_SIZES)
def test_sqnorm_multi_needle(gpu, n):
    L, st = _api()
    n4, nb, chunk = _multi_geometry(n)
    x = _buffer(n, gpu, 0)
    scr = torch.zeros(512, device=gpu)
    pos = _positions(n, n4, nb, chunk, extra=SQ_WRAP)
    out = torch.full((len(pos),), 5.0, device=gpu)
    got = _needles(x, pos, lambda g, o: L.call("dr_sqnorm_multi", n, L.ptr(g), L.ptr(o), L.ptr(scr), st), out)
    bad = [(p, float(v)) for p, v in zip(pos, got) if float(v) != 14.0]
    assert not bad, f"n={n} blocks={nb} chunk={chunk}: (position, result) {bad[:8]}"


@pytest.mark.parametrize("variant", ["offset1", "no_scratch"])
@pytest.mark.parametrize("n", SQ_SIZES + [4 * 4097 + 2])
def test_sqnorm_multi_fallback_needle(gpu, n, variant):
    """A pointer one float off alignment, or scratch = NULL: the single-workgroup kernel."""
    L, st = _api()
    x = _buffer(n, gpu, 1 if variant == "offset1" else 0)
    scr = torch.zeros(512, device=gpu) if variant == "offset1" else None
    pos = _positions(n, extra=SQ_WRAP)
    out = torch.full((len(pos),), 5.0, device=gpu)
    got = _needles(x, pos, lambda g, o: L.call("dr_sqnorm_multi", n, L.ptr(g), L.ptr(o), L.ptr(scr), st), out)
    bad = [(p, float(v)) for p, v in zip(pos, got) if float(v) != 14.0]
    assert not bad, f"n={n}: (position, result) {bad[:8]}"


# (na, nb): n / 4 in {2048, 2049, 256 * 2048, 256 * 2048 + 3} with every tail length, the two buffers of
# different sizes, and buffers smaller than one float4
CLIP_PAIRS = [(1, 5), (3, 4), (4 * 2048, 4 * 2049 + 1), (4 * 2049 + 3, 4 * 2048 + 2),
              (4 * 256 * 2048, 4 * (256 * 2048 + 3) + 1), (4 * (256 * 2048 + 3) + 2, 4 * 256 * 2048 + 3)]


def _clip(L, st, ga, gb, nloss, loss, sq, skip, scr):
    L.call("dr_clip_stats", ga.numel(), L.ptr(ga), gb.numel(), L.ptr(gb), nloss, L.ptr(loss), L.ptr(sq),
           L.ptr(skip), L.ptr(scr), st)


@pytest.mark.parametrize("na,nb", CLIP_PAIRS)
def test_clip_stats_needle(gpu, na, nb):
    """One 3.0 in either buffer: sq = (9, 0) or (0, 9) exactly, whatever sq held
    (it writes), skip = 0 whatever it held; every call on the same scratch."""
    L, st = _api()
    a, b = _buffer(na, gpu, 0), _buffer(nb, gpu, 0)
    scr = torch.zeros(1024, device=gpu)
    loss = torch.tensor([0.5, 1.5], device=gpu)
    for x, n, want in ((a, na, (9.0, 0.0)), (b, nb, (0.0, 9.0))):
        pos = _positions(n, *_clip_geometry(n))
        sq = torch.full((len(pos), 2), 5.0, device=gpu)
        sq[1::2] = float("nan")
        skip = torch.full((len(pos),), 7, dtype=torch.int32, device=gpu)
        for i, p in enumerate(pos):
            x[p:p + 1].fill_(3.0)
            _clip(L, st, a, b, 2, loss, sq[i], skip[i:i + 1], scr)
            x[p:p + 1].zero_()
        torch.cuda.synchronize()
        got = sq.cpu()
        bad = [(p, tuple(map(float, v))) for p, v in zip(pos, got) if tuple(map(float, v)) != want]
        assert not bad, f"needle in buffer of {n}: (position, sq) {bad[:8]}"
        assert int(skip.abs().sum()) == 0


def _sumsq_bound(x, L_chain, threads, serial):
    s = float((x.cpu().double() ** 2).sum())
    return s, (L_chain + math.log2(threads) + serial + 4) * U * s


def _randn(n, gpu, seed, offset=0):
    x = _buffer(n, gpu, offset)
    x.copy_(torch.randn(n, generator=torch.Generator().manual_seed(seed)))
    return x


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 5, 1023 * 4 + 1, 4103, 100_003])
def test_sqnorm_random(gpu, n, offset):
    L, st = _api()
    x = _randn(n, gpu, n, offset)
    acc = torch.zeros(1, device=gpu)
    L.call("dr_sqnorm", n, L.ptr(x), L.ptr(acc), st)
    torch.cuda.synchronize()
    chain = _cdiv(n, 1024) if offset else _cdiv(n // 4, 1024) + (1 if n % 4 else 0)
    want, tol = _sumsq_bound(x, chain, 1024, 0)
    err = abs(float(acc) - want)
    print(f"dr_sqnorm n={n} offset={offset}: err {err:.3g} bound {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("n", [5, 4 * 4097 + 1, 4 * 512 * 4096 + 7])
def test_sqnorm_multi_random(gpu, n):
    L, st = _api()
    n4, nb, chunk = _multi_geometry(n)
    x = _randn(n, gpu, n)
    acc, scr = torch.zeros(1, device=gpu), torch.zeros(512, device=gpu)
    L.call("dr_sqnorm_multi", n, L.ptr(x), L.ptr(acc), L.ptr(scr), st)
    torch.cuda.synchronize()
    want, tol = _sumsq_bound(x, _cdiv(chunk, 256), 256, _cdiv(nb, 256) + (1 if n % 4 else 0) + 8)
    err = abs(float(acc) - want)
    print(f"dr_sqnorm_multi n={n}: err {err:.3g} bound {tol:.3g}")
    assert err <= tol


@pytest.mark.parametrize("na,nb", CLIP_PAIRS)
def test_clip_stats_random_and_rearm(gpu, na, nb):
    """Two calls in a row on the same zeroed-once scratch with different data:
    both right (the arrival ticket re-arms), against the float64 sums."""
    L, st = _api()
    scr = torch.zeros(1024, device=gpu)
    loss = torch.tensor([0.5, 1.5], device=gpu)
    sq = torch.full((2, 2), float("nan"), device=gpu)
    skip = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    data = [(_randn(na, gpu, 10 * k + 1), _randn(nb, gpu, 10 * k + 2) * (0.1 + k)) for k in range(2)]
    for k, (a, b) in enumerate(data):
        b = b.contiguous()
        data[k] = (a, b)
        assert b.data_ptr() % 16 == 0
        _clip(L, st, a, b, 2, loss, sq[k], skip[k:k + 1], scr)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(data):
        for w, x in enumerate((a, b)):
            n4, blocks, chunk = _clip_geometry(x.numel())
            want, tol = _sumsq_bound(x, _cdiv(chunk, 256), 256, _cdiv(blocks, 256) + (1 if x.numel() % 4 else 0) + 8)
            err = abs(float(sq[k, w]) - want)
            print(f"dr_clip_stats call {k} buffer {w} n={x.numel()}: err {err:.3g} bound {tol:.3g}")
            assert err <= tol, (k, w, float(sq[k, w]), want)
    assert int(skip.abs().sum()) == 0


@pytest.mark.parametrize("slot", ["first", "last"])
@pytest.mark.parametrize("value,want", [(float("nan"), 1), (float("inf"), 1), (float("-inf"), 1), (F32_MAX, 0),
                                        (-F32_MAX, 0), (DENORMAL, 0), (-0.0, 0)])
def test_clip_stats_skip(gpu, value, want, slot):
    """skip = any non-finite value among the loss slots (Agent.py:137-139), written either way."""
    L, st = _api()
    a, b = _randn(37, gpu, 1), _randn(5, gpu, 2)
    scr = torch.zeros(1024, device=gpu)
    loss = torch.tensor([0.25, -3.0, 1e-3], device=gpu)
    loss[0 if slot == "first" else 2] = value
    for preset in (0, 1):
        skip = torch.full((1,), preset, dtype=torch.int32, device=gpu)
        sq = torch.zeros(2, device=gpu)
        _clip(L, st, a, b, 3, loss, sq, skip, scr)
        torch.cuda.synchronize()
        assert int(skip) == want, (value, slot, preset)
    # no loss slots: nothing to be non-finite, whatever the pointer holds
    skip = torch.ones(1, dtype=torch.int32, device=gpu)
    _clip(L, st, a, b, 0, loss, sq, skip, scr)
    torch.cuda.synchronize()
    assert int(skip) == 0


def test_clip_stats_refuses_unaligned(gpu):
    L, st = _api()
    a, b = _buffer(64, gpu, 1), _buffer(64, gpu, 0)
    scr = torch.zeros(1024, device=gpu)
    loss, sq = torch.zeros(2, device=gpu), torch.zeros(2, device=gpu)
    skip = torch.zeros(1, dtype=torch.int32, device=gpu)
    for ga, gb in ((a, b), (b, a)):
        with pytest.raises(L.HipError):
            _clip(L, st, ga, gb, 2, loss, sq, skip, scr)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------
# 2. dr_nonfinite
# ----------------------------------------------------------------------------
NF_SIZES = [1, 64, 65, 257, 100_003]


def _finite_edge_data(n, gpu):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    edge = torch.tensor([F32_MAX, -F32_MAX, DENORMAL, -DENORMAL, -0.0, 0.0])
    reps = _cdiv(n, 6)
    x[::2] = edge.repeat(reps)[:x[::2].numel()]
    x[-1] = -F32_MAX if n > 1 else DENORMAL
    return x.to(gpu)


@pytest.mark.parametrize("n", NF_SIZES)
def test_nonfinite_positions(gpu, n):
    """One NaN / +Inf / -Inf at the wave and workgroup edges and at n - 1 sets the
    flag; the finite edge values around it (+-3.4e38, denormals, -0.0) do not."""
    L, st = _api()
    x = _finite_edge_data(n, gpu)
    keep = x.clone()
    pos = sorted({p for p in (0, 63, 64, 255, 256, n - 1) if p < n})
    cases = [(p, v) for p in pos for v in (float("nan"), float("inf"), float("-inf"))]
    flags = torch.zeros(len(cases) + 2, dtype=torch.int32, device=gpu)
    flags[-1] = 1
    for i, (p, v) in enumerate(cases):
        x[p:p + 1].fill_(v)
        L.call("dr_nonfinite", n, L.ptr(x), L.ptr(flags[i:i + 1]), st)
        x[p:p + 1].copy_(keep[p:p + 1])
    L.call("dr_nonfinite", n, L.ptr(x), L.ptr(flags[-2:-1]), st)  # all finite: stays 0
    L.call("dr_nonfinite", n, L.ptr(x), L.ptr(flags[-1:]), st)    # all finite, preset 1: stays 1
    torch.cuda.synchronize()
    got = flags.cpu().tolist()
    missed = [c for c, f in zip(cases, got) if f != 1]
    assert not missed, f"n={n}: not flagged (position, value) {missed}"
    assert got[-2:] == [0, 1]


def test_nonfinite_preset_and_empty(gpu):
    L, st = _api()
    x = torch.full((65,), float("nan"), device=gpu)
    flag = torch.zeros(2, dtype=torch.int32, device=gpu)
    flag[1] = 1
    L.call("dr_nonfinite", 0, L.ptr(x), L.ptr(flag[0:1]), st)  # n = 0: OK, flag left alone
    L.call("dr_nonfinite", 0, L.ptr(x), L.ptr(flag[1:2]), st)
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [0, 1]
    L.call("dr_nonfinite", 65, L.ptr(x), L.ptr(flag[1:2]), st)  # a set flag stays set
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [0, 1]


# ----------------------------------------------------------------------------
# 3. dr_lambda_returns
# ----------------------------------------------------------------------------
def _returns_case(B, H, seed):
    """Rewards of mixed sign, continues in (0.5, 1]; two rows in three end an
    episode (c = 0 exactly) at step b % H, and everything after that step is
    1e30 in r and V, so a leak past the end is a huge error."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(B, H, generator=g) * 2
    c = 1.0 - 0.5 * torch.rand(B, H, generator=g)
    V = torch.randn(B, H + 1, generator=g) * 5
    cut = torch.full((B,), -1, dtype=torch.long)
    for b in range(B):
        if b % 3 != 2:
            t0 = b % H
            c[b, t0] = 0.0
            r[b, t0 + 1:] = 1e30
            V[b, t0 + 1:] = 1e30
            cut[b] = t0
    return r, c, V, cut


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 0.0), (1.0, 1.0), (0.5, 0.3)])
@pytest.mark.parametrize("H", [1, 2, 15])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_lambda_returns(gpu, B, H, gamma, lam):
    """Against the float64 recursion: |d| <= 8 (H - t) 2^-24 A_t, A_t the recursion
    on absolute values (6 roundings a step, and the float32 1 - lambda)."""
    L, st = _api()
    r, c, V, cut = _returns_case(B, H, 100 * B + H)
    R = torch.full((B, H), float("nan"), device=gpu)
    rd, cd, Vd = r.to(gpu), c.to(gpu), V.to(gpu)
    L.call("dr_lambda_returns", B, H, L.ptr(rd), L.ptr(cd), L.ptr(Vd), gamma, lam, L.ptr(R), st)
    torch.cuda.synchronize()
    got = R.cpu().double()
    want = PR.lambda_returns(r, c, V, gamma, lam)
    A = PR.lambda_returns_abs(r, c, V, gamma, lam)
    tol = 8 * torch.arange(H, 0, -1, dtype=torch.float64) * U * A
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all())
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f"dr_lambda_returns B={B} H={H} gamma={gamma} lam={lam}: worst err/bound {ratio:.3g}")
    assert bool((err <= tol).all()), f"{int((err > tol).sum())} out of bound, worst ratio {ratio:.3g}"
    for b in range(B):  # the step that ends an episode returns its reward, bit for bit
        if cut[b] >= 0:
            assert float(got[b, cut[b]]) == float(r[b, cut[b]])


@pytest.mark.parametrize("B,H", [(0, 3), (3, 0), (-1, 3), (3, -1)])
def test_lambda_returns_refuses_bad_dims(gpu, B, H):
    L, st = _api()
    t = torch.zeros(64, device=gpu)
    with pytest.raises(L.HipError):
        L.call("dr_lambda_returns", B, H, L.ptr(t), L.ptr(t), L.ptr(t), 0.99, 0.95, L.ptr(t), st)


# ----------------------------------------------------------------------------
# 4. dr_bucket_value
# ----------------------------------------------------------------------------
def _logit_patterns(M, nb, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn(M, nb, generator=g) * 2
    rows = torch.arange(M)
    out = {"random": rnd}
    sign = torch.where(rows % 2 == 0, 80.0, -80.0).unsqueeze(1)
    out["offset80"] = rnd + sign
    for name, hot in (("onehot_first", torch.zeros(M, dtype=torch.long)),
                      ("onehot_last", torch.full((M,), nb - 1)), ("onehot_spread", (rows * 37 + nb // 2) % nb)):
        t = torch.full((M, nb), -1e4)
        t[rows, hot] = 1.5
        out[name] = t
    inf = rnd.clone()
    mask = torch.rand(M, nb, generator=g) < 0.3
    mask[rows, (rows * 5) % nb] = False  # at least one finite logit a row
    inf[mask] = float("-inf")
    out["some_neg_inf"] = inf
    out["all_equal"] = torch.full((M, nb), 3.0)
    half = torch.randn(M, _cdiv(nb, 2), generator=g) * 2
    out["symmetric"] = torch.cat([half[:, :nb // 2], half.flip(1)], dim=1)  # l[k] == l[nb - 1 - k]
    return out


@pytest.mark.parametrize("nb", [2, 63, 64, 65, 255])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 9])
def test_bucket_value(gpu, M, nb):
    """symexp(sum softmax(l) b) against float64.  The float32 expectation is off
    by at most d = (ceil(nb / 64) + 12) 2^-24 sum p |b| (the lane's chain, the
    wave tree, expf, the division, the product and the same for the
    normaliser); through symexp's slope that is d e^(|x| + d), and symexp's
    own expf (1 ulp) and subtraction add 3 2^-24 e^|x|.  On the +-25 grid the
    one-hot rows put the expectation beyond symexp's clamp at +-20; the
    symmetric rows have expectation 0."""
    L, st = _api()
    worst = 0.0
    b20 = torch.linspace(-20, 20, nb)
    # torch.linspace is antisymmetric only up to rounding; (b - flip(b)) / 2 is exactly
    grids = {"lin20": b20, "lin25": torch.linspace(-25, 25, nb), "antisymmetric": (b20 - b20.flip(0)) / 2}
    patterns = _logit_patterns(M, nb, 1000 * M + nb)
    for gname, b in grids.items():
        bd = b.to(gpu)
        for name, lg in patterns.items():
            if gname == "antisymmetric" and name not in ("symmetric", "all_equal"):
                continue
            assert lg.shape == (M, nb)
            lgd = lg.to(gpu)
            out = torch.full((M,), float("nan"), device=gpu)
            L.call("dr_bucket_value", M, nb, L.ptr(lgd), L.ptr(bd), L.ptr(out), st)
            torch.cuda.synchronize()
            got = out.cpu().double()
            E, Eabs = PR.bucket_expectation(lg, b)
            want = PR.symexp(E)
            d = (_cdiv(nb, 64) + 12) * U * Eabs
            x = E.abs().clamp(max=20.0)
            tol = d * torch.exp((x + d).clamp(max=20.0)) + 3 * U * torch.exp(x)
            err = (got - want).abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert bool((err <= tol).all()), (f"{gname} {name}: got {got.tolist()} want {want.tolist()} "
                                              f"tol {tol.tolist()}")
            if gname == "antisymmetric":  # the expectation is 0 (to float64 rounding)
                assert float(E.abs().max()) <= 1e-13
            if gname == "lin25" and name in ("onehot_first", "onehot_last"):
                assert float(want.abs().min()) == math.expm1(20.0)  # symexp's clamp is what these rows test
    print(f"dr_bucket_value M={M} nb={nb}: worst err/bound {worst:.3g}")


# ----------------------------------------------------------------------------
# 5. critic two-hot cross-entropy
# ----------------------------------------------------------------------------
MID = 100  # "a middle bucket"


@pytest.fixture(scope="module")
def critic(gpu):
    """The small configuration's critic, with its bucket table inside a
    NaN-filled buffer: an index one off either end of the table poisons the
    loss instead of reading a neighbouring allocation."""
    from dreamer_amd import _lib as L
    from gpu_helpers import build
    d, P = build("small", gpu)
    ag = d.agent
    ag._ensure_flat()
    nb = ag.critic.num_buckets
    guard = torch.full((nb + 128,), float("nan"), device=gpu)
    guard[64:64 + nb] = ag.critic.buckets_crit
    cs = ag.critic_struct()
    cs.buckets = guard[64:64 + nb].data_ptr()
    net = ag.critic.value_net
    dm = L.dr_dims()
    dm.hidden, dm.rows, dm.cols = net[0].in_features - 64, 64, 1
    dm.action = 3
    dm.critic_h1, dm.critic_h2, dm.buckets = net[0].out_features, net[3].out_features, nb
    assert nb == 255 and dm.hidden == 64
    return dict(d=d, P=P, ag=ag, cs=cs, dm=dm, guard=guard, buckets=ag.critic.buckets_crit.cpu())


def _edge_returns(b):
    """float32 returns whose symlog is: a bucket value (first, a middle one, the
    last but one, the last), one float32 step of R and of symlog(R) either side
    of the middle bucket, 0, and beyond both ends."""
    f = lambda v: float(np.float32(float(PR.symexp(torch.tensor(float(v), dtype=torch.float64)))))
    mid = np.float32(f(b[MID]))
    return {
        "first": f(b[0]), "middle": float(mid), "last_but_one": f(b[253]), "last": f(b[254]),
        "mid_R_minus": float(np.nextafter(mid, np.float32(-np.inf))),
        "mid_R_plus": float(np.nextafter(mid, np.float32(np.inf))),
        "mid_v_minus": f(np.nextafter(np.float32(b[MID]), np.float32(-np.inf))),
        "mid_v_plus": f(np.nextafter(np.float32(b[MID]), np.float32(np.inf))),
        "zero": 0.0, "below": -1e9, "above": 1e9,
    }


EDGE_NAMES = ["first", "middle", "last_but_one", "last", "mid_R_minus", "mid_R_plus", "mid_v_minus", "mid_v_plus",
              "zero", "below", "above"]


def _states(B, H, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    h = torch.tanh(torch.randn(B, H + 1, 64, generator=g))
    idx = torch.randint(0, 8, (B, H + 1, 8), generator=g)
    z = torch.nn.functional.one_hot(idx, 8).float().reshape(B, H + 1, 64)
    return h, z


def _critic_loss_bwd(C, h, z, R, scale, gpu):
    """dr_critic_fwd (logits, tape) then dr_critic_loss_bwd; returns (logits
    [B, H+1, nb] on the CPU, loss, flat critic gradient)."""
    L, st = _api()
    ag, dm, cs = C["ag"], C["dm"], C["cs"]
    B, H = R.shape
    M = B * (H + 1)
    hd, zd, Rd = h.to(gpu).contiguous(), z.to(gpu).contiguous(), R.to(gpu).contiguous()
    tape = torch.zeros(L.query("dr_critic_tape_bytes", dm, M), dtype=torch.uint8, device=gpu)
    lg = torch.full((M, dm.buckets), float("nan"), device=gpu)
    L.call("dr_critic_fwd", dm, cs, M, L.ptr(hd), dm.hidden, L.ptr(zd), dm.rows, L.ptr(lg), None, L.ptr(tape), None, 0,
           st)
    ws = torch.zeros(L.query("dr_critic_workspace_bytes", dm, B, H), dtype=torch.uint8, device=gpu)
    loss = torch.full((1,), float("nan"), device=gpu)
    ag.fc.grad.zero_()
    L.call("dr_critic_loss_bwd", dm, cs, B, H, L.ptr(hd), L.ptr(zd), L.ptr(Rd), L.ptr(tape), scale, L.ptr(loss),
           ag.critic_struct(grad=True), L.ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()
    return lg.cpu().view(B, H + 1, -1), float(loss), ag.fc.grad.clone()


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_critic_ce_row_loss_at_edges(gpu, critic, name):
    """One row at a time (B = 1, H = 1: loss_out is that row's CE) with the
    return on a two-hot edge, against the float64 CE of the kernel's own
    logits: |d| <= 32 2^-24 (|loss| + max|logit - max|)."""
    b = critic["buckets"]
    Rv = _edge_returns(b)[name]
    h, z = _states(1, 1, 7 + EDGE_NAMES.index(name), gpu)
    R = torch.tensor([[Rv]], dtype=torch.float32)
    lg, loss, _ = _critic_loss_bwd(critic, h, z, R, 1.0, gpu)
    assert bool(torch.isfinite(lg).all())
    want = float(PR.critic_ce_rows(lg[:, :1], R, b))
    spread = float((lg[0, 0].double() - lg[0, 0].double().max()).abs().max())
    tol = 32 * U * (abs(want) + spread)
    lo, w = PR.twohot_parts(PR.symlog(R), b)
    print(f"critic CE {name}: R={Rv!r} lo={int(lo)} w={float(w):.9g} loss {loss:.9g} want {want:.9g} "
          f"err/bound {abs(loss - want) / tol:.3g}")
    assert abs(loss - want) <= tol, (name, loss, want, tol)


def _place_edges(b, B, H):
    vals = list(_edge_returns(b).values())
    assert B * H >= len(vals)
    g = torch.Generator().manual_seed(9)
    R = torch.randn(B * H, generator=g) * 30
    R[:len(vals)] = torch.tensor(vals)
    return R[torch.randperm(B * H, generator=g)].view(B, H).float()


def test_critic_ce_gradients(gpu, critic):
    """B = 3, H = 5: 18 logit rows (not a multiple of the 4 rows a workgroup
    takes), the t = H rows contribute nothing, every edge return in R.  Each
    parameter's gradient against float64 autograd through the oracle's critic
    with the parameters cast to double, to the epoch tests' gradient bound
    (tests/test_gpu_baseline.py): |d| <= 1e-4 |ref| + 1e-5 max|ref| per tensor.
    Then the t = H rows' h / z are perturbed: every gradient bit-identical."""
    from oracle import dreamer_oracle as O
    from gpu_helpers import close
    B, H = 3, 5
    b = critic["buckets"]
    ag = critic["ag"]
    R = _place_edges(b, B, H)
    h, z = _states(B, H, 21, gpu)
    lg, loss, grad = _critic_loss_bwd(critic, h, z, R, 1.0 / (B * H), gpu)
    keys = [O.AG + k for k in O.CRITIC_KEYS]
    P64 = {k: critic["P"][k].double().clone().requires_grad_(True) for k in keys}
    lg64 = O.critic_logits(h.double(), z.double(), P64)[:, :-1]
    want_loss = PR.critic_ce_rows(lg64, R, b).mean()
    g64 = torch.autograd.grad(want_loss, [P64[k] for k in keys])
    want_loss = float(want_loss.detach())
    assert abs(loss - want_loss) <= 1e-4 * abs(want_loss), (loss, want_loss)
    for k, g_ref in zip(O.CRITIC_KEYS, g64):
        o = ag.fc.offsets[k.split(".", 1)[1]]
        g_gpu = grad[o:o + g_ref.numel()].view(g_ref.shape)
        scale = float(g_ref.abs().max())
        assert scale > 0
        close(g_gpu, g_ref.float(), 1e-4, 1e-5 * scale, f"critic grad {k}")
    h2, z2 = h.clone(), z.clone()
    h2[:, H] = -h[:, H] + 0.25
    z2[:, H] = z[:, H].roll(1, dims=-1) * 3.0
    _, loss2, grad2 = _critic_loss_bwd(critic, h2, z2, R, 1.0 / (B * H), gpu)
    assert loss2 == loss
    assert torch.equal(grad2, grad), f"{int((grad2 != grad).sum())} gradient elements moved with the t = H rows"


# ----------------------------------------------------------------------------
# 6. dr_actor_loss_grad
# ----------------------------------------------------------------------------
# float32 operations on each output's path (k_actor_loss_grad, k_mean), doubled:
#   g_mus:    R - V, / norm, nu - ., scale * .  (4)  atanhf, x - mu (2)  sg * sg, d / ., gl * . (3)       ->  9
#   g_sigmas: the same 6, then d * d, sg * sg, * sg, /, 1 / sg, -, gl * . (7)                             -> 13
#   loss:     per action term atanhf, x - mu, d * d, sg * sg, 2 * ., /, logf, - ., - HALF_LOG_2PI (9),
#             -2 * x, expf, log1pf, LOG2 - x, - ., 2 * . (6), -ladj + lp, logp += (2), A - 1 <= 7 more
#             additions, R - V, / norm, logp * sadv, nu * ., the subtraction (5), k_mean's chain of 1,
#             its 10-level tree and the division (12)                                                    -> 41
K_MU, K_SIGMA, K_LOSS = 18, 26, 82


def _actor_case(B, H, A, seed):
    g = torch.Generator().manual_seed(seed)
    n = B * H * A
    a = torch.tanh(torch.randn(n, generator=g))
    special = torch.tensor([1.0, -1.0, 0.0, 1.0 - 1e-7, -(1.0 - 1e-7)])
    sp = torch.nn.functional.softplus
    s_lo, s_hi = float(sp(torch.tensor(-5.0)) + 1e-3), float(sp(torch.tensor(2.0)) + 1e-3)
    sigma = sp(torch.rand(n, generator=g) * 7 - 5) + 1e-3
    for i in range(n):
        if i % 2 == 0 or n < 6:
            a[i] = special[(i // 2 if n >= 6 else i) % 5]
        if i % 3 == 0:
            sigma[i] = s_lo if (i // 3) % 2 == 0 else s_hi
    if n == 1:
        sigma[0] = s_lo
    mu = torch.randn(n, generator=g)
    shape = (B, H, A)
    return (mu.view(shape), sigma.view(shape), a.view(shape), torch.randn(B, H, generator=g) * 3,
            torch.randn(B, H + 1, generator=g) * 3)


@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("B,H", [(1, 1), (127, 1), (16, 8), (43, 3)])
def test_actor_loss_grad(gpu, B, H, A):
    """g_mus, g_sigmas elementwise and loss_out[0] against float64 autograd at
    B H in {1, 127, 128, 129} (one workgroup takes 128 rows), actions of exactly
    +-1, 0 and +-(1 - 1e-7), sigma at both ends of the actor head's range, norm
    in {1, 37.5}, nu in {0, 3e-4} and a scale that is not 1 / (B H).

    Bound: K 2^-24 times the condition-weighted magnitude of the output, i.e.
    the output's formula with every difference replaced by the sum of its
    operands' magnitudes: with G = scale (|nu| + (|R| + |V|) / norm), D = |x| +
    |mu|: g_mu: G D / sigma^2; g_sigma: G (D^2 / sigma^3 + 1 / sigma); loss: the
    mean over rows of (|nu| + (|R| + |V|) / norm) times the summed magnitudes of
    the log-prob's terms.  K = twice the float32 operations on the output's
    path, counted above: K_MU = 18, K_SIGMA = 26, K_LOSS = 82; none was raised.
    Worst observed error / bound on the MI355X over all cases: g_mu 0.234,
    g_sigma 0.235, loss 0.016 (against the float64 references of
    primitives_ref.py)."""
    L, st = _api()
    mu, sigma, a, R, V = _actor_case(B, H, A, 1000 * B + 10 * H + A)
    dev = lambda t: t.to(gpu).contiguous()
    mud, sgd, ad, Rd, Vd = dev(mu), dev(sigma), dev(a), dev(R), dev(V)
    scale = 0.37 / (B * H)
    worst = [0.0, 0.0, 0.0]
    for norm in (1.0, 37.5):
        for nu in (0.0, 3e-4):
            normd = torch.tensor([norm], device=gpu)
            out = torch.full((1 + B * H,), float("nan"), device=gpu)
            gm, gs = torch.full_like(mud, float("nan")), torch.full_like(sgd, float("nan"))
            L.call("dr_actor_loss_grad", B, H, A, L.ptr(mud), L.ptr(sgd), L.ptr(ad), L.ptr(Rd), L.ptr(Vd), L.ptr(normd),
                   nu, scale, L.ptr(out), L.ptr(gm), L.ptr(gs), st)
            torch.cuda.synchronize()
            want_loss, want_gm, want_gs = PR.actor_loss_and_grads(mu, sigma, a, R, V, norm, nu, scale)
            x = torch.atanh(PR.clamp_actions(a))
            D = x.abs() + mu.double().abs()
            s = sigma.double()
            adv_mag = abs(float(np.float32(nu))) + (R.double().abs() + V.double()[:, :-1].abs()) / norm
            G = (float(np.float32(scale)) * adv_mag).unsqueeze(-1)
            _, term_mag = PR.tanh_normal_logprob_terms(a, mu, sigma)
            bounds = (K_MU * U * G * D / s ** 2, K_SIGMA * U * G * (D * D / s ** 3 + 1 / s),
                      K_LOSS * U * (adv_mag * term_mag.sum(-1)).mean())
            errs = ((gm.cpu().double() - want_gm).abs(), (gs.cpu().double() - want_gs).abs(),
                    (out[0].cpu().double() - want_loss).abs())
            ratios = [float((e / bd.clamp_min(1e-300)).max()) for e, bd in zip(errs, bounds)]
            worst = [max(w, r) for w, r in zip(worst, ratios)]
            for what, e, bd, r in zip(("g_mus", "g_sigmas", "loss"), errs, bounds, ratios):
                assert bool((e <= bd).all()), f"{what} norm={norm} nu={nu}: worst err/bound {r:.3g}"
    print(f"dr_actor_loss_grad B={B} H={H} A={A}: worst err/bound g_mu {worst[0]:.3g} g_sigma {worst[1]:.3g} "
          f"loss {worst[2]:.3g}")


@pytest.mark.parametrize("B,H,A", [(0, 1, 3), (1, 0, 3), (1, 1, 0), (-1, 1, 3)])
def test_actor_loss_grad_refuses_bad_dims(gpu, B, H, A):
    L, st = _api()
    t = torch.ones(64, device=gpu)
    with pytest.raises(L.HipError):
        L.call("dr_actor_loss_grad", B, H, A, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 3e-4, 1.0,
               L.ptr(t), L.ptr(t), L.ptr(t), st)
