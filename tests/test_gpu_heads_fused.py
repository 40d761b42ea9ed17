"""The grouped first Linear of the heads that read the imagined states (op_gemm_nt_split3_heads through
dr_internal_s3_heads_run) against float64, and dr_heads_fwd against the separate entry points.

Every output sits in a store poisoned with gemm_ref.SENT (a quiet NaN no kernel computes) and must keep those bits
outside the region the op writes: past column N of every row (ldy = N + 4), in GUARD floats before the first row and
in the rows after the last.  The bound is the project's split3 bound, gemm_ref.loose_bound: 1e-4 |ref| + 1e-5 max|ref|.
A head must hold the same bits in a group of 1, 2 or 4 heads: the K partition is a function of (M, K) alone."""
import ctypes

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = {"even": (200, 200, 200, 200), "mixed": (200, 72, 136, 8)}
KSEG = {"heads": (600, 1024), "small": (40, 64)}  # (the h segment, the z segment)
MS = (1024, 1024 + 40)
PAD_A = 8  # floats of input padding past each A segment's row (lda = k + PAD_A)


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_s3_heads_run
    f.restype = ctypes.c_int
    vp, ip, i = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int
    f.argtypes = [i, i, vp, i, vp, i, i, i, ip, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ip, vp, vp,
                  ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), vp, ctypes.c_char_p, i]
    return f


def _needs(M, K, widths):
    need = (ctypes.c_longlong * 3)(-1, -1, -1)
    rc = _hook()(M, K, None, 0, None, 0, 0, len(widths), (ctypes.c_int * len(widths))(*widths), None, None, None, None,
                 None, None, 0, need, None, None, 0)
    assert rc == 0
    return int(need[0]), int(need[1]), int(need[2])


def _poisoned(n, dev):
    return torch.full((n,), R.SENT, dtype=torch.int32, device=dev).view(torch.float32)


class _Operands:
    """A = [h | z] of the tallest M, four heads' weights and biases, and the float64 products: made once per K."""

    def __init__(self, kseg, dev):
        g = torch.Generator().manual_seed(11 + kseg[0])
        Mx = max(MS)
        self.ks, self.kz = kseg
        self.K = self.ks + self.kz
        self.h = torch.full((Mx, self.ks + PAD_A), R.PAD_IN)
        self.z = torch.full((Mx, self.kz + PAD_A), R.PAD_IN)
        self.h[:, :self.ks] = torch.randn(Mx, self.ks, generator=g)
        self.z[:, :self.kz] = torch.randn(Mx, self.kz, generator=g)
        nmax = max(max(w) for w in WIDTHS.values())
        self.W = [(torch.randn(nmax, self.K, generator=g) / self.K ** 0.5) for _ in range(4)]
        self.b = [torch.randn(nmax, generator=g) for _ in range(4)]
        A64 = torch.cat([self.h[:, :self.ks], self.z[:, :self.kz]], 1).double()
        self.ref = [A64 @ self.W[i].double().T + self.b[i].double() for i in range(4)]  # [Mx][nmax]
        self.h_d, self.z_d = self.h.to(dev), self.z.to(dev)
        self.W_d = [w.to(dev) for w in self.W]
        self.b_d = [b.to(dev) for b in self.b]


_OPS = {}


def _operands(name, dev):
    if name not in _OPS:
        _OPS[name] = _Operands(KSEG[name], dev)
    return _OPS[name]


def _run_group(op, M, heads, widths, dev):
    """heads: indices into op.W; widths: their N.  Returns the stores [GUARD + (M + 2) * ldy] after the run."""
    from dreamer_amd import hip
    nh = len(heads)
    wb, pf, splits = _needs(M, op.K, widths)
    wr = torch.empty(max(wb, 256), dtype=torch.uint8, device=dev)
    part = _poisoned(max(pf, 64), dev)
    ldy = [n + 4 for n in widths]
    stores = [_poisoned(R.GUARD + (M + 2) * ld, dev) for ld in ldy]
    # the first N rows of a head's [nmax][K] weight are that head at width N (contiguous rows, row stride K)
    vp = ctypes.c_void_p
    Wp = (vp * nh)(*[op.W_d[i].data_ptr() for i in heads])
    bp = (vp * nh)(*[op.b_d[i].data_ptr() for i in heads])
    Yp = (vp * nh)(*[s.data_ptr() + 4 * R.GUARD for s in stores])
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(M, op.K, op.h_d.data_ptr(), op.ks + PAD_A, op.z_d.data_ptr(), op.kz + PAD_A, op.ks, nh,
                 (ctypes.c_int * nh)(*widths), Wp, bp, Yp, (ctypes.c_int * nh)(*ldy), wr.data_ptr(), part.data_ptr(), pf,
                 None, hip.stream(), msg, 256)
    torch.cuda.synchronize()
    assert rc == 0, msg.value.decode()
    return [s.cpu() for s in stores], ldy, splits


def _split(store, M, N, ld):
    """(the written block [M][N], the int32 view of everything else)."""
    body = store[R.GUARD:].view(M + 2, ld)
    mask = torch.ones_like(store, dtype=torch.bool)
    mask[R.GUARD:].view(M + 2, ld)[:M, :N] = False
    return body[:M, :N], store.view(torch.int32)[mask]


@pytest.mark.parametrize("kname", sorted(KSEG))
@pytest.mark.parametrize("wname", sorted(WIDTHS))
@pytest.mark.parametrize("M", MS)
def test_grouped_first_linear_matches_float64_and_the_group_of_one(M, wname, kname, gpu):
    op = _operands(kname, gpu)
    W = WIDTHS[wname]
    alone = {}
    for nh in (1, 2, 4):
        groups = [[i] for i in range(4)] if nh == 1 else [list(range(nh))]
        for heads in groups:
            widths = [W[i] for i in heads]
            stores, ldy, splits = _run_group(op, M, heads, widths, gpu)
            for j, i in enumerate(heads):
                got, rest = _split(stores[j], M, widths[j], ldy[j])
                assert bool((rest == R.SENT).all()), f"head {i} of {nh}: the store changed outside [M][N]"
                ref = op.ref[i][:M, :widths[j]]
                d = (got.double() - ref).abs()
                bound = R.loose_bound(ref)
                print(f"M {M} K {op.K} widths {wname} group {nh} head {i}: splits {splits}, max err {float(d.max()):.3e}, "
                      f"worst err / bound {float((d / bound).max()):.3g}")
                assert not bool((d > bound).any()), f"head {i} of {nh}: max err {float(d.max()):.3e}"
                if nh == 1:
                    alone[i] = got.clone()
                else:
                    assert torch.equal(got.view(torch.int32), alone[i].view(torch.int32)), \
                        f"head {i} in a group of {nh} differs from the group of one"


def _heads_engine(B, H, dev):
    from gpu_helpers import build
    from dreamer_amd.engine import ImaginationEngine
    d, _ = build("full", dev, B=B, H=H)
    eng = ImaginationEngine(d, use_graph=False)
    g = torch.Generator().manual_seed(5)
    dm = eng.d
    idx = torch.randint(0, dm.cols, (B, dm.rows), generator=g)
    z0 = torch.nn.functional.one_hot(idx, dm.cols).float().reshape(B, -1)
    eng.z0.copy_(z0)
    eng.h0.copy_(torch.tanh(torch.randn(B, dm.hidden, generator=g)))
    return d, eng


def _tape_fields(eng):
    """The critic tape as dr_critic_loss_bwd reads it: pre1, x1, pre2, x2, logits, in the carve's order."""
    return eng.ctape.clone()


def test_heads_fwd_equals_the_separate_entry_points(gpu):
    """B = 68, H = 15 (M = 1088): rewards, continues, V_t, V_c and the whole online critic tape of dr_heads_fwd are
    the bits of dr_imagine_fwd's heads plus two dr_critic_fwd calls on the same imagined states."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, H = 68, 15
    d, eng = _heads_engine(B, H, gpu)
    assert eng.heads_fused and L.query("dr_heads_supported", eng.d, B, H) == 1
    dm = eng.d
    g = torch.Generator().manual_seed(6)
    eps = torch.randn(H, B, dm.action, generator=g).to(gpu)
    q = torch.empty(H, B * dm.rows, dm.cols).exponential_(generator=g).to(gpu)
    poison = lambda t: t.view(torch.int32).fill_(R.SENT)
    for t in (eng.rewards, eng.continues, eng.V_t, eng.V_c):
        poison(t)
    eng.ctape.fill_(0xFF)
    eng.imagine(eps=eps, q=q)
    torch.cuda.synchronize()
    assert eng.heads_done
    fused = {k: getattr(eng, k).clone() for k in ("rewards", "continues", "V_t", "V_c", "latents", "hiddens")}
    fused_tape = _tape_fields(eng)
    for k in ("rewards", "continues", "V_t", "V_c"):
        assert bool(torch.isfinite(fused[k]).all()), k
    # the separate entry points on the same tree
    eng.heads_fused = False
    for t in (eng.rewards, eng.continues, eng.V_t, eng.V_c):
        poison(t)
    eng.ctape.fill_(0xFF)
    eng.imagine(eps=eps, q=q)
    assert not eng.heads_done
    M, L_ = B * (H + 1), dm.rows * dm.cols
    ag = d.agent
    L.call("dr_critic_fwd", dm, ag.critic_struct(target=True), M, L.ptr(eng.hiddens), dm.hidden, L.ptr(eng.latents), L_,
           None, L.ptr(eng.V_t), None, L.ptr(eng.ws_cr), eng.ws_cr.numel(), hip.stream())
    L.call("dr_critic_fwd", dm, ag.critic_struct(), M, L.ptr(eng.hiddens), dm.hidden, L.ptr(eng.latents), L_, None,
           L.ptr(eng.V_c), L.ptr(eng.ctape), L.ptr(eng.ws_cr), eng.ws_cr.numel(), hip.stream())
    torch.cuda.synchronize()
    for k in fused:
        assert torch.equal(fused[k].view(torch.int32), getattr(eng, k).view(torch.int32)), k
    # the whole tape (pre1, x1, pre2, x2, logits; any carve padding keeps the 0xFF fill in both runs)
    assert torch.equal(fused_tape, eng.ctape), "critic tape"
    assert not bool((fused_tape.view(torch.int32)[:M * dm.critic_h1] == -1).any()), "the tape was not written"


def test_heads_fwd_reports_unsupported_and_writes_nothing(gpu):
    """B = 3, H = 2: 9 states, below the split3 first layer's 1024 rows."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, H = 3, 2
    d, eng = _heads_engine(B, H, gpu)
    assert not eng.heads_fused and L.query("dr_heads_supported", eng.d, B, H) == 0
    assert L.query("dr_heads_workspace_bytes", eng.d, B, H) == 0
    eng.imagine()
    torch.cuda.synchronize()
    outs = [eng.rewards, eng.continues, eng.V_t, eng.V_c]
    for t in outs:
        t.view(torch.int32).fill_(R.SENT)
    eng.ctape.fill_(0xFF)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    ag = d.agent
    with pytest.raises(L.HipError) as e:
        L.call("dr_heads_fwd", eng.d, d.world_model.packed(), ag.critic_struct(target=True), ag.critic_struct(), B, H,
               L.ptr(eng.latents), L.ptr(eng.hiddens), L.ptr(eng.rewards), L.ptr(eng.continues), L.ptr(eng.V_t),
               L.ptr(eng.V_c), L.ptr(eng.ctape), L.ptr(eng.ws_im), eng.ws_im.numel(), L.ptr(eng.ws_cr),
               eng.ws_cr.numel(), L.ptr(ws), ws.numel(), hip.stream())
    assert e.value.code == L.DR_E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.int32) == R.SENT).all())
    assert bool((eng.ctape == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------------
# the fused tail (k_heads_tail through dr_internal_heads_tail_run)
# ------------------------------------------------------------------------------------------------------------------
TAIL_N = (255, 1, 7, 255)      # reward-like (value only), continue-like (sigmoid), small bucket head, critic-like
TAIL_ACT = (0, 2, 0, 0)
TAIL_CHAIN1 = (0, 0, 0, 1)     # head 3 sums like the tile GEMM the critics ran on (one accumulator chain)
TAIL_ROWMAP = {9: 3, 68: 4, 1030: 5}  # rm_h1 of head 0 (rm_k0 = 1): its values land in a [M / h1][h1 - 1] layout
ROW_CONST, ROW_NAN = 1, 3      # needles: a constant row (0.5: its mean is exact, its variance zero), a NaN row


def _tail_hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_heads_tail_run
    f.restype = ctypes.c_int
    vp, i = ctypes.c_void_p, ctypes.c_int
    f.argtypes = [i, i, ctypes.POINTER(i), ctypes.POINTER(vp), i, vp, ctypes.c_char_p, i]
    return f


def _silu(x):
    return x * torch.sigmoid(x)


def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


class _TailCase:
    """Four heads of hidden width `wd` over the same M rows, and their float64 results: made once per (M, wd)."""

    def __init__(self, M, wd, dev):
        g = torch.Generator().manual_seed(100 * M + wd)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.M, self.wd = M, wd
        self.heads = []
        for h, N in enumerate(TAIL_N):
            X = rn(M, wd)
            X[ROW_CONST] = 0.5
            X[ROW_NAN] = float("nan")
            p = dict(X=X, ln1_g=1 + 0.1 * rn(wd), ln1_b=0.1 * rn(wd), W3=rn(wd, wd) / wd ** 0.5, b3=0.1 * rn(wd),
                     ln4_g=1 + 0.1 * rn(wd), ln4_b=0.1 * rn(wd), W6=rn(N, wd) / wd ** 0.5, b6=0.1 * rn(N),
                     buckets=torch.linspace(-3, 3, N) if N > 1 else torch.zeros(1))
            if N == 7:  # logits near +80 and -80
                p["b6"][0], p["b6"][1] = 80.0, -80.0
            d = {k: v.double() for k, v in p.items()}
            x1 = _silu(_ln(d["X"], d["ln1_g"], d["ln1_b"]))
            pre2 = x1 @ d["W3"].T + d["b3"]
            x2 = _silu(_ln(pre2, d["ln4_g"], d["ln4_b"]))
            out = x2 @ d["W6"].T + d["b6"]
            e = (torch.softmax(out, -1) * d["buckets"]).sum(-1)
            ref = dict(x1=x1, pre2=pre2, x2=x2, Y=torch.sigmoid(out) if TAIL_ACT[h] == 2 else out,
                       val=torch.sign(e) * torch.expm1(e.abs()))
            self.heads.append((p, {k: v.to(dev) for k, v in p.items()}, ref))


_TAILS = {}


def _tail_case(M, wd, dev):
    if (M, wd) not in _TAILS:
        _TAILS[(M, wd)] = _TailCase(M, wd, dev)
    return _TAILS[(M, wd)]


def _run_tail(case, heads, outs, rowmap, old_path, dev):
    """outs[h]: the names among Y, val, x1, pre2, x2 that head h stores.  Returns {h: {name: inner store on the CPU}}
    after checking that the GUARD floats either side of every store kept their bits."""
    from dreamer_amd import hip
    M, wd = case.M, case.wd
    nh = len(heads)
    v, p, st = [], [], {}
    for h in heads:
        N = TAIL_N[h]
        _, dv, _ = case.heads[h]
        h1 = rowmap.get(h, 0)
        rows = M if not h1 else (M // h1) * (h1 - 1)
        size = dict(Y=rows * N, val=rows, x1=M * wd, pre2=M * wd, x2=M * wd)
        st[h] = {k: _poisoned(size[k] + 2 * R.GUARD, dev) for k in outs[h]}
        ptr = lambda k: st[h][k].data_ptr() + 4 * R.GUARD if k in st[h] else None
        v += [wd, wd, N, TAIL_ACT[h], h1, 1 if h1 else 0, 0 if old_path else TAIL_CHAIN1[h], 0]
        p += [dv["X"].data_ptr(), dv["ln1_g"].data_ptr(), dv["ln1_b"].data_ptr(), dv["W3"].data_ptr(),
              dv["b3"].data_ptr(), dv["ln4_g"].data_ptr(), dv["ln4_b"].data_ptr(), dv["W6"].data_ptr(),
              dv["b6"].data_ptr(), dv["buckets"].data_ptr() if "val" in outs[h] else None, ptr("Y"), ptr("val"),
              ptr("x1"), ptr("pre2"), ptr("x2"), None]
    msg = ctypes.create_string_buffer(256)
    rc = _tail_hook()(M, nh, (ctypes.c_int * len(v))(*v), (ctypes.c_void_p * len(p))(*p), int(old_path), hip.stream(),
                      msg, 256)
    torch.cuda.synchronize()
    assert rc == 0, msg.value.decode()
    res = {}
    for h in heads:
        res[h] = {}
        for k, t in st[h].items():
            c = t.cpu()
            gi = c.view(torch.int32)
            assert bool((gi[:R.GUARD] == R.SENT).all()) and bool((gi[-R.GUARD:] == R.SENT).all()), (h, k, "guard")
            res[h][k] = c[R.GUARD:-R.GUARD]
    return res


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("wd", (200, 72))
@pytest.mark.parametrize("M", (9, 68, 1030))
def test_fused_tail_matches_float64_and_the_tail_it_succeeds(M, wd, gpu):
    case = _tail_case(M, wd, gpu)
    full = ("Y", "val", "x1", "pre2", "x2")
    # the launches k_heads_tail succeeds, head by head: k_mlp2_tail (+ k_bucket_value), every store on
    old = _run_tail(case, [0, 1, 2, 3], {0: full, 1: ("Y", "x1", "pre2", "x2"), 2: full, 3: full}, {}, True, gpu)
    # fused: head 0 stores its values only, through a row map; head 1 the sigmoid; head 2 logits and values; head 3
    # (saves on, beside heads whose saves are off) logits, values and the tape's three saves
    outs = {0: ("val",), 1: ("Y",), 2: ("Y", "val"), 3: full}
    h1 = TAIL_ROWMAP[M]
    runs = {nh: _run_tail(case, list(range(nh)), outs, {0: h1}, False, gpu) for nh in (1, 3, 4)}
    rows = torch.arange(M)
    live = rows != ROW_NAN
    mapped = rows[(rows % h1 >= 1) & (rows < (M // h1) * h1)]  # head 0's rows, in the order of its [B][h1 - 1] store
    for nh, got in runs.items():
        for h in range(nh):
            _, _, ref = case.heads[h]
            N = TAIL_N[h]
            for k in outs[h]:
                g = got[h][k]
                assert _same_bits(g, runs[1 if h == 0 else max(h + 1, 3)][h][k]), f"{nh} heads: head {h} {k} changed"
                if nh != max(h + 1, 3) and h > 0:
                    continue  # the same bits as the run compared below
                sel = mapped if (h == 0 and k == "val") else rows
                assert g.numel() == len(sel) * (ref[k].shape[1] if ref[k].dim() > 1 else 1), (h, k, "an unwritten row")
                g2 = g.view(len(sel), -1)
                r2 = ref[k][sel].reshape(len(sel), -1)
                o2 = old[h][k].view(M, -1)[sel]
                if not TAIL_CHAIN1[h]:  # (head 3's order is the tile GEMM's: test_fused_tails_keep_the_bits_...)
                    assert _same_bits(g2, o2), f"head {h} {k}: differs from k_mlp2_tail / k_bucket_value"
                nan_rows = sel == ROW_NAN
                # (the NaN row's value is whatever k_bucket_value makes of NaN logits -- its symexp clamps the
                # argument, so it is finite -- and was held to those bits above; every other store of the row is NaN)
                assert k == "val" or bool(torch.isnan(g2[nan_rows]).all()), f"head {h} {k}: the NaN row"
                if k == "val":
                    assert _same_bits(g2[nan_rows], o2[nan_rows]), f"head {h} val: the NaN row"
                ok = ~nan_rows
                assert bool(torch.isfinite(g2[ok]).all()), f"head {h} {k}: the NaN row leaked"
                d = (g2[ok].double() - r2[ok]).abs()
                bound = R.loose_bound(r2[ok])
                print(f"M {M} width {wd} N {N} head {h} {k}: max err {float(d.max()):.3e}, worst err / bound "
                      f"{float((d / bound.clamp_min(1e-300)).max()):.3g}")
                assert not bool((d > bound).any()), f"head {h} {k}: max err {float(d.max()):.3e}"
    assert live.sum() == M - 1


def test_fused_tails_keep_the_bits_of_the_launches_they_succeed(gpu):
    """B = 256, H = 15, the bench shape: with the fused tail switched off (dr_internal_heads_tail_enable(0)) the four
    heads run k_mlp2_tail, the critics' k_ln_silu_rows + tile GEMM layers, k_bucket_value and the copies, as before
    k_heads_tail; every output of dr_heads_fwd and of the single-head dr_critic_fwd must hold the same bits either way."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    B, H = 256, 15
    d, eng = _heads_engine(B, H, gpu)
    assert eng.heads_fused
    dm = eng.d
    g = torch.Generator().manual_seed(8)
    eps = torch.randn(H, B, dm.action, generator=g).to(gpu)
    q = torch.empty(H, B * dm.rows, dm.cols).exponential_(generator=g).to(gpu)
    sw = L.load().dr_internal_heads_tail_enable
    sw.restype, sw.argtypes = ctypes.c_int, [ctypes.c_int]
    M, L_ = B * (H + 1), dm.rows * dm.cols
    ag = d.agent
    V2, tape2 = torch.zeros_like(eng.V_c), torch.zeros_like(eng.ctape)

    def run():
        for t in (eng.rewards, eng.continues, eng.V_t, eng.V_c, V2):
            t.view(torch.int32).fill_(R.SENT)
        eng.ctape.fill_(0xFF)
        tape2.fill_(0xFF)
        eng.imagine(eps=eps, q=q)
        L.call("dr_critic_fwd", dm, ag.critic_struct(), M, L.ptr(eng.hiddens), dm.hidden, L.ptr(eng.latents), L_, None,
               L.ptr(V2), L.ptr(tape2), L.ptr(eng.ws_cr2), eng.ws_cr2.numel(), hip.stream())
        torch.cuda.synchronize()
        return [t.clone() for t in (eng.rewards, eng.continues, eng.V_t, eng.V_c, eng.ctape, V2, tape2)]

    new = run()
    assert sw(0) == 1
    try:
        old = run()
    finally:
        sw(1)
    for name, a, b in zip(("rewards", "continues", "V_t", "V_c", "tape", "V_c alone", "tape alone"), new, old):
        assert bool(torch.isfinite(a).all()) if a.dtype == torch.float32 else True, name
        assert torch.equal(a.view(torch.uint8).reshape(-1), b.view(torch.uint8).reshape(-1)), name
    assert torch.equal(new[3], new[5]) and torch.equal(new[4], new[6]), "the single-head critic differs from the group"
