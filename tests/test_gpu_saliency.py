"""Perturbation saliency on the GPU (include/dreamer_hip.h "perturbation
saliency", dreamer_amd/saliency.py): dr_occlude_frames against the
f32-emulating numpy reference, dr_saliency_scores and dr_saliency_map against
float64, Dreamer.saliency_frames against its stages called by hand (bit for
bit) and against the CPU oracle, and the replay-window front end.

The u8 rule of the occluder and the overlay: the output equals the
f32-emulating reference except where the float64 value lies within 1e-3 of a
half-integer; there it may differ by one level, and such pixels are at most
0.5 % of a case's pixels.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

import saliency_ref as SR
from formula import FULL, SMALL, replay_data
from gpu_helpers import build, close, cpu
from oracle import dreamer_oracle as O
from test_gpu_agent_trace import _close1e4
from test_gpu_closed_loop import _noise, _oracle, _rel, _stats_bounds
from test_gpu_open_loop import A, N_FILL, _same, _windows

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB


# ---------------------------------------------------------------- the occluder
def _patterns(H, W, which):
    rng = np.random.default_rng(H * 1000 + W)
    y, x = np.mgrid[0:H, 0:W]
    noise = rng.integers(0, 256, size=(3, H, W), dtype=np.uint8)
    const = np.stack([np.full((H, W), v, dtype=np.uint8) for v in (137, 0, 255)])
    ramp = np.stack([(x * 255) // (W - 1), (y * 255) // (H - 1), ((x + y) * 255) // (H + W - 2)]).astype(np.uint8)
    check = np.stack([(((x + y) & 1) * 255), (((x // 2 + y // 3) & 1) * 255), ((x & 1) * 255)]).astype(np.uint8)
    return np.stack({"a": (noise, const, ramp), "b": (check, noise[::-1], ramp[:, ::-1, ::-1])}[which])


def _ring(frames, gpu, offset=0, t0=1):
    """The F frames behind a wrapped ring of F + 1 slots, frame f at slot
    (starts[f] + t0) % cap; the ring's base `offset` bytes past an aligned one."""
    from dreamer_amd import _lib as L
    Fn = frames.shape[0]
    n = frames[0].size
    cap = Fn + 1
    starts = (np.arange(Fn) + cap - 2) % cap  # 2, 3, 0 for F = 3: slots 3, 0, 1 at t0 = 1
    host = np.random.default_rng(7).integers(0, 256, size=(cap, n), dtype=np.uint8)
    host[(starts + t0) % cap] = frames.reshape(Fn, n)
    buf = torch.zeros(cap * n + 64, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    ring = buf[offset:offset + cap * n]
    ring.copy_(torch.from_numpy(host.reshape(-1)))
    st = torch.from_numpy(starts.astype(np.int64)).to(gpu)
    return L.dr_frames(L.ptr(ring), cap, L.ptr(st), None, 0, 0, 1, t0), (buf, ring, st)


def _dims(H, W):
    from dreamer_amd import _lib as L
    d = L.dr_dims()
    d.img_h, d.img_w = H, W
    return d


def _occlude(gpu, frames, s, fill, wb, rb, gm, offset=0, out_offset=0):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    Fn, _, H, W = frames.shape
    G = (H // s) * (W // s)
    d = _dims(H, W)
    src, keep = _ring(frames, gpu, offset)
    total = Fn * (G + 1) * 3 * H * W
    obuf = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device=gpu)
    out = obuf[out_offset:out_offset + total]
    ws = torch.empty(L.query("dr_occlude_workspace_bytes", d, Fn), dtype=torch.uint8, device=gpu)
    wbd = None if wb is None else torch.from_numpy(wb).to(gpu)
    gmd = torch.from_numpy(gm).to(gpu)
    L.call("dr_occlude_frames", d, src, Fn, s, {"blur": 0, "mean": 1}[fill], L.ptr(wbd), rb, L.ptr(gmd), L.ptr(out),
           L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    assert bool((obuf[:out_offset] == SENTINEL).all()) and bool((obuf[out_offset + total:] == SENTINEL).all())
    return out.cpu().numpy().reshape(Fn, G + 1, 3, H, W)


def _check_u8(got, ref32, ref64, guard, what):
    """The u8 rule of the module text."""
    diff = got != ref32
    share = float(guard.mean())
    print(f"{what}: {int(diff.sum())} of {got.size} pixels off the f32 reference, guarded share {share:.4%}, "
          f"f32 vs float64 reference differ at {int((ref32 != ref64).sum())}")
    assert not bool((diff & ~guard).any()), f"{what}: {int((diff & ~guard).sum())} unguarded pixels differ"
    assert int(np.abs(got.astype(np.int16) - ref32.astype(np.int16)).max()) <= 1, what
    assert share <= 0.005, (what, share)


def _tables(H, W):
    from dreamer_amd.saliency import blur_taps, default_mask_sigma, mask_profile
    wb, rb = blur_taps(3.0)
    return wb, rb, mask_profile(default_mask_sigma(H), max(H, W))


CASES = [(16, 16, 4), (32, 32, 8), (24, 40, 8), (64, 64, 4), (128, 128, 16)]


@pytest.mark.parametrize("pattern", ["a", "b"])
@pytest.mark.parametrize("fill", ["blur", "mean"])
@pytest.mark.parametrize("HWs", CASES, ids=lambda c: "x".join(map(str, c)))
def test_occluder_matches_reference(HWs, fill, pattern, gpu):
    """F = 3 frames (uniform noise, constant, ramp / checkerboard, noise, ramp)
    behind a wrapped ring with t0 = 1.  sigma_b = 3 (rb = 9): at H = 16 the taps
    reach past both borders.  W = 40 takes the plain path, the others the
    16-byte one."""
    H, W, s = HWs
    frames = _patterns(H, W, pattern)
    wb, rb, gm = _tables(H, W)
    got = _occlude(gpu, frames, s, fill, wb, rb, gm)
    ref64, guard = SR.occlude64(frames, s, fill, wb, rb, gm)
    _check_u8(got, SR.occlude32(frames, s, fill, wb, rb, gm), ref64, guard, f"occlude {HWs} {fill} {pattern}")
    assert np.array_equal(got[:, 0], frames)  # variant 0 is the frame


@pytest.mark.parametrize("fill", ["blur", "mean"])
@pytest.mark.parametrize("offsets", [(4, 0), (0, 4), (16, 16)], ids=["ring+4", "out+4", "both+16"])
def test_occluder_unaligned_base(offsets, fill, gpu):
    """A ring or an output base that is not 16-byte aligned takes the plain
    path: the same bytes as the aligned call."""
    H, W, s = 32, 32, 8
    frames = _patterns(H, W, "a")
    wb, rb, gm = _tables(H, W)
    got = _occlude(gpu, frames, s, fill, wb, rb, gm, offset=offsets[0], out_offset=offsets[1])
    assert np.array_equal(got, _occlude(gpu, frames, s, fill, wb, rb, gm))
    ref64, guard = SR.occlude64(frames, s, fill, wb, rb, gm)
    _check_u8(got, SR.occlude32(frames, s, fill, wb, rb, gm), ref64, guard, f"occlude unaligned {offsets} {fill}")


def test_occluder_position_independent(gpu):
    """A frame's variants are the same bytes alone and at another position of the batch."""
    H, W, s = 32, 32, 8
    frames = _patterns(H, W, "a")
    wb, rb, gm = _tables(H, W)
    whole = _occlude(gpu, frames, s, "blur", wb, rb, gm)
    again = _occlude(gpu, frames[::-1].copy(), s, "blur", wb, rb, gm)
    assert np.array_equal(whole, again[::-1])
    assert np.array_equal(whole[2:3], _occlude(gpu, frames[2:3], s, "blur", wb, rb, gm))


def test_occluder_refusals_write_nothing(gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    H, W = 32, 32
    frames = _patterns(H, W, "a")
    wb, rb, gm = _tables(H, W)
    src, keep = _ring(frames, gpu)
    out = torch.full((3 * 17 * 3 * H * W,), SENTINEL, dtype=torch.uint8, device=gpu)
    ws = torch.full((3 * 3 * H * W * 4,), SENTINEL, dtype=torch.uint8, device=gpu)
    wbd, gmd = torch.from_numpy(np.resize(wb, 40)).to(gpu), torch.from_numpy(gm).to(gpu)
    f32 = torch.zeros(3, 3, H, W, device=gpu)
    d64 = _dims(64, 64)
    vec = _dims(H, W)
    vec.obs_dim = 12
    INV, UNS = L.DR_E_INVALID, L.DR_E_UNSUPPORTED
    cases = [(INV, _dims(H, W), src, 8, 0, wbd, 16, gmd),   # rb > 15
             (INV, d64, src, 1, 0, wbd, rb, gmd),            # G > 1024
             (INV, _dims(H, W), src, 5, 0, wbd, rb, gmd),    # the stride does not divide the frame
             (INV, _dims(H, W), src, 8, 0, None, rb, gmd),   # a table is NULL
             (INV, _dims(H, W), src, 8, 0, wbd, rb, None),
             (INV, _dims(H, W), src, 8, 1, None, rb, None),
             (UNS, _dims(H, W), L.dr_frames(None, 0, None, L.ptr(f32), 3 * H * W, 0, 1, 0), 8, 0, wbd, rb, gmd),
             (UNS, vec, src, 8, 0, wbd, rb, gmd)]
    for code, d, s_, stride, fill, w_, r_, g_ in cases:
        with pytest.raises(L.HipError) as e:
            L.call("dr_occlude_frames", d, s_, 3, stride, fill, L.ptr(w_), r_, L.ptr(g_), L.ptr(out), L.ptr(ws),
                   ws.numel(), hip.stream())
        assert e.value.code == code, (stride, fill, r_, e.value)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())


# ------------------------------------------------------------------ the scores
def _scores(gpu, F, G, A_, R, C, mu, V, logits, z, want=(0, 1, 2, 3, 4)):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    dv = [t.contiguous().to(gpu) for t in (mu, V, logits, z)]
    outs = [torch.full((F, G), float("nan"), device=gpu) for _ in range(4)] + \
        [torch.full((F, G), -7, dtype=torch.int32, device=gpu)]
    ptrs = [L.ptr(o) if k in want else None for k, o in enumerate(outs)]
    L.call("dr_saliency_scores", F, G, A_, R, C, *(L.ptr(t) for t in dv), *ptrs, hip.stream())
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("RC", [(8, 8), (32, 32)])
@pytest.mark.parametrize("A_", [1, 3, 17])
@pytest.mark.parametrize("G", [1, 5, 256])
def test_scores_kernel(G, A_, RC, gpu):
    """dr_saliency_scores on synthetic rows against float64.  actor and value:
    rtol 1e-5 (an exact-input f32 subtraction, then at most A + 2 roundings of
    2^-24 each); posterior_kl: test_gpu_closed_loop's bound for
    dr_latent_stats' kl; value_delta the f32 subtraction's bits; flips exact."""
    R, C = RC
    F = 2
    M = F * (G + 1)
    g = torch.Generator().manual_seed(1000 * G + 10 * A_ + R)
    mu, V = torch.randn(M, A_, generator=g), torch.randn(M, generator=g) * 5
    logits = torch.randn(M, R, C, generator=g) * 3
    idx = torch.randint(0, C, (M, R), generator=g)
    last = M - 1  # variant G of frame 1
    # identical rows: the last variant of frame 1 is its variant 0
    mu[last], V[last], logits[last], idx[last] = mu[G + 1], V[G + 1], logits[G + 1], idx[G + 1]
    # logits +-30: frame 0's variant 1 peaked, on another class in every second categorical
    logits[1] = -30.0
    logits[1, torch.arange(R), idx[1]] = 30.0
    if G >= 5:  # ... and against a peaked variant 0 of frame 1, the far variant peaked elsewhere
        logits[G + 1] = -30.0
        logits[G + 1, :, 0] = 30.0
        logits[G + 3] = -30.0
        logits[G + 3, :, 1] = 30.0
        logits[last] = logits[G + 1]
    z = torch.nn.functional.one_hot(idx, C).float()
    actor, value, delta, kl, flips = _scores(gpu, F, G, A_, R, C, mu, V, logits, z)
    r_actor, r_value, r_delta, r_kl, r_flips = SR.scores64(mu.numpy(), V.numpy(), logits.numpy(), z.numpy(), F, G, R, C)
    for name, got, ref in (("actor", actor, r_actor), ("value", value, r_value)):
        err = np.abs(got.numpy().astype(np.float64) - ref)
        rel = float((err / np.maximum(np.abs(ref), 1e-300)).max())
        print(f"scores G={G} A={A_} {RC} {name}: max rel err {rel:.3e}")
        assert bool((err <= 1e-5 * np.abs(ref)).all()), (name, rel)
    post = logits.view(F, G + 1, R, C)[:, :1].expand(F, G, R, C).reshape(F * G, R, C).contiguous()
    prior = logits.view(F, G + 1, R, C)[:, 1:].reshape(F * G, R, C).contiguous()
    (kl64, _, _), b_kl, _ = _stats_bounds(post, prior, f"scores G={G} {RC}")
    assert np.allclose(kl64.numpy(), r_kl.reshape(-1), rtol=1e-12, atol=1e-12)
    e_kl = _rel(kl.reshape(-1), kl64)
    print(f"scores G={G} A={A_} {RC} posterior_kl: max rel err {e_kl:.3e} (bound {b_kl:.3e})")
    assert e_kl <= b_kl
    Vn = V.numpy().reshape(F, G + 1)
    assert np.array_equal(delta.numpy(), (Vn[:, 1:] - Vn[:, :1]).astype(np.float32))
    assert np.array_equal(flips.numpy(), r_flips) and flips.dtype == torch.int32
    # identical rows give exactly 0 everywhere
    for t in (actor, value, delta, kl, flips):
        assert t[1, G - 1].item() == 0
    # any output may be NULL: the others keep their bits
    some = _scores(gpu, F, G, A_, R, C, mu, V, logits, z, want=(0, 3))
    assert torch.equal(some[0], actor) and torch.equal(some[3], kl)
    assert bool(torch.isnan(some[1]).all()) and bool((some[4] == -7).all())
    # a frame alone: the same bits
    one = _scores(gpu, 1, G, A_, R, C, mu[G + 1:], V[G + 1:], logits[G + 1:], z[G + 1:])
    for a, b in zip(one, (actor, value, delta, kl, flips)):
        assert torch.equal(a[0], b[1])


# --------------------------------------------------------------------- the map
@pytest.mark.parametrize("HWs", [(32, 32, 8), (24, 40, 8)], ids=lambda c: "x".join(map(str, c)))
def test_map_kernel(HWs, gpu):
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    H, W, s = HWs
    Gy, Gx = H // s, W // s
    Fn, ch = 3, 2
    rng = np.random.default_rng(H + W)
    S = (rng.random((Fn, Gy, Gx)) + 0.01).astype(np.float32)
    scale = np.array([1.0, 1.7, -0.5], dtype=np.float32)  # heat partly above 1; frame 2: heat 0 everywhere
    frames = _patterns(H, W, "a")
    src, keep = _ring(frames, gpu)
    Sd, sd = torch.from_numpy(S).to(gpu), torch.from_numpy(scale).to(gpu)
    m = torch.full((Fn, H, W), float("nan"), device=gpu)
    over = torch.full((Fn, 3, H, W), SENTINEL, dtype=torch.uint8, device=gpu)
    L.call("dr_saliency_map", _dims(H, W), Fn, s, L.ptr(Sd), L.ptr(sd), src, ch, L.ptr(m), L.ptr(over), hip.stream())
    m2 = torch.full((Fn, H, W), float("nan"), device=gpu)
    L.call("dr_saliency_map", _dims(H, W), Fn, s, L.ptr(Sd), L.ptr(sd), None, 0, L.ptr(m2), None, hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(m, m2)
    got, ref = m.cpu().numpy(), SR.map64(S, scale, H, W, s)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"map {HWs}: max rel err {float((err / np.abs(ref)).max()):.3e}")
    assert bool((err <= 1e-6 * np.abs(ref)).all())
    cy, cx = SR.centres(H, s), SR.centres(W, s)
    assert np.array_equal(got[:, cy[:, None], cx[None, :]], (scale[:, None, None] * S).astype(np.float32))
    ov = over.cpu().numpy()
    v32, v64 = SR.overlay_values(got, frames, ch)
    guard = np.abs(v64 - np.floor(v64) - 0.5) <= 1e-3
    _check_u8(ov[:, ch], SR.quantise(v32), SR.quantise(v64), guard, f"overlay {HWs}")
    for c in range(3):
        if c != ch:
            assert np.array_equal(ov[:, c], frames[:, c])
    assert np.array_equal(ov[2], frames[2]) and bool((ov[1, ch] == 255).any())


# ------------------------------------------------- saliency_frames is its stages
def _stages(d, frames, hiddens, su, q):
    """The six entry points by hand on the rows f (G + 1) + g of N device frames
    (N,3,H,W): a dict of everything they leave.  q: the frames' draws (N*R, C)."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    gpu = frames.device
    N = frames.shape[0]
    R, C = d.latent_state_dims
    Ad, Hd = d.action_dims, d.hidden_state_dims
    G, V1 = su.G, su.G + 1
    n = N * V1
    ag = d.agent
    ag._ensure_flat()
    dims, wm, st = d.world_model.dims(ag), d.world_model.packed(), hip.stream()
    buf = lambda nbytes: torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=gpu)
    starts = torch.arange(N, device=gpu, dtype=torch.int64)
    var = torch.empty(n, 3, su.H, su.W, dtype=torch.uint8, device=gpu)
    wb, gm = torch.from_numpy(su.wb).to(gpu), torch.from_numpy(su.gm).to(gpu)
    ws = buf(L.query("dr_occlude_workspace_bytes", dims, N))
    L.call("dr_occlude_frames", dims, L.dr_frames(L.ptr(frames), N, L.ptr(starts), None, 0, 0, 1, 0), N, su.stride,
           su.fill, L.ptr(wb), su.rb, L.ptr(gm), L.ptr(var), L.ptr(ws), ws.numel(), st)
    vstarts = torch.arange(n, device=gpu, dtype=torch.int64)
    feat = torch.empty(n, dims.enc_hidden, device=gpu)
    ws = buf(L.query("dr_encoder_workspace_bytes", dims, n))
    L.call("dr_encoder_features", dims, wm, L.dr_frames(L.ptr(var), n, L.ptr(vstarts), None, 0, 0, 1, 0), n, 1,
           L.ptr(feat), L.ptr(ws), ws.numel(), st)
    h_rep = hiddens.repeat_interleave(V1, dim=0).contiguous()
    q_rep = q.view(N, 1, R, C).expand(N, V1, R, C).reshape(n * R, C).contiguous()
    z, logits, h_out = (torch.empty(n, w, device=gpu) for w in (R * C, R * C, Hd))
    ws = buf(L.query("dr_observe_workspace_bytes", dims, n))
    L.call("dr_observe_scan", dims, wm, n, 1, L.ptr(feat), None, 0, 0, L.ptr(h_rep), None,
           hip.explicit_noise(q=q_rep, device=gpu), L.ptr(z), L.ptr(h_out), L.ptr(logits), L.ptr(ws), ws.numel(), st)
    a, mu, sg = (torch.empty(n, Ad, device=gpu) for _ in range(3))
    ws = buf(L.query("dr_actor_act_workspace_bytes", dims, n))
    L.call("dr_actor_act", dims, ag.actor_struct(), n, L.ptr(h_rep), L.ptr(z), L.dr_noise(), 1, L.ptr(a), L.ptr(mu),
           L.ptr(sg), L.ptr(ws), ws.numel(), st)
    V = torch.empty(n, device=gpu)
    ws = buf(L.query("dr_critic_workspace_bytes", dims, n, 0))
    L.call("dr_critic_fwd", dims, ag.critic_struct(), n, L.ptr(h_rep), Hd, L.ptr(z), R * C, None, L.ptr(V), None,
           L.ptr(ws), ws.numel(), st)
    sc = [torch.empty(N, G, device=gpu) for _ in range(4)] + [torch.empty(N, G, dtype=torch.int32, device=gpu)]
    L.call("dr_saliency_scores", N, G, Ad, R, C, L.ptr(mu), L.ptr(V), L.ptr(logits), L.ptr(z),
           *(L.ptr(t) for t in sc), st)
    torch.cuda.synchronize()
    g = lambda t: t.view(N, su.Gy, su.Gx)
    return dict(var=var, h_rep=h_rep, z=z, logits=logits, mu_rows=mu, V_rows=V, actor=g(sc[0]), value=g(sc[1]),
                value_delta=g(sc[2]), posterior_kl=g(sc[3]), latent_flips=g(sc[4]), mu=mu[::V1], sigma=sg[::V1],
                value_clean=V[::V1], latents=z[::V1].view(N, R, C))


FIELDS = ("actor", "value", "value_delta", "posterior_kl", "latent_flips", "mu", "sigma", "value_clean", "latents")


def _equal_fields(res, want, what):
    for k in FIELDS:
        a, b = getattr(res, k), want[k] if isinstance(want, dict) else getattr(want, k)
        assert a.shape == b.shape and torch.equal(a, b), (what, k)


@pytest.fixture(scope="module")
def small(gpu):
    d, P = build("small", gpu, B=2, H=3, S=8)
    # the fixture's mu head is the zero initialisation: every actor score would be 0.  Give it weights.
    g = torch.Generator().manual_seed(8)
    P = dict(P)
    for k in ("weight", "bias"):
        name = O.AG + "actor.mu_head." + k
        assert float(P[name].abs().max()) == 0.0
        P[name] = torch.randn(P[name].shape, generator=g) * 0.3
    d.load_state_dict({k: v.to(gpu) for k, v in P.items()})
    fr, ac, rw, ct = replay_data(N_FILL, tuple(SMALL["observation_dims"]), A, seed=0)
    d.buffer.load_arrays(fr, ac, rw, ct)
    return d, P, (fr, ac, rw, ct)


def _env_frames(N, H, W, seed):
    """Smooth-plus-noise u8 frames (N,H,W,3) as an environment gives them."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (127 + 100 * np.sin(x / 5.0 + np.arange(N)[:, None, None]) * np.cos(y / 7.0))[..., None]
    return np.clip(base + rng.integers(-40, 40, size=(N, H, W, 3)), 0, 255).astype(np.uint8)


def test_saliency_frames_is_its_stages(small, gpu):
    from dreamer_amd.saliency import setup
    d = small[0]
    N, s = 3, 8
    R, C = d.latent_state_dims
    frames = _env_frames(N, 32, 32, 1)
    hid = (torch.randn(N, d.hidden_state_dims, generator=torch.Generator().manual_seed(2)) * 0.5).to(gpu)
    su = setup(32, 32, s, "blur", 3.0, None)
    fd = torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 3, 1, 2))).to(gpu)
    with torch.no_grad():
        res = d.saliency_frames(frames, hid, stride=s)
        res_t = d.saliency_frames(fd, hid, stride=s, sample=False)
    torch.cuda.synchronize()
    want = _stages(d, fd, hid, su, torch.ones(N * R, C, device=gpu))
    _equal_fields(res, want, "mode")
    _equal_fields(res_t, want, "device frames")
    assert torch.equal(res.frames, fd) and res.stride == s and res.actor.shape == (N, 4, 4)
    assert res.latent_flips.dtype == torch.int32
    for k in FIELDS:
        assert bool(torch.isfinite(getattr(res, k).float()).all()), k
    for k in ("actor", "value", "posterior_kl"):  # the perturbation does reach the agent
        assert float(getattr(res, k).max()) > 0, k
    assert bool((res.actor >= 0).all()) and bool((res.value >= 0).all())
    # explicit draws, and the mean fill
    q = torch.empty(N * R, C).exponential_(generator=torch.Generator().manual_seed(3)).to(gpu)
    with torch.no_grad():
        res_q = d.saliency_frames(frames, hid, stride=s, fill="mean", mask_sigma=3.0, noise=q)
    _equal_fields(res_q, _stages(d, fd, hid, setup(32, 32, s, "mean", 3.0, 3.0), q), "explicit noise, mean fill")
    # a mask whose off-centre entries underflow, on frames whose centre pixels equal the fill: nothing changes
    const = np.empty((2, 32, 32, 3), dtype=np.uint8)
    const[0], const[1] = (10, 200, 77), (255, 0, 128)
    with torch.no_grad():
        res_0 = d.saliency_frames(const, hid[:2], stride=s, fill="mean", mask_sigma=0.01)
    for k in ("actor", "value", "value_delta", "posterior_kl", "latent_flips"):
        assert bool((getattr(res_0, k) == 0).all()), k


def test_saliency_semantics_against_oracle(small, gpu):
    """B = 2, T = 4, stride 16, explicit noise: the hidden states fed to step t
    are the oracle's filter states; the posterior logits of the GPU's own u8
    variants match the oracle's encoder on those frames; mu and V match the
    oracle's actor and critic on the GPU's own z'.  Bounds: test_gpu_closed_loop's
    (2e-4, 2e-5) for hiddens and logits, the standing 1e-4 of
    test_gpu_agent_trace for the heads."""
    from dreamer_amd.saliency import setup
    d, P, (fr, ac, rw, ct) = small
    B, T, S, s = 2, 4, 8, 16
    starts = [5, 40]
    R, C = d.latent_state_dims
    Hd = d.hidden_state_dims
    q_post, q_prior = _noise(61, T, B, R, C)
    o = _oracle(P, _windows(fr, starts, S).float(), _windows(ac, starts, S), T, R, C, q_post, q_prior, heads=False)
    q_var = torch.empty(B * T * R, C).exponential_(generator=torch.Generator().manual_seed(62))
    with torch.no_grad():
        res = d.saliency(starts=np.asarray(starts), length=T, stride=s, noise=(q_post.to(gpu), q_var.to(gpu)))
        tr = d.agent_trace(starts=np.asarray(starts), length=T, noise=q_post.to(gpu))
    torch.cuda.synchronize()
    close(tr.hiddens, o["hid"], 2e-4, 2e-5, "filter hiddens")
    frames = torch.from_numpy(_windows(fr, starts, S)[:, :T].numpy()).to(gpu).reshape(B * T, 3, 32, 32)
    assert torch.equal(res.frames.reshape(B * T, 3, 32, 32), frames)
    su = setup(32, 32, s, "blur", 3.0, None)
    st = _stages(d, frames, tr.hiddens.reshape(B * T, Hd).contiguous(), su, q_var.to(gpu))
    for k in FIELDS:  # the window front end fed the filter's states to the stages
        assert torch.equal(getattr(res, k).reshape(st[k].shape), st[k]), k
    n = B * T * (su.G + 1)
    h_rep, z = cpu(st["h_rep"]).view(n, 1, Hd), cpu(st["z"]).view(n, 1, R, C)
    with torch.no_grad():
        obs = O.normalise_obs(cpu(st["var"]).view(n, 1, 3, 32, 32))
        close(st["logits"].view(n, 1, R, C), O.encoder_logits(h_rep, obs, P).view(n, 1, R, C), 2e-4, 2e-5,
              "variant posterior logits")
        mu, _ = O.actor_forward(h_rep, z, P)
        V = O.critic_value(h_rep, z, P)
    _close1e4(st["mu_rows"].view(n, 1, -1), mu, "variant actor mu")
    _close1e4(st["V_rows"].view(n, 1, 1), V, "variant critic value")


def test_pass_independence(small, gpu):
    """N = 5 at stride 4 (G + 1 = 65): passes of 130 variant frames (2 + 2 + 1
    frames) against one pass."""
    from dreamer_amd.saliency import saliency_frames
    d = small[0]
    N = 5
    frames = _env_frames(N, 32, 32, 4)
    hid = (torch.randn(N, d.hidden_state_dims, generator=torch.Generator().manual_seed(5)) * 0.5).to(gpu)
    with torch.no_grad():
        one = saliency_frames(d, frames, hid, stride=4)
        cut = saliency_frames(d, frames, hid, stride=4, _pass_limit=130)
    torch.cuda.synchronize()
    assert one.actor.shape == (N, 8, 8)
    _equal_fields(cut, one, "pass limit 130 vs 8192")


# ------------------------------------------------------------ the window front end
def test_saliency_windows(small, gpu):
    from dreamer_amd import hip
    d = small[0]
    B, T, s = 2, 4, 16
    starts = np.asarray([3, 30])
    R, C = d.latent_state_dims
    with torch.no_grad():
        full = d.saliency(starts=starts, length=T, stride=s)
        last = d.saliency(starts=starts, length=T, steps=[T - 1], stride=s)
    assert full.actor.shape == (B, T, 2, 2) and last.actor.shape == (B, 1, 2, 2)
    assert full.mu.shape == (B, T, 3) and full.latents.shape == (B, T, R, C) and full.frames.shape == (B, T, 3, 32, 32)
    for k in FIELDS:
        assert torch.equal(getattr(last, k), getattr(full, k)[:, T - 1:]), k
    assert torch.equal(last.frames, full.frames[:, T - 1:])
    # explicit noise reproduces bit for bit
    g = torch.Generator().manual_seed(9)
    q = (torch.empty(T, B * R, C).exponential_(generator=g).to(gpu),
         torch.empty(B * T * R, C).exponential_(generator=g).to(gpu))
    with torch.no_grad():
        r1 = d.saliency(starts=starts, length=T, stride=s, noise=q)
        r2 = d.saliency(starts=starts, length=T, stride=s, noise=q)
    _equal_fields(r1, r2, "explicit noise twice")
    # sample=True consumes ad-hoc draws (the trace's stream and the variants'); explicit noise and the mode take none
    ar = hip.adhoc(gpu)
    c0 = ar.counter
    with torch.no_grad():
        d.saliency(starts=starts, length=T, stride=s, noise=q)
        d.saliency(starts=starts, length=T, stride=s)
    assert ar.counter == c0
    with torch.no_grad():
        r3 = d.saliency(starts=starts, length=T, stride=s, sample=True)
    assert ar.counter == (c0 + 2) & ar.COUNTER_MASK
    for k in FIELDS:
        assert bool(torch.isfinite(getattr(r3, k).float()).all()), k
    # the maps, the overlay and the video
    m = full.maps("actor")
    assert m.shape == (B, T, 32, 32) and m.dtype == torch.float32
    assert float(m.max()) <= 1.0 + 1e-6 and float(m.min()) >= 0.0
    assert float(full.maps("value", normalise="global").max()) <= 1.0 + 1e-6
    assert torch.equal(full.maps("posterior_kl", normalise=2.0), 2.0 * full.maps("posterior_kl", normalise=1.0))
    ov = full.overlay()
    assert ov.shape == (B, T, 3, 32, 32) and ov.dtype == torch.uint8
    assert torch.equal(ov[:, :, :2], full.frames[:, :, :2]) and bool((ov[:, :, 2] >= full.frames[:, :, 2]).all())
    v = full.video()
    assert v.shape == (T, 3, 3 * 32, B * 32) and v.dtype == torch.uint8 and v.is_contiguous()
    assert torch.equal(v[:, :, :32, :32], full.frames[0])
    c = full.concentration("actor")
    assert c.shape == (B, T) and bool(((c > 0) & (c <= 1)).all())


def test_evaluate_saliency_leaves_state(gpu):
    from dreamer_amd import hip
    np.random.seed(3)
    hip.rng(gpu).reseed(11)
    hip.adhoc(gpu).reseed(12)
    d, _ = build("small", gpu, B=2, H=3, S=8)
    fr, ac, rw, ct = replay_data(N_FILL, tuple(SMALL["observation_dims"]), A, seed=0)
    d.buffer.load_arrays(fr, ac, rw, ct)
    before_np, before = np.random.get_state(), d.training_state()
    counter = hip.adhoc(gpu).counter
    out = d.evaluate_saliency(batches=2, length=3, steps=[1, 2], stride=8, sample=True)
    after_np, after = np.random.get_state(), d.training_state()
    assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1]) and before_np[2:] == after_np[2:]
    _same(before, after)
    assert hip.adhoc(gpu).counter == counter
    assert set(out) == {"actor", "value", "posterior_kl", "concentration"}
    for k in ("actor", "value", "posterior_kl"):
        grid = np.asarray(out[k])
        assert grid.shape == (4, 4) and bool(np.isfinite(grid).all()) and bool((grid >= 0).all()), k
        assert 0.0 < out["concentration"][k] <= 1.0
    # the windows were sampled: without the restore np.random would have moved
    np.random.set_state(before_np)
    d.saliency(batch_size=2, length=3, stride=8)
    assert not np.array_equal(np.random.get_state()[1], before_np[1]) or np.random.get_state()[2] != before_np[2]


def test_saliency_vector_model_raises(gpu):
    from test_gpu_vector import _dreamer
    d = _dreamer(gpu, batch_size=2, sequence_length=4, horizon=3, buffer_size=N_FILL)
    with pytest.raises(ValueError):
        d.saliency(starts=np.asarray([0, 1]))
    with pytest.raises(ValueError):
        d.saliency_frames(np.zeros((1, 64, 64, 3), dtype=np.uint8), torch.zeros(1, d.hidden_state_dims, device=gpu))
    with pytest.raises(ValueError):
        d.evaluate_saliency()


def test_saliency_bf16_runs(gpu):
    """precision "bf16" on the FULL widths (the bf16 encoder takes 16, 32 or 64
    conv1 filters; SMALL has 8): everything is finite."""
    d, _ = build("full", gpu, B=2, H=3, S=4)
    d.precision = d.world_model.precision = "bf16"
    fr, ac, rw, ct = replay_data(N_FILL, tuple(FULL["observation_dims"]), A, seed=0)
    d.buffer.load_arrays(fr, ac, rw, ct)
    with torch.no_grad():
        res = d.saliency(starts=np.asarray([0, 17]), length=3, steps=[2], stride=16)
    torch.cuda.synchronize()
    assert res.actor.shape == (2, 1, 4, 4)
    for k in FIELDS:
        assert bool(torch.isfinite(getattr(res, k).float()).all()), k
    assert float(res.actor.max()) > 0


def test_saliency_deep_vae_runs(gpu):
    """The deeper-VAE configuration (128 x 128 frames, encoder_depth = 5) at stride 32."""
    from test_gpu_deep_vae import RES, _dreamer
    d = _dreamer(gpu, batch_size=2, sequence_length=4, horizon=3, buffer_size=N_FILL)
    fr, ac, rw, ct = replay_data(N_FILL, (RES, RES), d.action_dims, seed=0)
    d.buffer.load_arrays(fr, ac, rw, ct)
    with torch.no_grad():
        res = d.saliency(starts=np.asarray([0, 9]), length=2, steps=[1], stride=32)
    torch.cuda.synchronize()
    assert res.actor.shape == (2, 1, 4, 4) and res.frames.shape == (2, 1, 3, RES, RES)
    for k in FIELDS:
        assert bool(torch.isfinite(getattr(res, k).float()).all()), k
    assert res.maps("actor").shape == (2, 1, RES, RES) and res.video().shape == (1, 3, 3 * RES, 2 * RES)
