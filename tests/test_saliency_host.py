"""Host-side checks of perturbation saliency that need no GPU: the numpy
reference's own properties, the grid / centre / pass-size arithmetic, the
bilinear map at the cell centres, the result container's helpers, and the
argument errors, each raised before any random draw."""
import numpy as np
import pytest
import torch

import saliency_ref as SR
from formula import FULL, SMALL


def _tables(H, W, sigma_b=3.0, sigma_m=None):
    from dreamer_amd.saliency import blur_taps, default_mask_sigma, mask_profile
    wb, rb = blur_taps(sigma_b)
    return wb, rb, mask_profile(default_mask_sigma(H) if sigma_m is None else sigma_m, max(H, W))


def _frames(F, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(F, 3, H, W), dtype=np.uint8)


def test_tables():
    from dreamer_amd.saliency import blur_radius, blur_taps, default_mask_sigma, mask_profile
    wb, rb = blur_taps(3.0)
    assert rb == 9 and wb.dtype == np.float32 and wb.shape == (19,)
    assert abs(float(wb.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(wb, wb[::-1]) and wb.argmax() == rb
    assert blur_radius(5.0) == 15 and blur_radius(0.4) == 2
    gm = mask_profile(4.0, 64)
    assert gm.shape == (64,) and gm[0] == 1.0 and bool((np.diff(gm) <= 0).all())
    assert gm[3] == np.float32(np.exp(-9.0 / 32.0))
    assert default_mask_sigma(80) == 5.0 and default_mask_sigma(64) == 4.0
    # a mask so narrow that every off-centre entry underflows
    assert np.array_equal(mask_profile(0.01, 8), np.array([1] + [0] * 7, dtype=np.float32))


@pytest.mark.parametrize("fill", ["blur", "mean"])
def test_reference_properties(fill):
    H, W, s = 16, 24, 8
    wb, rb, gm = _tables(H, W)
    fr = _frames(2, H, W)
    G = (H // s) * (W // s)
    # a zero mask table gives the identity
    out = SR.occlude32(fr, s, fill, wb, rb, np.zeros_like(gm))
    assert out.shape == (2, G + 1, 3, H, W)
    assert all(np.array_equal(out[:, g], fr) for g in range(G + 1))
    # a constant frame stays the same under every variant (the taps sum to 1 within a rounding: rint absorbs it)
    const = np.full((1, 3, H, W), 137, dtype=np.uint8)
    const[:, 1], const[:, 2] = 0, 255
    out = SR.occlude32(const, s, fill, wb, rb, gm)
    assert all(np.array_equal(out[:, g], const) for g in range(G + 1))
    # a mask of ones gives rint(A)
    out = SR.occlude32(fr, s, fill, wb, rb, np.ones_like(gm))
    A = SR.fill_of(fr, fill, wb, rb, True)
    v = SR.fma32(np.ones_like(A), (A - fr.astype(np.float32)).astype(np.float32), fr.astype(np.float32))
    assert np.array_equal(out[:, 1], SR.quantise(v))
    assert int(np.abs(out[:, 1].astype(int) - SR.quantise(A).astype(int)).max()) <= 1
    assert np.array_equal(out[:, 0], fr)
    # the two references agree outside the guard
    o32 = SR.occlude32(fr, s, fill, wb, rb, gm)
    o64, guard = SR.occlude64(fr, s, fill, wb, rb, gm)
    assert np.array_equal(o32[~guard], o64[~guard])
    assert int(np.abs(o32.astype(int) - o64.astype(int)).max()) <= 1
    assert guard.mean() <= 0.005


def test_grid_and_centres():
    from dreamer_amd.saliency import cell_centres, grid_dims
    assert grid_dims(64, 64, 4) == (16, 16) and grid_dims(24, 40, 8) == (3, 5) and grid_dims(32, 32, 1) == (32, 32)
    assert cell_centres(16, 4) == [2, 6, 10, 14] and cell_centres(9, 3) == [1, 4, 7] and cell_centres(4, 1) == [0, 1, 2, 3]
    assert list(SR.centres(16, 4)) == cell_centres(16, 4) and list(SR.centres(9, 3)) == cell_centres(9, 3)
    for H, W, s in ((64, 64, 5), (24, 40, 16), (32, 32, 0), (32, 32, -4), (32, 32, 2.0), (32, 32, True)):
        with pytest.raises(ValueError):
            grid_dims(H, W, s)
    with pytest.raises(ValueError):
        grid_dims(64, 64, 1)       # 4096 cells
    assert grid_dims(64, 64, 2) == (32, 32)  # exactly 1024


def test_map_hits_cell_values_at_centres():
    H, W, s = 24, 40, 8
    rng = np.random.default_rng(1)
    S = rng.random((2, H // s, W // s)).astype(np.float32)
    m = SR.map64(S, np.ones(2, dtype=np.float32), H, W, s)
    cy, cx = SR.centres(H, s), SR.centres(W, s)
    assert np.array_equal(m[:, cy[:, None], cx[None, :]], S.astype(np.float64))
    # the border band is clamped to the outer cells; everything lies inside the grid's range
    assert np.array_equal(m[:, 0, 0], S[:, 0, 0].astype(np.float64)) and np.array_equal(m[:, -1, -1], S[:, -1, -1])
    assert m.min() >= S.min() - 1e-12 and m.max() <= S.max() + 1e-12
    # midway between two centres: the mean of the two cells
    assert np.allclose(m[:, cy[0], cx[0] + s // 2], 0.5 * (S[:, 0, 0].astype(np.float64) + S[:, 0, 1]), rtol=1e-15)


def test_pass_size():
    from dreamer_amd.saliency import PASS_VARIANTS, pass_frames
    assert PASS_VARIANTS == 8192
    assert pass_frames(256) == 31 and pass_frames(64) == 126 and pass_frames(1024) == 7 and pass_frames(1) == 4096
    assert pass_frames(64, 130) == 2 and pass_frames(64, 65) == 1 and pass_frames(64, 10) == 1
    # 32 frames at 64 x 64, stride 4: 8224 variant frames in two passes
    assert 32 * 257 == 8224 and -(-32 // pass_frames(256)) == 2


def test_check_steps():
    from dreamer_amd.saliency import check_steps
    assert check_steps(None, 4) == [0, 1, 2, 3] and check_steps([3], 4) == [3] and check_steps((2, 0), 4) == [2, 0]
    for bad in ([], [4], [-1], [0, 7]):
        with pytest.raises(ValueError):
            check_steps(bad, 4)


def _result(lead=(3,), Gy=4, Gx=4, seed=0):
    from dreamer_amd import SaliencyResult
    g = torch.Generator().manual_seed(seed)
    s = lambda: torch.rand(*lead, Gy, Gx, generator=g)
    return SaliencyResult(actor=s(), value=s(), value_delta=s(), posterior_kl=s(),
                          latent_flips=torch.zeros(*lead, Gy, Gx, dtype=torch.int32), mu=torch.zeros(*lead, 3),
                          sigma=torch.ones(*lead, 3), value_clean=torch.zeros(*lead), latents=torch.zeros(*lead, 8, 8),
                          frames=torch.zeros(*lead, 3, 32, 32, dtype=torch.uint8), stride=8)


def test_concentration():
    r = _result((2, 3))
    c = r.concentration("actor", top=0.1)  # ceil(1.6) = 2 of 16 cells
    s = r.actor.flatten(-2).numpy().astype(np.float64)
    want = np.sort(s, -1)[..., -2:].sum(-1) / s.sum(-1)
    assert c.shape == (2, 3) and np.allclose(c.numpy(), want, rtol=1e-5)
    assert torch.allclose(r.concentration("value", top=1.0), torch.ones(2, 3))
    r.posterior_kl.zero_()
    r.posterior_kl[0, 0, 1, 2] = 3.0
    c = r.concentration("posterior_kl", top=0.1)
    assert c[0, 0].item() == 1.0 and c[1, 2].item() == 2 / 16  # all-zero scores: the uniform share
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError):
            r.concentration("actor", top=bad)
    with pytest.raises(ValueError):
        r.concentration("latent_flips")


def test_argument_errors_fire_before_any_draw():
    """Every refusal leaves np.random untouched (the starts are not sampled yet)."""
    from dreamer_amd import Dreamer
    d = Dreamer(dict(SMALL), torch.device("cpu"))
    R, C = d.latent_state_dims
    fr = np.zeros((2, 32, 32, 3), dtype=np.uint8)
    h = torch.zeros(2, d.hidden_state_dims)
    np.random.seed(5)
    state = np.random.get_state()
    bad = (dict(stride=5), dict(stride=0), dict(blur_sigma=5.1), dict(blur_sigma=-1.0), dict(mask_sigma=0.0),
           dict(fill="median"), dict(noise=torch.ones(2 * R, C + 1)), dict(noise=torch.ones(3 * R, C)))
    for kw in bad:
        with pytest.raises(ValueError):
            d.saliency_frames(fr, h, **kw)
        with pytest.raises(ValueError):
            d.saliency(batch_size=2, **{k: (v if k != "noise" else (v, v)) for k, v in kw.items()})
    for frames, hid in ((fr[:, :16], h), (fr.astype(np.float32), h), (fr, h[:1]), (fr, torch.zeros(2, 5)),
                        (fr[:0], h[:0])):
        with pytest.raises(ValueError):
            d.saliency_frames(frames, hid)
    S = d.sequence_length
    for kw in (dict(length=1), dict(length=S + 1), dict(steps=[S]), dict(steps=[]), dict(length=3, steps=[3]),
               dict(noise=torch.ones(S, 2 * R, C))):
        with pytest.raises(ValueError):
            d.saliency(batch_size=2, **kw)
    with pytest.raises(ValueError):
        d.evaluate_saliency(batches=0)
    with pytest.raises(ValueError):
        d.evaluate_saliency(batches=1, batch_size=2, stride=3)
    # G > 1024 at 64 x 64
    cfg = dict(FULL)
    d64 = Dreamer(cfg, torch.device("cpu"))
    with pytest.raises(ValueError):
        d64.saliency_frames(np.zeros((1, 64, 64, 3), dtype=np.uint8), torch.zeros(1, d64.hidden_state_dims), stride=1)
    with pytest.raises(ValueError):
        d64.saliency(batch_size=2, stride=1)
    # vector observations
    cfg = dict(SMALL)
    cfg.update(observation_dims=[12])
    dv = Dreamer(cfg, torch.device("cpu"))
    with pytest.raises(ValueError):
        dv.saliency_frames(fr, h)
    with pytest.raises(ValueError):
        dv.saliency(batch_size=2)
    with pytest.raises(ValueError):
        dv.evaluate_saliency()
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def _code(L, code, name, *args):
    with pytest.raises(L.HipError) as e:
        L.call(name, *args)
    assert e.value.code == code, (name, args, e.value)


def test_entry_points_refuse_on_the_host():
    """The C entry points check their arguments before any launch, so the
    refusals need no GPU (non-null addresses are never dereferenced)."""
    from dreamer_amd import _lib as L
    p = 256
    d = L.dr_dims()
    d.img_h, d.img_w = 32, 32
    ring = L.dr_frames(p, 4, p, None, 0, 0, 1, 0)
    INV, UNS = L.DR_E_INVALID, L.DR_E_UNSUPPORTED
    occ = lambda dd, src, F, s, fill, wb, rb, gm: (dd, src, F, s, fill, wb, rb, gm, p, p, 1 << 30, None)
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 8, 0, p, 16, p))      # rb > 15
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 5, 0, p, 9, p))       # stride does not divide
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 0, 0, p, 9, p))
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 8, 0, None, 9, p))    # wb NULL (blur)
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 8, 0, p, 9, None))    # gm NULL
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 8, 1, None, 9, None))
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 3, 8, 2, p, 9, p))       # unknown fill
    _code(L, INV, "dr_occlude_frames", *occ(d, ring, 0, 8, 0, p, 9, p))
    d64 = L.dr_dims()
    d64.img_h, d64.img_w = 64, 64
    _code(L, INV, "dr_occlude_frames", *occ(d64, ring, 3, 1, 0, p, 9, p))     # 4096 cells
    f32 = L.dr_frames(None, 0, None, p, 3 * 32 * 32, 0, 1, 0)
    _code(L, UNS, "dr_occlude_frames", *occ(d, f32, 3, 8, 0, p, 9, p))        # f32 form
    dv = L.dr_dims()
    dv.img_h, dv.img_w, dv.obs_dim = 32, 32, 12
    _code(L, UNS, "dr_occlude_frames", *occ(dv, ring, 3, 8, 0, p, 9, p))      # vector observations
    _code(L, L.DR_E_WORKSPACE, "dr_occlude_frames", d, ring, 3, 8, 0, p, 9, p, p, p, 16, None)
    assert L.query("dr_occlude_workspace_bytes", d, 3) == 3 * 3 * 32 * 32 * 4
    # dr_saliency_scores(F, G, A, R, C, mu, V, logits, z, actor, value, value_delta, kl, flips, stream)
    for F, G, A, R, C in ((-1, 4, 3, 8, 8), (2, 0, 3, 8, 8), (2, 4, 0, 8, 8), (2, 4, 3, 0, 8), (2, 4, 3, 8, 0)):
        _code(L, INV, "dr_saliency_scores", F, G, A, R, C, p, p, p, p, p, p, p, p, p, None)
    _code(L, INV, "dr_saliency_scores", 2, 4, 3, 8, 65, p, p, p, p, p, p, p, p, p, None)  # C > 64 with the KL
    for k in (5, 6, 7, 8):  # an output without its input
        a = [2, 4, 3, 8, 8, p, p, p, p, p, p, p, p, p, None]
        a[k] = None
        _code(L, INV, "dr_saliency_scores", *a)
    L.call("dr_saliency_scores", 0, 4, 3, 8, 8, p, p, p, p, p, p, p, p, p, None)          # no rows: a no-op
    L.call("dr_saliency_scores", 2, 4, 3, 8, 8, None, None, None, None, None, None, None, None, None, None)
    # dr_saliency_map(d, F, s, scores, scale, frames, ch, map, overlay, stream)
    _code(L, INV, "dr_saliency_map", d, 2, 5, p, p, ring, 2, p, p, None)
    _code(L, INV, "dr_saliency_map", d, 2, 8, None, p, ring, 2, p, p, None)
    _code(L, INV, "dr_saliency_map", d, 2, 8, p, p, ring, 3, p, p, None)      # channel
    _code(L, INV, "dr_saliency_map", d, 2, 8, p, p, None, 2, p, p, None)      # overlay without frames
    _code(L, INV, "dr_saliency_map", d64, 2, 1, p, p, ring, 2, p, p, None)
    _code(L, UNS, "dr_saliency_map", d, 2, 8, p, p, f32, 2, p, p, None)
    _code(L, UNS, "dr_saliency_map", dv, 2, 8, p, p, ring, 2, p, p, None)
    L.call("dr_saliency_map", d, 0, 8, p, p, None, 0, p, None, None)
    _code(L, INV, "dr_saliency_draws", 4, 0, L.dr_noise(None, None, p, 0, 0), p, None)
    _code(L, INV, "dr_saliency_draws", 4, 8, L.dr_noise(), p, None)           # no Philox state
