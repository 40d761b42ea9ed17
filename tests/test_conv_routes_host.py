"""tests/conv_ref.py without a GPU: each float64 formula against torch.nn.functional.conv2d / conv_transpose2d and their
autograd gradients, the case table against FORMS (every instantiation a dispatcher can launch has a case, and every
case reaches the form it is filed under by the host restatement of the ladders), the materialiser's store, and the
checks themselves: the reference written into the store passes compare(), and each of three deliberate one-line breaks
fails it."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

f64 = torch.float64


def _rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=f64)


@pytest.mark.parametrize("n,ih,iw,ci,co", [(1, 2, 2, 4, 8), (3, 8, 16, 8, 12), (2, 2, 6, 16, 4), (2, 6, 4, 3, 5)])
def test_conv_formula_is_conv2d(n, ih, iw, ci, co):
    x, w, b = _rn(n, ih, iw, ci), _rn(co, ci, 4, 4, seed=1), _rn(co, seed=2)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(R.conv_acc(x, w) + b, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,h,w,ci,co", [(1, 1, 1, 8, 3), (3, 4, 8, 8, 16), (2, 1, 3, 16, 8), (2, 8, 1, 8, 3)])
def test_upsampling_formula_is_conv_transpose2d_and_the_conv2d_data_gradient(n, h, w, ci, co):
    x, wt = _rn(n, h, w, ci), _rn(ci, co, 4, 4, seed=1)
    ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), wt, stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(R.up_acc(x, wt), ref, rtol=1e-12, atol=1e-12)
    # a Conv2d weight [co2 = ci][ci2 = co][4][4] read as [cin][cout]: the Conv2d's input gradient
    inp = _rn(n, co, 2 * h, 2 * w, seed=3).requires_grad_(True)
    (F.conv2d(inp, wt, stride=2, padding=1) * x.permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(R.up_acc(x, wt), inp.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,h,w,ca,cb", [(1, 2, 2, 8, 4), (3, 1, 1, 4, 8), (5, 4, 4, 8, 8), (2, 2, 3, 4, 4)])
def test_weight_gradient_formula_is_autograd(n, h, w, ca, cb):
    lo, hi = _rn(n, h, w, ca), _rn(n, 2 * h, 2 * w, cb, seed=1)
    # Conv2d: lo = output gradient, hi = input -> dW [cout][cin][4][4]
    wc = _rn(ca, cb, 4, 4, seed=2).requires_grad_(True)
    (F.conv2d(hi.permute(0, 3, 1, 2), wc, stride=2, padding=1) * lo.permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(R.wgrad_acc(lo, hi), wc.grad, rtol=1e-12, atol=1e-12)
    # ConvTranspose2d: lo = input, hi = output gradient -> dW [cin][cout][4][4]
    wt = _rn(ca, cb, 4, 4, seed=3).requires_grad_(True)
    (F.conv_transpose2d(lo.permute(0, 3, 1, 2), wt, stride=2, padding=1) * hi.permute(0, 3, 1, 2)).sum().backward()
    assert torch.allclose(R.wgrad_acc(lo, hi), wt.grad, rtol=1e-12, atol=1e-12)


def test_epilogue_formulas_are_autograd():
    x = _rn(1000).requires_grad_(True)
    F.silu(x).sum().backward()
    assert torch.allclose(R.dsilu(x.detach()), x.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.silu(x.detach()), F.silu(x.detach()), rtol=1e-12, atol=1e-12)
    # the tanh-MSE epilogue: out = coef[f] err (1 - mu^2) is d/d(pre) of coef[f] / 2 sum err^2
    c = R.Case(R.OUT3, 3, 8, 3, 8, 4, bpart=True)
    m = R.materialise(c, "rand", 1)
    pre = (R.up_acc(m.f64["in"], m.f64["w"]) + m.f64["bias"]).requires_grad_(True)
    err = torch.tanh(pre) - m.f64["target"][..., :3]
    (0.5 * m.f64["coef"].reshape(-1, 1, 1, 1) * err * err).sum().backward()
    checks = {ck.name: ck for ck in R.reference(c, m.f64)[0]}
    assert torch.allclose(checks["out"].ref[..., :3], pre.grad, rtol=1e-12, atol=1e-15)
    assert bool((checks["out"].ref[..., 3] == 0).all())
    assert torch.allclose(checks["part"].ref, (err * err).sum((1, 2, 3)).detach())
    assert torch.allclose(checks["bpart"].ref, pre.grad.sum((1, 2)))


def test_table_covers_every_form_and_every_case_reaches_its_form():
    assert len(set(R.FORMS)) == len(R.FORMS)
    assert sorted(R.TABLE) == sorted(R.FORMS), (sorted(set(R.FORMS) - set(R.TABLE)), sorted(set(R.TABLE) - set(R.FORMS)))
    for form, cases in R.TABLE.items():
        assert len(cases) >= 2, form
        assert all(R.route(c) == form for c in cases)
    for name, c in R.REFUSALS.items():
        assert R.route(c) is None, name


def test_geometries_per_form():
    """Each conv form has a borders-only case (one frame, at most 4 low-resolution pixels -- or the smallest grid the
    form admits), a several-frames case with a ragged tail and one just past the form's tile; each weight-gradient form
    a K below one chunk, a K that is no multiple of the chunk, several splits with a ragged last one and h = w = 1."""
    for form, cases in R.TABLE.items():
        op = cases[0].op
        if op in (R.CONV, R.CONV_S3, R.CONVT, R.CONVT_S3):
            up = op in (R.CONVT, R.CONVT_S3)
            pix = [c.n * c.h * c.w if up else c.n * (c.h // 2) * (c.w // 2) for c in cases]
            if "k_convT_cls" in form:  # 8 x 16 anchor tiles of one frame
                assert {(c.n, c.h, c.w) for c in cases} == {(1, 8, 16), (3, 8, 16), (2, 8, 32)}, form
                continue
            # the form's own BM: 128 on the f32 kernels and k_conv1_direct, 256 on k_conv_s1 / k_convT_s1, 8 RW on the
            # LDS-DMA kernels (RW 32 with 128-channel tiles, 64 with 64-channel tiles)
            tile = 128
            if "_s1<" in form:
                tile = 256
            elif "glds" in form:
                tile = 256 if form.split(",")[2].rstrip(">") == "128" else 512
            assert min(pix) <= 4 and cases[pix.index(min(pix))].n == 1, form
            assert any(c.n == 3 and p < tile for c, p in zip(cases, pix)), form
            assert any(tile < p <= tile + 8 for p in pix), (form, tile, pix)
        elif op in (R.WGRAD, R.WGRAD_S3):
            K = [c.n * c.h * c.w for c in cases]
            chunk = 32 if op == R.WGRAD else 64
            assert min(K) < chunk and any(k > chunk and k % chunk for k in K), form
            assert any(c.h == c.w == 1 for c in cases) and all(c.w < 8 or c.op == R.WGRAD for c in cases), form
        elif op == R.OUT3:
            assert any(c.w > R.O3_TX for c in cases) and any(c.h > R.O3_TY for c in cases) and any(c.w == 1 for c in cases)


@pytest.mark.parametrize("form", ["k_conv_nhwc<128,16,8,nhwc,fwd>", "k_convT_nhwc<128,32,16,bias,plain>",
                                  "k_convT_out3<16,loss>", "k_conv_wgrad<32>", "k_wgrad_s1<64,256>",
                                  "k_conv_nhwc<128,64,32,nhwc,dsilu>", "k_chan_sum_part4", "k_conv_s1<256,64,32,nchw,fwd>"])
def test_reference_in_the_store_passes_both_passes(form):
    for c in R.TABLE[form]:
        for mode in ("int", "rand"):
            m = R.materialise(c, mode, 3, ws_need=1234)
            for name, r in m.regions.items():
                assert (4 * r.off) % 16 == c.nib.get(name, 0)
            assert R.compare(c, m, R.emulate(c, m), mode) == [], (form, c, mode)


def test_each_deliberate_break_is_caught():
    """Three one-line breaks of a CPU restatement, each run through the checks the GPU test applies.  Caught by: the
    integer pass (the ky = 0 taps dropped: `pre` is no longer bit-exact), the unwritten-element check (a ragged tile's
    last valid row masked), the integer pass and the guard check (dW rows strided by cb where cbo belongs: the rows
    land in the wrong place and past dW's end)."""
    conv = next(c for c in R.TABLE["k_conv_nhwc<128,16,8,nhwc,fwd>"] if c.save_pre and c.n == 33)
    m = R.materialise(conv, "int", 1)
    fails = R.compare(conv, m, R.emulate(conv, m, "drop_ky0"), "int")
    assert any("pre: integer pass" in f for f in fails), fails
    m = R.materialise(conv, "rand", 1)
    assert any(f.startswith("pre:") or f.startswith("out:") for f in R.compare(conv, m, R.emulate(conv, m, "drop_ky0"), "rand"))
    fails = R.compare(conv, m, R.emulate(conv, m, "ragged_row"), "rand")
    assert any("out:" in f and "unwritten" in f for f in fails), fails
    wg = next(c for c in R.TABLE["k_conv_wgrad<32>"] if c.cbo < c.cb and c.n * c.h * c.w > 32)
    m = R.materialise(wg, "int", 1, ws_need=100)
    fails = R.compare(wg, m, R.emulate(wg, m, "cb_for_cbo"), "int")
    assert any(f.startswith("dw:") for f in fails) and any("outside the outputs" in f for f in fails), fails


def test_a_stray_write_and_a_pad_read_show():
    c = R.TABLE["k_convT_nhwc<128,16,8,bias,plain>"][0]
    m = R.materialise(c, "rand", 2)
    final = R.emulate(c, m)
    r = m.regions["out"]
    final[r.off + r.span] = 1.0  # one float past the output
    assert any("outside the outputs" in f for f in R.compare(c, m, final, "rand"))
    r = m.regions["in"]
    assert float(m.store[r.off - 1]) == R.PAD_IN and float(m.store[r.off + r.span]) == R.PAD_IN
