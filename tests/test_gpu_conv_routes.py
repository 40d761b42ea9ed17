"""Every kernel instantiation the conv-family dispatchers can launch (tests/conv_ref.py FORMS), run on its own through
dr_internal_conv_run and compared with float64.

Per case, in this order: the form the hook reports equals the pinned string; the integer pass is bit-exact on every
output that is linear in the operands (`pre`, the bias epilogue without SiLU, weight gradients, bias_out, channel sums:
operands in [-3, 3], every partial sum below 2^24 in any order, the integers exact in bf16 and in the three-plane
split); the random pass holds the linear outputs of the f32 kernels and of the one-term forms (against the
rounded-operand reference) to gemm_ref.f32_bound with K the true term count, and the outputs behind SiLU, SiLU' or
tanh and the three-plane split -- no bound is derived for them, as for the GEMM's split3 routes -- to the project's
1e-4 |ref| + 1e-5 max|ref|, their observed error printed beside the f32 bound there (CONV_ROUTES_ERRORS: appended to
that file; profiles/conv_routes_errors.txt is one such run); the tanh-MSE per-frame sums to 1e-4 relative; then the
sentinels: no NaN or unwritten element inside an output, nothing outside the outputs and the scratch changed (guards,
rows past a ragged tile, channels past ldc, the workspace past the size the op reported).

Left out on purpose: the bf16-storage encoder kernels and the fused conv1 + conv2 kernels (op_conv_bf16,
op_conv1_bf16, op_enc12_*, op_conv_s1_bf16, op_conv_glds_bf16): tests/test_gpu_bf16.py and
tests/test_gpu_enc12_schedule.py compare them with an emulation at their only shapes."""
import ctypes
import os

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

ERRORS_FILE = os.environ.get("CONV_ROUTES_ERRORS")


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_conv_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_longlong), ctypes.c_char_p, ctypes.c_int,
                                          ctypes.c_char_p, ctypes.c_int]
    return f


def ws_need(c):
    """The workspace floats the op asks for (nothing is launched: no pointers)."""
    m = R.materialise(c, "int", 0, ws_need=1)
    v = (ctypes.c_int * len(R.CV))(*m.ints())
    need = ctypes.c_longlong(-1)
    rc = _hook()(v, None, None, None, ctypes.byref(need), None, 0, None, 0)
    assert rc == 0 and need.value >= 0
    return int(need.value)


def run(c, m, dev):
    """One call of the hook on the device copy of the store: (rc, form, message, the store back on the CPU)."""
    from dreamer_amd import hip
    d = m.store.to(dev)
    assert d.data_ptr() % 16 == 0
    slots = m.slots(d.data_ptr())
    for name in m.regions:
        assert m.pointer(name, d.data_ptr()) % 16 == c.nib.get(name, 0)
    v = (ctypes.c_int * len(R.CV))(*m.ints())
    num = (ctypes.c_double * 2)(c.scale, 0.0)
    ptrs = (ctypes.c_void_p * len(R.CP))(*slots)
    need = ctypes.c_longlong(-1)
    form = ctypes.create_string_buffer(96)
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(v, num, ptrs, hip.stream(), ctypes.byref(need), form, 96, msg, 256)
    torch.cuda.synchronize()
    return rc, form.value.decode(), msg.value.decode(), d.cpu()


def _report(what, form, name, err, fb):
    bound = "none (behind a non-linear epilogue)" if fb != fb else f"{fb:.3e}"
    line = f"{form} | {what} | {name} | max err {err:.3e} | derived f32 bound there {bound}"
    print(line)
    if ERRORS_FILE:
        with open(ERRORS_FILE, "a") as f:
            f.write(line + "\n")


def check_case(form, c, dev, seed=0):
    need = ws_need(c) if c.op in (R.WGRAD, R.WGRAD_S3, R.CHAN) else 0
    for mode in ("int", "rand"):
        m = R.materialise(c, mode, seed, ws_need=need)
        if mode == "int" and not any(ck.kind == "lin" for ck in R.reference(c, m.f64)[0]):
            continue
        rc, got_form, msg, final = run(c, m, dev)
        assert rc == 0, f"{form} {c}: rc {rc}: {msg}"
        assert got_form == form, f"{c}: ran {got_form}"
        rep = (lambda name, err, fb: _report(repr(c), form, name, err, fb)) if mode == "rand" else None
        fails = R.compare(c, m, final, mode, report=rep)
        assert not fails, f"{form} {c} ({mode} pass): " + "; ".join(fails)


@pytest.mark.parametrize("form", R.FORMS)
def test_form_runs_and_matches_float64(form, gpu):
    for k, c in enumerate(R.TABLE[form]):
        check_case(form, c, gpu, seed=k)


def test_refusals_return_invalid_and_launch_nothing(gpu):
    """cin = 24, a misaligned operand on the six-product forms, h % 8 != 0 for op_convT_out3, a non-power-of-two w for
    op_wgrad_split3, csum with NCHW: DR_E_INVALID with a message, and the whole store still at its initial contents."""
    from dreamer_amd import _lib
    for name, c in R.REFUSALS.items():
        need = ws_need(c) if c.op in (R.WGRAD, R.WGRAD_S3, R.CHAN) else 0
        m = R.materialise(c, "rand", 1, ws_need=max(need, 1))
        rc, form, msg, final = run(c, m, gpu)
        assert rc == _lib.DR_E_INVALID and msg, (name, rc, form, msg)
        assert form == "", (name, form)
        assert bool((final.view(torch.int32) == m.initial.view(torch.int32)).all()), f"{name}: the store changed"
        print(f"{name}: {msg}")


def _out(c, dev, seed, edit=None):
    m = R.materialise(c, "rand", seed)
    if edit:
        edit(m)
    rc, form, msg, final = run(c, m, dev)
    assert rc == 0, msg
    return m, form, final


def test_bit_equality_where_the_code_claims_it(gpu):
    """The all-class upsampling kernel gives frame 0 the same bits at n = 1 and as the first of n = 3 (a tile never
    straddles frames); a conv tile's rows come out the same whether the tile is full (128 pixels) or ragged (100)."""
    for terms in (3, 1):
        for epi in (R.CT_BIAS, R.CT_DSILU):
            c3 = R.Case(R.CONVT_S3, 3, 64, 32, 8, 16, terms=terms, epi=epi)
            c1 = R.Case(R.CONVT_S3, 1, 64, 32, 8, 16, terms=terms, epi=epi)
            m3, form, f3 = _out(c3, gpu, 5)

            def same(m1):
                for k in ("in", "w", "bias", "pre"):
                    if k in m1.regions:
                        m1.regions[k].view(m1.store).copy_(m3.regions[k].view(m3.store)[:m1.regions[k].shape[0]]
                                                           if k in ("in", "pre") else m3.regions[k].view(m3.store))
            m1, form1, f1 = _out(c1, gpu, 6, same)
            assert form == form1 == f"k_convT_cls<{'dsilu' if epi else 'bias'},{terms}>"
            assert torch.equal(m1.regions["out"].view(f1).view(torch.int32),
                               m3.regions["out"].view(f3)[:1].view(torch.int32)), (terms, epi)
    for C, co in ((8, 16), (32, 64)):
        full = R.Case(R.CONV, 32, C, co, 4, 4, save_pre=True)   # 32 frames of 2 x 2: one full 128-pixel tile
        ragged = R.Case(R.CONV, 25, C, co, 4, 4, save_pre=True)  # its first 100 rows
        mf, form, ff = _out(full, gpu, 7)

        def first(mr):
            for k in ("in", "w", "bias"):
                mr.regions[k].view(mr.store).copy_(mf.regions[k].view(mf.store)[:25] if k == "in"
                                                   else mf.regions[k].view(mf.store))
        mr, form_r, fr = _out(ragged, gpu, 8, first)
        assert form == form_r
        for k in ("out", "pre"):
            assert torch.equal(mr.regions[k].view(fr).view(torch.int32), mf.regions[k].view(ff)[:25].view(torch.int32)), k
