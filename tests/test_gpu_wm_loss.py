"""Every kernel of the world-model loss stage (dreamer_amd/csrc/wm.hip: k_wm_gather, k_wm_masksum + k_wm_coef, k_wm_kl<0>,
k_wm_heads, k_wm_stats, k_wm_final, k_wm_kl<1>, k_ste_bwd_add, k_vec_mse, k_wm_window_scores) and the row kernels of the
reverse scan (ops.hip: k_gru_bwd, k_ln_silu_bwd<true / false>, k_softmax_ste_bwd, k_colsum_multi / k_colsum), each run
alone through dr_internal_wm_loss_run -- the launchers the training step itself calls -- and held to the float64
references of tests/wm_loss_ref.py on the inputs of tests/wm_loss_cases.py (run on the MI355X box: pytest -m gpu).

The whole-step tests reach these kernels with well-behaved data, masks of one and a free-bit clamp that is shut (the
small fixture) or drowned by the clipped prediction gradient (the full one).  Here: every group width off the powers of
two, partly valid last workgroups, the 64-lane / 256-thread / 8-row loop boundaries, both forms of k_ln_silu_bwd, and
values on the edges (module doc of wm_loss_cases.py and the needles named in its builders).

Launch geometry (read from the launchers, used for the derived summation bounds (chain + tree + c) 2^-24 sum|terms|):
  k_wm_masksum, k_wm_stats   1 workgroup x 256 threads: a thread adds ceil(M1 / 256) rows (each row's nparts / R terms
                             first), LDS tree of depth 8
  k_wm_window_scores         a wave per window, 4 per workgroup: a lane adds ceil((T - 1) / 64) steps, DPP tree depth 6
  k_vec_mse                  a wave per row: a lane adds ceil(D / 64) squares, depth 6
  k_colsum_multi, k_colsum   16-column slabs x 64 row groups: a thread adds ceil(M / 64) rows (8 in flight), then two
                             fixed-order stages of 8 additions
  k_wm_kl, k_ste_bwd_add, k_softmax_ste_bwd   a latent group on W = pow2 >= C lanes, 256 / W groups per workgroup
  k_wm_heads, k_ln_silu_bwd  a wave per row, 4 rows per workgroup, 64-lane loops over nb / K
  k_wm_gather, k_gru_bwd     a thread per element, 256-thread workgroups
  k_wm_coef (1 x 256), k_wm_final (one thread)

Per case: the hook returns 0; two runs on fresh buffers give identical bits; nothing outside an output, no output a
mode leaves unused and no row >= M is written (NaN-poisoned, still the same bits); every element of every output is
within its tolerance of the reference -- a derived bound, or 4 x the error measured on the first run
(profiles/wm_loss_errors.txt; WM_LOSS_ERRORS=<file> appends such a table) -- and the exact claims hold bit for bit:
KL and both its gradients exactly 0 for identical distributions and on masked rows, unchanged under a constant offset
of the logits, zero gradients under a zero row factor, a fully masked window scoring 0, g_pre16 the bf16
round-to-nearest-even of the g_pre of the same launch.

The skip flag follows the float64 reference, isfinite(total): of the fifteen non-finite sums, +-inf in stats[0] (the
mask sum: loss_pred = x / inf = 0) and -inf in stats[4] (max(1, -inf) = 1) leave the total finite and skip == 0, on the
device as in torch; the other twelve set it."""
import ctypes
import os

import pytest
import torch

import wm_loss_cases as C
import wm_loss_ref as R

pytestmark = pytest.mark.gpu

ERRORS_FILE = os.environ.get("WM_LOSS_ERRORS")


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_wm_loss_run
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                  ctypes.c_int]
    return f


def run(case, dev):
    """One call of the hook on fresh device buffers: (rc, message, {output: the whole buffer back on the CPU})."""
    from dreamer_amd import hip
    held, outs, ptrs = [], {}, []
    for s in case.slots:
        if s is None:
            ptrs.append(None)
            continue
        d = (s.make() if isinstance(s, C.Out) else s.contiguous()).to(dev)
        held.append(d)
        if isinstance(s, C.Out):
            outs[s.name] = d
        ptrs.append(d.data_ptr())
    v = (ctypes.c_int * max(len(case.v), 8))(*case.v)
    num = (ctypes.c_double * max(len(case.num), 4))(*case.num)
    pa = (ctypes.c_void_p * max(len(ptrs), 16))(*ptrs)
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(case.op, v, num, pa, hip.stream(), msg, 256)
    torch.cuda.synchronize()
    return rc, msg.value.decode(), {k: d.cpu() for k, d in outs.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("op", R.OP_NAMES)
def test_op_matches_float64(op, gpu):
    worst, fails = {}, []

    def report(key, kind, x):
        worst[key, kind] = max(worst.get((key, kind), 0.0), x)
    for case in C.cases_by_op()[op]:
        rc, msg, got = run(case, gpu)
        assert rc == 0, f"{case}: rc {rc}: {msg}"
        rc2, _, again = run(case, gpu)
        assert rc2 == 0
        for k in got:
            if not torch.equal(_bits(got[k]), _bits(again[k])):
                fails.append(f"{case}: {k} differs between two runs on the same inputs")
        fails += [f"{case}: {f}" for f in C.compare(case, got, report=report)]
    for (key, kind), x in sorted(worst.items()):
        n = len(C.cases_by_op()[op])
        if kind == "measured":
            line = f"{key} | max err {x:.3f} x 2^-24 x scale over {n} cases | asserted at {C.bound(key):.3f}"
        else:
            line = f"{key} | max err {x:.3f} of its derived bound over {n} cases"
        print(line)
        if ERRORS_FILE:
            with open(ERRORS_FILE, "a") as f:
                f.write(line + "\n")
    assert not fails, f"{len(fails)} failures, first: " + " || ".join(fails[:6])

