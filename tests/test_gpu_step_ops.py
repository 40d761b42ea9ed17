"""The row kernels of the recurrent step and the actor head (dreamer_amd/csrc/gru.hip: k_gru_fused, k_gru_gates<8>,
k_onehot_index, k_zgather_add, k_transpose, k_transpose_multi; ops.hip: k_gru_fwd, k_sample, k_actor_head,
k_actor_head_bwd_x, k_sigmoid, k_mean, k_copy2d<true / false>, k_copy2d_multi, k_fill, k_fill4, k_vec_gather), each
run alone through dr_internal_step_run -- the launchers the engine itself calls -- and held to the float64 references
of tests/step_ops_ref.py on the inputs of tests/step_ops_cases.py (run on the MI355X box: pytest -m gpu).

The whole-run tests reach these kernels at the workload's widths with ordinary data.  Here: both forms of the GRU step
on either side of B = 128 and of their tiles, Hd below one MFMA wave's share and past one GRU_PRE round, dense-marked
latent groups, saturated gates, group widths that leave the sampler's padding lanes live, the clamp's edges in the
actor head's backward, partly valid last workgroups everywhere (module doc of step_ops_cases.py and the needles named
in its builders).

Launch geometry (read from the launchers, used for the derived summation bounds (chain + tree + c) 2^-24 sum|terms|):
  k_gru_fused        16 rows x 16 units per 512-thread workgroup, tiles dealt by dr_xcd_tile; gh: K over 4 MFMA waves
                     of kw = 16 ceil(Hd / 64) each, every wave one chain of kw products (a second GRU_PRE round past
                     kw = 160), then 3 additions of the partial sums and the bias: sghn at (kw + 4 + 2) 2^-24 sum|terms|
  k_gru_gates<8>     8 rows x 32 units per 192-thread workgroup; gh from gemm_launch(G_NT, AM_PLAIN): sghn and gh_ws at
                     gemm_ref.f32_bound(K = Hd)
  k_zgather_add      4 rows x 256 columns per workgroup: one fma chain over the R groups (+ C per dense group), then
                     base + v: (R + dense C + 2) 2^-24 (sum|terms| + |base|)
  k_actor_head_bwd_x 16 rows x 64 columns: gx one fma chain of 2 A products on the kernel's own g_heads:
                     (2 A + 2) 2^-24 sum|terms| + the g_heads tolerance carried through |wt|
  k_mean             1 workgroup x 1024 threads: a thread adds ceil(n / 1024) elements, LDS tree of depth 10, the
                     division: (ceil(n / 1024) + 10 + 2) 2^-24 mean|x|
  k_sample           a latent group on W = pow2 >= C lanes, 256 / W groups per workgroup
  k_onehot_index, k_gru_fwd, k_actor_head, k_sigmoid, k_fill, k_vec_gather   a thread per element, 256-thread workgroups
  k_fill4, k_copy2d, k_copy2d_multi   grid-stride, at most 2048 x 256 threads; k_transpose(_multi) 32 x 32 tiles

Per case: the hook returns 0; two runs on fresh buffers give identical bits; nothing outside an output, no output a
mode leaves unused and no row past the last is written (NaN-poisoned, still the same bits); every element of every
output is within its tolerance of the reference -- exact, a derived bound, or 4 x the error measured on the first run
(profiles/step_ops_errors.txt; STEP_OPS_ERRORS=<file> appends such a table) -- and the exact claims hold bit for bit:
hout16 the bf16 round-to-nearest-even of the hout of the same launch; saturated gates exactly 0 / 1 / +-1 and h' then
exactly n, or (h - n) + n in float32 (gru_cell's op order: at u = 1 that is h only to rounding); a NaN row of h
confined to its row; zgather_add's out = base under zero values; the sampler's z exactly (1 + pu) - pu of its own soft
at the winner and 0 elsewhere, soft unchanged under a constant offset and exactly one-hot under -inf; tanh exactly +-1
at +-20; no g_a contribution at a = +-1.  A refused call returns DR_E_INVALID with a message and leaves every output
POISON.  Twins: the rows that B = 17 and B = 33 (fused), B = 129 and B = 136 (split) share have the same bits in
every output, so a row's result does not depend on the tile it lands in; g_heads has the same bits at every N.  The split
form with gh_ready = 1 on the scratch a gh_ready = 0 call left gives that call's bits."""
import ctypes
import os

import pytest
import torch

import step_ops_cases as C
import step_ops_ref as R

pytestmark = pytest.mark.gpu

ERRORS_FILE = os.environ.get("STEP_OPS_ERRORS")


def _hook():
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_step_run
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
        off = 0
        if isinstance(s, C.Shift):
            s, off = s.slot, s.off
        d = (s.make() if isinstance(s, C.Out) else s.contiguous()).to(dev)
        held.append(d)
        if isinstance(s, C.Out):
            outs[s.name] = d
        ptrs.append(d.data_ptr() + 4 * off)
    v = (ctypes.c_int * max(len(case.v), 64))(*case.v)
    num = (ctypes.c_double * max(len(case.num), 4))(*case.num)
    pa = (ctypes.c_void_p * max(len(ptrs), 32))(*ptrs)
    msg = ctypes.create_string_buffer(256)
    rc = _hook()(case.op, v, num, pa, hip.stream(), msg, 256)
    try:
        torch.cuda.synchronize()
        back = {k: d.cpu() for k, d in outs.items()}
    except RuntimeError as e:  # a device fault: nothing more is launched on this device
        pytest.exit(f"{case}: device error after the launch: {e}", returncode=3)
    return rc, msg.value.decode(), back


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _rows(case, got, rows):
    return {o.name: _bits(got[o.name][o.region][:rows]) for o in case.outs() if o.name != "gh_ws" and o.name != "gx"}


@pytest.mark.parametrize("op", R.OP_NAMES)
def test_op_matches_float64(op, gpu):
    worst, fails, twins = {}, [], {}
    cases = C.cases_by_op()[op]

    def report(key, kind, x):
        worst[key, kind] = max(worst.get((key, kind), 0.0), x)
    for case in cases:
        rc, msg, got = run(case, gpu)
        if case.refuse:
            assert rc == C.DR_E_INVALID and msg and case.refuse in msg, f"{case}: rc {rc}: {msg!r}"
            fails += [f"{case}: {f}" for f in C.untouched(case, got)]
            continue
        assert rc == 0, f"{case}: rc {rc}: {msg}"
        rc2, _, again = run(case, gpu)
        assert rc2 == 0
        for k in got:
            if not torch.equal(_bits(got[k]), _bits(again[k])):
                fails.append(f"{case}: {k} differs between two runs on the same inputs")
        fails += [f"{case}: {f}" for f in C.compare(case, got, report=report)]
        if case.twin:
            key, rows = case.twin
            mine = _rows(case, got, rows)
            if key in twins:
                first, theirs = twins[key]
                fails += [f"{case}: rows of {k} differ in bits from {first}" for k in mine
                          if k in theirs and not torch.equal(mine[k], theirs[k])]
            else:
                twins[key] = (case, mine)
        if op == "gru" and "gh_ws" in case.wants():  # the split form: gh_ready = 1 on the scratch this call left
            rc3, msg3, ready = run(C.with_ready(case, got["gh_ws"]), gpu)
            assert rc3 == 0, f"{case}: gh_ready = 1: rc {rc3}: {msg3}"
            fails += [f"{case}: {k} differs with gh_ready = 1" for k in ready if not torch.equal(_bits(ready[k]), _bits(got[k]))]
    for (key, kind), x in sorted(worst.items()):
        n = len([c for c in cases if not c.refuse])
        if kind == "measured":
            line = f"{key} | max err {x:.3f} x 2^-24 x scale over {n} cases | asserted at {C.bound(key):.3f}"
        else:
            line = f"{key} | max err {x:.3f} of its derived bound over {n} cases"
        print(line)
        if ERRORS_FILE:
            with open(ERRORS_FILE, "a") as f:
                f.write(line + "\n")
    assert not fails, f"{len(fails)} failures, first: " + " || ".join(fails[:6])
