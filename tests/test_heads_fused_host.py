"""Host-only: the support predicate of dr_heads_fwd and the K partition of the grouped first Linear."""
import ctypes

import torch

from formula import FULL, SMALL


def _dims(cfg, precision=None):
    from dreamer_amd import Dreamer
    c = dict(cfg)
    if precision is not None:
        c["precision"] = precision
    d = Dreamer(c, torch.device("cpu"))
    return d.world_model.dims(d.agent)


def test_heads_support_predicate():
    from dreamer_amd import _lib as L
    d = _dims(FULL)
    ok = lambda B, H, dd=d: L.query("dr_heads_supported", dd, B, H)
    assert ok(256, 15) == 1 and ok(64, 15) == 1 and ok(68, 15) == 1
    assert ok(63, 15) == 0 and ok(3, 2) == 0  # under 1024 states
    assert ok(0, 15) == 0 and ok(64, 0) == 0
    assert L.query("dr_heads_workspace_bytes", d, 256, 15) > 0 and L.query("dr_heads_workspace_bytes", d, 3, 2) == 0
    # a width that is no multiple of 4, or past the tail kernel's 208, is refused; 208 itself is taken
    for field, value, want in (("rew_h1", 202, 0), ("cont_h2", 212, 0), ("critic_h1", 198, 0), ("rew_h2", 208, 1),
                               ("critic_h1", 256, 1)):
        dd = type(d).from_buffer_copy(d)
        setattr(dd, field, value)
        assert ok(256, 15, dd) == want, (field, value)
    # bf16 mode keeps the separate launches
    db = type(d).from_buffer_copy(d)
    db.precision = 1
    assert ok(256, 15, db) == 0


def test_k_partition_depends_on_k_alone():
    """splits = the largest power of two <= 4 that leaves every split at least 8 chunks of 32 k: the reference widths
    (K = 1624) take 4, which is what the ungrouped product picked at the bench shape; M, the widths and the head count
    do not enter (the hook takes M and ignores the widths)."""
    from dreamer_amd import _lib
    f = _lib.load().dr_internal_s3_heads_splits
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int]

    def rule(K):
        nch, sp = (K + 31) // 32, 1
        while sp < 4 and nch // (2 * sp) >= 8:
            sp *= 2
        return sp

    assert f(4096, 1624) == 4
    for K in (4, 104, 256, 508, 512, 1020, 1024, 1624, 4096, 65536):
        got = {f(M, K) for M in (1, 9, 1024, 1064, 1088, 4096, 8192, 1 << 20)}
        assert got == {rule(K)}, (K, got)
