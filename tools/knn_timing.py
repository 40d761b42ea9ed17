"""Time the fused k-nearest-neighbour search and the particle-entropy reward (profiles/knn_timing.txt)
against the composed form a user would otherwise write, torch.cdist + torch.topk, on the same tensors in the same
process: D = 600, k = 12, queries = bank with self-exclusion, at M = 4096 (the north-star B (H + 1)) and M = 1550 (the
reference config's 50 x 31).

  dr_knn                 Dreamer.knn's call: distances and indices
  dr_state_entropy_fwd   the one call engine.returns() adds per train_Agent epoch: the rewards rewritten in place
  cdist + topk           torch.cdist(h, h), the diagonal set to inf, torch.topk(k, largest=False): writes and reads the
                         M x M matrix
  epochs                 one Dreamer.train_Agent epoch (B = 256, CarRacing widths) with explore absent, "entropy" and
                         "disagreement", the three alternating in one process

HIP events on the stream, a warm-up then 3 x reps repetitions per path; min / max of the 3 per-call means (an event
interval around back-to-back calls: launch gaps included).  Needs the GPU.

    python tools/knn_timing.py [--out profiles/knn_timing.txt]
"""
import numpy as np
import torch

from timing_common import CFG, fill_ring, setup, timed, write_out

K, D = 12, 600
F32_MFMA_TFLOPS = 155.0  # measured f32-input MFMA rate of the device


def main():
    args, off = setup("knn_timing", 20)
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    dev = off.device
    st = hip.stream()
    lines = [
        f"Fused k-NN and particle-entropy reward, 1 x MI355X, D = {D}, k = {K}, queries = bank, self-exclusion, fp32.",
        "tools/knn_timing.py: HIP events on the stream, warm-up then 3 x N calls per path; us per call, min / max of",
        "the 3 means (an event interval around back-to-back calls: launch gaps included).  Rows are tanh of normals.",
        "",
    ]
    for M in (4096, 1550):
        g = torch.Generator(device="cpu").manual_seed(M)
        h = torch.tanh(torch.randn(M, D, generator=g)).to(dev)
        grp = torch.arange(M, dtype=torch.int32, device=dev)
        n = L.query("dr_knn_workspace_bytes", M, M, D, K)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        d2 = torch.empty(M, K, device=dev)
        idx = torch.empty(M, K, dtype=torch.int32, device=dev)
        rew = torch.zeros(M, device=dev)
        eye = torch.eye(M, dtype=torch.bool, device=dev)
        common = (D, K, M, L.ptr(h), D, L.ptr(grp), M, L.ptr(h), D, L.ptr(grp))

        def knn():
            L.call("dr_knn", *common, L.ptr(d2), L.ptr(idx), L.ptr(ws), n, st)

        def ent():
            L.call("dr_state_entropy_fwd", *common, None, None, None, L.ptr(rew), 0, 0, 0, 1, 1.0, 0.0, L.ptr(ws), n, st)

        def composed():
            dist = torch.cdist(h, h)
            dist.masked_fill_(eye, float("inf"))
            return torch.topk(dist, K, dim=1, largest=False)

        paths = (("dr_knn", knn), ("dr_state_entropy_fwd", ent), ("torch.cdist + torch.topk", composed))
        for _ in range(3):
            for _, p in paths:
                p()
        torch.cuda.synchronize()
        res = {name: [] for name, _ in paths}
        for _ in range(3):
            for name, p in paths:
                res[name].append(timed(p, 50))
        # agreement of the two forms on this data (the composed form's distances are cdist's Gram form)
        ref_d, ref_i = composed()
        knn()
        torch.cuda.synchronize()
        same = float((ref_i.int() == idx).float().mean())
        flop = 2.0 * M * M * D
        lines.append(f"  M = {M} ({flop / 1e9:.1f} GFLOP of f32 product, a {4.0 * M * M / 1e6:.1f} MB distance matrix never "
                     "formed):")
        for name, _ in paths:
            v = res[name]
            lines.append(f"    {name:26s} {min(v):9.1f} / {max(v):9.1f}")
        best = min(res["dr_knn"])
        lines += [
            f"    dr_knn: {flop / best / 1e6:.1f} TFLOP/s of the product = {flop / best / 1e6 / F32_MFMA_TFLOPS:.2f} of the "
            f"measured f32-MFMA rate ({F32_MFMA_TFLOPS:.0f} TF)",
            f"    composed - fused: {min(res['torch.cdist + torch.topk']) - max(res['dr_knn']):.1f} ... "
            f"{max(res['torch.cdist + torch.topk']) - min(res['dr_knn']):.1f}",
            f"    neighbour slots equal to the composed form's: {same:.4f}",
            "",
        ]
        del eye, ref_d, ref_i

    B = 256
    torch.manual_seed(0)
    ent_d = Dreamer(dict(CFG, explore="entropy"), dev)
    torch.manual_seed(0)
    dis_d = Dreamer(dict(CFG, explore="disagreement"), dev)
    modes = (("explore absent", off), ("explore entropy", ent_d), ("explore disagreement", dis_d))
    for _, d in modes:
        d.batch_size = B
        fill_ring(d, B)
    np.random.seed(1)
    for _ in range(3):
        for _, d in modes:
            d.train_Agent()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in modes}
    for _ in range(3):
        for name, d in modes:
            res[name].append(timed(d.train_Agent, args.reps))
    lines.append(f"  one train_Agent epoch, B = {B} (3 x {args.reps} epochs per mode, the modes alternating):")
    for name, _ in modes:
        lines.append(f"    {name:22s} {min(res[name]):10.1f} / {max(res[name]):10.1f}")
    a, b = res["explore absent"], res["explore entropy"]
    lines += [f"    entropy - absent       {min(b) - max(a):10.1f} ... {max(b) - min(a):.1f}   "
              f"(spread of the absent means: {max(a) - min(a):.1f})", ""]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
