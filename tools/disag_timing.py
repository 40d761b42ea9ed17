"""Time the latent-disagreement ensemble (profiles/disag_timing.txt) at the north-star shape: B = 256,
H = 15, T = 15, CarRacing widths, K = 8 members of the default width (200), fp32.

  dr_disag_fwd        the one call engine.returns() adds per train_Agent epoch: B (H + 1) = 4096 hidden states, the
                      rewards rewritten in place
  explorer.train_step the one call train_world_model adds per world-model step: B (T - 1) = 3584 rows of (h, z)
  epochs              one Dreamer.train_Agent epoch and one Dreamer.train_world_model epoch, each on a Dreamer with
                      explore = "disagreement" and on one without, the two alternating in one process

HIP events on the stream, a warm-up then 3 x reps repetitions per path; min / max of the 3 per-call means (an event
interval around back-to-back calls: launch gaps included).  Needs the GPU.

    python tools/disag_timing.py [--out profiles/disag_timing.txt]
"""
import numpy as np
import torch

from timing_common import CFG, alternate, fill_ring, setup, warm_up, write_out

K = 8


def main():
    args, off = setup("disag_timing", 20)
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    dev = off.device
    B = 256
    torch.manual_seed(0)
    on = Dreamer(dict(CFG, explore="disagreement", explore_ensemble=K), dev)
    for d in (off, on):
        d.batch_size = B
        fill_ring(d, B)
    H, T = on.horizon, on.world_model.horizon
    ex = on.explorer
    W, Hd, Lt = ex.width, ex.hidden, ex.latent
    eng = on.engine
    M_im, M_wm = B * (H + 1), B * (T - 1)
    lines = [
        f"Latent-disagreement ensemble, 1 x MI355X, CarRacing widths, K = {K}, W = {W}, default init, fp32.",
        "tools/disag_timing.py: HIP events on the stream, warm-up then 3 x N calls per path; us per call, min / max of",
        "the 3 means (an event interval around back-to-back calls: launch gaps included).",
        "",
    ]
    np.random.seed(1)
    on.train_Agent()  # fills eng.hiddens / eng.rewards
    torch.cuda.synchronize()
    st = hip.stream()

    def fwd():
        L.call("dr_disag_fwd", ex.struct(), Hd, Lt, M_im, L.ptr(eng.hiddens), Hd, None, None, L.ptr(eng.rewards), H + 1,
               1, H, 1, 1.0, 0.0, L.ptr(eng.ws_disag), eng.ws_disag.numel(), st)

    h = torch.randn(M_wm, Hd, device=dev)
    z = torch.nn.functional.one_hot(torch.randint(0, 32, (M_wm, 32), device=dev), 32).float().reshape(M_wm, Lt)

    def step():
        ex.train_step(h, z)

    warm_up(fwd, step)
    a, b = alternate(fwd, step, 100)
    pred_im, pred_wm = 4 * K * M_im * Lt, 4 * K * M_wm * Lt
    lines += [
        f"  dr_disag_fwd, M = {M_im} rows (one per train_Agent epoch)        {min(a):9.1f} / {max(a):9.1f}",
        f"  explorer.train_step, M = {M_wm} rows (one per world-model step)  {min(b):9.1f} / {max(b):9.1f}",
        f"  the K x M x L predictions: {pred_im / 1e6:.1f} MB written and {pred_im / 1e6:.1f} MB read back per dr_disag_fwd"
        f" ({2 * pred_im / 8e12 * 1e6:.1f} us of HBM time at 8 TB/s);",
        f"  per train_step {pred_wm / 1e6:.1f} MB written and read by the loss kernel, and dL/dp of the same size written and"
        f" read three times (input-gradient product, weight-gradient product, bias sums): {6 * pred_wm / 8e12 * 1e6:.1f} us"
        " at 8 TB/s.  A kernel fusing the last product with the moments would save the forward's share.",
        "",
    ]

    def agent(d):
        return lambda: d.train_Agent()

    def world(d):
        return lambda: d.train_world_model()

    for name, path in (("train_Agent epoch", agent), ("train_world_model epoch", world)):
        p_off, p_on = path(off), path(on)
        warm_up(p_off, p_on)
        a, b = alternate(p_off, p_on, args.reps)
        lines += [
            f"  one {name}, B = {B} (3 x {args.reps} epochs per mode, the modes alternating):",
            f"    explore absent        {min(a):10.1f} / {max(a):10.1f}",
            f"    explore disagreement  {min(b):10.1f} / {max(b):10.1f}",
            f"    on - off              {min(b) - max(a):10.1f} ... {max(b) - min(a):.1f}   "
            f"(spread of the off means: {max(a) - min(a):.1f})",
            "",
        ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
