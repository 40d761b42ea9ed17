"""Time prioritised ("curious") replay (profiles/replay_priority_timing.txt,
DESIGN.md 5n).

  kernels, on bare priority arrays (no frame ring): dr_replay_sample (B = 256,
      Philox) and dr_replay_priority_update (B = 256) at cap = 1e5 and 1e6;
      dr_wm_window_scores on the workspace of a B = 256, T = 15 step;
  epoch: one Dreamer.train_world_model epoch at B = 256, T = 15 with
      replay = "uniform" (host np.random starts, one H2D copy) and with
      replay = "curious" (device sample -> step with scores -> priority
      update), the same Dreamer in the same process, the two alternating.

CarRacing widths, default init, fp32.  HIP events on the stream, a warm-up
then 3 x reps repetitions per path; min / max of the 3 per-call means.  Needs
the GPU.

    python tools/replay_priority_timing.py [--out profiles/replay_priority_timing.txt]
"""
import numpy as np
import torch

from timing_common import alternate, fill_ring, setup, timed, warm_up, write_out


def main():
    args, d = setup("replay_priority_timing", 10)
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    dev = d.device
    B, T = 256, d.horizon
    d.batch_size = B
    fill_ring(d, B)
    buf, wm = d.buffer, d.world_model
    stream = hip.stream()
    g = np.random.default_rng(0)
    lines = [
        "Prioritised replay, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32.",
        f"tools/replay_priority_timing.py: HIP events on the stream, warm-up then 3 x N calls per path;",
        "us per call, min / max of the 3 means (an event interval around back-to-back launches: launch gaps included).",
        "",
        f"  kernels on bare arrays, B = {B} (3 x 200 calls each):",
    ]
    rng_state = hip.adhoc(dev).state
    for cap in (100_000, 1_000_000):
        pri = torch.from_numpy(np.exp(g.uniform(np.log(0.04), np.log(1e5), cap)).astype(np.float32)).to(dev)
        vis = torch.zeros(cap, dtype=torch.int32, device=dev)
        starts = torch.empty(B, dtype=torch.int64, device=dev)
        prob = torch.empty(B, device=dev)
        scores = torch.from_numpy(g.standard_normal(B).astype(np.float32) * 30).to(dev)
        ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=dev)

        def sample():
            L.call("dr_replay_sample", cap, cap, cap // 2, 64, B, L.ptr(pri), 0.01 ** 0.7, None, rng_state.data_ptr(),
                   5 << 17, L.ptr(starts), L.ptr(prob), L.ptr(ws), ws.numel(), stream)

        def update():
            L.call("dr_replay_priority_update", cap, B, L.ptr(starts), L.ptr(scores), 1e4, 0.7, 0.7, 0.01, 1e5,
                   L.ptr(pri), L.ptr(vis), stream)

        warm_up(sample, update)
        a, b = alternate(sample, update, 200)
        lines += [f"    cap = {cap:>9,d}  dr_replay_sample          {min(a):8.1f} / {max(a):8.1f}"
                  f"   ({4 * cap / (min(a) * 1e-6) / 1e12:.3f} TB/s of the 4 cap bytes at its fastest mean)",
                  f"    cap = {cap:>9,d}  dr_replay_priority_update {min(b):8.1f} / {max(b):8.1f}"]

    # the score kernel on the workspace a B = 256, T = 15 step leaves
    buf.replay = "curious"
    d.train_world_model()
    torch.cuda.synchronize()
    dd = wm.dims()
    wsb = hip.workspace(dev).get("wm_train", L.query("dr_wm_train_workspace_bytes", dd, B, T))
    cfg = L.dr_wm_loss_cfg(wm.beta_pred, wm.beta_dyn, wm.beta_rep)
    out = torch.empty(B, device=dev)

    def score():
        L.call("dr_wm_window_scores", dd, B, T, cfg, L.ptr(wsb), wsb.numel(), L.ptr(out), stream)

    warm_up(score, score)
    a, _ = alternate(score, lambda: None, 200)
    lines += [f"    B = {B}, T = {T}     dr_wm_window_scores       {min(a):8.1f} / {max(a):8.1f}", ""]

    def epoch(mode):
        def run():
            buf.replay = mode
            d.train_world_model()
        return run

    uni, cur = epoch("uniform"), epoch("curious")
    warm_up(uni, cur)
    a, b = alternate(uni, cur, args.reps)
    lines += [
        f"  one train_world_model epoch, B = {B}, T = {T}, ring of {buf.size} slots (3 x {args.reps} epochs per mode,",
        "  the modes alternating):",
        f"    replay = uniform   {min(a):10.1f} / {max(a):10.1f}",
        f"    replay = curious   {min(b):10.1f} / {max(b):10.1f}",
        f"    curious - uniform  {min(b) - max(a):10.1f} ... {max(b) - min(a):.1f}   "
        f"(spread of the uniform means: {max(a) - min(a):.1f})",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
