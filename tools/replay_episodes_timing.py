"""Time episode-aware replay (profiles/replay_episodes_timing.txt),
by the protocol of tools/replay_priority_timing.py.

  kernels, on bare arrays (no frame ring), S = 64, B = 256, Philox:
      dr_replay_spans at cap = 1e5 and 1e6 (continues with a break every ~1000
      slots, a first flag on a third of them);
      dr_replay_sample against dr_replay_sample_spans with the priorities and
      with none;
  epoch: one Dreamer.train_world_model epoch at B = 256, T = 15 with replay =
      "curious", replay_episodes "ignore" against "respect", the same Dreamer
      in the same process, the two alternating (the ring does not change
      between epochs, so the span pass does not run inside the timed epochs:
      that is the steady state between two rollouts).

CarRacing widths, default init, fp32.  HIP events on the stream, a warm-up
then 3 x reps repetitions per path; min / max of the 3 per-call means.  Needs
the GPU.  The parent commit's figures come from its own
tools/replay_priority_timing.py run in the same session.

    python tools/replay_episodes_timing.py [--out profiles/replay_episodes_timing.txt]
"""
import numpy as np
import torch

from timing_common import alternate, fill_ring, setup, warm_up, write_out


def main():
    args, d = setup("replay_episodes_timing", 10)
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    dev = d.device
    B, T, S = 256, d.horizon, 64
    d.batch_size = B
    fill_ring(d, B)
    buf = d.buffer
    stream = hip.stream()
    g = np.random.default_rng(0)
    lines = [
        "Episode-aware replay, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32.",
        "tools/replay_episodes_timing.py: HIP events on the stream, warm-up then 3 x N calls per path;",
        "us per call, min / max of the 3 means (an event interval around back-to-back launches: launch gaps included).",
        "",
        f"  kernels on bare arrays, S = {S}, B = {B} (3 x 200 calls each):",
    ]
    rng_state = hip.adhoc(dev).state
    for cap in (100_000, 1_000_000):
        pri = torch.from_numpy(np.exp(g.uniform(np.log(0.04), np.log(1e5), cap)).astype(np.float32)).to(dev)
        cont_np = np.ones(cap, dtype=np.float32)
        first_np = np.zeros(cap, dtype=np.uint8)
        ends = np.cumsum(g.integers(500, 1500, cap // 1000))
        ends = ends[ends < cap - 1]
        cont_np[ends[::3]] = 0.0
        cont_np[ends[1::3]] = 0.0
        first_np[ends[2::3] + 1] = 1
        cont, first = torch.from_numpy(cont_np).to(dev), torch.from_numpy(first_np).to(dev)
        span = torch.empty(cap, dtype=torch.int32, device=dev)
        n_valid = torch.zeros(1, dtype=torch.int64, device=dev)
        starts = torch.empty(B, dtype=torch.int64, device=dev)
        prob = torch.empty(B, device=dev)
        ws = torch.empty(L.query("dr_replay_sample_workspace_bytes", cap), dtype=torch.uint8, device=dev)
        ws2 = torch.empty(L.query("dr_replay_spans_workspace_bytes", cap), dtype=torch.uint8, device=dev)

        def spans():
            L.call("dr_replay_spans", cap, cap, cap // 2, L.ptr(cont), L.ptr(first), S, L.ptr(span), L.ptr(n_valid),
                   L.ptr(ws2), ws2.numel(), stream)

        def sample():
            L.call("dr_replay_sample", cap, cap, cap // 2, S, B, L.ptr(pri), 0.01 ** 0.7, None, rng_state.data_ptr(),
                   5 << 17, L.ptr(starts), L.ptr(prob), L.ptr(ws), ws.numel(), stream)

        def masked(p):
            def run():
                L.call("dr_replay_sample_spans", cap, cap, cap // 2, S, B, p, 0.01 ** 0.7, L.ptr(span), None,
                       rng_state.data_ptr(), 5 << 17, L.ptr(starts), L.ptr(prob), L.ptr(ws), ws.numel(), stream)
            return run

        with_p, without = masked(L.ptr(pri)), masked(None)
        warm_up(spans, sample)
        warm_up(with_p, without)
        sp, a = alternate(spans, sample, 200)
        b, c = alternate(with_p, without, 200)
        lines += [f"    cap = {cap:>9,d}  dr_replay_spans (3 launches)        {min(sp):8.1f} / {max(sp):8.1f}"
                  f"   ({int(n_valid.item()):,d} valid starts; 2 x 5 cap bytes read, 4 cap written)",
                  f"    cap = {cap:>9,d}  dr_replay_sample                    {min(a):8.1f} / {max(a):8.1f}",
                  f"    cap = {cap:>9,d}  dr_replay_sample_spans, priorities  {min(b):8.1f} / {max(b):8.1f}",
                  f"    cap = {cap:>9,d}  dr_replay_sample_spans, none        {min(c):8.1f} / {max(c):8.1f}"]
    lines.append("")

    buf.replay = "curious"

    def epoch(mode):
        def run():
            buf.replay_episodes = mode
            d.train_world_model()
        return run

    ign, res = epoch("ignore"), epoch("respect")
    warm_up(ign, res)
    a, b = alternate(ign, res, args.reps)
    lines += [
        f"  one train_world_model epoch, replay = curious, B = {B}, T = {T}, ring of {buf.size} slots "
        f"(3 x {args.reps} epochs per mode,",
        "  the modes alternating):",
        f"    replay_episodes = ignore    {min(a):10.1f} / {max(a):10.1f}",
        f"    replay_episodes = respect   {min(b):10.1f} / {max(b):10.1f}",
        f"    respect - ignore            {min(b) - max(a):10.1f} ... {max(b) - min(a):.1f}   "
        f"(spread of the ignore means: {max(a) - min(a):.1f})",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
