"""Time Dreamer.open_loop against the composition of older API calls that
produces the same tensors (profiles/open_loop_timing.txt).

  (a) Dreamer.open_loop: replay gather, dr_encoder_features on the ring's u8
      frames, dr_observe_scan, dr_imagine_actions, dr_decoder_fwd,
      dr_frame_metrics -- and its split into those stages;
  (b) Buffer window gather to f32, warm_start_generator, H calls of
      WorldModel.imagine_step, one decoder module call, a torch squared-error
      reduction.

CarRacing widths, default init, B = 64, context 32, horizon 15, fp32.  HIP
events on the stream, a warm-up then 3 x 20 repetitions per path, the two paths
alternating; min / max of the 3 per-call means.  Needs the GPU.

    python tools/open_loop_timing.py [--out profiles/open_loop_timing.txt]
"""
import torch

from timing_common import HBM_BYTES_PER_S, alternate, fill_ring, setup, stage_lines, staged, warm_up, write_out

STAGES = ("gather", "encoder", "scan", "unroll", "decoder", "metrics")


def main():
    args, d = setup("open_loop_timing", 20)
    dev = d.device
    B, Tc, H = 64, 32, 15
    S = d.sequence_length
    st = fill_ring(d, B)
    wm = d.world_model

    def new_path(mark=None):
        return d.open_loop(starts=st, context=Tc, horizon=H, _mark=mark)

    def old_path():
        m = d.buffer._mirror()
        idx = (st[:, None] + torch.arange(S, device=dev)[None, :]) % d.buffer.capacity
        obs, act = m["frames"][idx].float(), m["actions"][idx]  # the f32 windows Buffer.sample_sequences returns
        z, h = d.warm_start_generator(obs[:, :2 * Tc], act[:, :2 * Tc], 2 * Tc)
        zs, hs = [z], [h]
        for k in range(1, H + 1):
            h, z, _, _ = wm.imagine_step(h, z, act[:, Tc + k - 2:Tc + k - 1])
            zs.append(z)
            hs.append(h)
        mu = wm.decoder(torch.cat(hs, 1), torch.cat(zs, 1))
        x = obs[:, Tc - 1:Tc + H] / 255.0 - 0.5
        return (mu - x).pow(2).flatten(2).sum(-1)

    with torch.no_grad():
        warm_up(new_path, old_path)
        a, b = alternate(new_path, old_path, args.reps)
        split = [staged(STAGES, new_path, args.reps) for _ in range(3)]
    frame = 3 * 64 * 64
    mbytes = B * (H + 1) * frame * (4 + 1 + 1 + 1)
    lines = [
        "Open-loop prediction, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"B = {B} windows, context {Tc}, horizon {H} ({B * Tc} context frames encoded, {B * (H + 1)} frames decoded).",
        f"tools/open_loop_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  (a) Dreamer.open_loop (gather, dr_encoder_features on the u8 ring, dr_observe_scan,",
        "      dr_imagine_actions, dr_decoder_fwd, dr_frame_metrics)",
        "  (b) f32 window gather, warm_start_generator, H x WorldModel.imagine_step, decoder module call,",
        "      torch squared-error reduction (the older calls that give the same tensors)",
        "",
        f"  (a) open_loop      {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) older calls    {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)          {min(b) / max(a):10.2f} ... {max(b) / min(a):.2f}",
        "",
        "  stages of (a), us (events between the stages' launches; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 8)
    mv = [s["metrics"] for s in split]
    lines += [
        "",
        f"  dr_frame_metrics moves {mbytes / 1e6:.1f} MB (4 + 1 + 1 + 1 bytes per element: mu and the u8 truth read,",
        f"  two u8 frames written): {mbytes / (min(mv) * 1e-6) / 1e12:.2f} TB/s at its fastest mean, "
        f"{mbytes / (min(mv) * 1e-6) / HBM_BYTES_PER_S:.2f} of the {HBM_BYTES_PER_S / 1e12:.0f} TB/s HBM peak",
        "  (the stage time is an event interval around one launch, so it includes the launch gap).",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
