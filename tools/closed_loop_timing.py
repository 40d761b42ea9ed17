"""Time Dreamer.closed_loop against the composition of older API calls that
produces the same tensors (profiles/closed_loop_timing.txt).

  (a) Dreamer.closed_loop: replay gather, dr_encoder_features on the ring's u8
      frames, dr_observe_trace, dr_latent_stats, dr_categorical_sample on the
      prior logits, dr_decoder_fwd twice, dr_frame_metrics twice -- and its
      split into those stages;
  (b) Buffer window gather to f32, Encoder.encode on frame 0 and T - 1 calls of
      WorldModel.observe_step, the dynamics_predictor module on the hiddens, a
      torch KL / entropy, two decoder module calls, a torch squared error.

CarRacing widths, default init, B = 64, T = 32, fp32.  HIP events on the
stream, a warm-up then 3 x 20 repetitions per path, the two paths alternating;
min / max of the 3 per-call means.  Needs the GPU.

    python tools/closed_loop_timing.py [--out profiles/closed_loop_timing.txt]
"""
import torch

from timing_common import HBM_BYTES_PER_S, alternate, fill_ring, setup, stage_lines, staged, warm_up, write_out

STAGES = ("gather", "encoder", "trace", "stats", "prior_sample", "decoder", "metrics")


def main():
    args, d = setup("closed_loop_timing", 20)
    dev = d.device
    B, T = 64, 32
    S = d.sequence_length
    R, C = d.latent_state_dims
    st = fill_ring(d, B)
    wm = d.world_model

    def new_path(mark=None):
        return d.closed_loop(starts=st, length=T, _mark=mark)

    def old_path():
        m = d.buffer._mirror()
        idx = (st[:, None] + torch.arange(S, device=dev)[None, :]) % d.buffer.capacity
        obs, act = m["frames"][idx].float(), m["actions"][idx]  # the f32 windows Buffer.sample_sequences returns
        x = obs[:, :T] / 255.0 - 0.5
        h = torch.zeros(B, 1, d.hidden_state_dims, device=dev)
        lg, z = wm.encoder._hip(h, x[:, 0:1], sample=True)
        z, lg = z.view(B, 1, R, C), lg.view(B, 1, R, C)
        zs, hs, lgs = [z], [h], [lg]
        for t in range(1, T):
            z, h, lg = wm.observe_step(z, h, act[:, t - 1:t], x[:, t:t + 1])
            zs.append(z)
            hs.append(h)
            lgs.append(lg)
        lat, hid, post = torch.cat(zs, 1), torch.cat(hs, 1), torch.cat(lgs, 1)
        prior = wm.dynamics_predictor.logit_net(hid).view(B, T, R, C)
        lp, lq = torch.log_softmax(post, -1), torch.log_softmax(prior, -1)
        kl = (lp.exp() * (lp - lq)).sum((-1, -2))
        hq, hp = -(lp.exp() * lp).sum((-1, -2)), -(lq.exp() * lq).sum((-1, -2))
        zp = torch.nn.functional.one_hot(torch.distributions.Categorical(logits=prior).sample(), C).float()
        mu_q, mu_p = wm.decoder(hid, lat), wm.decoder(hid, zp)
        return kl, hq, hp, (mu_q - x).pow(2).flatten(2).sum(-1), (mu_p - x).pow(2).flatten(2).sum(-1)

    with torch.no_grad():
        warm_up(new_path, old_path)
        a, b = alternate(new_path, old_path, args.reps)
        split = [staged(STAGES, new_path, args.reps) for _ in range(3)]
    sbytes = B * T * (2 * R * C * 4 + 3 * 4)
    lines = [
        "Closed-loop posterior trace, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"B = {B} windows, T = {T} steps ({B * T} frames encoded, 2 x {B * T} frames decoded).",
        f"tools/closed_loop_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  (a) Dreamer.closed_loop (gather, dr_encoder_features on the u8 ring, dr_observe_trace, dr_latent_stats,",
        "      dr_categorical_sample on the prior logits, 2 x dr_decoder_fwd, 2 x dr_frame_metrics)",
        "  (b) f32 window gather, Encoder.encode + (T - 1) x WorldModel.observe_step, dynamics_predictor module,",
        "      torch KL / entropies, torch Categorical sample, 2 decoder module calls, torch squared errors",
        "      (the older calls that give the same tensors)",
        "",
        f"  (a) closed_loop    {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) older calls    {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)          {min(b) / max(a):10.2f} ... {max(b) / min(a):.2f}",
        "",
        "  stages of (a), us (events between the stages' launches; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 12)
    sv = [s["stats"] for s in split]
    lines += [
        "",
        f"  dr_latent_stats moves {sbytes / 1e6:.2f} MB (two [B*T][R*C] f32 logit arrays read, three f32 per row written):",
        f"  {sbytes / (min(sv) * 1e-6) / 1e12:.3f} TB/s at its fastest mean, "
        f"{sbytes / (min(sv) * 1e-6) / HBM_BYTES_PER_S:.3f} of the {HBM_BYTES_PER_S / 1e12:.0f} TB/s HBM peak",
        "  (the stage time is an event interval around one launch, so it includes the launch gap; the",
        "  kernel's own time was not measured).",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
