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
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak

CFG = dict(
    hidden_state_dims=600, latent_state_dims=[32, 32], action_dims=3, observation_dims=[64, 64],
    encoder_filter_num_1=32, encoder_filter_num_2=64, encoder_hidden_layer_nodes=200,
    decoder_filter_num_1=32, decoder_filter_num_2=64, decoder_hidden_layer_nodes=200,
    dyn_pred_hidden_num_nodes_1=200, dyn_pred_hidden_num_nodes_2=200,
    rew_pred_hidden_num_nodes_1=200, rew_pred_hidden_num_nodes_2=200,
    cont_pred_hidden_num_nodes_1=200, cont_pred_hidden_num_nodes_2=200,
    hidden_layer_actor_1_size=200, hidden_layer_actor_2_size=200,
    hidden_layer_critic_1_size=200, hidden_layer_critic_2_size=200, device="cuda",
    horizon=15, batch_size=64, nu=0.0003, lambda_=0.95, gamma=0.99, buffer_size=4096,
    sequence_length=64, seed=42, training_iterations=1, random_iterations=1,
    actor_lr=0.00008, actor_betas=[0.9, 0.999], actor_eps=0.00001, critic_lr=0.0001,
    critic_betas=[0.9, 0.999], critic_eps=0.00001, AC_epochs=1, world_model_lr=0.0001,
    world_model_betas=[0.9, 0.999], world_model_eps=0.00001, WM_epochs=1,
    beta_prediction=1.0, beta_dynamics=0.5, beta_representation=0.1, critic_reward_buckets=255,
)
STAGES = ("gather", "encoder", "scan", "unroll", "decoder", "metrics")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("open_loop_timing: needs the GPU (no CPU path)")
    from dreamer_amd import Dreamer
    dev = torch.device("cuda:0")
    B, Tc, H = 64, 32, 15
    torch.manual_seed(0)
    d = Dreamer(dict(CFG), dev)
    S, A = d.sequence_length, d.action_dims
    rng = np.random.default_rng(0)
    n = 1024
    d.buffer.load_arrays(rng.integers(0, 256, (n, 3, 64, 64), dtype=np.uint8),
                         rng.uniform(-1, 1, (n, A)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
                         np.ones(n, np.float32))
    np.random.seed(0)
    starts = d.buffer.sample_start_indices(B)
    st = torch.as_tensor(starts, dtype=torch.int64).to(dev)
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

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    def staged(reps):
        tot = dict.fromkeys(STAGES, 0.0)
        for _ in range(reps):
            ev = [torch.cuda.Event(enable_timing=True)]
            ev[0].record()

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append(e)
            new_path(mark)
            ev[-1].synchronize()
            for name, a, b in zip(STAGES, ev[:-1], ev[1:]):
                tot[name] += a.elapsed_time(b) * 1e3
        return {k: v / reps for k, v in tot.items()}

    with torch.no_grad():
        for _ in range(3):  # warm-up: code objects, workspaces, allocator
            new_path()
            old_path()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(3):  # alternate the two paths
            a.append(timed(new_path, args.reps))
            b.append(timed(old_path, args.reps))
        split = [staged(args.reps) for _ in range(3)]
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
    for k in STAGES:
        v = [s[k] for s in split]
        lines.append(f"    {k:8s} {min(v):10.1f} / {max(v):10.1f}")
    mv = [s["metrics"] for s in split]
    lines += [
        "",
        f"  dr_frame_metrics moves {mbytes / 1e6:.1f} MB (4 + 1 + 1 + 1 bytes per element: mu and the u8 truth read,",
        f"  two u8 frames written): {mbytes / (min(mv) * 1e-6) / 1e12:.2f} TB/s at its fastest mean, "
        f"{mbytes / (min(mv) * 1e-6) / HBM_BYTES_PER_S:.2f} of the {HBM_BYTES_PER_S / 1e12:.0f} TB/s HBM peak",
        "  (the stage time is an event interval around one launch, so it includes the launch gap).",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
