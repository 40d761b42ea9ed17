"""What the tools/*_timing.py scripts share: the CarRacing config, the ring
fill, HIP-event timing of a path and of its stages, the warm-up / three
alternating rounds, and the write-out."""
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


def setup(name, reps):
    """(args with .out and .reps, a default-init CarRacing Dreamer on cuda:0)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=reps)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{name}: needs the GPU (no CPU path)")
    from dreamer_amd import Dreamer
    torch.manual_seed(0)
    return args, Dreamer(dict(CFG), torch.device("cuda:0"))


def fill_ring(d, B, n=1024):
    """n random transitions into the ring; B window starts as an int64 device tensor."""
    rng = np.random.default_rng(0)
    d.buffer.load_arrays(rng.integers(0, 256, (n, 3, 64, 64), dtype=np.uint8),
                         rng.uniform(-1, 1, (n, d.action_dims)).astype(np.float32),
                         rng.standard_normal(n).astype(np.float32), np.ones(n, np.float32))
    np.random.seed(0)
    return torch.as_tensor(d.buffer.sample_start_indices(B), dtype=torch.int64).to(d.device)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


def staged(stages, fn, reps):
    """Mean us per call between the marks fn(mark) makes, summed by the mark's name."""
    tot = dict.fromkeys(stages, 0.0)
    for _ in range(reps):
        ev = [(None, torch.cuda.Event(enable_timing=True))]
        ev[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))
        fn(mark)
        ev[-1][1].synchronize()
        for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
            tot[name] += a.elapsed_time(b) * 1e3
    return {k: v / reps for k, v in tot.items()}


def warm_up(path_a, path_b, n=3):
    """Code objects, workspaces, allocator."""
    for _ in range(n):
        path_a()
        path_b()
    torch.cuda.synchronize()


def alternate(path_a, path_b, reps, each_round=None):
    """Three rounds of timed(path_a), timed(path_b): the two lists of per-call means."""
    a, b = [], []
    for _ in range(3):
        a.append(timed(path_a, reps))
        b.append(timed(path_b, reps))
        if each_round is not None:
            each_round()
    return a, b


def stage_lines(stages, split, width):
    out = []
    for k in stages:
        v = [s[k] for s in split]
        out.append(f"    {k:{width}s} {min(v):10.1f} / {max(v):10.1f}")
    return out


def write_out(lines, out):
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
