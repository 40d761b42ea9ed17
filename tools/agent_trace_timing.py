"""Time Dreamer.agent_trace against the composition of older API calls that
produces the same tensors (profiles/agent_trace_timing.txt).

  (a) Dreamer.agent_trace: replay gather, dr_encoder_features on the ring's u8
      frames, dr_observe_trace (states only), dr_critic_fwd twice, dr_actor_act,
      dr_replay_returns, dr_value_stats, dr_action_logprob -- and its split into
      those stages;
  (b) Buffer window gather to f32, Encoder.encode on frame 0 and T - 1 calls of
      WorldModel.observe_step, the critic module (logits and value) and the
      target critic module, the actor module, torch's TransformedDistribution
      log_prob, a Python lambda-return loop (twice: lambda and 1) and a torch
      two-hot cross-entropy, entropy and spread.

CarRacing widths, default init, B = 64, T = 32, fp32.  HIP events on the
stream, a warm-up then 3 x 20 repetitions per path, the two paths alternating;
min / max of the 3 per-call means.  Needs the GPU.

    python tools/agent_trace_timing.py [--out profiles/agent_trace_timing.txt]
"""
import torch

from timing_common import alternate, fill_ring, setup, stage_lines, staged, warm_up, write_out

STAGES = ("gather", "encoder", "trace", "critics", "actor", "returns", "value_stats", "logprob")
NEW_KERNELS = ("returns", "value_stats", "logprob")


def main():
    args, d = setup("agent_trace_timing", 20)
    from dreamer_amd.utils import symexp, symlog, to_twohot
    dev = d.device
    B, T = 64, 32
    S = d.sequence_length
    R, C = d.latent_state_dims
    st = fill_ring(d, B)
    wm, ag = d.world_model, d.agent
    gamma, lam = ag.gamma, ag.lambda_
    TD = torch.distributions

    def new_path(mark=None):
        return d.agent_trace(starts=st, length=T, _mark=mark)

    def returns(r, c, V, lm):  # Agent.py:156-172 as the reference writes it
        nxt = r[:, -1] + gamma * c[:, -1] * V[:, -1]
        seq = [nxt]
        for t in reversed(range(T - 2)):
            nxt = r[:, t] + gamma * c[:, t] * ((1 - lm) * V[:, t + 1] + lm * nxt)
            seq.insert(0, nxt)
        return torch.stack(seq, dim=1)

    def old_path():
        m = d.buffer._mirror()
        idx = (st[:, None] + torch.arange(S, device=dev)[None, :]) % d.buffer.capacity
        obs, act = m["frames"][idx].float(), m["actions"][idx]  # the f32 windows Buffer.sample_sequences returns
        rew, cont = m["rewards"][idx].squeeze(-1), m["continues"][idx].squeeze(-1)
        x = obs[:, :T] / 255.0 - 0.5
        h = torch.zeros(B, 1, d.hidden_state_dims, device=dev)
        lg, z = wm.encoder._hip(h, x[:, 0:1], sample=True)
        z = z.view(B, 1, R, C)
        zs, hs = [z], [h]
        for t in range(1, T):
            z, h, _ = wm.observe_step(z, h, act[:, t - 1:t], x[:, t:t + 1])
            zs.append(z)
            hs.append(h)
        lat, hid = torch.cat(zs, 1), torch.cat(hs, 1)
        logits = ag.critic(hid, lat)
        V, Vt = ag.critic.value(hid, lat).squeeze(-1), ag.target_critic.value(hid, lat).squeeze(-1)
        _, mu, sg = ag.actor.act(hid, lat, deterministic=True)
        dist = TD.TransformedDistribution(TD.Normal(mu, sg), [TD.transforms.TanhTransform()])
        logp = dist.log_prob(torch.clamp(act[:, :T], -1.0 + 1e-6, 1.0 - 1e-6)).sum(-1)
        r, c = symexp(rew[:, :T - 1]), cont[:, :T - 1]
        Rl, Rmc = returns(r, c, Vt, lam), returns(r, c, Vt, 1.0)
        td = (r + gamma * c * Vt[:, 1:]) - Vt[:, :-1]
        bk = ag.critic.buckets_crit
        ls = torch.log_softmax(logits, -1)
        ce = -(to_twohot(symlog(Rl).unsqueeze(-1), bk) * ls[:, :-1]).sum(-1)
        p = ls.exp()
        ent = -(p * ls).sum(-1)
        spread = (p * (bk - (p * bk).sum(-1, keepdim=True)) ** 2).sum(-1).sqrt()
        return V, logp, Rl, Rmc, td, ce, ent, spread

    with torch.no_grad():
        warm_up(new_path, old_path)
        a, b = alternate(new_path, old_path, args.reps)
        split = [staged(STAGES, new_path, args.reps) for _ in range(3)]
    lines = [
        "Agent trace on replay windows, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"B = {B} windows, T = {T} steps ({B * T} frames encoded, {B * T} states through both critics and the actor).",
        f"tools/agent_trace_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  (a) Dreamer.agent_trace (gather, dr_encoder_features on the u8 ring, dr_observe_trace without prior and",
        "      heads, 2 x dr_critic_fwd, dr_actor_act, 2 x dr_replay_returns, dr_value_stats, dr_action_logprob)",
        "  (b) f32 window gather, Encoder.encode + (T - 1) x WorldModel.observe_step, critic module (logits, value),",
        "      target critic module, actor module, torch TransformedDistribution.log_prob, Python lambda-return",
        "      loops (lambda and 1), torch two-hot CE, entropy and spread (the older calls that give the same tensors)",
        "",
        f"  (a) agent_trace    {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) older calls    {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)          {min(b) / max(a):10.2f} ... {max(b) / min(a):.2f}",
        "",
        "  stages of (a), us (events between the stages' launches; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 12)
    nk = [sum(s[k] for k in NEW_KERNELS) for s in split]
    lines += [
        "",
        f"  the three new kernels together (returns holds two launches of dr_replay_returns): {min(nk):.1f} / {max(nk):.1f} us",
        "  (event intervals around the launches, so they include the launch gaps and the output allocations;",
        "  the kernels' own times were not measured).",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
