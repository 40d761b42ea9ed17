"""Time Dreamer.plan against the same search written with torch ops around the
same rollout and critic calls (profiles/plan_timing.txt).

  (a) Dreamer.plan: one dr_imagine_fwd for the actor's sequences, then per
      iteration dr_plan_sample, dr_imagine_actions, dr_critic_fwd on state H in
      place, dr_plan_update -- and its split into those stages;
  (b) the same actor sequences, then per iteration torch.randn, the clamp and a
      concatenation with the actor's rows, the same WorldModel._imagine_actions
      and dr_critic_fwd calls, a Python discount loop over the H steps,
      torch.topk and the weighted moments in torch.

CarRacing widths, default init, E = 8 environments, N = 512 candidates (24 the
actor's), K = 64 elites, H = 15, J = 6 iterations, fp32.  HIP events on the
stream, a warm-up then 3 x reps calls per path, the two paths alternating;
min / max of the 3 per-call means.  Needs the GPU.

    python tools/plan_timing.py [--out profiles/plan_timing.txt]
"""
import torch

from timing_common import alternate, setup, stage_lines, staged, warm_up, write_out

STAGES_A = ("policy", "sample", "rollout", "critic", "update", "stats")
STAGES_B = ("policy", "sample", "rollout", "critic", "score", "refit")


def main():
    args, d = setup("plan_timing", 10)
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    from dreamer_amd.plan import _policy_sequences, plan_dims
    dev = d.device
    E, N, N_pi, K, H, J = 8, 512, 24, 64, 15, 6
    temperature, momentum, std_init, std_min, std_max = 0.5, 0.1, 0.5, 0.05, 2.0
    R, C = d.latent_state_dims
    A, Hd = d.action_dims, d.hidden_state_dims
    wm, ag = d.world_model, d.agent
    gamma = ag.gamma
    B = E * N
    g = torch.Generator().manual_seed(1)
    h = (torch.randn(E, Hd, generator=g) * 0.5).to(dev)
    z = torch.nn.functional.one_hot(torch.randn(E, R, C, generator=g).argmax(-1), C).float().reshape(E, R * C).to(dev)

    def new_path(mark=None):
        return d.plan(z, h, horizon=H, candidates=N, policy_candidates=N_pi, elites=K, iterations=J,
                      temperature=temperature, momentum=momentum, std_init=std_init, std_min=std_min,
                      std_max=std_max, _mark=mark)

    def old_path(mark=None):
        mark = mark or (lambda name: None)
        ag._ensure_flat()
        dm = plan_dims(d)
        hB, zB = h.repeat_interleave(N, 0), z.repeat_interleave(N, 0)
        pol = _policy_sequences(d, dm, E, N, N_pi, H, z, h, None, None, True).view(E, N_pi, H, A)
        mark("policy")
        mean = torch.zeros(E, H, A, device=dev)
        std = torch.full((E, H, A), std_init, device=dev)
        v = torch.empty(B, device=dev)
        ws = hip.workspace(dev).get("plan_crit", L.query("dr_critic_workspace_bytes", dm, B, 0))
        for _ in range(J):
            eps = torch.randn(E, N - N_pi, H, A, device=dev)
            cand = torch.cat((pol, (mean[:, None] + std[:, None] * eps).clamp(-1.0, 1.0)), dim=1).contiguous()
            mark("sample")
            lat, hid, rew, cont = wm._imagine_actions(dm, B, H, zB, hB, cand.data_ptr(), H * A, A, None)
            mark("rollout")
            L.call("dr_critic_fwd", dm, ag.critic_struct(), B, hid.data_ptr() + 4 * H * Hd, (H + 1) * Hd,
                   lat.data_ptr() + 4 * H * R * C, (H + 1) * R * C, None, L.ptr(v), None, L.ptr(ws), ws.numel(),
                   hip.stream())
            mark("critic")
            r, c = rew.view(B, H), cont.view(B, H)
            G = v
            for k in reversed(range(H)):
                G = r[:, k] + gamma * c[:, k] * G
            G = G.view(E, N)
            G = torch.where(torch.isfinite(G), G, torch.full_like(G, float("-inf")))
            mark("score")
            top, idx = G.topk(K, dim=1)
            w = torch.exp((top - top[:, :1]) / temperature)
            W = w.sum(1)
            el = cand.gather(1, idx[:, :, None, None].expand(-1, -1, H, A))
            m = (w[:, :, None, None] * el).sum(1) / W[:, None, None]
            s = ((w[:, :, None, None] * (el - m[:, None]) ** 2).sum(1) / W[:, None, None]).sqrt()
            mean = momentum * mean + (1.0 - momentum) * m
            std = s.clamp(std_min, std_max)
            mark("refit")
        return mean, std

    with torch.no_grad():
        warm_up(new_path, old_path, 2)
        a, b = alternate(new_path, old_path, args.reps)
        split_a = [staged(STAGES_A, new_path, args.reps) for _ in range(3)]
        split_b = [staged(STAGES_B, old_path, args.reps) for _ in range(3)]
    lines = [
        "Latent planning, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"E = {E} environments, N = {N} candidates ({N_pi} the actor's), K = {K} elites, H = {H}, J = {J} iterations",
        f"({B} rollout rows per iteration), temperature {temperature}, bootstrap from the critic, Philox draws.",
        f"tools/plan_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  (a) Dreamer.plan (dr_imagine_fwd once; per iteration dr_plan_sample, dr_imagine_actions, dr_critic_fwd on",
        "      state H in place, dr_plan_update; the result's curves once at the end)",
        "  (b) the same dr_imagine_fwd; per iteration torch.randn, clamp and cat, the same dr_imagine_actions and",
        "      dr_critic_fwd calls, a Python discount loop over H, torch.topk, weighted moments in torch",
        "",
        f"  (a) Dreamer.plan   {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) torch search   {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)          {min(b) / max(a):10.3f} ... {max(b) / min(a):.3f}",
        f"  (b) - (a), per iteration: {(min(b) - max(a)) / J:.1f} ... {(max(b) - min(a)) / J:.1f} us",
        "",
        f"  stages of (a), us per call, the {J} iterations summed (events between the stages' launches; min / max of 3",
        "  means):",
    ]
    lines += stage_lines(STAGES_A, split_a, 12)
    lines += ["", "  stages of (b), likewise:"]
    lines += stage_lines(STAGES_B, split_b, 12)
    lines += [
        "",
        "  (event intervals around the launches, so they include the launch gaps and the output allocations; the",
        "  kernels' own times were not measured.  sample + update of (a) are the two new kernels; sample + score +",
        "  refit of (b) are the torch ops they replace.)",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
