"""Time Dreamer.dream_trace by stage, and dr_dream_stats against the
composition it replaces (profiles/dream_trace_timing.txt).

  (a) dr_dream_stats: one launch, every output;
  (b) the same outputs from dr_lambda_returns x 2 (lambda and lambda = 1),
      dr_action_logprob and torch ops (the advantages, a cumprod for the
      weights, the saturation count, mean / population std reductions over the
      dreams, the ranking), on the same device tensors.

CarRacing widths, default init, B = 64 windows, M = 8 dreams, context 32,
horizon 15, fp32.  HIP events on the stream, a warm-up then 3 x 10 repetitions
per path, the two paths alternating; min / max of the 3 per-call means.  Needs
the GPU.

    python tools/dream_trace_timing.py [--out profiles/dream_trace_timing.txt]
"""
import torch

from timing_common import alternate, fill_ring, setup, stage_lines, staged, warm_up, write_out

STAGES = ("gather", "encoder", "scan", "replicate", "dream", "critics", "stats", "decoder")


def main():
    args, d = setup("dream_trace_timing", 10)
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    from dreamer_amd.dream_trace import PER_DREAM, PER_WINDOW, dream_stats, dream_trace
    from dreamer_amd.futures import best_index
    B, M, Tc, H = 64, 8, 32, 15
    N, A = B * M, d.action_dims
    st = fill_ring(d, B)
    ag = d.agent
    gamma, lam, sat = ag.gamma, ag.lambda_, 0.99

    def trace(mark=None):
        return dream_trace(d, starts=st, context=Tc, horizon=H, samples=M, _mark=mark)

    with torch.no_grad():
        res = trace()
        c = lambda t, *s: t.reshape(N, *s).contiguous()
        rew, cont = c(res.rewards, H), c(res.continues, H)
        Vt, V = c(res.value_target, H + 1), c(res.value, H + 1)
        mus, sgs, act = c(res.mus, H, A), c(res.sigmas, H, A), c(res.actions, H, A)
        norm = res.norm
        stream = hip.stream()

        def path_a():
            return dream_stats(B, M, H, A, rew, cont, Vt, V, mus, sgs, act, gamma, lam, norm, sat)

        def path_b():
            Rl, Rmc, logp, base = (torch.empty(N, H, device=d.device) for _ in range(4))
            L.call("dr_lambda_returns", N, H, L.ptr(rew), L.ptr(cont), L.ptr(Vt), gamma, lam, L.ptr(Rl), stream)
            L.call("dr_lambda_returns", N, H, L.ptr(rew), L.ptr(cont), L.ptr(Vt), gamma, 1.0, L.ptr(Rmc), stream)
            L.call("dr_action_logprob", N, H, A, L.ptr(mus), L.ptr(sgs), L.ptr(act), H * A, A, L.ptr(logp), None,
                   L.ptr(base), stream)
            adv = Rl - V[:, :H]
            w = torch.cat((torch.ones(N, 1, device=d.device), (gamma * cont).cumprod(1)), 1)
            o = dict(R_lambda=Rl, R_mc=Rmc, adv=adv, adv_norm=adv / norm, weight=w, logp=logp, base_entropy=base,
                     saturated=(act.abs() >= sat).sum(-1, dtype=torch.int32))
            o = {k: v.view(B, M, *v.shape[1:]) for k, v in o.items()}
            for name, x in (("reward", rew.view(B, M, H)), ("ret", o["R_lambda"]), ("logp", o["logp"])):
                o[name + "_mean"], o[name + "_std"] = x.mean(1), x.std(1, unbiased=False)
            o["alive"] = o["weight"].mean(1)
            o["action_spread"] = act.view(B, M, H, A).var(1, unbiased=False).mean(-1).sqrt()
            mc0 = o["R_mc"][:, :, 0]
            fin = torch.isfinite(mc0)
            inf = torch.full_like(mc0, float("inf"))
            o["best"] = best_index(torch.where(fin, -mc0, inf)).int()
            o["worst"] = best_index(torch.where(fin, mc0, inf)).int()
            o["n_finite"] = fin.sum(1, dtype=torch.int32)
            return o

        warm_up(path_a, path_b)
        ra, rb = path_a(), path_b()
        torch.cuda.synchronize()
        agree = {k: float((ra[k].float() - rb[k].float()).abs().max()) for k in PER_DREAM + PER_WINDOW}
        a, b = alternate(path_a, path_b, args.reps)
        for _ in range(3):
            trace()
        torch.cuda.synchronize()
        split = [staged(STAGES, trace, args.reps) for _ in range(3)]
        whole = [sum(s.values()) for s in split]
    lines = [
        "Dream trace, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"B = {B} windows x M = {M} dreams = {N} rollout rows, context {Tc}, horizon {H}",
        f"({B * Tc} context frames encoded, {N * (H + 1)} states valued twice and decoded).",
        f"tools/dream_trace_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  stages of Dreamer.dream_trace, us (events between the stages' launches; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 9)
    lines += [
        f"    {'sum':9s} {min(whole):10.1f} / {max(whole):10.1f}",
        "",
        "  the statistics on one result's tensors:",
        "  (a) dr_dream_stats: one launch, every output",
        "  (b) dr_lambda_returns x 2, dr_action_logprob and torch ops for the rest (advantages, cumprod weights,",
        "      saturation count, mean / population-std reductions over the dreams, ranking)",
        "",
        f"  (a) dr_dream_stats   {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) composition      {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)            {min(b) / max(a):10.2f} ... {max(b) / min(a):.2f}",
        "  (both include the allocation of their outputs; (a) is one launch of B workgroups)",
        "",
        "  largest absolute difference between the two paths' outputs: "
        + ", ".join(f"{k} {v:.3g}" for k, v in agree.items()),
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
