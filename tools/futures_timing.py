"""Time Dreamer.sample_futures against the same call with its two new kernels
replaced by torch ops (profiles/futures_timing.txt).

  (a) Dreamer.sample_futures: replay gather, dr_encoder_features on the ring's
      u8 frames, dr_observe_scan (B windows, once), replication to B*M rows,
      dr_imagine_actions, dr_decoder_fwd, dr_frame_metrics, dr_frame_ssim,
      dr_ensemble_metrics (+ dr_frame_ssim on the mean frames) -- and its split
      into those stages;
  (b) the same call with the SSIM / ensemble stage done by torch: SSIM by a
      grouped conv2d with the same 11 x 11 window on the five planes, the mean,
      variance and u8 frames by torch reductions.

CarRacing widths, default init, B = 16 windows, M = 16 samples, context 32,
horizon 15, fp32.  HIP events on the stream, a warm-up then 3 x 10 repetitions
per path, the two paths alternating; min / max of the 3 per-call means.  Needs
the GPU.

    python tools/futures_timing.py [--out profiles/futures_timing.txt]
"""
import numpy as np
import torch

from timing_common import alternate, fill_ring, setup, stage_lines, staged, warm_up, write_out

STAGES = ("gather", "encoder", "scan", "replicate", "unroll", "decoder", "metrics", "ssim", "ensemble")


def torch_metrics(window2d):
    """The SSIM / ensemble stage in torch ops, with sample_futures' _metrics signature."""
    C1, C2 = 1e-4, 9e-4

    def ssim(mu, x):  # (N,3,h,w) each -> (N,)
        p = mu.clamp(-0.5, 0.5)
        planes = torch.cat((p, x, p * p, x * x, p * x), dim=1)  # (N,15,h,w)
        f = torch.nn.functional.conv2d(planes, window2d.expand(15, 1, 11, 11), groups=15)
        mp, mx, pp, xx, px = f.split(3, dim=1)
        vp, vx, c = pp - mp * mp, xx - mx * mx, px - mp * mx
        up, ux = mp + 0.5, mx + 0.5
        smap = ((2 * up * ux + C1) * (2 * c + C2)) / ((up * up + ux * ux + C1) * (vp + vx + C2))
        return smap.flatten(2).mean(-1).mean(-1)

    def metrics(mu, truth_rep, truth, mu_mean, sq_mean, spread, do_ssim, frames_true=None):
        B, M, K = mu.shape[:3]
        x = frames_true.float() / 255.0 - 0.5  # (B,K,3,h,w)
        ss = ss_ens = None
        if do_ssim:
            xr = x.unsqueeze(1).expand(B, M, K, *x.shape[2:]).reshape(-1, *x.shape[2:])
            ss = ssim(mu.reshape(-1, *mu.shape[3:]), xr).view(B, M, K)
        mean = mu.mean(1)
        var = mu.var(1, unbiased=False)
        mu_mean.copy_(mean)
        sq_mean.copy_((mean - x).pow(2).flatten(2).sum(-1))
        spread.copy_(var.flatten(2).sum(-1))
        f_mean = ((mean + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8)
        f_std = (255.0 * var.sqrt()).round().clamp(max=255).to(torch.uint8)
        if do_ssim:
            ss_ens = ssim(mean.reshape(-1, *mean.shape[2:]), x.reshape(-1, *x.shape[2:])).view(B, K)
        return f_mean, f_std, ss, ss_ens

    return metrics


def main():
    args, d = setup("futures_timing", 10)
    from dreamer_amd.futures import sample_futures
    from dreamer_amd.open_loop import target_slots
    dev = d.device
    B, M, Tc, H = 16, 16, 32, 15
    st = fill_ring(d, B)
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / 4.5)
    w = torch.from_numpy((g / g.sum()).astype(np.float32)).to(dev)
    tm = torch_metrics(torch.outer(w, w).view(1, 1, 11, 11))
    frames = d.buffer._mirror()["frames"]
    fslots = target_slots(st.cpu(), Tc, H, d.buffer.capacity)[0].to(dev)
    hook_ev = []

    def hook(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tm(*a, frames_true=frames[fslots])
        e1.record()
        hook_ev.append((e0, e1))
        return out

    def path_a(mark=None):
        return sample_futures(d, starts=st, context=Tc, horizon=H, samples=M, _mark=mark)

    def path_b():
        return sample_futures(d, starts=st, context=Tc, horizon=H, samples=M, _metrics=hook)

    hb = []

    def torch_stage():  # (b)'s torch stage over the round's calls
        hb.append(sum(e0.elapsed_time(e1) for e0, e1 in hook_ev) * 1e3 / len(hook_ev))
        hook_ev.clear()

    with torch.no_grad():
        warm_up(path_a, path_b)
        # the two paths on the same explicit draws: how far the torch stage is from the kernels
        R, C = d.latent_state_dims
        gen = torch.Generator(device=dev).manual_seed(1)
        nz = (torch.empty(Tc, B * R, C, device=dev).exponential_(generator=gen),
              torch.empty(H, B * M * R, C, device=dev).exponential_(generator=gen))
        ra = sample_futures(d, starts=st, context=Tc, horizon=H, samples=M, noise=nz)
        rb = sample_futures(d, starts=st, context=Tc, horizon=H, samples=M, noise=nz, _metrics=hook)
        torch.cuda.synchronize()
        agree = {k: float((getattr(ra, k).float() - getattr(rb, k).float()).abs().max())
                 for k in ("ssim", "ssim_ensemble", "sqerr_mean", "spread", "frames_mean", "frames_std")}
        hook_ev.clear()
        a, b = alternate(path_a, path_b, args.reps, each_round=torch_stage)
        split = [staged(STAGES, path_a, args.reps) for _ in range(3)]
    rows = B * M
    lines = [
        "Sampled futures, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0), fp32,",
        f"B = {B} windows x M = {M} samples = {rows} rollout rows, context {Tc}, horizon {H}",
        f"({B * Tc} context frames encoded, {rows * (H + 1)} frames decoded).",
        f"tools/futures_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls per path,",
        "the paths alternating; us per call, min / max of the 3 means.",
        "",
        "  (a) Dreamer.sample_futures (gather, dr_encoder_features on the u8 ring, dr_observe_scan, replication,",
        "      dr_imagine_actions, dr_decoder_fwd, dr_frame_metrics, dr_frame_ssim, dr_ensemble_metrics +",
        "      dr_frame_ssim on the mean frames)",
        "  (b) the same call with the SSIM / ensemble stage in torch ops (grouped conv2d with the same window,",
        "      mean / var reductions, round / clamp to u8)",
        "",
        f"  (a) sample_futures   {min(a):10.1f} / {max(a):10.1f}",
        f"  (b) torch metrics    {min(b):10.1f} / {max(b):10.1f}",
        f"  (b) / (a)            {min(b) / max(a):10.2f} ... {max(b) / min(a):.2f}",
        f"  (b)'s torch stage    {min(hb):10.1f} / {max(hb):10.1f}",
        "",
        "  stages of (a), us (events between the stages' launches; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 9)
    lines += ["", "  largest absolute difference between the two paths' outputs on the same explicit draws: "
              + ", ".join(f"{k} {v:.3g}" for k, v in agree.items())]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
