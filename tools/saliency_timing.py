"""Time the stages of Dreamer.saliency (profiles/saliency_timing.txt).

The default 64 x 64 model, B = 4 windows, T = 8 steps, stride 4: 32 source
frames of 257 variants each, 8224 variant frames in two passes (31 + 1 frames).
The yardstick is the encoder stage of the same call (existing code, about
55.8 MFLOP per frame): the occluder (about 16 bytes moved per output pixel)
should stay under a quarter of it, scores and map together under a tenth.

CarRacing widths, default init, fp32.  HIP events on the stream, a warm-up then
3 x reps calls; min / max of the 3 per-call means.  The stage marks of the two
passes add up; "encoder" also holds the window prologue's encoder over the B * T
clean frames, reported apart as "encoder (trace)".  Needs the GPU.

    python tools/saliency_timing.py [--out profiles/saliency_timing.txt]
"""
import torch

from timing_common import HBM_BYTES_PER_S, fill_ring, setup, stage_lines, staged, timed, write_out

STAGES = ("gather", "encoder (trace)", "trace", "frames", "occlude", "encoder", "posterior", "actor", "critic",
          "scores", "collect", "map")


def main():
    args, d = setup("saliency_timing", 5)
    B, T, s = 4, 8, 4
    st = fill_ring(d, B)
    H, W = 64, 64
    G = (H // s) * (W // s)
    n_var = B * T * (G + 1)

    def path(mark=None):
        first = [True]

        def m(name):  # the prologue's encoder runs before the trace: keep it apart from the variants'
            if mark is not None:
                mark("encoder (trace)" if name == "encoder" and first[0] else name)
            if name == "encoder":
                first[0] = False
        r = d.saliency(starts=st, length=T, stride=s, _mark=m)
        r.maps("actor")
        r.overlay("value", 0)
        if mark is not None:
            mark("map")
        return r

    with torch.no_grad():
        for _ in range(2):
            path()
        torch.cuda.synchronize()
        whole = [timed(path, args.reps) for _ in range(3)]
        split = [staged(STAGES, path, args.reps) for _ in range(3)]
    enc = [x["encoder"] for x in split]
    occ = [x["occlude"] for x in split]
    sm = [x["scores"] + x["map"] for x in split]
    out_bytes = n_var * 3 * H * W
    lines = [
        "Perturbation saliency on replay windows, 1 x MI355X, CarRacing widths, default init under torch.manual_seed(0),",
        f"fp32, 64 x 64 frames, B = {B} windows, T = {T} steps, stride {s}: {B * T} source frames x {G + 1} variants =",
        f"{n_var} variant frames in two passes (31 + 1 source frames).  fill = blur (sigma_b = 3), sigma_m = 4, mode draws.",
        f"tools/saliency_timing.py: HIP events on the stream, warm-up then 3 x {args.reps} calls; us per call,",
        "min / max of the 3 means.  One call = Dreamer.saliency, then maps(\"actor\") and overlay(\"value\").",
        "",
        f"  whole call         {min(whole):10.1f} / {max(whole):10.1f}",
        "",
        "  stages, us (events between the stages' launches, the two passes added up; min / max of 3 means):",
    ]
    lines += stage_lines(STAGES, split, 16)
    lines += [
        "",
        f"  occlude / encoder          {min(occ) / max(enc):.3f} ... {max(occ) / min(enc):.3f}   (target: under 0.25)",
        f"  (scores + map) / encoder   {min(sm) / max(enc):.3f} ... {max(sm) / min(enc):.3f}   (target: under 0.10)",
        f"  the occluder writes {out_bytes / 1e6:.1f} MB of variants per call: {out_bytes / (min(occ) * 1e-6) / 1e9:.0f} GB/s",
        f"  of stores at the best mean ({100.0 * out_bytes / (min(occ) * 1e-6) / HBM_BYTES_PER_S:.1f} % of the HBM peak; event",
        "  intervals around the two launches of a pass, so they include the launch gaps; the kernels' own times",
        "  were not measured).  \"collect\" is the strided torch copies of the unperturbed rows' outputs; \"map\" is two",
        "  dr_saliency_map launches and their torch scale reductions.",
    ]
    write_out(lines, args.out)


if __name__ == "__main__":
    main()
