"""Phase table and timing of the fp32 conv1 + conv2 kernel (k_enc12_split3_x8):
dr_encoder_features over 8192 synthetic 64x64 frames (one train_Agent epoch's
warm-start frames at B = 256, S = 64).  Prints ms per encode, a sha256 of the
features (two library variants whose sums are bitwise the same print the same)
and, with the timestamp build (tools/build_e12_ts.sh, DREAMER_LIB_VARIANT=e12ts),
us per phase of the first tiles of the first workgroups, for wave 0 and wave 4.
  DREAMER_LIB_VARIANT=e12ts python tools/enc12_probe.py      (GPU box)"""
import ctypes as C
import hashlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WGS, TILES, MARKS = 4, 4, 8  # E12_TS_* of conv_split.hip
PHASES = ["conv1", "barrier", "conv2", "exchange", "staging", "epilogue"]  # between marks 0..6


def main():
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    from formula import FULL
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    d = Dreamer(dict(FULL), dev)
    wm = d.world_model
    dims = wm.dims(d.agent)
    enc = wm.packed()
    n = int(os.environ.get("ENC12_FRAMES", "8192"))
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (n, 3, 64, 64), generator=g, dtype=torch.uint8).to(dev)
    starts = torch.arange(n, dtype=torch.int64, device=dev)
    fr = L.dr_frames(L.ptr(frames), n, L.ptr(starts), None, 0, 0, 1, 0)
    feat = torch.empty(n, dims.enc_hidden, device=dev)
    ws = torch.empty(L.query("dr_encoder_workspace_bytes", dims, n), dtype=torch.uint8, device=dev)
    run = lambda: L.call("dr_encoder_features", dims, enc, fr, n, 1, L.ptr(feat), L.ptr(ws), ws.numel(), hip.stream())
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    reps = 10
    t = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) * 1e3 / reps
    var = os.environ.get("DREAMER_LIB_VARIANT", "")
    sha = hashlib.sha256(feat.cpu().numpy().tobytes()).hexdigest()[:16]
    print(f"variant '{var}': {ms:.3f} ms per encode of {n} frames; features sha256 {sha}", flush=True)
    lib = L.load()
    if not hasattr(lib, "dr_e12_ts_read"):
        return
    buf = (C.c_longlong * (WGS * TILES * 2 * MARKS))()
    if lib.dr_e12_ts_read(buf) != 0:
        raise RuntimeError("dr_e12_ts_read failed")
    names = PHASES
    us = lambda a, b: (b - a) / 100.0  # 100 MHz constant clock
    print("us per phase (workgroup, tile ordinal, wave): " + " ".join(f"{p:>9}" for p in names) + "    period")
    tot = [[0.0] * 7 for _ in range(2)]
    cnt = 0
    for wg in range(WGS):
        for it in range(TILES):
            for kh in range(2):
                m = [buf[((wg * TILES + it) * 2 + kh) * MARKS + k] for k in range(7)]
                ph = [us(m[k], m[k + 1]) for k in range(6)]
                nxt = buf[((wg * TILES + it + 1) * 2 + kh) * MARKS] if it + 1 < TILES else 0
                period = us(m[0], nxt) if nxt else float("nan")
                print(f"  wg {wg} tile {it} wave {4 * kh}:                       " +
                      " ".join(f"{x:9.2f}" for x in ph) + f" {period:9.2f}")
                if it in (1, 2):  # steady state: neither the first tile nor the last stamped one
                    for k in range(6):
                        tot[kh][k] += ph[k]
                    tot[kh][6] += period
            cnt += 1 if it in (1, 2) else 0
    for kh in range(2):
        print(f"  mean of tiles 1-2, wave {4 * kh}:                       " +
              " ".join(f"{x / cnt:9.2f}" for x in tot[kh][:6]) + f" {tot[kh][6] / cnt:9.2f}")


if __name__ == "__main__":
    main()
