"""The fp32 conv1 + conv2 kernel's tile schedule (k_enc12_split3_x8: one
persistent workgroup per CU walking half-frame tiles, the next tile's input
loads, the carried staging, the exchanged tap halves and the zero padding
columns of the conv1 planes) at the smallest frame counts at which each part
first runs, through the C ABI (dr_encoder_features) against torch's f32 conv
stack on the CPU.  Every frame is checked on its own: worst frame <= 1e-5
normwise, the bound of tests/test_gpu_bf16.py's fp32 checks (f32 summation
order only; the kernel measures 2.7e-7 there).

With C compute units (a tile is half a frame, workgroup w walks tiles w, w + C, ...):
  n = 1        2 tiles: no workgroup has a next tile
  n = 3        an odd frame count, 6 workgroups
  n = C/2 + 1  exactly two workgroups walk a second tile: the first use of the
               input prefetch and of the carried staging
  n = C + 3    six workgroups walk three tiles, the others two: the steady
               state and the drain
The frame pool holds one frame of all 0, one of all 255 and one whose first
and last rows and columns differ from the interior (the padding rows and
columns), placed so that they fall on first, second and third tiles.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL_FRAME = 1e-5


@pytest.fixture(scope="module")
def pool(gpu):
    """(world model, dims, u8 frame pool of C + 3 frames, torch f32 reference features, C)"""
    from dreamer_amd import Dreamer
    from formula import FULL
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    torch.manual_seed(0)
    d = Dreamer(dict(FULL), gpu)
    wm = d.world_model
    g = torch.Generator().manual_seed(11)
    n = cus + 3
    frames = torch.randint(0, 256, (n, 3, 64, 64), generator=g, dtype=torch.uint8)
    frames[0] = 0                      # first tiles
    frames[cus // 2] = 255             # tiles C, C + 1: the second tile of workgroups 0 and 1
    edge = frames[n - 1]               # tiles 2 C + 4, 2 C + 5: third tiles
    edge[:] = 100
    edge[:, 0, :], edge[:, -1, :], edge[:, :, 0], edge[:, :, -1] = 255, 0, 3, 250
    P = {k: v.detach().cpu() for k, v in wm.encoder.state_dict().items()}
    x = frames.float() / 255.0 - 0.5
    for i in range(4):
        x = F.silu(F.conv2d(x, P[f"feature_extractor.{2 * i}.weight"], P[f"feature_extractor.{2 * i}.bias"],
                            stride=2, padding=1))
    flat = x.flatten(1)
    ref = flat @ P["latent_mapper.0.weight"][:, :flat.shape[1]].t() + P["latent_mapper.0.bias"]
    return wm, wm.dims(d.agent), frames, ref, cus


def _encode(wm, dims, ring, starts, B, T, t0, dev):
    """dr_encoder_features over the B x T window of a u8 ring (time-major rows f = t B + b)."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    ring = ring.contiguous().to(dev)
    starts = starts.to(dev)
    fr = L.dr_frames(L.ptr(ring), ring.shape[0], L.ptr(starts), None, 0, 0, 1, t0)
    n = B * T
    feat = torch.empty(n, dims.enc_hidden, device=dev)
    ws = torch.empty(L.query("dr_encoder_workspace_bytes", dims, n), dtype=torch.uint8, device=dev)
    L.call("dr_encoder_features", dims, wm.packed(), fr, B, T, L.ptr(feat), L.ptr(ws), ws.numel(), hip.stream())
    torch.cuda.synchronize()
    return feat.cpu()


def _worst_frame(got, ref):
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max())


@pytest.mark.parametrize("case", ["one", "three", "half_plus_one", "all_plus_three"])
def test_enc12_tile_walk_matches_torch(gpu, pool, case):
    wm, dims, frames, ref, cus = pool
    n = {"one": 1, "three": 3, "half_plus_one": cus // 2 + 1, "all_plus_three": cus + 3}[case]
    got = _encode(wm, dims, frames[:n], torch.arange(n, dtype=torch.int64), n, 1, 0, gpu)
    err = _worst_frame(got, ref[:n])
    print(f"{case}: n = {n} frames on {cus} CUs, worst frame {err:.2e}")
    assert torch.isfinite(got).all()
    assert err <= TOL_FRAME, err


def test_enc12_ring_window_wraps(gpu, pool):
    """B = 3 rows x T = 5 steps from a ring of capacity 7 at t0 = 2: every row's
    slots (starts[b] + t0 + t) % 7 wrap; compared with the same frames gathered
    on the host."""
    wm, dims, frames, ref, cus = pool
    cap, B, T, t0 = 7, 3, 5, 2
    starts = torch.tensor([1, 3, 6], dtype=torch.int64)
    slots = torch.stack([(starts + t0 + t) % cap for t in range(T)])  # [T][B]: row f = t B + b
    assert all(((starts[b] + t0 + T - 1) >= cap) for b in range(B))  # each row wraps
    got = _encode(wm, dims, frames[:cap], starts, B, T, t0, gpu)
    err = _worst_frame(got, ref[slots.flatten()])
    print(f"ring window: worst frame {err:.2e}")
    assert err <= TOL_FRAME, err
