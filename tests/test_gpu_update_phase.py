"""The update phase at the batches where its kernels change path: the BPTT
(dr_imagine_fwd + dr_imagine_bwd, launch form) at B = 128 (the smallest batch
on the weight-plane path), B = 256 (the hidden-state gradient with the fused
GRU backward on its 16 x 48 LayerNorm-backward tile: one dispatch round) and
B = 512 (64-row tiles), and the critic's weight gradients
(dr_critic_loss_bwd) at B (H + 1) = 384 rows of the full-width critic.

The BPTT cases follow tests/test_gpu_persistent.py's
test_bptt_on_narrow_stream_vs_oracle: the actor gradient of
L = sum(g_mu mu + g_sigma sigma) through the H-step unroll against the
oracle's autograd, |d| <= 2e-3 |ref| + 2e-4 max|ref| per tensor.  bf16 mode
takes tests/test_gpu_bf16.py's bounds: no flipped draw on the widely guarded
noise (flip fraction <= 1e-3), actor gradient normwise relative <= 2e-2.
The critic case takes test_gpu_primitives.py's critic-gradient bound against
float64 autograd: |d| <= 1e-4 |ref| + 1e-5 max|ref| per tensor."""
import pytest
import torch

from baseline_case import TieGuard
from formula import FULL
from gpu_helpers import close
from oracle import dreamer_oracle as O
from widths_cases import bptt_case, critic_case

pytestmark = pytest.mark.gpu
R, C, A, HD = 32, 32, 3, 600


@pytest.mark.parametrize("B,H", [(128, 3), (256, 2), (512, 2)])
def test_bptt_actor_gradients_vs_oracle(B, H, gpu):
    c = bptt_case(FULL, B, H, gpu)
    got, ref_g = c.got, c.ref_g
    for k, g_, r_ in zip(O.ACTOR_KEYS, got, ref_g):
        scale = float(r_.abs().max()) + 1e-12
        print(f"B{B} H{H} grad {k}: max|d| {float((g_ - r_).abs().max()):.3g} of max|ref| {scale:.3g}")
        close(g_, r_, 2e-3, 2e-4 * scale, f"B{B} H{H}: grad {k}")


def test_bptt_actor_gradients_bf16(gpu):
    from test_gpu_bf16 import BF16_TIE_REL, BF16_TIE_SCALE, _nw
    B, H = 256, 2
    c = bptt_case(FULL, B, H, gpu, "bf16", TieGuard(BF16_TIE_REL, BF16_TIE_SCALE))
    got, ref_g, lat, lat_ref = c.got, c.ref_g, c.out[0], c.ref[0]
    flips = float((lat.reshape(-1, C).argmax(-1) != lat_ref.reshape(-1, C).argmax(-1)).float().mean())
    err = _nw(torch.cat([t.reshape(-1) for t in got]), torch.cat([t.reshape(-1) for t in ref_g]))
    print(f"bf16 B{B} H{H}: flip fraction {flips:.3g}, actor gradient normwise rel err {err:.3g}")
    assert flips <= 1e-3
    assert err <= 2e-2


def test_critic_weight_gradients_vs_float64(gpu):
    B, H = 128, 2
    c = critic_case(FULL, B, H, gpu)
    loss, want = c.loss, c.want
    assert abs(float(loss) - want) <= 1e-4 * abs(want), (float(loss), want)
    for k, g_gpu, g_ref in c.grads:
        scale = float(g_ref.abs().max())
        assert scale > 0
        print(f"critic grad {k}: max|d| {float((g_gpu.cpu() - g_ref.float()).abs().max()):.3g} of {scale:.3g}")
        close(g_gpu, g_ref.float(), 1e-4, 1e-5 * scale, f"critic grad {k}")
