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

import primitives_ref as PR
from baseline_case import TieGuard
from gpu_helpers import close
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
R, C, A, HD = 32, 32, 3, 600


def _bptt_case(B, H, gpu, precision="fp32", guard=None):
    """(actor gradient tensors of the library, the oracle's, imagined latents
    of both) for one dr_imagine_fwd + dr_imagine_bwd call."""
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    from formula import FULL
    cfg = dict(FULL)
    cfg.update(batch_size=B, horizon=H, precision=precision)
    torch.manual_seed(0)
    d = Dreamer(cfg, gpu)
    P = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    g = torch.Generator().manual_seed(31 + B)
    h0 = torch.randn(B, 1, HD, generator=g)
    z0 = torch.nn.functional.one_hot(torch.randint(0, C, (B, 1, R), generator=g), C).float()
    eps = torch.randn(H, B, 1, A, generator=g)
    q = torch.empty(H, B * R, C).exponential_(generator=g)
    g_mu = torch.randn(B, H, A, generator=g)
    g_sg = torch.randn(B, H, A, generator=g)
    leaves = []
    for k in O.ACTOR_KEYS:
        P["agent." + k] = P["agent." + k].clone().requires_grad_(True)
        leaves.append(P["agent." + k])
    with (guard or TieGuard()):
        ref = O.dream(z0, h0, P, eps, q, H, R, C)
    loss = (g_mu * ref[5]).sum() + (g_sg * ref[6]).sum()
    ref_g = torch.autograd.grad(loss, leaves)
    dims = d.world_model.dims(d.agent)
    assert not L.query("dr_persistent_kernels", dims, B, 32, H) & 4, "launch-form BPTT expected"
    out, tape = d._imagine_raw(z0.to(gpu), h0.to(gpu), eps=eps.to(gpu), q=q.to(gpu))
    ag = d.agent
    f = ag.fa
    grad_flat = torch.zeros_like(f.flat)
    gptr = lambda n: grad_flat.data_ptr() + 4 * f.offsets[n]
    gs = L.dr_actor(*(L.dr_linear(gptr(w), gptr(b)) for w, b in (
        ("base_net.0.weight", "base_net.0.bias"), ("base_net.1.weight", "base_net.1.bias"),
        ("base_net.3.weight", "base_net.3.bias"), ("base_net.4.weight", "base_net.4.bias"),
        ("mu_head.weight", "mu_head.bias"), ("log_sig_head.weight", "log_sig_head.bias"))))
    ws = torch.zeros(L.query("dr_imagine_workspace_bytes", dims, B, H), dtype=torch.uint8, device=gpu)
    gm, gsd = g_mu.to(gpu).contiguous(), g_sg.to(gpu).contiguous()
    L.call("dr_imagine_bwd", dims, d.world_model.packed(), ag.actor_struct(), B, H, L.ptr(out[0]),
           L.ptr(out[1]), L.ptr(out[2]), L.ptr(gm), L.ptr(gsd), None, None, None, L.ptr(tape), gs, L.ptr(ws),
           ws.numel(), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    got = []
    for k, r_ in zip(O.ACTOR_KEYS, ref_g):
        name = k.split(".", 1)[1]
        got.append(grad_flat[f.offsets[name]:f.offsets[name] + r_.numel()].view(r_.shape).cpu())
    return got, ref_g, out[0].cpu(), ref[0]


@pytest.mark.parametrize("B,H", [(128, 3), (256, 2), (512, 2)])
def test_bptt_actor_gradients_vs_oracle(B, H, gpu):
    got, ref_g, _, _ = _bptt_case(B, H, gpu)
    for k, g_, r_ in zip(O.ACTOR_KEYS, got, ref_g):
        scale = float(r_.abs().max()) + 1e-12
        print(f"B{B} H{H} grad {k}: max|d| {float((g_ - r_).abs().max()):.3g} of max|ref| {scale:.3g}")
        close(g_, r_, 2e-3, 2e-4 * scale, f"B{B} H{H}: grad {k}")


def test_bptt_actor_gradients_bf16(gpu):
    from test_gpu_bf16 import BF16_TIE_REL, BF16_TIE_SCALE, _nw
    B, H = 256, 2
    got, ref_g, lat, lat_ref = _bptt_case(B, H, gpu, "bf16", TieGuard(BF16_TIE_REL, BF16_TIE_SCALE))
    flips = float((lat.reshape(-1, C).argmax(-1) != lat_ref.reshape(-1, C).argmax(-1)).float().mean())
    err = _nw(torch.cat([t.reshape(-1) for t in got]), torch.cat([t.reshape(-1) for t in ref_g]))
    print(f"bf16 B{B} H{H}: flip fraction {flips:.3g}, actor gradient normwise rel err {err:.3g}")
    assert flips <= 1e-3
    assert err <= 2e-2


def test_critic_weight_gradients_vs_float64(gpu):
    from dreamer_amd import Dreamer, hip
    from dreamer_amd import _lib as L
    from formula import FULL
    B, H = 128, 2
    M = B * (H + 1)
    cfg = dict(FULL)
    cfg.update(batch_size=B, horizon=H)
    torch.manual_seed(0)
    d = Dreamer(cfg, gpu)
    ag = d.agent
    ag._ensure_flat()
    P = {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}
    b = ag.critic.buckets_crit.cpu()
    g = torch.Generator().manual_seed(77)
    h = torch.tanh(torch.randn(B, H + 1, HD, generator=g))
    z = torch.nn.functional.one_hot(torch.randint(0, C, (B, H + 1, R), generator=g), C).float().reshape(B, H + 1, R * C)
    Rt = (torch.randn(B, H, generator=g) * 30).float()
    dims = d.world_model.dims(ag)
    st = hip.stream()
    hd, zd, Rd = h.to(gpu).contiguous(), z.to(gpu).contiguous(), Rt.to(gpu).contiguous()
    tape = torch.zeros(L.query("dr_critic_tape_bytes", dims, M), dtype=torch.uint8, device=gpu)
    ws = torch.zeros(L.query("dr_critic_workspace_bytes", dims, B, H), dtype=torch.uint8, device=gpu)
    V = torch.empty(B, H + 1, device=gpu)
    loss = torch.full((1,), float("nan"), device=gpu)
    L.call("dr_critic_fwd", dims, ag.critic_struct(), M, L.ptr(hd), HD, L.ptr(zd), R * C, None, L.ptr(V),
           L.ptr(tape), L.ptr(ws), ws.numel(), st)
    ag.fc.grad.zero_()
    L.call("dr_critic_loss_bwd", dims, ag.critic_struct(), B, H, L.ptr(hd), L.ptr(zd), L.ptr(Rd), L.ptr(tape),
           1.0 / (B * H), L.ptr(loss), ag.critic_struct(grad=True), L.ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()
    grad = ag.fc.grad.clone()
    keys = [O.AG + k for k in O.CRITIC_KEYS]
    P64 = {k: P[k].double().clone().requires_grad_(True) for k in keys}
    lg64 = O.critic_logits(h.double(), z.double(), P64)[:, :-1]
    want = PR.critic_ce_rows(lg64, Rt, b).mean()
    g64 = torch.autograd.grad(want, [P64[k] for k in keys])
    want = float(want.detach())
    assert abs(float(loss) - want) <= 1e-4 * abs(want), (float(loss), want)
    for k, g_ref in zip(O.CRITIC_KEYS, g64):
        o = ag.fc.offsets[k.split(".", 1)[1]]
        g_gpu = grad[o:o + g_ref.numel()].view(g_ref.shape)
        scale = float(g_ref.abs().max())
        assert scale > 0
        print(f"critic grad {k}: max|d| {float((g_gpu.cpu() - g_ref.float()).abs().max()):.3g} of {scale:.3g}")
        close(g_gpu, g_ref.float(), 1e-4, 1e-5 * scale, f"critic grad {k}")
