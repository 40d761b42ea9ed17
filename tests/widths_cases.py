"""Configs off the two tested width sets (formula.SMALL, formula.FULL / CAR)
and the case builders shared by the tests that compare the library with the
oracle at a given config: the imagination unroll + BPTT, the critic's loss and
weight gradients, the world-model training step.  Test infrastructure only.

Each builder has an oracle stage that needs no GPU (`*_oracle`: the model, the
inputs, the CPU reference; tests/test_widths_host.py runs these alone) and a
library stage on top of it (`bptt_case`, `critic_case`, `wm_case`).

cpu_init: the parameters are the reference default init under
torch.manual_seed(0) either on the model's own device (the older tests'
cases) or, with cpu_init, on the CPU and then loaded into the model, so the
oracle stage sees the same parameters with and without a GPU (the tie-guard
counts test_widths_host.py pins are then the GPU tests' counts)."""
from types import SimpleNamespace

import numpy as np
import torch

import primitives_ref as PR
from baseline_case import TieGuard
from formula import SMALL
from oracle import dreamer_oracle as O


def _widths(hidden, latent, actions, buckets, h1, h2):
    """SMALL (32 x 32 frames, filters 8 / 16, its buffer and sequence length)
    with other widths: h1 / h2 for the prior, reward, continue, actor and
    critic; h1 for the encoder's and the decoder's hidden layer."""
    cfg = dict(SMALL)
    cfg.update(hidden_state_dims=hidden, latent_state_dims=list(latent), action_dims=actions,
               critic_reward_buckets=buckets, encoder_hidden_layer_nodes=h1, decoder_hidden_layer_nodes=h1)
    for k in ("dyn_pred_hidden_num_nodes", "rew_pred_hidden_num_nodes", "cont_pred_hidden_num_nodes"):
        cfg[k + "_1"], cfg[k + "_2"] = h1, h2
    for k in ("hidden_layer_actor", "hidden_layer_critic"):
        cfg[k + "_1_size"], cfg[k + "_2_size"] = h1, h2
    return cfg


# which host predicate of the engine each config sends to the side FULL / SMALL never take
WIDTHS = {
    # Hd % 8 != 0 (no weight planes at B >= 128), actor_h1 % 8 != 0, R not a power of two, C = 8
    # (the skinny kernel's sampler epilogue, STE backward with C / 4 = 2), h1 != h2
    "hundred": _widths(100, [12, 8], 3, 255, 36, 52),
    # every K % 4 != 0 (non-vec skinny kernel and its LN prologue), zg off (lin2 actor first layer),
    # LN-backward fallback (op_ln_silu_bwd + plain NT GEMM), N = 41 buckets, A = 1, C = 16
    "notby4": _widths(60, [4, 16], 1, 41, 30, 22),
    # K > 208 (no mlp2 tail) and > 256 (no staged rows on 64-row tiles), planes on at non-FULL N, K
    # (wsplit_np padding at N = 264), A = 8 (2A = 16), L = 896
    "wide": _widths(128, [28, 32], 8, 255, 264, 216),
    # Hd % 8 == 0 with hundred's MLPs: weight planes on at B >= 128 with N = 36 (wsplit_np pads 36 rows to 128),
    # actor planes off (actor_h1 % 8 != 0) while the GRU's are on, the BPTT's planes at N = L + A = 67 split
    # between gZ and gA
    "planes36": _widths(128, [8, 8], 3, 255, 36, 52),
}


def _stack(frame, enc, dec):
    """SMALL's MLP widths with another conv stack: frame (H, W), encoder and decoder filters (f1, f2)."""
    cfg = dict(SMALL)
    cfg.update(observation_dims=list(frame), encoder_filter_num_1=enc[0], encoder_filter_num_2=enc[1],
               decoder_filter_num_1=dec[0], decoder_filter_num_2=dec[1])
    return cfg


# which conv-family routes each stack forces that SMALL (32 x 32, 8 / 16: every layer on the f32-MFMA kernels) and
# FULL (64 x 64, 32 / 64: conv2.. and the decoder on the six-product / LDS-DMA kernels) never take
CONV_WIDTHS = {
    # feature grid 1 x 3: every f32 kernel (k_conv_nhwc, k_convT_nhwc, k_conv_wgrad, both channel sums) at h = 1,
    # non-square and with w not a power of two; the last conv writes 3 pixels per frame (no NCHW float4 epilogue
    # would fit: oh ow % 4 != 0 is refused, so this pins that the encoder's last layer at 1 x 3 has a route)
    "strip": _stack((16, 48), (8, 16), (8, 16)),
    # encoder 3 -> 16 -> 32 -> 64 -> 128: conv1 / conv2 stay on k_conv_nhwc (cin 4, 16), conv3 (32 -> 64) and conv4
    # (64 -> 128) take the six-product kernels; decoder 128 -> 64 -> 32 -> 16 -> 3: 128 -> 64 on the LDS-DMA kernel,
    # 64 -> 32 at 4 x 8 misses the all-class kernel (h % 8) and falls to k_convT_nhwc, k_convT_out3<16>
    "rect": _stack((32, 64), (16, 32), (16, 32)),
    # encoder 3 -> 32 -> 16 -> 32 -> 64: conv2 (32 -> 16) and conv3 (cin 16) have no six-product form between conv1
    # and conv4 (32 -> 64) that do; decoder 256 -> 128 -> 64 -> 8 -> 3: 256 and 128 input channels at 4 x 2 and
    # 8 x 4, 64 -> 8 on k_convT_nhwc's 16-column tile, k_convT_out3<8>
    "mixed": _stack((64, 32), (32, 16), (8, 64)),
}


def widths_config(name, **over):
    cfg = dict(WIDTHS[name] if name in WIDTHS else CONV_WIDTHS[name])
    cfg.update(over)
    return cfg


def guard_cap(tg):
    """Tie guarding is a cap on what a test leaves out: at most 1e-3 of all draws."""
    assert tg.draws > 0 and tg.guarded <= 1e-3 * tg.draws, f"tie guard touched {tg.guarded} of {tg.draws} draws"


def build_dreamer(cfg, dev, cpu_init=False):
    """(Dreamer on dev, its parameters on the CPU): default init under
    torch.manual_seed(0) (module doc for cpu_init)."""
    from dreamer_amd import Dreamer
    if cpu_init and torch.device(dev).type != "cpu":
        torch.manual_seed(0)
        src = Dreamer(dict(cfg, device="cpu"), "cpu")
        P = {k: v.detach().clone() for k, v in src.state_dict().items()}
        d = Dreamer(cfg, dev)
        d.load_state_dict({k: v.to(dev) for k, v in P.items()})
        return d, P
    torch.manual_seed(0)
    d = Dreamer(cfg, dev)
    return d, {k: v.detach().cpu().clone() for k, v in d.state_dict().items()}


# ---------------------------------------------------------------------------
# imagination unroll + BPTT (dr_imagine_fwd + dr_imagine_bwd)
# ---------------------------------------------------------------------------
def bptt_oracle(cfg, B, H, dev, precision="fp32", guard=None, cpu_init=False):
    """The model, the inputs (seed 31 + B) and the oracle's dream with the
    actor gradients of L = sum(g_mu mu + g_sigma sigma) by autograd."""
    cfg = dict(cfg)
    cfg.update(batch_size=B, horizon=H, precision=precision)
    R, C = cfg["latent_state_dims"]
    A, HD = cfg["action_dims"], cfg["hidden_state_dims"]
    d, P = build_dreamer(cfg, dev, cpu_init)
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
    guard = guard or TieGuard()
    with guard:
        ref = O.dream(z0, h0, P, eps, q, H, R, C)
    loss = (g_mu * ref[5]).sum() + (g_sg * ref[6]).sum()
    ref_g = torch.autograd.grad(loss, leaves)
    return SimpleNamespace(d=d, B=B, H=H, h0=h0, z0=z0, eps=eps, q=q, g_mu=g_mu, g_sg=g_sg,
                           ref=tuple(t.detach() for t in ref), ref_g=ref_g, guard=guard)


def bptt_case(cfg, B, H, gpu, precision="fp32", guard=None, cpu_init=False):
    """bptt_oracle plus one dr_imagine_fwd + dr_imagine_bwd call (launch form):
    .out the unroll's outputs (latents, hiddens, actions, rewards, continues,
    mus, sigmas) and .got the actor gradient tensors in O.ACTOR_KEYS order."""
    from dreamer_amd import _lib as L
    c = bptt_oracle(cfg, B, H, gpu, precision, guard, cpu_init)
    d = c.d
    dims = d.world_model.dims(d.agent)
    assert not L.query("dr_persistent_kernels", dims, B, 32, H) & 4, "launch-form BPTT expected"
    out, tape = d._imagine_raw(c.z0.to(gpu), c.h0.to(gpu), eps=c.eps.to(gpu), q=c.q.to(gpu))
    ag = d.agent
    f = ag.fa
    grad_flat = torch.zeros_like(f.flat)
    gptr = lambda n: grad_flat.data_ptr() + 4 * f.offsets[n]
    gs = L.dr_actor(*(L.dr_linear(gptr(w), gptr(b)) for w, b in (
        ("base_net.0.weight", "base_net.0.bias"), ("base_net.1.weight", "base_net.1.bias"),
        ("base_net.3.weight", "base_net.3.bias"), ("base_net.4.weight", "base_net.4.bias"),
        ("mu_head.weight", "mu_head.bias"), ("log_sig_head.weight", "log_sig_head.bias"))))
    ws = torch.zeros(L.query("dr_imagine_workspace_bytes", dims, B, H), dtype=torch.uint8, device=gpu)
    gm, gsd = c.g_mu.to(gpu).contiguous(), c.g_sg.to(gpu).contiguous()
    L.call("dr_imagine_bwd", dims, d.world_model.packed(), ag.actor_struct(), B, H, L.ptr(out[0]),
           L.ptr(out[1]), L.ptr(out[2]), L.ptr(gm), L.ptr(gsd), None, None, None, L.ptr(tape), gs, L.ptr(ws),
           ws.numel(), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    got = []
    for k, r_ in zip(O.ACTOR_KEYS, c.ref_g):
        name = k.split(".", 1)[1]
        got.append(grad_flat[f.offsets[name]:f.offsets[name] + r_.numel()].view(r_.shape).cpu())
    c.got = got
    c.out = tuple(t.cpu() for t in out)
    return c


# ---------------------------------------------------------------------------
# critic loss + weight gradients (dr_critic_fwd + dr_critic_loss_bwd)
# ---------------------------------------------------------------------------
def critic_oracle(cfg, B, H, dev, cpu_init=False):
    """The model, B (H + 1) states with returns (seed 77) and the critic's
    cross-entropy loss with its weight gradients by float64 autograd."""
    cfg = dict(cfg)
    cfg.update(batch_size=B, horizon=H)
    R, C = cfg["latent_state_dims"]
    HD = cfg["hidden_state_dims"]
    d, P = build_dreamer(cfg, dev, cpu_init)
    b = d.agent.critic.buckets_crit.cpu()
    g = torch.Generator().manual_seed(77)
    h = torch.tanh(torch.randn(B, H + 1, HD, generator=g))
    z = torch.nn.functional.one_hot(torch.randint(0, C, (B, H + 1, R), generator=g), C).float().reshape(B, H + 1, R * C)
    Rt = (torch.randn(B, H, generator=g) * 30).float()
    keys = [O.AG + k for k in O.CRITIC_KEYS]
    P64 = {k: P[k].double().clone().requires_grad_(True) for k in keys}
    lg64 = O.critic_logits(h.double(), z.double(), P64)[:, :-1]
    want = PR.critic_ce_rows(lg64, Rt, b).mean()
    g64 = torch.autograd.grad(want, [P64[k] for k in keys])
    return SimpleNamespace(d=d, B=B, H=H, h=h, z=z, Rt=Rt, want=float(want.detach()), g64=g64)


def critic_case(cfg, B, H, gpu, cpu_init=False):
    """critic_oracle plus dr_critic_fwd + dr_critic_loss_bwd on the same
    states: .loss the library's loss, .grads [(key, library gradient, float64
    gradient)] in O.CRITIC_KEYS order."""
    from dreamer_amd import hip
    from dreamer_amd import _lib as L
    c = critic_oracle(cfg, B, H, gpu, cpu_init)
    d = c.d
    M = B * (H + 1)
    R, C = d.latent_state_dims
    HD = d.hidden_state_dims
    ag = d.agent
    ag._ensure_flat()
    dims = d.world_model.dims(ag)
    st = hip.stream()
    hd, zd, Rd = c.h.to(gpu).contiguous(), c.z.to(gpu).contiguous(), c.Rt.to(gpu).contiguous()
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
    c.loss = float(loss)
    c.grads = []
    for k, g_ref in zip(O.CRITIC_KEYS, c.g64):
        o = ag.fc.offsets[k.split(".", 1)[1]]
        c.grads.append((k, grad[o:o + g_ref.numel()].view(g_ref.shape), g_ref))
    return c


# ---------------------------------------------------------------------------
# world-model training step (WorldModel.train_step_hip)
# ---------------------------------------------------------------------------
def wm_oracle(cfg, B, T, dev, replay, precision="fp32", cpu_init=False):
    """The model, B windows of T = horizon steps of `replay` (frames, actions,
    rewards, continues; starts from RandomState(300 + B)) and the oracle's step
    on the CPU with a tie-guarded posterior noise draw (seed 400 + B).
    Returns (d, wm, (obs, act, rew, cont), ref, q, names, P0, tg)."""
    cfg = dict(cfg)
    cfg.update(batch_size=B, horizon=T, precision=precision)
    d, _ = build_dreamer(cfg, dev, cpu_init)
    wm = d.world_model
    R, C = wm.latent_num_rows, wm.latent_num_columns
    frames, acts, rews, conts = replay
    n = len(frames)
    starts = np.random.RandomState(300 + B).randint(0, n - T + 1, size=B)
    idx = starts[:, None] + np.arange(T)[None, :]
    obs = torch.tensor(frames[idx], dtype=torch.float32)
    act = torch.tensor(acts[idx])
    rew = torch.tensor(rews[idx]).unsqueeze(-1)
    cont = torch.tensor(conts[idx]).unsqueeze(-1)
    q = torch.empty(T, B * R, C).exponential_(generator=torch.Generator().manual_seed(400 + B))
    names = [nm for nm, _ in wm.named_parameters()]
    P0 = {("world_model." + k): v.detach().cpu().clone() for k, v in wm.state_dict().items()}
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    torch.set_num_threads(16)
    with TieGuard() as tg:  # widens near-tie margins of q in place, the oracle's draws unchanged
        ref = O.wm_train_step(obs, act, rew, cont, P, q, R, C, T, ["world_model." + nm for nm in names],
                              betas=(wm.beta_pred, wm.beta_dyn, wm.beta_rep))
    return d, wm, (obs, act, rew, cont), ref, q, names, P0, tg


def wm_case(cfg, B, T, gpu, replay, precision="fp32", cpu_init=False):
    """wm_oracle plus the library's step (step=True) on the same windows and
    noise.  Returns (d, wm, out, ref, q, names, P0, tg)."""
    d, wm, (obs, act, rew, cont), ref, q, names, P0, tg = wm_oracle(cfg, B, T, gpu, replay, precision, cpu_init)
    out = {}
    wm.train_step_hip(obs.to(gpu), act.to(gpu), rew.to(gpu), cont.to(gpu), noise_q=q.to(gpu), outputs=out,
                      step=True)
    torch.cuda.synchronize()
    return d, wm, out, ref, q, names, P0, tg
