"""Parity off the two tested width sets (fp32 mode).  Every other GPU test
builds the model at formula.SMALL or FULL / CAR, where each host predicate of
the engine (weight planes, the one-hot gather of the actor's first layer, the
fused LayerNorm / STE backward prologues, float4 loads of the skinny GEMM, the
fused heads tail, the tile routes) always lands on the same side.  Here:

* model level, library vs the live oracle at widths_cases.WIDTHS (hundred,
  notby4, wide, planes36 -- which predicate each flips is noted there): imagination +
  BPTT at B = 4, 20, 128 (H = 3), the critic at 60 and 384 rows against
  float64 autograd, the world-model step at (B, T) = (4, 4) and (128, 3).
  The bounds are the neighbouring tests': test_imagine_unroll's (indices
  exact under the tie guard, 2e-4 / 2e-5 on states and heads),
  test_bptt_actor_gradients_vs_oracle's (2e-3 |ref| + 2e-4 max|ref|), the
  critic's (loss 1e-4 relative, gradients 1e-4 |ref| + 1e-5 max|ref|) and
  test_wm_step_matches_oracle_at_baseline_shape's.  The tie guard is capped:
  at most 1e-3 of a case's draws (tests/test_widths_host.py: 0 or 1 here).
* dr_mlp3_fwd over an M x K x N table against O.mlp3 in float64, one row per
  GEMM route (MLP3_SHAPES), at test_blocks_teacher_forced's bound.
* the conv stack off SMALL's and FULL's (widths_cases.CONV_WIDTHS: strip, rect, mixed -- non-square frames, a
  1 x 3 feature grid, filter sets that send neighbouring layers to different kernel families): the world-model
  step at (B, T) = (4, 4) and (24, 3) under the same checks, dr_encoder_features and dr_decoder_fwd on their own.
* the supported widths: a config outside them is refused by
  the first call, before any launch, with a message naming the limit."""
import pytest
import torch

from formula import replay_data
from gpu_helpers import close, cpu, flip_report
from mlp3_shapes import MLP3_SHAPES
from oracle import dreamer_oracle as O
from test_gpu_wm import check_grads_and_params
from widths_cases import CONV_WIDTHS, WIDTHS, bptt_case, critic_case, guard_cap, widths_config, wm_case

pytestmark = pytest.mark.gpu
NAMES = sorted(WIDTHS)
CONV_NAMES = sorted(CONV_WIDTHS)


def _err(a, b):
    a, b = cpu(a), cpu(b)
    return f"max|d| {float((a - b).abs().max()):.3g} of max|ref| {float(b.abs().max()):.3g}"


def _check_dream(c, tag):
    C = c.d.latent_state_dims[1]
    guard_cap(c.guard)
    lat, hid, act, rew, cont, mu, sg = c.out
    la, lb = lat.reshape(-1, C).argmax(-1), c.ref[0].reshape(-1, C).argmax(-1)
    assert torch.equal(la, lb), f"{tag}: imagined latent flips: {int((la != lb).sum())}"
    for name, got, ref in (("hiddens", hid, c.ref[1]), ("mus", mu, c.ref[5]), ("sigmas", sg, c.ref[6]),
                           ("rewards", rew, c.ref[3]), ("continues", cont, c.ref[4])):
        print(f"{tag} {name}: {_err(got, ref.reshape(got.shape))}")
    print(f"{tag}: guarded {c.guard.guarded}/{c.guard.draws} draws")
    for name, got, ref in (("hiddens", hid, c.ref[1]), ("mus", mu, c.ref[5]), ("sigmas", sg, c.ref[6]),
                           ("rewards", rew, c.ref[3]), ("continues", cont, c.ref[4])):
        close(got, ref.reshape(got.shape), 2e-4, 2e-5, f"{tag} {name}")
    for k, g_, r_ in zip(O.ACTOR_KEYS, c.got, c.ref_g):
        scale = float(r_.abs().max()) + 1e-12
        print(f"{tag} grad {k}: max|d| {float((g_ - r_).abs().max()):.3g} of max|ref| {scale:.3g}")
    for k, g_, r_ in zip(O.ACTOR_KEYS, c.got, c.ref_g):
        scale = float(r_.abs().max()) + 1e-12
        close(g_, r_, 2e-3, 2e-4 * scale, f"{tag}: grad {k}")


@pytest.mark.parametrize("B", [4, 20, 128])
@pytest.mark.parametrize("name", NAMES)
def test_imagine_and_bptt_vs_oracle(name, B, gpu):
    H = 3
    c = bptt_case(widths_config(name), B, H, gpu, cpu_init=True)
    _check_dream(c, f"{name} B{B} H{H}")


@pytest.mark.parametrize("B,H", [(20, 2), (128, 2)])
@pytest.mark.parametrize("name", NAMES)
def test_critic_vs_float64(name, B, H, gpu):
    c = critic_case(widths_config(name), B, H, gpu, cpu_init=True)
    tag = f"{name} critic M{B * (H + 1)}"
    print(f"{tag} loss: {c.loss:.7g} (float64 {c.want:.7g})")
    for k, g_gpu, g_ref in c.grads:
        print(f"{tag} grad {k}: max|d| {float((g_gpu.cpu() - g_ref.float()).abs().max()):.3g} of "
              f"{float(g_ref.abs().max()):.3g}")
    assert abs(c.loss - c.want) <= 1e-4 * abs(c.want), (c.loss, c.want)
    for k, g_gpu, g_ref in c.grads:
        scale = float(g_ref.abs().max())
        assert scale > 0
        close(g_gpu, g_ref.float(), 1e-4, 1e-5 * scale, f"{tag} grad {k}")


def _check_wm_step(name, B, T, gpu):
    """One library step against the oracle's at widths_config(name): the checks of test_wm_step_vs_oracle."""
    cfg = widths_config(name)
    d, wm, out, ref, q, names, P0, tg = wm_case(cfg, B, T, gpu, replay_data(512, tuple(cfg["observation_dims"]),
                                                                            cfg["action_dims"]), cpu_init=True)
    tag = f"{name} WM B{B} T{T}"
    guard_cap(tg)
    C = wm.latent_num_columns
    ls = cpu(wm.last_losses)
    print(f"{tag} posterior hiddens: {_err(out['hiddens'], ref['hiddens'].transpose(0, 1))}")
    print(f"{tag} posterior logits: {_err(out['post_logits'], ref['post_logits'].transpose(0, 1))}")
    print(f"{tag}: loss {float(ls[0]):.6f} (oracle {float(ref['total']):.6f}), norm "
          f"{float(wm.last_sqnorm.sqrt()):.4f} (oracle {float(ref['norm']):.4f}), guarded {tg.guarded}/{tg.draws} draws")
    close(out["hiddens"], ref["hiddens"].transpose(0, 1), 2e-4, 2e-5, "posterior hiddens")
    close(out["post_logits"], ref["post_logits"].transpose(0, 1), 2e-4, 2e-5, "posterior logits")
    n_flip, _ = flip_report(out["latents"], ref["latents"].transpose(0, 1), ref["post_logits"].transpose(0, 1),
                            q.reshape(T, B, -1), C)
    assert n_flip == 0, f"{n_flip} posterior one-hot flips"
    for i, k in ((0, "total"), (1, "loss_pred"), (2, "kl_dyn"), (3, "kl_rep")):
        r = float(ref[k])
        assert abs(float(ls[i]) - r) <= 1e-4 * max(1.0, abs(r)), (k, float(ls[i]), r)
    assert int(wm.last_skip.item()) == 0
    assert float(ref["norm"]) > 100.0  # clip_grad_norm_(100) scales the gradients
    assert abs(float(wm.last_sqnorm.sqrt()) - float(ref["norm"])) <= 2e-4 * float(ref["norm"])
    named = {"world_model." + n: p for n, p in wm.named_parameters()}
    keys = ["world_model." + n for n in names]
    gref = dict(zip(keys, ref["grads_clipped"]))
    for k in keys:
        g_gpu = cpu(named[k].grad)
        print(f"{tag} grad {k}: max|d| {float((g_gpu - gref[k]).abs().max()):.3g} of max|ref| "
              f"{float(gref[k].abs().max()):.3g}")
    post = {}
    for k in keys:  # the oracle's own AdamW step (lr 1e-4) on its clipped gradients
        p0 = P0[k]
        post[k], _, _ = O.adamw_step(p0, gref[k], torch.zeros_like(p0), torch.zeros_like(p0), 1, 1e-4)
    n_amb = check_grads_and_params(named, keys, P0, lambda k: gref[k], lambda k: post[k],
                                   lambda t: t.reshape(-1), tag)
    print(f"{tag}: {n_amb} sign-ambiguous parameters")


@pytest.mark.parametrize("B,T", [(4, 4), (128, 3)])
@pytest.mark.parametrize("name", NAMES)
def test_wm_step_vs_oracle(name, B, T, gpu):
    _check_wm_step(name, B, T, gpu)


# ---------------------------------------------------------------------------
# the conv stack off SMALL and FULL (widths_cases.CONV_WIDTHS: strip, rect, mixed)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(4, 4), (24, 3)])
@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_stack_wm_step_vs_oracle(name, B, T, gpu):
    _check_wm_step(name, B, T, gpu)


@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_stack_encoder_and_decoder_vs_oracle(name, gpu):
    """dr_encoder_features and dr_decoder_fwd on their own at the conv-stack configs against the oracle's encoder
    conv stack + feature projection and its decoder_forward, rtol 1e-4 / atol 1e-5 (test_decoder_forward's)."""
    import torch.nn.functional as F
    from test_gpu_bf16 import _features
    from widths_cases import build_dreamer
    cfg = widths_config(name, batch_size=4, horizon=3)
    d, P = build_dreamer(cfg, gpu, cpu_init=True)
    wm = d.world_model
    H, W = cfg["observation_dims"]
    R, C = cfg["latent_state_dims"]
    g = torch.Generator().manual_seed(11)
    for n in (1, 13):  # one frame; several frames in one pixel tile with a ragged tail
        frames = torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)
        got = _features(wm.packed(), wm.dims(d.agent), frames, gpu)
        x = O.normalise_obs(frames.float())
        for i in range(4):
            x = F.silu(F.conv2d(x, P[f"world_model.encoder.feature_extractor.{2 * i}.weight"],
                                P[f"world_model.encoder.feature_extractor.{2 * i}.bias"], stride=2, padding=1))
        flat = x.flatten(1)
        ref = (flat @ P["world_model.encoder.latent_mapper.0.weight"][:, :flat.shape[1]].t()
               + P["world_model.encoder.latent_mapper.0.bias"])
        print(f"{name} encoder features n{n}: {_err(got, ref)}")
        close(got, ref, 1e-4, 1e-5, f"{name} encoder features n{n}")
    h = torch.randn(3, 2, cfg["hidden_state_dims"], generator=g)
    z = torch.nn.functional.one_hot(torch.randn(3, 2, R, C, generator=g).argmax(-1), C).float()
    with torch.no_grad():
        mu = wm.decoder(h.to(gpu), z.to(gpu))
    ref = O.decoder_forward(h, z, P, (wm.observation_dim_x, wm.observation_dim_y))
    print(f"{name} decoder mu: {_err(mu, ref)}")
    close(mu, ref, 1e-4, 1e-5, f"{name} decoder mu")


# ---------------------------------------------------------------------------
# dr_mlp3_fwd over MLP3_SHAPES (tests/mlp3_shapes.py: one case per GEMM route,
# the routes themselves pinned without a GPU by tests/test_gemm_plan_host.py)
# ---------------------------------------------------------------------------


def _mlp3_params(in_dim, h1, h2, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    P = {}
    for i, (o, k) in (("0", (h1, in_dim)), ("3", (h2, h1)), ("6", (n_out, h2))):
        P[f"m.{i}.weight"] = rn(o, k) / k ** 0.5
        P[f"m.{i}.bias"] = 0.05 * rn(o)
    for i, k in (("1", h1), ("4", h2)):
        P[f"m.{i}.weight"] = 1.0 + 0.1 * (2 * torch.rand(k, generator=g) - 1)
        P[f"m.{i}.bias"] = 0.05 * rn(k)
    return P, g


@pytest.mark.parametrize("M,in_h,in_z,h1,h2,n_out,how", MLP3_SHAPES)
def test_mlp3_shape_sweep(M, in_h, in_z, h1, h2, n_out, how, gpu):
    from dreamer_amd import hip
    from dreamer_amd import _lib as L
    P, g = _mlp3_params(in_h + in_z, h1, h2, n_out, seed=M * 7 + h1)
    h = torch.randn(M, in_h, generator=g)
    z = torch.randn(M, in_z, generator=g) if in_z else None
    x = h if z is None else torch.cat([h, z], -1)
    ref = O.mlp3(x.double(), {k: v.double() for k, v in P.items()}, "m")
    Pd = {k: v.to(gpu).contiguous() for k, v in P.items()}
    lin = lambda i: L.dr_linear(L.ptr(Pd[f"m.{i}.weight"]), L.ptr(Pd[f"m.{i}.bias"]))
    m = L.dr_mlp3(lin("0"), lin("1"), lin("3"), lin("4"), lin("6"))
    if how == "packed":
        hd = h.to(gpu).contiguous()
        hp, ldh = hd.data_ptr(), in_h
    elif how == "ldh65":
        hd = torch.zeros(M, in_h + 1, device=gpu)
        hd[:, :in_h] = h.to(gpu)
        hp, ldh = hd.data_ptr(), in_h + 1
    else:  # the rows start one float past a 16-byte boundary
        hd = torch.zeros(M * in_h + 4, device=gpu)
        hd[1:1 + M * in_h] = h.to(gpu).reshape(-1)
        hp, ldh = hd.data_ptr() + 4, in_h
        assert hd.data_ptr() % 16 == 0
    zd = None if z is None else z.to(gpu).contiguous()
    out = torch.full((M, n_out), float("nan"), device=gpu)
    ws = torch.zeros(4 * M * (h1 + h2) + 1024, dtype=torch.uint8, device=gpu)
    L.call("dr_mlp3_fwd", m, M, in_h, hp, ldh, in_z, L.ptr(zd), in_z, h1, h2, n_out, L.ptr(out), n_out, L.ptr(ws),
           ws.numel(), hip.stream())
    torch.cuda.synchronize()
    ref = ref.float()
    scale = max(1.0, float(ref.abs().max()))
    print(f"mlp3 M{M} in {in_h}+{in_z} h {h1}/{h2} N{n_out} {how}: {_err(out, ref)}")
    close(out, ref, 1e-4, 1e-5 * scale, f"mlp3 M{M} K{in_h + in_z} h {h1}/{h2} N{n_out} {how}")


# ---------------------------------------------------------------------------
# the supported widths, refused up front
# ---------------------------------------------------------------------------
OUTSIDE = [
    # (config change, the limit's field, the value, words of the message)
    (dict(hidden_state_dims=90), "hidden", 90, "multiple of 4"),
    (dict(latent_state_dims=[10, 8]), "rows", 10, "multiple of 4"),
    (dict(latent_state_dims=[40, 8]), "rows", 40, "at most 32"),
    (dict(latent_state_dims=[12, 12]), "cols", 12, "divide 32"),
    (dict(action_dims=9), "action", 9, "at most 8"),
    # filter counts no conv kernel is instantiated for: the imagination runs no conv, the training step refuses
    (dict(encoder_filter_num_1=24), "enc_f1", 24, "one of 8, 16, 32, 64, 128, 256"),
    (dict(decoder_filter_num_1=128), "dec_f1", 128, "one of 8, 16, 32, 64"),
]
CONV_FIELDS = ("enc_f1", "enc_f2", "dec_f1", "dec_f2")


def test_outside_supported_widths_is_refused_up_front(gpu):
    """hidden 90, rows 10, rows 40, cols 12, actions 9, and the filter counts
    enc_f1 = 24 and dec_f1 = 128 (training step only): the model builds; the
    first _imagine_raw and the first train_step_hip raise DR_E_INVALID with
    the limit and the value before any launch (dims_envelope is the entry
    points' first statement after their null checks; what precedes the call
    in Python are size queries and allocations).  A config inside the widths
    then still runs in the same process."""
    from dreamer_amd import Dreamer
    from dreamer_amd import _lib as L
    for over, field, value, words in OUTSIDE:
        cfg = widths_config("hundred", batch_size=4, horizon=3, **over)
        torch.manual_seed(0)
        d = Dreamer(cfg, gpu)
        R, C = cfg["latent_state_dims"]
        A, Hd = cfg["action_dims"], cfg["hidden_state_dims"]
        B, T = 4, 3
        g = torch.Generator().manual_seed(1)
        z0 = torch.nn.functional.one_hot(torch.randint(0, C, (B, 1, R), generator=g), C).float().to(gpu)
        h0 = torch.randn(B, 1, Hd, generator=g).to(gpu)
        if field in CONV_FIELDS:
            d._imagine_raw(z0, h0)  # no conv stack behind the imagination: these widths do not concern it
        else:
            with pytest.raises(L.HipError) as ei:
                d._imagine_raw(z0, h0)
            msg = str(ei.value)
            assert ei.value.code == L.DR_E_INVALID and "dr_imagine_fwd" in msg, msg
            assert f"{field} = {value}" in msg and words in msg and "supported widths" in msg, msg
        fr, ac, rw, ct = replay_data(16, (32, 32), A)
        obs = torch.tensor(fr[:B * T].reshape(B, T, 3, 32, 32), dtype=torch.float32).to(gpu)
        act = torch.tensor(ac[:B * T].reshape(B, T, A)).to(gpu)
        rew = torch.tensor(rw[:B * T].reshape(B, T, 1)).to(gpu)
        cont = torch.tensor(ct[:B * T].reshape(B, T, 1)).to(gpu)
        with pytest.raises(L.HipError) as ei:
            d.world_model.train_step_hip(obs, act, rew, cont)
        msg = str(ei.value)
        assert ei.value.code == L.DR_E_INVALID and "dr_wm_train" in msg, msg
        assert f"{field} = {value}" in msg and words in msg and "supported widths" in msg, msg
        print(f"{over}: {msg}")
    torch.cuda.synchronize()
    c = bptt_case(widths_config("hundred"), 4, 3, gpu, cpu_init=True)
    _check_dream(c, "hundred B4 H3 after the refusals")
