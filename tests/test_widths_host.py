"""The oracle side of tests/test_gpu_widths.py, without a GPU: the
configs off the tested width sets (widths_cases.WIDTHS) construct on the CPU,
the oracle runs the dream, the world-model step and the float64 critic at
every (config, batch) the GPU tests use, and the tie guard stays under its cap
(<= 1e-3 of a case's draws) for the oracle alone.  With cpu_init the GPU tests
see the same parameters, inputs and noise, so these are their guard counts."""
import pytest
import torch

from formula import replay_data
from widths_cases import CONV_WIDTHS, WIDTHS, bptt_oracle, critic_oracle, guard_cap, widths_config, wm_oracle

DREAM_BATCHES = (4, 20, 128)
DREAM_H = 3
CRITIC_SHAPES = ((20, 2), (128, 2))       # B (H + 1) = 60 and 384 rows
WM_SHAPES = ((4, 4), (128, 3))
NAMES = sorted(WIDTHS)
CONV_WM_SHAPES = ((4, 4), (24, 3))        # the conv-stack configs (widths_cases.CONV_WIDTHS): 128 and 576 draws
CONV_NAMES = sorted(CONV_WIDTHS)


def wm_replay(cfg):
    return replay_data(512, tuple(cfg["observation_dims"]), cfg["action_dims"])


@pytest.mark.parametrize("name", NAMES)
def test_config_constructs_on_cpu(name):
    from dreamer_amd import Dreamer
    cfg = widths_config(name)
    d = Dreamer(cfg, "cpu")
    R, C = cfg["latent_state_dims"]
    Hd, A = cfg["hidden_state_dims"], cfg["action_dims"]
    sd = d.state_dict()
    assert tuple(sd["world_model.sequence_model.GRU.weight_ih"].shape) == (3 * Hd, R * C + A)
    assert tuple(sd["agent.actor.base_net.0.weight"].shape) == (cfg["hidden_layer_actor_1_size"], Hd + R * C)
    assert tuple(sd["agent.actor.base_net.3.weight"].shape) == (cfg["hidden_layer_actor_2_size"],
                                                                cfg["hidden_layer_actor_1_size"])
    assert tuple(sd["agent.critic.value_net.6.weight"].shape) == (cfg["critic_reward_buckets"],
                                                                  cfg["hidden_layer_critic_2_size"])
    assert tuple(sd["world_model.dynamics_predictor.logit_net.6.weight"].shape) == (
        R * C, cfg["dyn_pred_hidden_num_nodes_2"])


@pytest.mark.parametrize("B", DREAM_BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_dream(name, B):
    c = bptt_oracle(widths_config(name), B, DREAM_H, "cpu")
    guard_cap(c.guard)
    assert c.guard.draws == DREAM_H * B * widths_config(name)["latent_state_dims"][0]
    print(f"{name} B{B}: dream guarded {c.guard.guarded}/{c.guard.draws} draws")
    for t in c.ref + tuple(c.ref_g):
        assert bool(torch.isfinite(t).all())
    assert any(float(g.abs().max()) > 0 for g in c.ref_g)


@pytest.mark.parametrize("B,H", CRITIC_SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_critic(name, B, H):
    c = critic_oracle(widths_config(name), B, H, "cpu")
    assert c.want > 0 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in c.g64)


@pytest.mark.parametrize("B,T", WM_SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_wm_step(name, B, T):
    cfg = widths_config(name)
    d, wm, _, ref, q, names, P0, tg = wm_oracle(cfg, B, T, "cpu", wm_replay(cfg))
    guard_cap(tg)
    assert tg.draws == T * B * cfg["latent_state_dims"][0]
    print(f"{name} B{B} T{T}: WM step guarded {tg.guarded}/{tg.draws} draws, norm before clipping "
          f"{float(ref['norm']):.1f}")
    assert float(ref["norm"]) > 100.0  # the clip path is live
    assert bool(torch.isfinite(ref["total"])) and all(bool(torch.isfinite(g).all()) for g in ref["grads_clipped"])


@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_config_constructs_on_cpu(name):
    from dreamer_amd import Dreamer
    cfg = widths_config(name)
    sd = Dreamer(cfg, "cpu").state_dict()
    H, W = cfg["observation_dims"]
    e1, e2 = cfg["encoder_filter_num_1"], cfg["encoder_filter_num_2"]
    d1, d2 = cfg["decoder_filter_num_1"], cfg["decoder_filter_num_2"]
    assert tuple(sd["world_model.encoder.feature_extractor.0.weight"].shape) == (e1, 3, 4, 4)
    assert tuple(sd["world_model.encoder.feature_extractor.6.weight"].shape) == (4 * e2, 2 * e2, 4, 4)
    assert sd["world_model.encoder.latent_mapper.0.weight"].shape[1] == 4 * e2 * (H // 16) * (W // 16) + cfg[
        "hidden_state_dims"]
    assert tuple(sd["world_model.decoder.image_builder.0.weight"].shape) == (4 * d2, 2 * d2, 4, 4)
    assert tuple(sd["world_model.decoder.image_builder.6.weight"].shape) == (d1, 3, 4, 4)


@pytest.mark.parametrize("B,T", CONV_WM_SHAPES)
@pytest.mark.parametrize("name", CONV_NAMES)
def test_oracle_wm_step_conv_stacks(name, B, T):
    """The conv-stack configs' oracle stage: no guarded draw of the 128 / 576, gradient norms of 198 to 828."""
    cfg = widths_config(name)
    d, wm, _, ref, q, names, P0, tg = wm_oracle(cfg, B, T, "cpu", wm_replay(cfg))
    guard_cap(tg)
    assert tg.draws == T * B * cfg["latent_state_dims"][0] == {4: 128, 24: 576}[B]
    print(f"{name} B{B} T{T}: WM step guarded {tg.guarded}/{tg.draws} draws, norm before clipping "
          f"{float(ref['norm']):.1f}")
    assert tg.guarded == 0
    assert 190.0 < float(ref["norm"]) < 840.0  # above 100: the clip path is live
    assert bool(torch.isfinite(ref["total"])) and all(bool(torch.isfinite(g).all()) for g in ref["grads_clipped"])
