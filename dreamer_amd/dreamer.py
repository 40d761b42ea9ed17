"""Dreamer: the reference's top-level agent (Dreamer.py) on the MI355X engine.

Same constructor (config dict + device), attributes, methods and state_dict
layout, so train_car_racer.py runs unchanged.  train_Agent -- the metric's
unit of work -- runs as one fused device-resident epoch (engine.py); the
world-model step stays PyTorch-ROCm this round."""
import os

import numpy as np
import torch
import torch.nn as nn
from tqdm import tqdm

from . import _lib as L
from . import hip
from .agent import Agent
from .buffer import REPLAY_DEFAULTS, Buffer, check_replay, check_replay_episodes
from .utils import _sanitize_for_save
from .world_model import WorldModel


class _DreamFn(torch.autograd.Function):
    """dream_episodes as one autograd node: forward = dr_imagine_fwd, backward
    = dr_imagine_bwd (BPTT through the unroll into the actor's parameters).
    The world model receives no gradient (the reference's WM grads from this
    path are discarded, WorldModel.py:195)."""

    @staticmethod
    def forward(ctx, dreamer, z0, h0, *actor_params):
        ctx.set_materialize_grads(False)
        out, tape = dreamer._imagine_raw(z0, h0)
        ctx.dreamer, ctx.tape = dreamer, tape
        ctx.save_for_backward(out[0], out[1], out[2])
        return out

    @staticmethod
    def backward(ctx, g_lat, g_hid, g_act, g_rew, g_cont, g_mu, g_sig):
        for g, n in ((g_rew, "rewards"), (g_cont, "continues")):
            if g is not None and bool(torch.any(g != 0)):
                raise NotImplementedError(f"gradient through imagined {n} is not part of the reference's loss")
        lat, hid, act = ctx.saved_tensors
        dr = ctx.dreamer
        ag = dr.agent
        grad_flat = torch.zeros_like(ag.fa.flat)
        f = ag.fa
        gptr = lambda n: grad_flat.data_ptr() + 4 * f.offsets[n]
        gs = L.dr_actor(*(L.dr_linear(gptr(w), gptr(b)) for w, b in (
            ("base_net.0.weight", "base_net.0.bias"), ("base_net.1.weight", "base_net.1.bias"),
            ("base_net.3.weight", "base_net.3.bias"), ("base_net.4.weight", "base_net.4.bias"),
            ("mu_head.weight", "mu_head.bias"), ("log_sig_head.weight", "log_sig_head.bias"))))
        B, H1 = hid.shape[:2]
        d = dr.world_model.dims(ag)
        c = lambda t: None if t is None else t.float().contiguous()
        g_mu, g_sig, g_act, g_lat, g_hid = (c(t) for t in (g_mu, g_sig, g_act, g_lat, g_hid))
        ws = hip.workspace(hid.device).get("im_bwd", L.query("dr_imagine_workspace_bytes", d, B, H1 - 1))
        L.call("dr_imagine_bwd", d, dr.world_model.packed(), ag.actor_struct(), B, H1 - 1, L.ptr(lat), L.ptr(hid),
               L.ptr(act), L.ptr(g_mu), L.ptr(g_sig), L.ptr(g_act), L.ptr(g_lat), L.ptr(g_hid), L.ptr(ctx.tape), gs,
               L.ptr(ws), ws.numel(), hip.stream())
        grads = [grad_flat[f.offsets[n]:f.offsets[n] + p.numel()].view_as(p) for n, p in zip(f.names, f.params)]
        return (None, None, None, *grads)


class Dreamer(nn.Module):
    def __init__(self, config, device):
        super().__init__()
        c = config
        self.hidden_state_dims = c["hidden_state_dims"]
        self.action_dims = c["action_dims"]
        self.observation_dims = tuple(c["observation_dims"])
        self.latent_state_dims = tuple(c["latent_state_dims"])
        device = torch.device(device)
        self.world_model = WorldModel(
            c["hidden_state_dims"], tuple(c["latent_state_dims"]), tuple(c["observation_dims"]), c["action_dims"],
            c["horizon"], c["batch_size"], c["world_model_lr"], tuple(c["world_model_betas"]), c["world_model_eps"],
            c["beta_prediction"], c["beta_dynamics"], c["beta_representation"], c["encoder_filter_num_1"],
            c["encoder_filter_num_2"], c["encoder_hidden_layer_nodes"], c["decoder_filter_num_1"],
            c["decoder_filter_num_2"], c["decoder_hidden_layer_nodes"], c["dyn_pred_hidden_num_nodes_1"],
            c["dyn_pred_hidden_num_nodes_2"], c["rew_pred_hidden_num_nodes_1"], c["rew_pred_hidden_num_nodes_2"],
            c["critic_reward_buckets"], c["cont_pred_hidden_num_nodes_1"], c["cont_pred_hidden_num_nodes_2"],
            device=device, encoder_depth=int(c.get("encoder_depth", 4)))
        self.agent = Agent(
            c["action_dims"], tuple(c["latent_state_dims"]), c["hidden_state_dims"], c["hidden_layer_actor_1_size"],
            c["hidden_layer_actor_2_size"], c["hidden_layer_critic_1_size"], c["hidden_layer_critic_2_size"],
            c["critic_reward_buckets"], c["actor_lr"], tuple(c["actor_betas"]), c["actor_eps"], c["critic_lr"],
            tuple(c["critic_betas"]), c["critic_eps"], c["nu"], c["lambda_"], c["gamma"], device=device)
        self.buffer = Buffer(c["buffer_size"], c["sequence_length"], c["action_dims"], tuple(c["observation_dims"]),
                             device=device)
        self.horizon = c["horizon"]
        self.batch_size = c["batch_size"]
        self.sequence_length = c["sequence_length"]
        self.training_iterations = c["training_iterations"]
        self.random_iterations = c["random_iterations"]
        self.WM_epochs = c["WM_epochs"]
        self.AC_epochs = c["AC_epochs"]
        self.seed = c["seed"]
        # extra config key: "fp32" parity mode (default) or "bf16" perf mode
        self.precision = c.get("precision", "fp32")
        # on by default from round 4: bit-equal to sequential epochs
        # (test_pipelined_epochs_match_sequential), 1.04x at AC_epochs = 2 and
        # 1.16x at 10; pipeline_epochs: false restores
        # the sequential loop
        self.pipeline_epochs = bool(c.get("pipeline_epochs", True))
        self.world_model.precision = self.precision  # encoder kernels: bf16 MFMA in perf mode
        if self.precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {self.precision!r}")
        # extra config keys: "uniform" replay (default: the
        # reference's np.random starts, untouched) or "curious" -- prioritised
        # window sampling on the device (Curious Replay, Kauvar et al. 2023;
        # the defaults are the paper's constants)
        buf = self.buffer
        buf.replay = c.get("replay", "uniform")
        for k, v in REPLAY_DEFAULTS.items():
            setattr(buf, k, float(c.get(k, v)))
        check_replay(buf.replay, buf.replay_c, buf.replay_beta, buf.replay_alpha, buf.replay_eps, buf.replay_p_new)
        # extra config key: replay_episodes = "ignore" (default: windows may run across the
        # end of an episode, as the reference's do) or "respect" -- the device sampler draws only windows that
        # lie inside one stream of data, in either replay mode
        buf.replay_episodes = c.get("replay_episodes", "ignore")
        check_replay_episodes(buf.replay_episodes)
        # extra config keys: explore = "none" (default: nothing below exists) or
        # "disagreement" -- Plan2Explore's ensemble; its disagreement on imagined states is added to the
        # reward train_Agent learns from (engine.returns); Agent.train_step, the reference-API path, is left alone
        from .networks import explore_config
        ex = explore_config(c)
        self.explore = ex["explore"]
        # "entropy" (DESIGN.md 5p): the particle-entropy reward of the imagined states among themselves; no module,
        # parameter, optimiser or state of its own
        self.explore_knn, self.explore_knn_exclude = ex["explore_knn"], ex["explore_knn_exclude"]
        if self.explore != "none":
            self.explore_scale, self.explore_extrinsic = ex["explore_scale"], ex["explore_extrinsic"]
        if self.explore == "disagreement":
            from .networks import DisagreementEnsemble
            self.explorer = DisagreementEnsemble(
                c["hidden_state_dims"], c["latent_state_dims"][0] * c["latent_state_dims"][1], ex["explore_ensemble"],
                ex["explore_width"], ex["explore_lr"], tuple(c["world_model_betas"]), c["world_model_eps"],
                seed=c["seed"], device=device)
        self.device = device
        self.agent_obs = None
        self.agent_hidden = None
        self.agent_latent = None
        self.vec_obs = self.vec_hidden = self.vec_latent = None  # rollout_policy_vec's per-env state
        self._engine = None
        self.world = None  # (rank, size, group) for data-parallel train_Agent

    # ------------------------------------------------------------- imagination
    def _imagine_raw(self, z0, h0, eps=None, q=None):
        L.require_gpu(h0)
        B = h0.shape[0]
        H = self.horizon
        R, C = self.latent_state_dims
        A = self.action_dims
        dev = h0.device
        d = self.world_model.dims(self.agent)
        lat = torch.empty(B, H + 1, R, C, device=dev)
        hid = torch.empty(B, H + 1, self.hidden_state_dims, device=dev)
        act, mu, sg = (torch.empty(B, H, A, device=dev) for _ in range(3))
        rew, cont = torch.empty(B, H, 1, device=dev), torch.empty(B, H, 1, device=dev)
        tape = torch.empty(L.query("dr_imagine_tape_bytes", d, B, H), dtype=torch.uint8, device=dev)
        ws = hip.workspace(dev).get("im", L.query("dr_imagine_workspace_bytes", d, B, H))
        if eps is None and q is None:
            nz = hip.adhoc(dev).noise()
        else:
            nz = hip.explicit_noise(q=q, eps=eps, device=dev)
        z = z0.reshape(B, -1).float().contiguous()
        h = h0.reshape(B, -1).float().contiguous()
        L.call("dr_imagine_fwd", d, self.world_model.packed(), self.agent.actor_struct(), B, H, L.ptr(z), L.ptr(h),
               nz, 0, L.ptr(lat), L.ptr(hid), L.ptr(act), L.ptr(rew), L.ptr(cont), L.ptr(mu), L.ptr(sg), L.ptr(tape),
               L.ptr(ws), ws.numel(), hip.stream())
        return (lat, hid, act, rew, cont, mu, sg), tape

    def dream_episodes(self, starting_latent_state_batch, starting_hidden_state_batch):
        """Dreamer.dream_episodes (Dreamer.py:143-175) as one HIP unroll."""
        self.agent._ensure_flat()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.agent.actor.parameters()):
            return _DreamFn.apply(self, starting_latent_state_batch.detach(), starting_hidden_state_batch.detach(),
                                  *self.agent.fa.params)
        return self._imagine_raw(starting_latent_state_batch, starting_hidden_state_batch)[0]

    def warm_start_generator(self, observation_seq_batch, action_seq_batch, sequence_length):
        """Dreamer.warm_start_generator (Dreamer.py:244-262): time-batched conv
        encoder over the S/2 warm-up frames, then the posterior scan."""
        obs = observation_seq_batch.float().contiguous()
        L.require_gpu(obs)
        B, S = obs.shape[:2]
        T = sequence_length // 2
        d = self.world_model.dims(self.agent)
        wm = self.world_model.packed()
        dev = obs.device
        fe = int(np.prod(obs.shape[2:]))
        fr = L.dr_frames(None, 0, None, L.ptr(obs), S * fe, fe, 1)
        feat = torch.empty(T * B, d.enc_hidden, device=dev)
        st = hip.stream()
        ws = hip.workspace(dev).get("enc", L.query("dr_encoder_workspace_bytes", d, T * B))
        L.call("dr_encoder_features", d, wm, fr, B, T, L.ptr(feat), L.ptr(ws), ws.numel(), st)
        act = action_seq_batch.float().contiguous()
        A = act.shape[-1]
        R, C = self.latent_state_dims
        z = torch.empty(B, 1, R, C, device=dev)
        h = torch.empty(B, 1, self.hidden_state_dims, device=dev)
        ws2 = hip.workspace(dev).get("obs", L.query("dr_observe_workspace_bytes", d, B))
        L.call("dr_observe_scan", d, wm, B, T, L.ptr(feat), L.ptr(act), act.shape[1] * A, A, None, None,
               hip.adhoc(dev).noise(), L.ptr(z), L.ptr(h), None, L.ptr(ws2), ws2.numel(), st)
        return z, h

    # ------------------------------------------- world-model evaluation (HIP)
    def open_loop(self, starts=None, batch_size=None, context=None, horizon=None, sample=True, noise=None,
                  _mark=None):
        """Open-loop prediction on replay windows (open_loop.py): filter the
        first `context` frames of each window (warm_start_generator's scan,
        Dreamer.py:244-262), roll the prior forward `horizon` steps under the
        recorded actions (WorldModel.py:72-77), decode states 0..horizon and
        compare them with what the ring holds.  Returns an OpenLoopResult.

        starts: window starts (default: buffer.sample_start_indices(batch_size
        or self.batch_size)); context defaults to S // 2 (the warm start's),
        horizon to min(self.horizon, S - context).  noise: optional pair of
        explicit Exp(1) draws (q_context (Tc, B*R, C), q (H, B*R, C)), else
        Philox; sample=False takes the mode of every categorical (q == 1).
        Frames are read straight from the device ring; everything runs on the
        current stream without a sync.  _mark: stage hook of
        tools/open_loop_timing.py (called with the stage's name once it is
        enqueued)."""
        from .open_loop import open_loop
        return open_loop(self, starts=starts, batch_size=batch_size, context=context, horizon=horizon, sample=sample,
                         noise=noise, _mark=_mark)

    def evaluate_world_model(self, batches=1, batch_size=None, context=None, horizon=None, sample=True):
        """Per-step open-loop error curves averaged over `batches` sampled
        batches of windows: a dict of CPU float lists -- mse and psnr (length
        H+1: state 0 is the posterior reconstruction; psnr is None for vector
        observations), reward_abs_err (symlog space) and continue_bce (length
        H).  Leaves np.random's state and the Philox {seed, offset} as it
        found them, so calling it between training iterations does not change
        the training run."""
        from .open_loop import evaluate_world_model
        return evaluate_world_model(self, batches=batches, batch_size=batch_size, context=context, horizon=horizon,
                                    sample=sample)

    def sample_futures(self, starts=None, batch_size=None, context=None, horizon=None, samples=8, noise=None,
                       ssim=True, _mark=None):
        """M = `samples` futures per replay window (futures.py; the metric
        definitions are in include/dreamer_hip.h): open_loop's gather, encoder
        and context filter once for the B windows (same defaults, same
        check_lengths), the posterior and the recorded actions replicated M
        times (rollout row b*M + m), one dr_imagine_actions at B*M rows -- the
        prior's draws are keyed by row, so the replicas differ -- one
        dr_decoder_fwd over the B*M*(H+1) states, dr_frame_metrics on the B*M
        rows (and dr_frame_ssim, pixel models with ssim=True), then
        dr_ensemble_metrics for the mean frame's error and the spread.  Returns
        a FuturesResult (best(), mse / psnr / ssim_curve in mean / best /
        best_sample / ensemble variants, coverage(), reward_spread(), video()).

        samples: an integer in 1 .. 64 with B * samples <= plan.PLAN_MAX_ROWS
        (ValueError otherwise).  noise: optional pair of explicit Exp(1) draws
        (q_context (Tc, B*R, C), q (H, B*M*R, C)), else Philox.  Everything
        runs on the current stream without a sync.  _mark: stage hook of
        tools/futures_timing.py."""
        from .futures import sample_futures
        return sample_futures(self, starts=starts, batch_size=batch_size, context=context, horizon=horizon,
                              samples=samples, noise=noise, ssim=ssim, _mark=_mark)

    def evaluate_futures(self, batches=1, batch_size=None, context=None, horizon=None, samples=8):
        """Per-step curves of sample_futures averaged over `batches` sampled
        batches of windows: a dict of CPU float lists -- mse_mean, mse_best (the
        smallest of the M per step and window), mse_ensemble, spread (per
        element), psnr_mean, psnr_best, ssim_mean, ssim_best, coverage (length
        H+1; the psnr / ssim entries are None for vector observations) and
        reward_spread (length H).  Leaves np.random's state and the Philox
        {seed, offset} and stream counter as it found them, like
        evaluate_world_model."""
        from .futures import evaluate_futures
        return evaluate_futures(self, batches=batches, batch_size=batch_size, context=context, horizon=horizon,
                                samples=samples)

    def closed_loop(self, starts=None, batch_size=None, length=None, sample=True, noise=None, predict=True,
                    _mark=None):
        """Posterior trace on replay windows (closed_loop.py): run the filter
        (warm_start_generator's scan, Dreamer.py:244-262) over the first
        `length` frames of each window keeping every step, and report per step
        the posterior and prior logits, KL(posterior || prior) and the two
        entropies, the posterior's reconstruction and -- predict=True -- the
        decode of a sample of the prior of h_t (what the model expected before
        frame t arrived), both against the ring's frame t, and the reward /
        continue heads against the stored values.  Returns a ClosedLoopResult.

        starts: window starts (default: buffer.sample_start_indices(batch_size
        or self.batch_size)); length defaults to S.  noise: optional pair of
        explicit Exp(1) draws (q_post (T, B*R, C), q_prior (T, B*R, C)), else
        Philox on two distinct ad-hoc streams; sample=False takes the mode of
        every categorical (q == 1 for both).  Frames are read straight from the
        device ring; everything runs on the current stream without a sync.
        _mark: stage hook of tools/closed_loop_timing.py."""
        from .closed_loop import closed_loop
        return closed_loop(self, starts=starts, batch_size=batch_size, length=length, sample=sample, noise=noise,
                           predict=predict, _mark=_mark)

    def evaluate_filter(self, batches=1, batch_size=None, length=None, sample=True):
        """Per-step closed-loop curves averaged over `batches` sampled batches
        of windows: a dict of CPU float lists -- kl, post_entropy,
        prior_entropy, mse_post, mse_prior, psnr_post, psnr_prior (length T;
        the psnr entries are None for vector observations), reward_abs_err
        (symlog space) and continue_bce (length T - 1).  Leaves np.random's
        state and the Philox {seed, offset} and stream counter as it found
        them, like evaluate_world_model."""
        from .closed_loop import evaluate_filter
        return evaluate_filter(self, batches=batches, batch_size=batch_size, length=length, sample=sample)

    def agent_trace(self, starts=None, batch_size=None, length=None, sample=True, noise=None, _mark=None):
        """Agent trace on replay windows (agent_trace.py): run closed_loop's
        filter over the first `length` frames of each window and report per
        step what the actor and the critic make of real data -- the online and
        target values and the critic's logits with their entropy and spread,
        the lambda-returns, discounted real returns and TD errors of the
        recorded rewards under the target values (Agent.py:156-172), the
        critic's two-hot loss against those returns (Agent.py:127-135), and the
        log-probability of the recorded actions under the current actor
        (Agent.py:110-115).  Returns an AgentTraceResult.

        starts: window starts (default: buffer.sample_start_indices(batch_size
        or self.batch_size)); length defaults to S, 2 <= length <= S.  noise:
        optional explicit Exp(1) draws q_post (T, B*R, C), else Philox;
        sample=False takes the mode of every categorical (q == 1).  gamma and
        lambda are the agent's.  Frames are read straight from the device
        ring; everything runs on the current stream without a sync.  _mark:
        stage hook of tools/agent_trace_timing.py."""
        from .agent_trace import agent_trace
        return agent_trace(self, starts=starts, batch_size=batch_size, length=length, sample=sample, noise=noise,
                           _mark=_mark)

    def evaluate_values(self, batches=1, batch_size=None, length=None, sample=True):
        """Per-step agent-trace curves averaged over `batches` sampled batches
        of windows: a dict of CPU float lists -- value, value_target,
        value_entropy, value_std_symlog, action_logprob, actor_sigma (length
        T), returns_lambda, returns_mc, abs_td, critic_ce, abs_advantage
        (length T - 1) -- and the scalar explained_variance (the mean over the
        batches).  Leaves np.random's state and the Philox {seed, offset} and
        stream counter as it found them, like evaluate_filter."""
        from .agent_trace import evaluate_values
        return evaluate_values(self, batches=batches, batch_size=batch_size, length=length, sample=sample)

    def dream_trace(self, starts=None, batch_size=None, context=None, horizon=None, samples=1, deterministic=False,
                    sample=True, noise=None, decode=True, saturation=0.99, _mark=None):
        """M = `samples` imagined rollouts under the current actor per replay
        window (dream_trace.py; the definitions are in include/dreamer_hip.h):
        what train_Agent learns from (Dreamer.py:143-175, Agent.py:96-135),
        kept per dream.  open_loop's gather, encoder and context filter once
        for the B windows, the posteriors replicated M times (rollout row
        b*M + m), one dr_imagine_fwd of `horizon` steps at B*M rows -- Philox is
        keyed by row, so the replicas differ --, one dr_critic_fwd each for the
        online and the target critic over the B*M*(H+1) states, one
        dr_dream_stats for the lambda-returns, Monte-Carlo returns, advantages
        (raw and divided by the agent's max(S, 1), which is read and not
        updated), discount weights, action log-probabilities and saturation
        counts of every dream and their mean / spread over a window's dreams,
        and -- decode=True -- one dr_decoder_fwd of all the states.  Returns a
        DreamResult (entropy(), curves(), pick(), video()).

        starts: window starts (default: buffer.sample_start_indices(batch_size
        or self.batch_size) -- uniform also with replay = "curious": evaluation
        sees the data distribution, not the training distribution); context
        defaults to S // 2 (the warm start's),
        1 <= context <= S; horizon defaults to self.horizon, any H >= 1 (a dream
        needs no ring frames).  samples: an integer in 1 .. 64 with B * samples
        <= 4096 (ValueError otherwise, raised before np.random is drawn from,
        like every argument check).  noise: optional explicit draws (q_context
        (Tc, B*R, C), q_dream (H, B*M*R, C), both Exp(1), and eps (H, B*M, A),
        N(0,1)), else Philox; sample=False takes the mode of every categorical
        (q == 1) and leaves the actor's draws to Philox; deterministic=True
        acts with tanh(mu).  saturation: the |a| from which an action dimension
        counts as saturated.  Vector models have no u8 frames.  Everything
        runs on the current stream without a sync.  _mark: stage hook of
        tools/dream_trace_timing.py."""
        from .dream_trace import dream_trace
        return dream_trace(self, starts=starts, batch_size=batch_size, context=context, horizon=horizon,
                           samples=samples, deterministic=deterministic, sample=sample, noise=noise, decode=decode,
                           saturation=saturation, _mark=_mark)

    def evaluate_dreams(self, batches=1, batch_size=None, context=None, horizon=None, samples=8, real=False):
        """Per-step dream curves averaged over `batches` sampled batches of
        windows and their dreams: a dict of CPU float lists -- reward, cont,
        ret_lambda, advantage, advantage_norm, neg_logp, sigma, saturated_frac,
        action_spread, ret_std (length H), alive and value (the online
        critic's; length H+1).  Leaves np.random's state, the Philox {seed,
        offset} and stream counter and the agent's S as it found them, like
        evaluate_values.

        real=True also runs agent_trace on the same starts (both filters at the
        posterior's mode, sample=False, so both see the same states; needs
        context <= S - 1) and adds the scalar
            gap = mean_b (mean_m R_mc[b][m][0] - real R_mc[b][context - 1]),
        the model's optimism about the current policy.  The two sides are not
        the same quantity: the dream's is H imagined steps under the current
        actor bootstrapped by the target critic at state H, the replay's is
        the S - context recorded steps (the actions of whatever policy filled
        the ring) bootstrapped by the target critic at the window's last
        state.  Two estimates over different horizons, both resting on the
        same target critic; read it as a trend, not as a model error."""
        from .dream_trace import evaluate_dreams
        return evaluate_dreams(self, batches=batches, batch_size=batch_size, context=context, horizon=horizon,
                               samples=samples, real=real)

    def saliency_frames(self, frames, hiddens, stride=4, fill="blur", blur_sigma=3.0, mask_sigma=None, sample=False,
                        noise=None, _mark=None):
        """Perturbation saliency of N frames (saliency.py; Greydanus et al. 2018):
        per cell of a stride-`stride` grid, how far the actor's mean, the
        critic's value and the posterior move when a blurred (fill="blur",
        Gaussian of blur_sigma) or averaged (fill="mean") copy of the frame is
        blended in around the cell under a Gaussian mask of mask_sigma (default
        5 * H / 80).  include/dreamer_hip.h "perturbation saliency" has the
        definitions.  Pixel models only (ValueError otherwise).

        frames: u8 (N, H, W, 3) numpy as the env gives them, or a u8 (N, 3, H, W)
        device tensor.  hiddens (N, hidden): the hidden state about to encode
        each frame, e.g. the h' act_step_batch returned.  All variants of a
        frame share one block of Exp(1) draws: sample=False (the default) takes
        the mode of every categorical, noise (N*R, C) gives them, sample=True
        draws one block per frame from the ad-hoc Philox stream.  Runs in passes
        of at most 8192 variant frames on the current stream without a sync.
        Returns a SaliencyResult with lead (N,).  _mark: stage hook of
        tools/saliency_timing.py."""
        from .saliency import saliency_frames
        return saliency_frames(self, frames, hiddens, stride=stride, fill=fill, blur_sigma=blur_sigma,
                               mask_sigma=mask_sigma, sample=sample, noise=noise, _mark=_mark)

    def saliency(self, starts=None, batch_size=None, length=None, steps=None, **kw):
        """Perturbation saliency on replay windows: run closed_loop's filter
        (as agent_trace does) over the first `length` frames (default S) of each
        window, then saliency_frames on the ring's frames of the window steps
        `steps` (default: all) with the filter's hidden states -- hiddens[t] is
        the state about to encode frame t.  Returns a SaliencyResult with lead
        (B, K = len(steps)).  Keywords as saliency_frames; noise, if given, is
        the pair (the trace's draws (T, B*R, C), the variants' draws (B*K*R, C)),
        and sample applies to both.  Every argument check fires before np.random
        is drawn from."""
        from .saliency import saliency
        return saliency(self, starts=starts, batch_size=batch_size, length=length, steps=steps, **kw)

    def evaluate_saliency(self, batches=1, batch_size=None, length=None, steps=None, **kw):
        """Saliency averaged over `batches` sampled batches of windows: a dict
        with the mean actor, value and posterior_kl grids (Gy x Gx nested
        lists, over frames and batches) and "concentration", the mean share of
        each score in its top 10 % of cells (top=...).  Leaves np.random's state
        and the Philox {seed, offset} and stream counter as it found them."""
        from .saliency import evaluate_saliency
        return evaluate_saliency(self, batches=batches, batch_size=batch_size, length=length, steps=steps, **kw)

    # ------------------------------------------------------- exploration read-outs
    def disagreement(self, hidden):
        """Ensemble disagreement of hidden states: any (..., hidden) device tensor -> (...).  Needs explore =
        "disagreement"."""
        return self._explorer().disagreement(hidden)

    def knn(self, queries, bank=None, k=None, query_groups=None, bank_groups=None):
        """k nearest neighbours (include/dreamer_hip.h, dr_knn) of any device tensors (..., D): (dist (..., k)
        Euclidean, not squared; idx (..., k) int32 rows of the flattened bank, -1 / inf past the eligible rows).
        bank = None: the queries among themselves, a row never its own neighbour.  Groups are int tensors of the
        rows' shapes: a bank row of the query's group is not eligible.  k defaults to explore_knn.  Works in every
        explore mode."""
        from .novelty import knn
        return knn(queries, bank, self.explore_knn if k is None else k, query_groups, bank_groups)

    def state_entropy(self, hidden, k=None):
        """Particle-entropy reward log1p(mean distance to the k nearest other rows) of hidden states among
        themselves: any (..., hidden) device tensor -> (...) (dr_state_entropy_fwd).  Works in every explore mode."""
        from .novelty import state_entropy
        return state_entropy(hidden, self.explore_knn if k is None else k)

    def novelty(self, starts=None, batch_size=None, length=None):
        """Per-step disagreement of the posterior filter's hidden states on replay windows (where the ensemble has
        seen too little data): see dreamer_amd/novelty.py.  Needs explore = "disagreement", or "entropy": then the
        per-step entropy reward of the hidden states among the B * length states of the batch."""
        from .novelty import novelty
        return novelty(self, starts=starts, batch_size=batch_size, length=length)

    def evaluate_novelty(self, batches=1, batch_size=None, length=None):
        """novelty over `batches` batches of windows drawn without disturbing the training run's random state, like
        the other evaluate_*; returns the mean per-step disagreement (length,) and its overall mean."""
        from .novelty import evaluate_novelty
        return evaluate_novelty(self, batches=batches, batch_size=batch_size, length=length)

    # --------------------------------------------------------------- training
    @property
    def engine(self):
        if self._engine is None:
            from .engine import ImaginationEngine
            self._engine = ImaginationEngine(self, world=self.world)
        return self._engine

    def train_Agent(self):
        """Dreamer.train_Agent (Dreamer.py:264-287): AC_epochs fused epochs.
        replay = "curious": the starts come from the device sampler (the
        sequential epoch loop; priorities and visits are not touched), and so
        they do with replay_episodes = "respect" in either replay mode.
        explore = "disagreement": the epochs learn from explore_extrinsic * reward +
        explore_scale * disagreement (engine.returns)."""
        self._exploring()  # (ValueError under data parallelism)
        host = not self._device_starts()  # replay = "curious" or replay_episodes = "respect": device starts
        B = self.batch_size if self.world is None else self.engine.B
        if self.AC_epochs > 1 and host and self.pipeline_epochs and not self.engine.persistent_chain():
            # config key pipeline_epochs (default on): the epochs' window
            # starts are drawn up front (same np.random order); the warm start
            # of epoch e+1 then overlaps epoch e's update (engine.run_many),
            # bit for bit the sequential launch-form epochs.  Where the chain
            # runs as the persistent kernels (B <= 128 per GPU) the sequential
            # epochs below are faster (a persistent kernel needs every CU, so
            # it cannot share the chip with an overlapped warm start; measured
            # in bench.py's configs1_B64_ac_epochs2)
            losses = self.engine.run_many([self._window_starts(B) for _ in range(self.AC_epochs)])
            return losses[:, 0].mean(dim=0), losses[:, 1].mean(dim=0)
        if self.AC_epochs == 1:
            # one epoch: one copy of the two loss slots (the loop below costs
            # clone + cat + mean per loss, six small launches outside the
            # captured graphs, each behind a dispatch gap); the mean of one
            # value is that value, bit for bit
            starts = self._window_starts(B)
            self.engine.run(starts)
            losses = self.agent.loss_buffer[0:2].clone()
            return losses[0], losses[1]
        la, lc = [], []
        for _ in tqdm(range(self.AC_epochs), desc="Training Agent in Dreams", leave=False):
            starts = self._window_starts(B)
            a, c = self.engine.run(starts)
            la.append(a.clone())
            lc.append(c.clone())
        return torch.cat(la).mean(dim=0), torch.cat(lc).mean(dim=0)

    def _window_starts(self, B):
        """One epoch's B window starts: a device tensor from the device sampler (no np.random draw) where
        _device_starts(), else the reference's host draw.  Invariant of the callers: with device starts the first
        draw comes before the first look at self.engine -- the first device draw seeds the ad-hoc generator and the
        first engine the engine's, both from torch's CPU generator, in that order.  train_Agent keeps it because
        device starts exclude data parallelism (so B is not read from the engine) and its pipelining condition tests
        `host` before it touches self.engine."""
        if self._device_starts():
            return self.buffer.sample_start_indices_device(B)[0]
        return self.buffer.sample_start_indices(B)

    def _data_parallel(self):
        return self.world is not None or self.world_model._dp is not None

    def _curious(self):
        """True in prioritised-replay mode (ValueError under data parallelism:
        per-rank priorities need a design of their own)."""
        if self.buffer.replay == "uniform":
            return False
        if self._data_parallel():
            raise ValueError("replay = 'curious' is not supported under data parallelism")
        return True

    def _device_starts(self):
        """True where the window starts come from the device sampler: replay = "curious" or replay_episodes =
        "respect" (ValueError under data parallelism for either)."""
        curious = self._curious()
        if self.buffer.replay_episodes == "ignore":
            return curious
        if self._data_parallel():
            raise ValueError("replay_episodes = 'respect' is not supported under data parallelism")
        return True

    def _exploring(self):
        """True with explore = "disagreement" (ValueError under data parallelism in either exploring mode: the
        ensemble's gradients have no all-reduce, the entropy's bank would be one rank's states)."""
        if self.explore == "none":
            return False
        if self._data_parallel():
            raise ValueError(f"explore = {self.explore!r} is not supported under data parallelism")
        return self.explore == "disagreement"

    def _explorer(self):
        if not self._exploring():
            raise RuntimeError("this Dreamer has no disagreement ensemble: set the config key explore = 'disagreement'")
        return self.explorer

    def _train_explorer(self, outputs):
        """One ensemble step on rows t >= 1 of the world-model step's posterior trace (time-major copies the step
        handed out: the world model's own launches, and so its bits, are what they are without exploration)."""
        self.explorer.train_step(outputs["hiddens"][1:], outputs["latents"][1:])

    def train_world_model(self):  # Dreamer.py:228-242
        out = []
        explore = self._exploring()
        trace = {} if explore else None
        device, curious = self._device_starts(), self._curious()
        for _ in tqdm(range(self.WM_epochs), desc="Training World Model On Buffer Data", leave=False):
            if device or self.device.type == "cuda":
                # the step fed from the replay ring (frames stay u8 in HBM).  Host starts: the same np.random draws
                # as sample_sequences.  Device starts: no host round trip; in curious mode the step also leaves the
                # per-window scores, which update the priorities (replay_episodes = "respect" in uniform mode: the
                # device sample and the step alone)
                starts = self._window_starts(self.batch_size)
                out.append(self.world_model.train_step_ring(self.buffer, starts, scores=curious, outputs=trace))
                if curious:
                    self.buffer.update_priorities(starts, self.world_model.last_window_scores)
                if explore:
                    self._train_explorer(trace)
            else:
                obs, act, rew, cont, _ = self.buffer.sample_sequences(batch_size=self.batch_size)
                out.append(self.world_model.training_step(obs, act, rew, cont))
        return out

    def load_pretrained_dreamer(self, path):
        self.load_state_dict(torch.load(path, weights_only=True))

    def save_trained_Dreamer(self, save_path):
        torch.save(self.state_dict(), save_path)

    # ---- true resume (beyond the reference, whose checkpoints are weights only:
    # Dreamer.py:289-293, 347-354).  One torch.save file of tensors and plain
    # scalars (loads with weights_only=True): the reference-layout state_dict,
    # the three AdamW states (moments + step), S, the engine / ad-hoc Philox
    # states, numpy's and torch's CPU generators (window sampling), the replay
    # ring and the env seed counter.  Resuming reproduces the uninterrupted
    # run's TRAINING UPDATES (train_world_model / train_Agent) bit for bit
    # (tests/test_gpu_api.py::test_training_state_resume).  The in-progress env
    # episode is not part of the state (the env object, agent_obs / hidden /
    # latent): after a resume rollout_policy starts a fresh episode with
    # env.reset(seed), so runs that resume mid-episode diverge from there.
    TRAINING_STATE_FORMAT = "dreamer_amd.training_state.v1"

    def training_state(self):
        ag, wm, buf = self.agent, self.world_model, self.buffer
        ag._ensure_flat()
        wm._ensure_flat()
        cpu = lambda t: t.detach().cpu().clone()
        opt = lambda o: {"exp_avg": cpu(o.exp_avg), "exp_avg_sq": cpu(o.exp_avg_sq), "step": cpu(o.step_dev)}
        name, keys, pos, has_gauss, gauss = np.random.get_state()
        er, ar = hip.rng(self.device), hip.adhoc(self.device)
        st = {
            "format": self.TRAINING_STATE_FORMAT,
            "model": {k: cpu(v) for k, v in self.state_dict().items()},
            "opt_actor": opt(ag.actor_optimiser), "opt_critic": opt(ag.critic_optimiser), "opt_wm": opt(wm.optimiser),
            "S": cpu(ag.S_dev),
            "rng_engine": cpu(er.state), "rng_engine_counter": int(er.counter),
            "rng_adhoc": cpu(ar.state), "rng_adhoc_counter": int(ar.counter),
            "np_rng": {"keys": torch.from_numpy(np.asarray(keys, dtype=np.int64)), "pos": int(pos),
                       "has_gauss": int(has_gauss), "gauss": float(gauss)},
            "torch_rng": torch.get_rng_state(),
            "buffer": {"obs": torch.from_numpy(buf.observation_buffer.copy()),
                       "act": torch.from_numpy(buf.action_buffer.copy()),
                       "rew": torch.from_numpy(buf.reward_buffer.copy()),
                       "cont": torch.from_numpy(buf.continue_buffer.copy()),
                       "next_idx": int(buf.next_idx), "size": int(buf.size)},
            "seed": int(self.seed),
        }
        if buf.replay != "uniform":  # prioritised replay: the per-slot state (uniform mode: exactly the keys above)
            m = buf._mirror()
            st["buffer"].update(priority=cpu(m["priority"]), visits=cpu(m["visits"]))
        if buf.replay_episodes != "ignore":  # episode-aware replay: the per-slot flags (ignore mode: no such key)
            st["buffer"]["first"] = torch.from_numpy(buf.first_buffer.copy())
        if self.explore == "disagreement":  # the ensemble's AdamW state (its weights are in "model"); absent otherwise
            self.explorer._ensure_flat()
            st["opt_explorer"] = opt(self.explorer.optimiser)
        return st

    def save_training_state(self, path):
        torch.save(self.training_state(), path)

    def load_training_state(self, path_or_state):
        st = path_or_state if isinstance(path_or_state, dict) else torch.load(path_or_state, weights_only=True)
        if st.get("format") != self.TRAINING_STATE_FORMAT:
            raise ValueError(f"not a {self.TRAINING_STATE_FORMAT} file: {st.get('format')!r}")
        if self.explore == "disagreement" and "opt_explorer" not in st:
            raise ValueError("the training state was saved without exploration: it has no ensemble optimiser state")
        if self.buffer.replay_episodes != "ignore" and "first" not in st["buffer"]:
            raise ValueError("the training state was saved with replay_episodes = 'ignore': it has no first flags")
        self.load_state_dict({k: v.to(self.device) for k, v in st["model"].items()})
        ag, wm, buf = self.agent, self.world_model, self.buffer
        ag._ensure_flat()
        wm._ensure_flat()
        opts = [(ag.actor_optimiser, "opt_actor"), (ag.critic_optimiser, "opt_critic"), (wm.optimiser, "opt_wm")]
        if self.explore == "disagreement":
            self.explorer._ensure_flat()
            opts.append((self.explorer.optimiser, "opt_explorer"))
        for o, k in opts:
            o.exp_avg.copy_(st[k]["exp_avg"])
            o.exp_avg_sq.copy_(st[k]["exp_avg_sq"])
            o.step_dev.copy_(st[k]["step"])
        ag.S_dev.copy_(st["S"])
        er, ar = hip.rng(self.device), hip.adhoc(self.device)
        er.state.copy_(st["rng_engine"])
        er.counter = int(st["rng_engine_counter"])
        ar.state.copy_(st["rng_adhoc"])
        ar.counter = int(st["rng_adhoc_counter"])
        r = st["np_rng"]
        np.random.set_state(("MT19937", r["keys"].numpy().astype(np.uint32), int(r["pos"]), int(r["has_gauss"]),
                             float(r["gauss"])))
        torch.set_rng_state(st["torch_rng"])
        b = st["buffer"]
        buf.observation_buffer[...] = b["obs"].numpy()
        buf.action_buffer[...] = b["act"].numpy()
        buf.reward_buffer[...] = b["rew"].numpy()
        buf.continue_buffer[...] = b["cont"].numpy()
        buf.next_idx, buf.size = int(b["next_idx"]), int(b["size"])
        buf.first_buffer[...] = b["first"].numpy() if "first" in b else 0
        buf._dirty = list(range(buf.capacity))  # the device mirror re-uploads on next use
        if buf.replay != "uniform":
            if "priority" not in b:
                raise ValueError("the training state was saved in uniform replay mode: it has no priorities")
            m = buf._mirror()  # the re-upload marks every slot new; the saved per-slot state goes in after it
            m["priority"].copy_(b["priority"])
            m["visits"].copy_(b["visits"])
        self.seed = int(st["seed"])

    # ------------------------------------------------- acting (batch-1, HIP)
    def _obs_tensor(self, observation):
        obs = observation.transpose(2, 0, 1).astype(np.uint8)
        norm = (obs.astype(np.float32) / 255.0) - 0.5
        return norm, torch.tensor(norm, dtype=torch.float32, device=self.device).unsqueeze(0).unsqueeze(0)

    def act_step(self, observation, z=None, h=None, a=None, deterministic=False):
        """One env step of the acting loop in ONE launch (dr_act_step): with
        (z, h, a) from the previous step, h' = GRU(z, h, a) (observe_step,
        WorldModel.py:79-82); without them, h' = 0 (episode start,
        Dreamer.py:186-187).  Then z' = Encoder.encode(h', observation) and
        a' = Actor.act(h', z', deterministic).  observation: the env's H x W x 3
        uint8 frame.  Returns (a', mu, sigma, z', h') shaped (1, 1, ...).

        A vector-observation model (observation: D floats) runs the same step
        as dr_act_vec with one row, where the vector dispatch says fused
        (ACT_VEC_FUSED_N, act_batch_path)."""
        dev = self.device
        L.require_gpu(torch.empty(0, device=dev))
        if self.world_model.vector_obs:
            if self._act_batch_route(1) == "fused":
                out = self._act_vec(np.asarray(observation, dtype=np.float32).reshape(1, -1),
                                    None if z is None else (z, h, a), np.full(1, z is None), deterministic)
                if out is not None:
                    return out
            return self._act_step_unfused(observation, z, h, a, deterministic)
        if not getattr(self, "_act_unfused", False):
            out = self._act_fused("dr_act_step", self.__dict__, "_act_bufs", {},
                                  np.asarray(observation, dtype=np.uint8).reshape(-1), np.full(1, z is None),
                                  None if z is None else (z, h, a), deterministic)
            if out is not None:
                return out
            # the device cannot hold the one-launch grid, or the widths are not the ones the
            # kernel's register batches are sized for (e.g. the 5-layer VAE): the unfused launches
            self._act_unfused = True
        return self._act_step_unfused(observation, z, h, a, deterministic)

    def _act_fused(self, entry, bufs, key, tag, payload, first, state, deterministic):
        """The launch path of the three one-launch entry points: dr_act_step
        (act_step), dr_act_batch (act_step_batch) and dr_act_vec (_act_vec).
        payload: the N observations as bytes (u8 frames or f32 vectors); first:
        bool [N]; state: the previous (z, h, a), or None where every row is
        first.  bufs[key]: the entry point's buffers at this N (pinned and
        device staging of payload + first flags, zero state, status word,
        workspace), made on first use; tag: the keys _act_sync names the entry
        point by.  Returns (a', mu, sigma, z', h') shaped (N, 1, ...), or None
        where the entry point answered DR_E_UNSUPPORTED: the caller sets its
        fallback flag and runs the unfused launches."""
        dev = self.device
        N, nb = first.shape[0], payload.size
        d = self.world_model.dims(self.agent)
        self.agent._ensure_flat()
        R, C = self.latent_state_dims
        A, Hd = self.action_dims, self.hidden_state_dims
        st = bufs.get(key)
        if st is None:
            ws = L.query(entry + "_workspace_bytes", d, *(() if entry == "dr_act_step" else (N,)))
            st = bufs[key] = dict(
                tag, nb=nb,
                pin=torch.empty(nb + N, dtype=torch.uint8).pin_memory(),  # the observations, then the first flags
                dev=torch.empty(nb + N, dtype=torch.uint8, device=dev),
                z0=torch.zeros(N, R * C, device=dev), h0=torch.zeros(N, Hd, device=dev),
                a0=torch.zeros(N, A, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev),
                status_host=torch.zeros(1, dtype=torch.int32).pin_memory(),
                ws=torch.empty(ws, dtype=torch.uint8, device=dev))
        self._act_sync()  # the previous step's copy out of the pinned staging buffer has run (and it was ok)
        nb = st["nb"]  # (an observation of another size than the buffers were made for raises here)
        pin = st["pin"].numpy()
        pin[:nb] = payload
        pin[nb:] = first
        st["dev"].copy_(st["pin"], non_blocking=True)
        if state is None:
            zp, hp, ap = st["z0"], st["h0"], st["a0"]
        else:
            zp, hp, ap = (t.reshape(N, -1).float().contiguous() for t in state)
        z2 = torch.empty(N, 1, R, C, device=dev)
        h2 = torch.empty(N, 1, Hd, device=dev)
        a2, mu, sg = (torch.empty(N, 1, A, device=dev) for _ in range(3))
        obs = L.ptr(st["dev"])
        # dr_act_step takes its row's flag on the host (has_prev); the others read the flags behind the observations
        rows = (obs, int(not first[0])) if entry == "dr_act_step" else (N, obs, obs + nb)
        try:
            L.call(entry, d, self.world_model.packed(), self.agent.actor_struct(), *rows, L.ptr(zp), L.ptr(hp),
                   L.ptr(ap), hip.adhoc(dev).noise(), int(deterministic), L.ptr(z2), L.ptr(h2), L.ptr(a2), L.ptr(mu),
                   L.ptr(sg), None, L.ptr(st["status"]), L.ptr(st["ws"]), st["ws"].numel(), hip.stream())
        except L.HipError as e:
            if e.code != L.DR_E_UNSUPPORTED:
                raise
            return None
        # the status word travels back with the step (4 bytes behind the kernel);
        # _act_sync / act_check raise on a timed-out grid barrier
        st["status_host"].copy_(st["status"], non_blocking=True)
        self._act_last = st
        self._act_ev = torch.cuda.Event()
        self._act_ev.record()
        return a2, mu, sg, z2, h2

    def act_check(self):
        """Wait for the last act_step / act_step_batch and raise if its
        one-launch kernel hit a grid-barrier timeout (its outputs are then NaN,
        never a state)."""
        self._act_sync()

    # ------------------------------------------- acting (N environments, HIP)
    # Batch sizes at which act_step_batch runs the one-launch dr_act_batch:
    # those where it beat both the batched unfused launches and N sequential
    # act_step calls by more than the run-to-run spread
    # (profiles/act_batch_timing.txt): measured at N =
    # 1, 2, 4 and 8 (at N = 1 act_step is one launch of the same kernel, so
    # only the unfused launches are a contender there); at N = 16 the unfused
    # launches are faster, and 9 ... 15 were not measured, so they go with 16.
    # At the other sizes the faster of the other two runs
    # (ACT_BATCH_SEQUENTIAL_N: the sizes where that is the sequential one --
    # none: the unfused launches cost about the same at every N, below three
    # act_step calls, and the sizes not fused are above 8).
    ACT_BATCH_FUSED_N = frozenset(range(1, 9))
    ACT_BATCH_SEQUENTIAL_N = frozenset()
    # None: dispatch by the table; "fused" / "unfused" / "sequential": that path (tests, timing)
    act_batch_path = None

    # The same table for vector-observation models (dr_act_vec, which also
    # serves act_step as N = 1): the sizes where the one-launch kernel beat the
    # batched unfused launches by more than the spread of the repetitions
    # (profiles/act_vec_timing.txt) -- measured at N = 1,
    # 2, 4 and 8; at N = 16 the unfused launches are faster, and 9 ... 15 were
    # not measured, so they go with 16.
    ACT_VEC_FUSED_N = frozenset(range(1, 9))

    def _act_batch_route(self, N):
        vec = self.world_model.vector_obs
        fusable = not (N > L.DR_ACT_MAX_ENVS
                       or getattr(self, "_act_vec_unsupported" if vec else "_act_batch_unsupported", False))
        want = self.act_batch_path
        if want is None and vec:
            want = "fused" if N in self.ACT_VEC_FUSED_N else "unfused"
        if want is None:
            want = "fused" if N in self.ACT_BATCH_FUSED_N else (
                "sequential" if N in self.ACT_BATCH_SEQUENTIAL_N else "unfused")
        if want == "fused" and not fusable:
            want = "unfused"
        if want == "sequential" and self.world_model.vector_obs:
            want = "unfused"
        return want

    def act_step_batch(self, observations, state=None, first=None, deterministic=False):
        """One env step of N environments at once.  observations: (N, H, W, 3)
        uint8; state: the (z, h, a) this method returned for the previous step
        (None: every row starts an episode); first: bool [N], True = that row
        starts an episode (h' = 0, its state row is ignored and may be stale);
        default all True without state, all False with it.  Per row the
        semantics (and, on the one-launch path, the bits) of act_step.
        Returns (a', mu, sigma, z', h') shaped (N, 1, ...).

        Runs dr_act_batch (one launch) at the batch sizes in ACT_BATCH_FUSED_N
        -- for vector observations ((N, D) floats) dr_act_vec at those in
        ACT_VEC_FUSED_N; otherwise, for the deeper VAE, N > DR_ACT_MAX_ENVS,
        an observation vector above DR_ACT_VEC_MAX_OBS or a device that cannot
        hold the grid, the batched unfused launches (_act_step_batch_unfused)
        or N act_step calls."""
        dev = self.device
        L.require_gpu(torch.empty(0, device=dev))
        observations = np.asarray(observations)
        N = observations.shape[0]
        if N < 1:
            raise ValueError("act_step_batch needs at least one environment")
        if first is None:
            first = np.ones(N, dtype=bool) if state is None else np.zeros(N, dtype=bool)
        first = np.asarray(first, dtype=bool).reshape(N)
        if state is None and not first.all():
            raise ValueError("act_step_batch: a row that continues an episode needs the previous state")
        route = self._act_batch_route(N)
        if route == "fused" and self.world_model.vector_obs:
            out = self._act_vec(np.asarray(observations, dtype=np.float32).reshape(N, -1), state, first,
                                deterministic)
            if out is not None:
                return out
            route = "unfused"
        if route == "unfused":
            return self._act_step_batch_unfused(observations, state, first, deterministic)
        if route == "sequential":
            return self._act_step_batch_sequential(observations, state, first, deterministic)
        nf = observations.size
        out = self._act_fused("dr_act_batch", self.__dict__.setdefault("_act_batch_bufs", {}), N, dict(nf=nf),
                              np.asarray(observations, dtype=np.uint8).reshape(-1), first, state, deterministic)
        if out is None:
            # the device cannot hold the grid, or the widths are not the kernel's (e.g. the 5-layer VAE)
            self._act_batch_unsupported = True
            return self._act_step_batch_unfused(observations, state, first, deterministic)
        return out

    def _act_vec(self, observations, state, first, deterministic):
        """N rows of vector observations ((N, D) f32) through dr_act_vec in one
        launch; act_step is the N = 1 call.  Returns None once the entry point
        answered DR_E_UNSUPPORTED (observation dim above DR_ACT_VEC_MAX_OBS,
        widths outside the kernel's, a device that cannot hold the grid): the
        caller then runs the unfused launches, and so does every later step."""
        N = observations.shape[0]
        bufs = self.__dict__.setdefault("_act_vec_bufs", {})
        out = self._act_fused("dr_act_vec", bufs, N, dict(vec=True),
                              np.ascontiguousarray(observations, dtype=np.float32).reshape(-1).view(np.uint8),
                              np.asarray(first, dtype=bool).reshape(N), state, deterministic)
        if out is None:
            self._act_vec_unsupported = True
            del bufs[N]
        return out

    def _act_step_batch_unfused(self, observations, state, first, deterministic):
        """act_step_batch through the batched launches that exist: dr_gru_cell,
        dr_encoder_features + dr_observe_scan (Encoder.encode) and dr_actor_act
        on N rows, h' = where(first, 0, GRU(...))."""
        dev = self.device
        wm = self.world_model
        N = observations.shape[0]
        if wm.vector_obs:
            obs = torch.as_tensor(np.asarray(observations, dtype=np.float32), device=dev).view(N, 1, -1)
        else:
            u8 = torch.from_numpy(np.ascontiguousarray(observations, dtype=np.uint8)).to(dev)
            obs = (u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5).unsqueeze(1).contiguous()
        h2 = torch.zeros(N, 1, self.hidden_state_dims, device=dev)
        if state is not None and not first.all():
            z, h, a = state
            hg = wm.sequence_model(z.reshape(N, 1, -1), h.reshape(N, 1, -1), a.reshape(N, 1, -1))
            h2 = torch.where(torch.from_numpy(first).to(dev).view(N, 1, 1), h2, hg.reshape(N, 1, -1))
        z2, _ = wm.encoder.encode(h2, obs)
        a2, mu, sg = self.agent.actor.act(h2, z2, deterministic=deterministic)
        return a2, mu, sg, z2, h2

    def _act_step_batch_sequential(self, observations, state, first, deterministic):
        """act_step_batch as N act_step calls (explicit noise is handed on row by row)."""
        R, C = self.latent_state_dims
        ov = hip._override[-1] if hip._override else None
        rows = []
        for e in range(observations.shape[0]):
            s = (None, None, None) if first[e] else tuple(t[e] for t in state)
            if ov is None:
                rows.append(self.act_step(observations[e], *s, deterministic=deterministic))
                continue
            q, eps = ov
            with hip.noise_override(q=None if q is None else q.reshape(-1, R, C)[e].contiguous(),
                                    eps=None if eps is None else eps.reshape(-1, self.action_dims)[e].contiguous()):
                rows.append(self.act_step(observations[e], *s, deterministic=deterministic))
        return tuple(torch.cat(ts, dim=0) for ts in zip(*rows))

    def _act_step_unfused(self, observation, z, h, a, deterministic):
        """The same step through the unfused HIP launches -- dr_gru_cell,
        dr_encoder_features + dr_observe_scan (Encoder.encode), dr_actor_act:
        devices that cannot hold the one-launch grid co-resident, widths
        outside dr_act_step's / dr_act_vec's, and vector-observation models
        where the dispatch says unfused."""
        dev = self.device
        wm = self.world_model
        if wm.vector_obs:
            obs = torch.as_tensor(np.asarray(observation, dtype=np.float32), device=dev).view(1, 1, -1)
        else:
            _, obs = self._obs_tensor(observation)
        if z is None:
            h2 = torch.zeros(1, 1, self.hidden_state_dims, device=dev)
        else:
            h2 = wm.sequence_model(z.reshape(1, 1, -1), h.reshape(1, 1, -1), a.reshape(1, 1, -1))
        z2, _ = wm.encoder.encode(h2, obs)
        a2, mu, sg = self.agent.actor.act(h2, z2, deterministic=deterministic)
        return a2, mu, sg, z2, h2

    def _agent_obs(self, observation):
        """The env observation as the agent keeps it (Dreamer.py:181-183): a
        normalised CHW frame, or the raw f32 vector."""
        if self.world_model.vector_obs:
            return np.asarray(observation, dtype=np.float32)
        return (observation.transpose(2, 0, 1).astype(np.float32) / 255.0) - 0.5

    def _buffer_obs(self, agent_obs):
        if self.world_model.vector_obs:
            return agent_obs
        return ((agent_obs + 0.5) * 255.0).astype(np.uint8)

    def _act_sync(self):
        ev = getattr(self, "_act_ev", None)
        if ev is None:
            return
        ev.synchronize()
        st = self._act_last  # the buffers of the step the event follows (act_step's, or act_step_batch's for its N)
        if int(st["status_host"][0]) != 0:
            st["status"].zero_()
            st["status_host"].zero_()
            self._act_ev = None
            name = "dr_act_vec" if "vec" in st else "dr_act_batch" if "nf" in st else "dr_act_step"
            raise RuntimeError(f"{name}: a grid barrier timed out (the acting grid was not co-resident, e.g. "
                               "beside a long-running kernel); that step's outputs are NaN")

    def rollout_policy(self, env, random_policy=False):  # Dreamer.py:177-226
        """Same env / buffer sequence as the reference; the device work of each
        env step (observe_step + the next step's act) is one dr_act_step launch."""
        with torch.no_grad():
            if self.agent_obs is None:
                observation, _ = env.reset(seed=self.seed)
                self.agent_obs = self._agent_obs(observation)
                _, _, _, self.agent_latent, self.agent_hidden = self.act_step(observation)
            action = None
            if not random_policy:  # the current actor's action for the current state
                action, _, _ = self.agent.actor.act(self.agent_hidden, self.agent_latent, deterministic=False)
            for _ in range(self.sequence_length):
                if random_policy:
                    action_np = env.action_space.sample()
                    action = torch.tensor(action_np, dtype=torch.float32, device=self.device).view(1, 1, -1)
                else:
                    action_np = action.detach().cpu().numpy().reshape(-1)
                    self.act_check()
                observation_, reward, terminated, truncated, _ = env.step(action_np)
                done = terminated or truncated
                self.buffer.add_to_buffer(self._buffer_obs(self.agent_obs), action_np, reward, 1 - done)
                if done:
                    self.seed += 1
                    observation, _ = env.reset(seed=self.seed)
                    self.agent_obs = self._agent_obs(observation)
                    action, _, _, self.agent_latent, self.agent_hidden = self.act_step(observation)
                else:
                    self.agent_obs = self._agent_obs(observation_)
                    action, _, _, self.agent_latent, self.agent_hidden = self.act_step(
                        observation_, self.agent_latent, self.agent_hidden, action)

    def evaluate_agent(self, env, eval_episodes):  # Dreamer.py:295-322
        rewards = []
        with torch.no_grad():
            for _ in tqdm(range(eval_episodes), desc="Evaluating Agent", leave=False):
                self.seed += 1
                total = 0
                observation, _ = env.reset(seed=self.seed)
                action, _, _, latent, hidden = self.act_step(observation, deterministic=True)
                done = False
                while not done:
                    action_np = action.detach().cpu().numpy().squeeze(0).squeeze(0)
                    self.act_check()
                    observation_, reward, terminated, truncated, _ = env.step(action_np)
                    total += reward
                    done = terminated or truncated
                    if not done:
                        action, _, _, latent, hidden = self.act_step(observation_, latent, hidden, action,
                                                                     deterministic=True)
                rewards.append(total)
        return torch.tensor(rewards, dtype=torch.float32, device=self.device).mean()

    def rollout_policy_vec(self, envs, random_policy=False):
        """rollout_policy over a list of environments stepped in lockstep for
        sequence_length steps, the device work of each step one act_step_batch.
        Per-env state (agent observation, latent, hidden) is kept between
        calls.  First call: env e is reset with seed self.seed + e, then
        self.seed += N - 1.  On done, in env-index order: self.seed += 1, reset
        with it, and that row starts an episode on the next step.

        After the S steps the transitions go into the ring through
        add_to_buffer as N consecutive blocks of S -- env 0's steps, then env
        1's, ... -- so every block is one env's contiguous stream.  A sampled
        window that crosses a block boundary joins two envs' streams, the same
        way the reference's windows already join two episodes across a done.
        With N > 1 the first transition of each block goes in with first=True,
        so replay_episodes = "respect" draws no such window."""
        N = len(envs)
        with torch.no_grad():
            if self.vec_obs is None or len(self.vec_obs) != N:
                frames = [env.reset(seed=self.seed + e)[0] for e, env in enumerate(envs)]
                self.seed += N - 1
                self.vec_obs = [self._agent_obs(o) for o in frames]
                _, _, _, self.vec_latent, self.vec_hidden = self.act_step_batch(np.stack(frames))
            action = None
            if not random_policy:  # the current actor's actions for the current states
                action, _, _ = self.agent.actor.act(self.vec_hidden, self.vec_latent, deterministic=False)
            blocks = [[] for _ in range(N)]
            for _ in range(self.sequence_length):
                if random_policy:
                    action_np = np.stack([np.asarray(env.action_space.sample(), dtype=np.float32) for env in envs])
                    action = torch.tensor(action_np, dtype=torch.float32, device=self.device).view(N, 1, -1)
                else:
                    action_np = action.detach().cpu().numpy().reshape(N, -1)
                    self.act_check()
                frames, first = [], np.zeros(N, dtype=bool)
                for e, env in enumerate(envs):
                    observation_, reward, terminated, truncated, _ = env.step(action_np[e])
                    done = terminated or truncated
                    blocks[e].append((self._buffer_obs(self.vec_obs[e]), action_np[e], reward, 1 - done))
                    if done:
                        self.seed += 1
                        observation_, _ = env.reset(seed=self.seed)
                        first[e] = True
                    frames.append(observation_)
                    self.vec_obs[e] = self._agent_obs(observation_)
                action, _, _, self.vec_latent, self.vec_hidden = self.act_step_batch(
                    np.stack(frames), (self.vec_latent, self.vec_hidden, action), first)
            for block in blocks:
                for t, transition in enumerate(block):
                    self.buffer.add_to_buffer(*transition, first=N > 1 and t == 0)

    def evaluate_agent_vec(self, envs, eval_episodes):
        """evaluate_agent with len(envs) episodes in flight: eval_episodes
        deterministic episodes seeded self.seed + 1 ... self.seed +
        eval_episodes in the order they start (the first len(envs) together; an
        env that finishes takes the next seed and its row starts an episode).
        An env with no episode left drops out of the batch.  Returns the mean
        total reward (taken in episode order) as a device scalar."""
        def step(frames, state, first, carried):
            action, _, _, latent, hidden = self.act_step_batch(frames, state, first, deterministic=True)
            return action, latent, hidden, None

        return self._run_episodes(envs, eval_episodes, step)

    def _run_episodes(self, envs, eval_episodes, step, carry=None):
        """The episode loop of evaluate_agent_vec and evaluate_planner.
        step(frames (N,...), state, first, carried) -> (action, latent, hidden,
        extra) acts for the N episodes in flight: state is the (latent, hidden,
        action) of the surviving rows (None on the first step), first marks
        the rows that start an episode.  carry(extra, idx), if given, makes the
        next step's `carried` out of this step's `extra`, idx (a device int64
        tensor) being the rows that go on."""
        totals = [0] * eval_episodes
        with torch.no_grad():
            slots = []  # [env, episode index] in flight
            for env in envs[:eval_episodes]:
                self.seed += 1
                slots.append([env, len(slots)])
            started = len(slots)
            frames = [env.reset(seed=self.seed - started + 1 + ep)[0] for env, ep in slots]
            state, carried, first = None, None, np.ones(len(slots), dtype=bool)
            while slots:
                action, latent, hidden, extra = step(np.stack(frames), state, first, carried)
                action_np = action.detach().cpu().numpy().reshape(len(slots), -1)
                self.act_check()
                keep, frames, first = [], [], []
                for i, slot in enumerate(slots):
                    env, ep = slot
                    observation_, reward, terminated, truncated, _ = env.step(action_np[i])
                    totals[ep] += reward
                    if not (terminated or truncated):
                        first.append(False)
                    elif started < eval_episodes:
                        self.seed += 1
                        observation_, _ = env.reset(seed=self.seed)
                        slot[1] = started
                        started += 1
                        first.append(True)
                    else:
                        continue
                    keep.append(i)
                    frames.append(observation_)
                slots = [slots[i] for i in keep]
                first = np.asarray(first, dtype=bool)
                if slots:
                    idx = torch.tensor(keep, device=self.device)
                    state = tuple(t.index_select(0, idx) for t in (latent, hidden, action))
                    if carry is not None:
                        carried = carry(extra, idx)
        return torch.tensor(totals, dtype=torch.float32, device=self.device).mean()

    # ------------------------------------------------- latent planning (HIP)
    def plan(self, z, h, horizon=None, candidates=512, policy_candidates=24, elites=64, iterations=6,
             temperature=0.5, momentum=0.1, std_init=0.5, std_min=0.05, std_max=2.0, mean_init=None, sample=True,
             bootstrap="critic", noise=None, _mark=None):
        """Choose actions by a CEM / MPPI search over world-model rollouts
        (plan.py; the definitions are in include/dreamer_hip.h).  z (E, R*C) or
        the (E,1,R,C) act_step_batch returns, h (E, hidden) or (E,1,hidden): the
        belief states of E environments.  Per environment `candidates` action
        sequences of `horizon` (default self.horizon) steps are drawn around a
        mean (mean_init (E,H,A), default zeros) with std_init, the first
        `policy_candidates` of them the sampling actor's own; they are rolled
        out through the prior (dr_imagine_actions), scored by their discounted
        predicted rewards (gamma is the agent's) plus the value of the end state
        (bootstrap: "critic", "target" for the target critic, None for 0), and
        the best `elites` refit mean and std (weights exp((G - G_best) /
        temperature), all 1 at temperature 0; mean <- momentum mean + (1 -
        momentum) m; std clamped to [std_min, std_max]), `iterations` times.
        Returns a PlanResult; its action is the final mean's first step.

        sample=False takes the prior's mode (q == 1) in every rollout, as
        open_loop does.  noise: a pair (eps (J,E,N,H*A), q (J,H,E*N*R,C)) of
        explicit N(0,1) / Exp(1) draws (either may be None: Philox, or the mode);
        the actor's sequence (e, n) then takes the draws of candidate (e, n) of
        iteration 0.  Every argument is checked (plan.check_plan, ValueError)
        before the device is touched.  Everything is enqueued on the current
        stream without a sync, every launch in launch form (never a persistent
        kernel: the planner may run beside training); the engine's random state
        is not used.  _mark: stage hook of tools/plan_timing.py."""
        from .plan import plan
        return plan(self, z, h, horizon=horizon, candidates=candidates, policy_candidates=policy_candidates,
                    elites=elites, iterations=iterations, temperature=temperature, momentum=momentum,
                    std_init=std_init, std_min=std_min, std_max=std_max, mean_init=mean_init, sample=sample,
                    bootstrap=bootstrap, noise=noise, _mark=_mark)

    def plan_step(self, observations, state=None, first=None, plan_state=None, **plan_kw):
        """One env step of E environments under the planner: the filter of
        act_step_batch(observations, state, first, deterministic=True), then
        plan on its (z', h').  plan_state: the previous step's PlanResult (its
        shifted() mean warm-starts the search) or an (E,H,A) mean; rows with
        `first` start from zeros.  A row whose search ended without an elite
        (PlanResult.ok false) takes the actor's deterministic action.  Returns
        (actions (E,1,A), (z', h', actions), PlanResult): the state tuple feeds
        the next call as act_step_batch's does."""
        from .plan import plan_step
        return plan_step(self, observations, state=state, first=first, plan_state=plan_state, **plan_kw)

    def evaluate_planner(self, envs, eval_episodes, **plan_kw):
        """evaluate_agent_vec with plan_step in place of act_step_batch: the
        same seeds, episode order and bookkeeping; each env's plan is warm-
        started from its previous step's.  Returns the mean total reward (taken
        in episode order) as a device scalar."""
        from .plan import evaluate_planner
        return evaluate_planner(self, envs, eval_episodes, **plan_kw)

    def train_dreamer(self, env, eval_env):  # Dreamer.py:324-372
        """A list or tuple of environments in either position selects the
        vectorised methods (rollout_policy_vec / evaluate_agent_vec) for it."""
        rollout = self.rollout_policy_vec if isinstance(env, (list, tuple)) else self.rollout_policy
        evaluate = self.evaluate_agent_vec if isinstance(eval_env, (list, tuple)) else self.evaluate_agent
        WM_loss_list, actor_loss_list, critic_loss_list, evaluation_list = [], [], [], []
        print("Starting Training...")
        print("Starting Random Kickstart.")
        for _ in tqdm(range(self.random_iterations), desc="Kickstarting Dreamer Agent.", leave=True):
            rollout(env, random_policy=True)
            WM_loss_list.append([x.detach().cpu().item() for x in self.train_world_model()])
        print("Starting Training Loop...")
        evaluation_list.append(evaluate(eval_env, eval_episodes=3).detach().cpu().item())
        for it in tqdm(range(self.training_iterations), desc="Training Dreamer Agent.", leave=True):
            rollout(env, random_policy=False)
            wm_loss = self.train_world_model()
            actor_loss, critic_loss = self.train_Agent()
            WM_loss_list.append([x.detach().cpu().item() for x in wm_loss])
            actor_loss_list.append(actor_loss.detach().cpu().item())
            critic_loss_list.append(critic_loss.detach().cpu().item())
            if it % 1000 == 0:
                os.makedirs("./models", exist_ok=True)
                self.save_trained_Dreamer(os.path.join("./models", f"agent_checkpoint_{it}.pth"))
                self.save_trained_Dreamer(os.path.join("./models", "agent_latest.pth"))
                np.savez(os.path.join("./models", "training_logs.npz"),
                         world_model_loss=_sanitize_for_save(WM_loss_list),
                         actor_loss=_sanitize_for_save(actor_loss_list),
                         critic_loss=_sanitize_for_save(critic_loss_list),
                         rewards=_sanitize_for_save(evaluation_list))
            if it % 500 == 0:
                evaluation_list.append(evaluate(eval_env, eval_episodes=3).detach().cpu().item())
        print("Training Complete.")
        evaluation_list.append(evaluate(eval_env, eval_episodes=10).detach().cpu().item())
        return WM_loss_list, actor_loss_list, critic_loss_list, evaluation_list

    def Run(self, env, env_seed, render=True):  # Dreamer.py:374-401
        total = 0
        observation, _ = env.reset(seed=env_seed)
        with torch.no_grad():
            action, _, _, latent, hidden = self.act_step(observation, deterministic=True)
        done = False
        while not done:
            if render:
                env.render()
            action_np = action.detach().cpu().numpy().squeeze(0).squeeze(0)
            self.act_check()
            observation_, reward, terminated, truncated, _ = env.step(action_np)
            total += reward
            done = terminated or truncated
            if not done:
                with torch.no_grad():
                    action, _, _, latent, hidden = self.act_step(observation_, latent, hidden, action,
                                                                 deterministic=True)
        return total
