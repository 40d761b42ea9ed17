"""Agent trace on replay windows: ``Dreamer.agent_trace`` and
``evaluate_values``, their result container and the window arithmetic they
share with the tests (the front end is replay_eval.py's).

A window b is S = sequence_length consecutive ring slots from starts[b].  Slot
t holds the frame x_t, the action a_t taken on seeing x_t and the symlog
reward / continue flag of that transition (rollout_policy, Dreamer.py:212).
The states s_t = (h_t, z_t), t < T, are closed_loop's filter
(warm_start_generator, Dreamer.py:244-262): state t has seen frames 0..t and
actions 0..t-1, so the actor's distribution at s_t is what the current policy
would do where the replay did a_t, and state t + 1's heads are compared with
slot t (unroll_model, WorldModel.py:113-123).

For t < T: V_t = critic.value(s_t), Vbar_t = target_critic.value(s_t)
(Agent.py:237-241), the online critic's logits, (mu_t, sigma_t) =
actor.forward(s_t) (Agent.py:191-200).  For t <= T - 2, r_t = symexp(stored
symlog reward of slot t) with DreamerUtils.py:35-37's clamp, c_t = the stored
flag, and the returns are compute_batched_R_lambda_returns (Agent.py:156-172)
with H = T - 1 on real r and c and the target values:

    R_t = r_t + gamma c_t ((1 - lambda) Vbar_{t+1} + lambda R_{t+1}),
    R_{T-2} = r_{T-2} + gamma c_{T-2} Vbar_{T-1};
    R^mc: the same at lambda = 1;  td_t = (r_t + gamma c_t Vbar_{t+1}) - Vbar_t.

A continue flag of 0 cuts the recursion; the filter is not reset there
(warm_start_generator does not reset it either)."""
from dataclasses import dataclass

import torch

from . import _lib as L
from . import hip
from .replay_eval import average_curves, check_window, resolve_noise, ring_slots, window_prologue


def action_step(t):
    """Window step of the recorded action the actor at state t is scored on."""
    if t < 0:
        raise ValueError("state index must be >= 0")
    return t


def transition_step(t):
    """Window step of the stored reward / continue flag of the transition out of state t."""
    if t < 0:
        raise ValueError("state index must be >= 0")
    return t


def trace_slots(starts, length, capacity):
    """(frame / action slots [B][T], reward / continue slots [B][T-1]) in the ring, as int64 tensors."""
    return ring_slots(starts, 0, length, capacity), ring_slots(starts, 0, length - 1, capacity)


def check_length(length, sequence_length):
    check_window(2 <= length <= sequence_length, "agent trace needs 2 <= length <= sequence_length", length,
                 sequence_length)


@dataclass
class AgentTraceResult:
    """Device tensors of one agent trace over B windows of T = length steps.

    latents (B,T,R,C), hiddens (B,T,hidden): the filtered states.
    value, value_target (B,T): critic.value / target_critic.value at the states.
    critic_logits (B,T,nb): the online critic's; value_entropy (B,T) their
    entropy, value_std_symlog (B,T) the spread of the bucket distribution in
    symlog units.
    actor_mu, actor_sigma (B,T,A): actor.forward; actions (B,T,A) the recorded
    ones; action_logprob (B,T) their log-probability under the current actor
    (Agent.py:110-115), action_logprob_dims (B,T,A) its terms,
    policy_entropy_base (B,T) the Normal's entropy sum_i (1/2 + 1/2 log 2 pi +
    log sigma_i).
    reward (natural space), cont (B,T-1): slot t's stored transition.
    returns_lambda, returns_mc, td (B,T-1): see the module text; critic_ce
    (B,T-1) the online critic's two-hot cross-entropy against returns_lambda
    (Agent.py:127-135)."""
    latents: torch.Tensor
    hiddens: torch.Tensor
    value: torch.Tensor
    value_target: torch.Tensor
    value_entropy: torch.Tensor
    value_std_symlog: torch.Tensor
    critic_logits: torch.Tensor
    actor_mu: torch.Tensor
    actor_sigma: torch.Tensor
    actions: torch.Tensor
    action_logprob: torch.Tensor
    policy_entropy_base: torch.Tensor
    action_logprob_dims: torch.Tensor
    reward: torch.Tensor
    cont: torch.Tensor
    returns_lambda: torch.Tensor
    returns_mc: torch.Tensor
    td: torch.Tensor
    critic_ce: torch.Tensor
    length: int

    def advantage(self):
        """returns_lambda - value[:, :-1] (B,T-1): the actor loss's advantage (Agent.py:105-107) on real data."""
        return self.returns_lambda - self.value[:, :-1]

    def explained_variance(self):
        """1 - Var(R - V) / Var(R) over all (b, t <= T-2), population variances;
        NaN when Var(R) = 0."""
        R = self.returns_lambda.reshape(-1)
        res = (self.returns_lambda - self.value[:, :-1]).reshape(-1)
        var_r = R.var(unbiased=False)
        if float(var_r) == 0.0:
            return torch.full_like(var_r, float("nan"))
        return 1.0 - res.var(unbiased=False) / var_r

    def value_error(self):
        """value[:, :-1] - returns_mc (B,T-1): the critic against the discounted real return."""
        return self.value[:, :-1] - self.returns_mc


def agent_trace(dr, starts=None, batch_size=None, length=None, sample=True, noise=None, _mark=None):
    """Dreamer.agent_trace (see its docstring)."""
    mark = _mark or (lambda name: None)
    S = dr.sequence_length
    T = S if length is None else int(length)
    check_length(T, S)
    ag = dr.agent
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims

    def draws(B, dev):
        return resolve_noise(None if noise is None else (noise,), sample, ((T, B * R, C),),
                             f"noise must be one tensor of shape ({T}, {B * R}, {C})", dev)

    w = window_prologue(dr, starts, batch_size, T, draws, mark)
    B, dev, d, stream = w.B, w.st.device, w.d, w.stream
    act, rew, cont = w.act, w.rew, w.cont
    # action t-1 drives frame t: closed_loop's filter, without the prior and the heads
    lat, hid, _, _, _, _ = dr.world_model._observe_trace(d, B, T, w.feat, act.data_ptr(), S * A, A, None, None,
                                                         w.noise[0], heads=False, prior=False)
    mark("trace")
    # both critics over the M = B*T states, rows straight from the trace's arrays
    ag._ensure_flat()
    M, nb = B * T, ag.buckets
    logits = torch.empty(B, T, nb, device=dev)
    V, Vt = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    ws = hip.workspace(dev).get("at_crit", L.query("dr_critic_workspace_bytes", d, B, T - 1))
    L.call("dr_critic_fwd", d, ag.critic_struct(), M, L.ptr(hid), Hd, L.ptr(lat), R * C, L.ptr(logits), L.ptr(V),
           None, L.ptr(ws), ws.numel(), stream)
    L.call("dr_critic_fwd", d, ag.critic_struct(target=True), M, L.ptr(hid), Hd, L.ptr(lat), R * C, None, L.ptr(Vt),
           None, L.ptr(ws), ws.numel(), stream)
    mark("critics")
    mu, sg, a_mode = (torch.empty(B, T, A, device=dev) for _ in range(3))
    ws = hip.workspace(dev).get("act", L.query("dr_actor_act_workspace_bytes", d, M))
    L.call("dr_actor_act", d, ag.actor_struct(), M, L.ptr(hid), L.ptr(lat), L.dr_noise(), 1, L.ptr(a_mode),
           L.ptr(mu), L.ptr(sg), L.ptr(ws), ws.numel(), stream)
    mark("actor")
    # slot t's stored transition leaves state t: real rewards (symexp of the ring's symlog) under the target values
    Rl, Rmc, td, ce = (torch.empty(B, T - 1, device=dev) for _ in range(4))
    L.call("dr_replay_returns", B, T, L.ptr(rew), S, L.ptr(cont), S, 1, L.ptr(Vt), ag.gamma, ag.lambda_, L.ptr(Rl),
           L.ptr(Rmc), L.ptr(td), stream)
    # the natural-space rewards as that kernel formed them: at gamma = 0 the recursion is r + 0, so
    # returns_lambda follows from the result's own reward / cont / value_target bit for bit
    r_nat = torch.empty(B, T - 1, device=dev)
    L.call("dr_replay_returns", B, T, L.ptr(rew), S, L.ptr(cont), S, 1, L.ptr(Vt), 0.0, 0.0, L.ptr(r_nat), None,
           None, stream)
    mark("returns")
    ent, std = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    L.call("dr_value_stats", B, T, T - 1, nb, L.ptr(logits), nb, L.ptr(ag.critic.buckets_crit), L.ptr(Rl),
           L.ptr(ent), L.ptr(std), L.ptr(ce), stream)
    mark("value_stats")
    logp, hbase = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    logp_dims = torch.empty(B, T, A, device=dev)
    L.call("dr_action_logprob", B, T, A, L.ptr(mu), L.ptr(sg), L.ptr(act), S * A, A, L.ptr(logp), L.ptr(logp_dims),
           L.ptr(hbase), stream)
    mark("logprob")
    return AgentTraceResult(latents=lat, hiddens=hid, value=V, value_target=Vt, value_entropy=ent,
                            value_std_symlog=std, critic_logits=logits, actor_mu=mu, actor_sigma=sg,
                            actions=act[:, :T].clone(), action_logprob=logp, policy_entropy_base=hbase,
                            action_logprob_dims=logp_dims, reward=r_nat,
                            cont=cont[:, :T - 1].clone(), returns_lambda=Rl, returns_mc=Rmc, td=td, critic_ce=ce,
                            length=T)


CURVES = ("value", "value_target", "value_entropy", "value_std_symlog", "action_logprob", "actor_sigma",
          "returns_lambda", "returns_mc", "abs_td", "critic_ce", "abs_advantage")


def curves_of(r):
    return [r.value.mean(0), r.value_target.mean(0), r.value_entropy.mean(0), r.value_std_symlog.mean(0),
            r.action_logprob.mean(0), r.actor_sigma.mean((0, 2)), r.returns_lambda.mean(0), r.returns_mc.mean(0),
            r.td.abs().mean(0), r.critic_ce.mean(0), r.advantage().abs().mean(0)]


def evaluate_values(dr, batches=1, batch_size=None, length=None, sample=True):
    """Dreamer.evaluate_values (see its docstring)."""
    ev = []  # the extra scalar: explained_variance of every batch

    def curves(r):
        cur = curves_of(r)
        ev.append(float(r.explained_variance()))
        return cur

    out = average_curves("evaluate_values", dr, batches, CURVES, lambda: dr.agent_trace(
        batch_size=batch_size, length=length, sample=sample), curves)
    out["explained_variance"] = sum(ev) / float(batches)
    return out
