"""Agent trace on replay windows: the result container of
``Dreamer.agent_trace`` and the window arithmetic it shares with the tests.

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
    st = torch.as_tensor(starts, dtype=torch.int64).reshape(-1, 1)
    kf = torch.arange(0, length, dtype=torch.int64).reshape(1, -1)
    kt = torch.arange(0, length - 1, dtype=torch.int64).reshape(1, -1)
    return (st + kf) % capacity, (st + kt) % capacity


def check_length(length, sequence_length):
    if length < 2 or length > sequence_length:
        raise ValueError(f"agent trace needs 2 <= length <= sequence_length (got {length} vs {sequence_length})")


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
