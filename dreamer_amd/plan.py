"""Latent planning: a CEM / MPPI action search over world-model rollouts
(Dreamer.plan, plan_step, evaluate_planner; include/dreamer_hip.h "latent
planning" has the definitions the kernels fix).

E environments with belief states (h_e, z_e), horizon H, N candidate action
sequences per environment of which the first N_pi are the actor's own, K
elites, J iterations.  Per environment the search keeps mean[H][A] and
std[H][A].  One iteration: dr_plan_sample draws the candidates
(clamp(mean + std * eps, -1, 1)), dr_imagine_actions rolls the prior forward
under all E*N of them from the replicated states, dr_critic_fwd values state H
of every row straight out of the rollout's arrays, and dr_plan_update scores
the rows (G = the lambda = 1 return: r_1 + gamma c_1 (r_2 + ... gamma c_H V_H)),
ranks them within their environment (score descending, ties by the lower
index, non-finite scores never elite), weighs the K' = min(K, finite) elites
(1 at temperature 0, else exp((G_j - G_0) / temperature)) and refits
mean <- momentum mean + (1 - momentum) m, std <- clamp(s) from their weighted
moments.  The action is the final mean's first step.

The actor's sequences are one dr_imagine_fwd at B = E*N_pi (sampling actor)
per call, reused by every iteration.  Every launch of the planner is in launch
form (dr_dims.launch_form = 1): it may run on an acting thread beside
training, and a persistent launch needs every CU."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import hip

# rows of one rollout (E * N): DR_ACT_MAX_ENVS environments of DR_PLAN_MAX_CANDIDATES candidates
PLAN_MAX_ROWS = L.DR_ACT_MAX_ENVS * L.DR_PLAN_MAX_CANDIDATES


def check_plan(E, N, N_pi, K, H, J, A=1, temperature=0.5, momentum=0.1, std_init=0.5, std_min=0.05, std_max=2.0,
               bootstrap="critic"):
    """Raise ValueError unless these are sizes and settings Dreamer.plan can
    run: E >= 1 environments, N candidates (1 <= N <= DR_PLAN_MAX_CANDIDATES,
    E * N <= PLAN_MAX_ROWS), 0 <= N_pi <= N of them the actor's, 1 <= K <= N
    elites, horizon H >= 1 with H * A <= DR_PLAN_MAX_ELEMS, J >= 1 iterations,
    temperature >= 0, 0 <= momentum < 1, 0 <= std_min <= std_max, std_init >=
    0, all finite, and bootstrap one of "critic", "target", None."""
    for name, v, lo in (("environments", E, 1), ("candidates", N, 1), ("policy_candidates", N_pi, 0),
                        ("elites", K, 1), ("horizon", H, 1), ("iterations", J, 1), ("action dims", A, 1)):
        if int(v) != v or v < lo:
            raise ValueError(f"plan: {name} must be an integer >= {lo} (got {v!r})")
    if K > N:
        raise ValueError(f"plan: elites ({K}) above candidates ({N})")
    if N_pi > N:
        raise ValueError(f"plan: policy_candidates ({N_pi}) above candidates ({N})")
    if N > L.DR_PLAN_MAX_CANDIDATES:
        raise ValueError(f"plan: candidates ({N}) above DR_PLAN_MAX_CANDIDATES = {L.DR_PLAN_MAX_CANDIDATES}")
    if E * N > PLAN_MAX_ROWS:
        raise ValueError(f"plan: {E} environments x {N} candidates is above {PLAN_MAX_ROWS} rollout rows")
    if H * A > L.DR_PLAN_MAX_ELEMS:
        raise ValueError(f"plan: horizon x action dims ({H} x {A}) above DR_PLAN_MAX_ELEMS = {L.DR_PLAN_MAX_ELEMS}")
    for name, v in (("temperature", temperature), ("momentum", momentum), ("std_init", std_init),
                    ("std_min", std_min), ("std_max", std_max)):
        if not math.isfinite(float(v)):
            raise ValueError(f"plan: {name} must be finite (got {v!r})")
    if temperature < 0:
        raise ValueError(f"plan: temperature must be >= 0 (got {temperature})")
    if not 0 <= momentum < 1:
        raise ValueError(f"plan: momentum must be in [0, 1) (got {momentum})")
    if not 0 <= std_min <= std_max:
        raise ValueError(f"plan: need 0 <= std_min <= std_max (got {std_min}, {std_max})")
    if std_init < 0:
        raise ValueError(f"plan: std_init must be >= 0 (got {std_init})")
    if bootstrap not in ("critic", "target", None):
        raise ValueError(f"plan: bootstrap must be 'critic', 'target' or None (got {bootstrap!r})")


@dataclass
class PlanResult:
    """Device tensors of one Dreamer.plan call over E environments.

    action (E,A): the final mean's first step.  mean, std (E,H,A): the final
    sampling distribution.  best_actions (E,H,A), best_score (E,): the
    top-ranked candidate of the last iteration (NaN where it had no elite).
    score_mean, score_best, elite_score_mean (J,E): per iteration the mean of
    the finite scores, the top-ranked score and the plain mean of the elites'
    scores (NaN where there is none).  policy_score (E,): the mean score of the
    actor's candidates in the last iteration, NaN when N_pi = 0.  n_elite (J,E)
    int32.  ok (E,) bool: the last iteration had an elite.  scores (E,N): the
    last iteration's raw scores.  candidates (E,N,H,A): its action sequences;
    elite_idx (E,K) int32 (-1 past n_elite) and elite_w (E,K): its elites in
    rank order and their normalised weights."""
    action: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    best_actions: torch.Tensor
    best_score: torch.Tensor
    score_mean: torch.Tensor
    score_best: torch.Tensor
    elite_score_mean: torch.Tensor
    policy_score: torch.Tensor
    n_elite: torch.Tensor
    ok: torch.Tensor
    scores: torch.Tensor
    candidates: torch.Tensor = None
    elite_idx: torch.Tensor = None
    elite_w: torch.Tensor = None

    def shifted(self):
        """mean moved one step earlier with the last step repeated (E,H,A): the next env step's mean_init."""
        return torch.cat((self.mean[:, 1:], self.mean[:, -1:]), dim=1)


def _fresh_noise(dev, q=None, eps=None):
    """A fresh ad-hoc Philox noise struct; the given variates replace its draws."""
    nz = hip.adhoc(dev).noise()
    nz.q = L.ptr(q) if q is not None else None
    nz.eps = L.ptr(eps) if eps is not None else None
    return nz


def plan_dims(dr):
    """The dims every launch of the planner runs under: the model's, in launch form."""
    d = dr.world_model.dims(dr.agent)
    d.launch_form = 1
    return d


def _policy_sequences(dr, d, E, N, N_pi, H, z0, h0, eps0, q0, sample):
    """[E][N_pi][H][A] action sequences of the sampling actor from the replicated
    states: one dr_imagine_fwd at B = E * N_pi in launch form.  Explicit noise:
    row (e, n) takes the draws candidate (e, n) has in iteration 0 (eps0
    (E,N,H*A), q0 (H,E*N*R,C)); sample=False takes the prior's mode."""
    wmod, ag = dr.world_model, dr.agent
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    dev = h0.device
    B = E * N_pi
    zP, hP = z0.repeat_interleave(N_pi, 0), h0.repeat_interleave(N_pi, 0)
    eps = q = None
    if eps0 is not None:
        eps = eps0.reshape(E, N, H, A)[:, :N_pi].permute(2, 0, 1, 3).reshape(H, B, A).contiguous()
    if q0 is not None:
        q = q0.reshape(H, E, N, R, C)[:, :, :N_pi].reshape(H, B * R, C).contiguous()
    elif not sample:
        q = torch.ones(H, B * R, C, device=dev)
    lat = torch.empty(B, H + 1, R, C, device=dev)
    hid = torch.empty(B, H + 1, Hd, device=dev)
    act, mu, sg = (torch.empty(B, H, A, device=dev) for _ in range(3))
    rew, cont = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
    tape = torch.empty(L.query("dr_imagine_tape_bytes", d, B, H), dtype=torch.uint8, device=dev)
    ws = hip.workspace(dev).get("plan_im", L.query("dr_imagine_workspace_bytes", d, B, H))
    L.call("dr_imagine_fwd", d, wmod.packed(), ag.actor_struct(), B, H, L.ptr(zP), L.ptr(hP),
           _fresh_noise(dev, q=q, eps=eps), 0, L.ptr(lat), L.ptr(hid), L.ptr(act), L.ptr(rew), L.ptr(cont), L.ptr(mu),
           L.ptr(sg), L.ptr(tape), L.ptr(ws), ws.numel(), hip.stream())
    return act


def plan(dr, z, h, horizon=None, candidates=512, policy_candidates=24, elites=64, iterations=6, temperature=0.5,
         momentum=0.1, std_init=0.5, std_min=0.05, std_max=2.0, mean_init=None, sample=True, bootstrap="critic",
         noise=None, _mark=None):
    """Dreamer.plan (see its docstring)."""
    mark = _mark or (lambda name: None)
    H = dr.horizon if horizon is None else horizon
    N, N_pi, K, J = candidates, policy_candidates, elites, iterations
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    if h.dim() < 2 or h.shape[0] < 1 or h.numel() != h.shape[0] * Hd:
        raise ValueError(f"plan: h must be (E, {Hd}) or (E, 1, {Hd}), got {tuple(h.shape)}")
    E = h.shape[0]
    if z.numel() != E * R * C or z.shape[0] != E:
        raise ValueError(f"plan: z must be ({E}, {R * C}) or ({E}, 1, {R}, {C}), got {tuple(z.shape)}")
    check_plan(E, N, N_pi, K, H, J, A, temperature, momentum, std_init, std_min, std_max, bootstrap)
    N, N_pi, K, H, J = int(N), int(N_pi), int(K), int(H), int(J)  # (integers, as check_plan has seen)
    if mean_init is not None and tuple(mean_init.shape) != (E, H, A):
        raise ValueError(f"plan: mean_init must be ({E}, {H}, {A}), got {tuple(mean_init.shape)}")
    eps_all = q_all = None
    if noise is not None:
        eps_all, q_all = noise
        if eps_all is not None and tuple(eps_all.shape) != (J, E, N, H * A):
            raise ValueError(f"plan: noise eps must be ({J}, {E}, {N}, {H * A}), got {tuple(eps_all.shape)}")
        if q_all is not None and tuple(q_all.shape) != (J, H, E * N * R, C):
            raise ValueError(f"plan: noise q must be ({J}, {H}, {E * N * R}, {C}), got {tuple(q_all.shape)}")
    L.require_gpu(h)
    # the planner's draws are its own: an acting-shaped hip.noise_override around the call is set aside
    with hip.noise_override_suspended():
        return _search(dr, E, N, N_pi, K, J, H, z, h, float(temperature), float(momentum), float(std_init),
                       float(std_min), float(std_max), mean_init, sample, bootstrap, eps_all, q_all, mark)


def _search(dr, E, N, N_pi, K, J, H, z, h, temperature, momentum, std_init, std_min, std_max, mean_init, sample,
            bootstrap, eps_all, q_all, mark):
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    dev = h.device
    wmod, ag = dr.world_model, dr.agent
    ag._ensure_flat()
    d = plan_dims(dr)
    stream = hip.stream()
    B = E * N
    h0, z0 = h.reshape(E, Hd).float().contiguous(), z.reshape(E, R * C).float().contiguous()
    hB, zB = h0.repeat_interleave(N, 0), z0.repeat_interleave(N, 0)
    if eps_all is not None:
        eps_all = eps_all.to(dev).float().contiguous()
    if q_all is not None:
        q_all = q_all.to(dev).float().contiguous()
    q_mode = torch.ones(H, B * R, C, device=dev) if (q_all is None and not sample) else None
    if mean_init is None:
        mean = torch.zeros(E, H, A, device=dev)
    else:  # a copy in the kernels' [E][H][A] layout, whatever the strides of the caller's tensor
        mean = mean_init.to(dev).float().clone(memory_format=torch.contiguous_format)
    std = torch.full((E, H, A), float(std_init), device=dev)
    pol = None
    if N_pi > 0:
        pol = _policy_sequences(dr, d, E, N, N_pi, H, z0, h0, None if eps_all is None else eps_all[0],
                                None if q_all is None else q_all[0], sample)
    mark("policy")
    cand = torch.empty(E, N, H, A, device=dev)
    scores = torch.empty(J, E, N, device=dev)
    elite_idx = torch.empty(J, E, K, dtype=torch.int32, device=dev)
    elite_w = torch.empty(J, E, K, device=dev)
    n_elite = torch.empty(J, E, dtype=torch.int32, device=dev)
    v_last = critic = None
    if bootstrap is not None:
        v_last = torch.empty(B, device=dev)
        critic = ag.critic_struct(target=(bootstrap == "target"))
        ws = hip.workspace(dev).get("plan_crit", L.query("dr_critic_workspace_bytes", d, B, 0))
    for j in range(J):
        nz = _fresh_noise(dev, eps=None if eps_all is None else eps_all[j])
        L.call("dr_plan_sample", E, N, N_pi, H, A, L.ptr(mean), L.ptr(std), L.ptr(pol), nz, L.ptr(cand), stream)
        mark("sample")
        lat, hid, rew, cont = wmod._imagine_actions(d, B, H, zB, hB, cand.data_ptr(), H * A, A,
                                                    q_mode if q_all is None else q_all[j])
        mark("rollout")
        if v_last is not None:  # state H of every row, read in place with the row stride of the rollout's arrays
            L.call("dr_critic_fwd", d, critic, B, hid.data_ptr() + 4 * H * Hd, (H + 1) * Hd,
                   lat.data_ptr() + 4 * H * R * C, (H + 1) * R * C, None, L.ptr(v_last), None, L.ptr(ws), ws.numel(),
                   stream)
            mark("critic")
        L.call("dr_plan_update", E, N, H, A, K, L.ptr(rew), L.ptr(cont), L.ptr(v_last), float(ag.gamma),
               float(temperature), float(momentum), float(std_min), float(std_max), L.ptr(cand), L.ptr(mean),
               L.ptr(std), L.ptr(scores[j]), L.ptr(elite_idx[j]), L.ptr(elite_w[j]), L.ptr(n_elite[j]), stream)
        mark("update")
    # the per-iteration curves, once, from what the J updates left behind
    nan = torch.full((), float("nan"), device=dev)
    fin = torch.isfinite(scores)
    score_mean = torch.where(fin, scores, torch.zeros_like(scores)).sum(-1) / fin.sum(-1)
    valid = elite_idx >= 0
    es = torch.gather(scores, -1, elite_idx.clamp(min=0).long())
    elite_score_mean = torch.where(valid, es, torch.zeros_like(es)).sum(-1) / valid.sum(-1)
    score_best = torch.where(valid[..., 0], es[..., 0], nan)
    ok = n_elite[-1] > 0
    top = elite_idx[-1, :, 0].clamp(min=0).long()
    best_actions = torch.where(ok.view(E, 1, 1), cand[torch.arange(E, device=dev), top], nan)
    policy_score = scores[-1, :, :N_pi].mean(-1) if N_pi > 0 else torch.full((E,), float("nan"), device=dev)
    mark("stats")
    return PlanResult(action=mean[:, 0].clone(), mean=mean, std=std, best_actions=best_actions,
                      best_score=score_best[-1], score_mean=score_mean, score_best=score_best,
                      elite_score_mean=elite_score_mean, policy_score=policy_score, n_elite=n_elite, ok=ok,
                      scores=scores[-1], candidates=cand, elite_idx=elite_idx[-1], elite_w=elite_w[-1])


def plan_step(dr, observations, state=None, first=None, plan_state=None, **plan_kw):
    """Dreamer.plan_step (see its docstring)."""
    observations = np.asarray(observations)
    E = observations.shape[0]
    if first is None:
        first = np.ones(E, dtype=bool) if state is None else np.zeros(E, dtype=bool)
    first = np.asarray(first, dtype=bool).reshape(E)
    a_pi, _, _, z2, h2 = dr.act_step_batch(observations, state, first, deterministic=True)
    mean_init = None
    if plan_state is not None:
        mean_init = plan_state.shifted() if isinstance(plan_state, PlanResult) else plan_state
        restart = torch.from_numpy(first).to(mean_init.device).view(E, 1, 1)
        mean_init = torch.where(restart, torch.zeros_like(mean_init), mean_init)
    res = plan(dr, z2, h2, mean_init=mean_init, **plan_kw)
    actions = torch.where(res.ok.view(E, 1, 1), res.action.view(E, 1, -1), a_pi)
    return actions, (z2, h2, actions), res


def evaluate_planner(dr, envs, eval_episodes, **plan_kw):
    """Dreamer.evaluate_planner (see its docstring)."""
    def step(frames, state, first, plan_mean):
        action, (latent, hidden, _), res = plan_step(dr, frames, state, first, plan_mean, **plan_kw)
        return action, latent, hidden, res

    # beyond the state, each surviving env carries its plan's shifted mean
    return dr._run_episodes(envs, eval_episodes, step, carry=lambda res, idx: res.shifted().index_select(0, idx))
