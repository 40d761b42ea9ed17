"""Batched acting: dr_act_batch (one launch for N environments) and the
Dreamer methods on top of it -- act_step_batch, evaluate_agent_vec,
rollout_policy_vec and train_dreamer with lists of environments.

The kernel's contract is row independence: row e's outputs depend on row e's
inputs and noise alone and are the bits dr_act_step gives on them, so the
kernel tests compare rows with ``torch.equal`` against Dreamer.act_step and
pin the one-launch path with ``act_batch_path = "fused"`` (the default
dispatch follows the timing table).  dr_act_step is the
one-row launch of the same kernel, so those comparisons are about the batch a
row travels in (size, position, first flags, instantiation); what the kernel
computes is checked against the CPU oracle.  Against the CPU
oracle the tolerances are test_act_step_matches_oracle's: latent indices
exact (inputs are tie-guarded), |d| <= 1e-6 + 1e-4 |ref| on h', mu, sigma
and the action, 1e-6 on the straight-through latent values."""
import time

import numpy as np
import pytest
import torch

from baseline_case import TieGuard
from conftest import state_layout
from formula import FULL, formula_state_dict
from gpu_helpers import close, cpu
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
R, C, A, HD = 32, 32, 3, 600
NAMES = ("a", "mu", "sigma", "z", "h")


def _dreamer(dev, formula=True, **over):
    """CarRacing widths; formula weights (or the default init)."""
    from dreamer_amd import Dreamer
    cfg = dict(FULL)
    cfg.update(over)
    torch.manual_seed(0)
    d = Dreamer(cfg, dev)
    if not formula:
        return d, None
    P = formula_state_dict(dict(state_layout("full")))
    d.load_state_dict({k: v.to(dev) for k, v in P.items()})
    return d, P


@pytest.fixture(scope="module")
def fused(gpu):
    """One Dreamer with formula weights, pinned to the one-launch path."""
    d, P = _dreamer(gpu)
    d.act_batch_path = "fused"
    return d, P


def _idx(z):
    return cpu(z).reshape(-1, C).argmax(-1)


def _case(N, seed):
    """Frames, a random previous state and explicit noise for N rows."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, 64, 64, 3), generator=g, dtype=torch.uint8).numpy()
    z = torch.nn.functional.one_hot((torch.randn(N, 1, R, C, generator=g) * 2).argmax(-1), C).float()
    h = torch.randn(N, 1, HD, generator=g)
    a = torch.rand(N, 1, A, generator=g) * 2 - 1
    q = torch.empty(N * R, C).exponential_(generator=g)
    eps = torch.randn(N, A, generator=g)
    return frames, (z, h, a), q, eps


def _single(d, gpu, frame, state, first, q, eps, deterministic=False):
    """Dreamer.act_step on one row with that row's noise."""
    from dreamer_amd import hip
    with hip.noise_override(q=q.reshape(1, R, C).to(gpu), eps=eps.reshape(1, 1, A).to(gpu)):
        if first:
            out = d.act_step(frame, deterministic=deterministic)
        else:
            out = d.act_step(frame, *(t.to(gpu) for t in state), deterministic=deterministic)
    d.act_check()
    return tuple(cpu(t) for t in out)


def _batch(d, gpu, frames, state, first, q, eps, deterministic=False):
    from dreamer_amd import hip
    N = len(frames)
    with hip.noise_override(q=q.reshape(1, N * R, C).to(gpu), eps=eps.reshape(1, N, A).to(gpu)):
        out = d.act_step_batch(frames, None if state is None else tuple(t.to(gpu) for t in state), first,
                               deterministic=deterministic)
    d.act_check()
    return tuple(cpu(t) for t in out)


def _rows(q, e):
    return q[e * R:(e + 1) * R]


def test_act_batch_matches_oracle(fused, gpu):
    """N = 5 rows over 4 env steps against the CPU oracle run per row
    (O.encode at an episode start, else O.observe_step, then O.actor_act),
    fresh tie-guarded q / eps per step.  Step 0 is all first; at step 2 rows
    1 and 3 start a new episode and are handed a deliberately stale (NaN)
    state, rows 0, 2 and 4 continue."""
    d, P = fused
    N, n_steps = 5, 4
    g = torch.Generator().manual_seed(71)
    st_o = [None] * N  # per row (z, h, a)
    st_f = None
    guarded = 0
    with torch.no_grad():
        for k in range(n_steps):
            frames = torch.randint(0, 256, (N, 64, 64, 3), generator=g, dtype=torch.uint8).numpy()
            q = torch.empty(N * R, C).exponential_(generator=g)
            eps = torch.randn(N, A, generator=g)
            first = np.ones(N, dtype=bool) if k == 0 else np.isin(np.arange(N), [1, 3]) & (k == 2)
            ref = []
            for e in range(N):
                obs = torch.tensor(frames[e].transpose(2, 0, 1), dtype=torch.float32).view(1, 1, 3, 64, 64) / 255.0 - 0.5
                with TieGuard() as tg:  # widens near-tie margins in q (in place)
                    if first[e]:
                        h_o = torch.zeros(1, 1, HD)
                        z_o, _ = O.encode(h_o, obs, P, _rows(q, e), R, C)
                    else:
                        z_o, h_o, _ = O.observe_step(*st_o[e], obs, P, _rows(q, e), R, C)
                guarded += tg.guarded
                a_o, mu_o, sg_o = O.actor_act(h_o, z_o, P, eps[e].view(1, 1, A))
                st_o[e] = (z_o, h_o, a_o)
                ref.append((a_o, mu_o, sg_o, z_o, h_o))
            if st_f is not None and first.any():  # stale rows: nothing of them may reach a result
                st_f = tuple(t.clone() for t in st_f)
                for t in st_f:
                    t[torch.from_numpy(first)] = float("nan")
            a_f, mu_f, sg_f, z_f, h_f = _batch(d, gpu, frames, st_f, first if k else None, q, eps)
            st_f = (z_f, h_f, a_f)
            for e in range(N):
                a_o, mu_o, sg_o, z_o, h_o = ref[e]
                zi_f, zi_o = _idx(z_f[e]), z_o.reshape(-1, C).argmax(-1)
                assert torch.equal(zi_f, zi_o), f"step {k} row {e}: {int((zi_f != zi_o).sum())} latent groups differ"
                close(h_f[e], h_o.reshape(h_f[e].shape), 1e-4, 1e-6, f"h' step {k} row {e}")
                close(z_f[e], z_o.reshape(z_f[e].shape), 0, 1e-6, f"latent values step {k} row {e}")
                close(mu_f[e], mu_o.reshape(mu_f[e].shape), 1e-4, 1e-6, f"mu step {k} row {e}")
                close(sg_f[e], sg_o.reshape(sg_f[e].shape), 1e-4, 1e-6, f"sigma step {k} row {e}")
                close(a_f[e], a_o.reshape(a_f[e].shape), 1e-4, 1e-6, f"action step {k} row {e}")
    assert int(d._act_batch_bufs[N]["status"].item()) == 0
    print(f"act_step_batch vs oracle: {N} rows x {n_steps} env steps, {guarded} tie-guarded groups")


@pytest.mark.parametrize("first", [True, False], ids=["first", "continuing"])
def test_act_batch_row_independence_bitwise(fused, gpu, first):
    """Row 3 of an N = 5 call, row 0 of an N = 1 call, row 15 of an N = 16
    call (where the sampler stage has exactly as many tasks as waves) and
    act_step on the same frame, state and noise rows: the same bits."""
    d, _ = fused
    frames5, state5, q5, eps5 = _case(5, seed=5)
    frames16, state16, q16, eps16 = _case(16, seed=16)
    e = 3
    frames16[15] = frames5[e]
    for t16, t5 in zip(state16, state5):
        t16[15] = t5[e]
    _rows(q16, 15)[...] = _rows(q5, e)
    eps16[15] = eps5[e]
    row_state = tuple(t[e:e + 1] for t in state5)
    with torch.no_grad():
        ref = _single(d, gpu, frames5[e], row_state, first, _rows(q5, e), eps5[e])
        f5 = np.full(5, first)
        out5 = _batch(d, gpu, frames5, None if first else state5, f5, q5, eps5)
        out1 = _batch(d, gpu, frames5[e:e + 1], None if first else row_state, np.full(1, first), _rows(q5, e),
                      eps5[e:e + 1])
        # in the N = 16 call the other rows do the opposite of the row under test
        f16 = np.full(16, not first)
        f16[15] = first
        out16 = _batch(d, gpu, frames16, state16, f16, q16, eps16)
    for name, r, o5, o1, o16 in zip(NAMES, ref, out5, out1, out16):
        assert bool(torch.isfinite(r).all()), name
        assert torch.equal(o5[e], r[0]), f"{name}: row 3 of N = 5 differs from act_step"
        assert torch.equal(o1[0], r[0]), f"{name}: row 0 of N = 1 differs from act_step"
        assert torch.equal(o16[15], r[0]), f"{name}: row 15 of N = 16 differs from act_step"


@pytest.mark.parametrize("N", [2, 16])
def test_act_batch_edge_sizes_bitwise(fused, gpu, N):
    """N = 2 and N = 16 (the cap), a mix of starting and continuing rows:
    every row equals act_step bit for bit."""
    d, _ = fused
    frames, state, q, eps = _case(N, seed=100 + N)
    first = (np.arange(N) % 3) == 1
    with torch.no_grad():
        out = _batch(d, gpu, frames, state, first, q, eps)
        for e in range(N):
            ref = _single(d, gpu, frames[e], tuple(t[e:e + 1] for t in state), bool(first[e]), _rows(q, e), eps[e])
            for name, r, o in zip(NAMES, ref, out):
                assert torch.equal(o[e], r[0]), f"N = {N}, row {e}, {name}"
    assert int(d._act_batch_bufs[N]["status"].item()) == 0


def _assert_rows_match_act_step(d, gpu, out, frames, state, first, q, eps):
    """Two different paths: indices exact, values at 1e-5 / 1e-6
    (test_act_step_matches_unfused's bounds between those two paths)."""
    for e in range(len(frames)):
        a_r, mu_r, sg_r, z_r, h_r = _single(d, gpu, frames[e], tuple(t[e:e + 1] for t in state), bool(first[e]),
                                            _rows(q, e), eps[e])
        a_b, mu_b, sg_b, z_b, h_b = (t[e:e + 1] for t in out)
        assert torch.equal(_idx(z_b), _idx(z_r)), f"row {e}: latent groups differ"
        close(z_b, z_r, 0, 1e-6, f"latent values row {e}")
        close(h_b, h_r, 1e-5, 1e-6, f"h' row {e}")
        close(mu_b, mu_r, 1e-5, 1e-6, f"mu row {e}")
        close(sg_b, sg_r, 1e-5, 1e-6, f"sigma row {e}")
        close(a_b, a_r, 1e-5, 1e-6, f"action row {e}")


def test_act_batch_above_cap_runs_unfused(fused, gpu):
    """N = 17 is above DR_ACT_MAX_ENVS: the entry point answers
    DR_E_UNSUPPORTED (DR_E_INVALID for n_env < 1), and act_step_batch takes
    the batched unfused launches without raising, matching per-row act_step."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    d, _ = fused
    dims = d.world_model.dims(d.agent)
    buf = torch.zeros(64, device=gpu)
    for n_env, code in ((L.DR_ACT_MAX_ENVS + 1, L.DR_E_UNSUPPORTED), (0, L.DR_E_INVALID)):
        with pytest.raises(L.HipError) as ei:  # rejected before any pointer is used
            L.call("dr_act_batch", dims, d.world_model.packed(), d.agent.actor_struct(), n_env, *([L.ptr(buf)] * 5),
                   hip.explicit_noise(device=gpu), 0, *([L.ptr(buf)] * 5), None, None, L.ptr(buf), 256, hip.stream())
        assert ei.value.code == code
    N = 17
    assert d._act_batch_route(N) == "unfused"
    frames, state, q, eps = _case(N, seed=17)
    first = (np.arange(N) % 4) == 2
    with torch.no_grad():
        out = _batch(d, gpu, frames, state, first, q, eps)
        assert N not in getattr(d, "_act_batch_bufs", {})  # no fused launch was prepared
        _assert_rows_match_act_step(d, gpu, out, frames, state, first, q, eps)


def test_act_batch_noise_keys(fused, gpu):
    """Sixteen identical rows.  Deterministic with the same explicit q in every
    row: all rows bitwise equal.  Philox noise, sampling: row e is keyed row0 +
    e, so neither the sixteen actions nor the sixteen latent index vectors
    are all equal."""
    d, _ = fused
    frames, _, q, eps = _case(1, seed=4)
    frames16 = np.repeat(frames, 16, axis=0)
    with torch.no_grad():
        out = _batch(d, gpu, frames16, None, None, q.repeat(16, 1), eps.repeat(16, 1), deterministic=True)
        for name, t in zip(NAMES, out):
            assert bool(torch.isfinite(t).all()), name
            assert all(torch.equal(t[e], t[0]) for e in range(1, 16)), f"{name}: identical rows differ"
        a, _, _, z, _ = d.act_step_batch(frames16, deterministic=False)
        d.act_check()
    zi = _idx(z).reshape(16, R)
    assert not all(torch.equal(zi[e], zi[0]) for e in range(1, 16)), "every row drew the same latent"
    assert not all(torch.equal(cpu(a)[e], cpu(a)[0]) for e in range(1, 16)), "every row drew the same action"


def test_act_batch_failure_paths(gpu, monkeypatch):
    """DREAMER_ACT_FORCE on the batched entry point.  =timeout: every output
    of every row is NaN, act_check() raises, and the next call without the
    variable is finite with status 0.  =nonresident: DR_E_UNSUPPORTED, the
    call lands on the unfused path and matches per-row act_step."""
    d, _ = _dreamer(gpu)
    d.act_batch_path = "fused"
    N = 3
    frames, state, q, eps = _case(N, seed=44)
    first = np.array([False, True, False])
    with torch.no_grad():
        monkeypatch.setenv("DREAMER_ACT_FORCE", "timeout")
        out = d.act_step_batch(frames, tuple(t.to(gpu) for t in state), first)
        with pytest.raises(RuntimeError, match="grid barrier timed out"):
            d.act_check()
        for name, t in zip(NAMES, out):
            assert tuple(t.shape)[:2] == (N, 1)
            assert bool(torch.isnan(t).all()), f"{name} must be NaN in every row after a barrier timeout"
        monkeypatch.delenv("DREAMER_ACT_FORCE")
        out = d.act_step_batch(frames, tuple(t.to(gpu) for t in state), first)
        d.act_check()
        assert all(bool(torch.isfinite(t).all()) for t in out)
        assert int(d._act_batch_bufs[N]["status"].item()) == 0
        assert not getattr(d, "_act_batch_unsupported", False)
        ref_rows = [_single(d, gpu, frames[e], tuple(t[e:e + 1] for t in state), bool(first[e]), _rows(q, e), eps[e])
                    for e in range(N)]
        monkeypatch.setenv("DREAMER_ACT_FORCE", "nonresident")
        out = _batch(d, gpu, frames, state, first, q, eps)
        assert getattr(d, "_act_batch_unsupported", False), "DR_E_UNSUPPORTED must switch to the unfused path"
        assert d._act_batch_route(N) == "unfused"
        monkeypatch.delenv("DREAMER_ACT_FORCE")
    for e in range(N):
        a_r, mu_r, sg_r, z_r, h_r = ref_rows[e]
        a_b, mu_b, sg_b, z_b, h_b = (t[e:e + 1] for t in out)
        assert torch.equal(_idx(z_b), _idx(z_r)), f"row {e}: latent groups differ"
        close(z_b, z_r, 0, 1e-6, f"latent values row {e}")
        for name, x, y in (("h'", h_b, h_r), ("mu", mu_b, mu_r), ("sigma", sg_b, sg_r), ("action", a_b, a_r)):
            close(x, y, 1e-5, 1e-6, f"{name} row {e}")


class _Space:
    def __init__(self, rng):
        self.rng = rng

    def sample(self):
        return self.rng.uniform(-1, 1, size=3).astype(np.float32)


class SeededEnv:
    """gymnasium-shaped env whose episode is a function of the reset seed:
    the frames (seed, t) and the length (3 ... 9 steps).  Reward tanh(sum(a)).
    Records the seeds it was reset with and each episode's total reward;
    `replay` makes a clone take a recorded seed list instead of the caller's."""

    def __init__(self, space_seed=0, replay=None):
        self.action_space = _Space(np.random.default_rng(space_seed))
        self.replay = None if replay is None else list(replay)
        self.seeds, self.totals = [], {}

    def _obs(self):
        return np.random.default_rng([self.ep_seed, self.t]).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)

    def reset(self, seed=None):
        if self.replay is not None:
            seed = self.replay.pop(0)
        self.seeds.append(seed)
        self.ep_seed, self.t, self.length = seed, 0, 3 + seed % 7
        self.totals[seed] = 0
        return self._obs(), {}

    def step(self, action):
        a = np.asarray(action, dtype=np.float32)
        assert a.shape == (3,) and np.all(np.isfinite(a)) and np.all(np.abs(a) <= 1.0)
        self.t += 1
        reward = float(np.tanh(a.sum()))
        self.totals[self.ep_seed] += reward
        return self._obs(), reward, self.t >= self.length, False, {}


def test_evaluate_agent_vec(fused, gpu):
    """5 deterministic episodes over 3 envs == evaluate_agent on one env from
    the same starting seed: the same per-episode totals (the rows are the
    bits act_step gives), the same mean, self.seed advanced by 5 in both.
    The actor is deterministic but the latent is still sampled, so both runs
    read the same explicit Exp(1) variates in every row and step (Philox
    would key each call differently)."""
    from dreamer_amd import hip
    d, _ = fused
    seed0 = 40
    q = torch.empty(R, C).exponential_(generator=torch.Generator().manual_seed(6)).repeat(3, 1).to(gpu)
    envs = [SeededEnv(), SeededEnv(), SeededEnv()]
    d.seed = seed0
    with hip.noise_override(q=q):
        mean_vec = d.evaluate_agent_vec(envs, eval_episodes=5)
    assert d.seed == seed0 + 5
    one = SeededEnv()
    d.seed = seed0
    with hip.noise_override(q=q):
        mean_one = d.evaluate_agent(one, eval_episodes=5)
    assert d.seed == seed0 + 5
    got = {}
    for env in envs:
        got.update(env.totals)
    assert sorted(got) == sorted(one.totals) == list(range(seed0 + 1, seed0 + 6))
    assert [env.seeds[0] for env in envs] == [seed0 + 1, seed0 + 2, seed0 + 3]  # the first three start together
    assert sorted(got.values()) == sorted(one.totals.values())
    assert got == one.totals
    assert mean_vec.is_cuda and float(mean_vec) == float(mean_one)


def test_rollout_policy_vec(gpu):
    """3 envs, sequence_length 8, two calls with the random policy: the ring
    holds six blocks of 8 in call-major then env-major order, each identical
    to what rollout_policy writes for a clone of that env given the same reset
    seeds.  With the actor's policy the run is finite and fills 48 slots."""
    S, N = 8, 3
    d, _ = _dreamer(gpu, sequence_length=S, buffer_size=128)
    seed0 = d.seed
    envs = [SeededEnv(space_seed=10 + e) for e in range(N)]
    d.rollout_policy_vec(envs, random_policy=True)
    d.rollout_policy_vec(envs, random_policy=True)
    d.act_check()
    buf = d.buffer
    assert buf.size == 2 * N * S and buf.next_idx == 2 * N * S
    assert [env.seeds[0] for env in envs] == [seed0 + e for e in range(N)]
    n_resets = sum(len(env.seeds) for env in envs)
    assert n_resets > N and d.seed == seed0 + n_resets - 1  # some episode ended (lengths 3 ... 9 over 16 steps)
    ring = [x[:2 * N * S].copy() for x in (buf.observation_buffer, buf.action_buffer, buf.reward_buffer,
                                           buf.continue_buffer)]
    for e in range(N):
        clone = SeededEnv(space_seed=10 + e, replay=envs[e].seeds)
        d.agent_obs = None
        buf.next_idx = buf.size = 0
        d.rollout_policy(clone, random_policy=True)
        d.rollout_policy(clone, random_policy=True)
        assert clone.seeds == envs[e].seeds
        for call in range(2):
            lo = call * N * S + e * S
            for name, vec, one in zip(("observations", "actions", "symlog rewards", "continues"), ring,
                                      (buf.observation_buffer, buf.action_buffer, buf.reward_buffer,
                                       buf.continue_buffer)):
                assert np.array_equal(vec[lo:lo + S], one[call * S:(call + 1) * S]), f"env {e} call {call}: {name}"
    # the actor's policy
    d2, _ = _dreamer(gpu, sequence_length=S, buffer_size=128)
    envs = [SeededEnv(space_seed=20 + e) for e in range(N)]
    d2.rollout_policy_vec(envs, random_policy=False)
    d2.rollout_policy_vec(envs, random_policy=False)
    d2.act_check()
    assert d2.buffer.size == 48
    assert np.isfinite(d2.buffer.action_buffer[:48]).all() and np.isfinite(d2.buffer.reward_buffer[:48]).all()
    assert np.abs(d2.buffer.action_buffer[:48]).max() <= 1.0
    assert all(bool(torch.isfinite(t).all()) for t in (d2.vec_latent, d2.vec_hidden))


def test_train_dreamer_with_env_lists(gpu, tmp_path, monkeypatch):
    """train_dreamer([env, env2], [eval_env, eval_env2]) end to end with tiny
    iteration counts (settings as test_train_dreamer_with_fake_env): finite
    losses and evaluations, two blocks of sequence_length per rollout."""
    monkeypatch.chdir(tmp_path)
    d, _ = _dreamer(gpu, batch_size=4, sequence_length=16, horizon=5, buffer_size=256, random_iterations=2,
                    training_iterations=2, AC_epochs=2)
    envs = [SeededEnv(space_seed=1), SeededEnv(space_seed=2)]
    eval_envs = [SeededEnv(space_seed=3), SeededEnv(space_seed=4)]
    wm, al, cl, ev = d.train_dreamer(envs, eval_envs)
    assert len(wm) == 2 + 2 and len(al) == 2 and len(cl) == 2 and len(ev) == 1 + 1 + 1
    for x in [v for row in wm for v in row] + al + cl + ev:
        assert np.isfinite(x)
    assert d.buffer.size == (2 + 2) * 16 * 2
    assert all(len(env.seeds) >= 1 for env in envs + eval_envs)


def test_act_batch_timing(gpu):
    """Prints the table the dispatch follows: per env
    step of N environments, H2D of the frames included, (a) the one-launch
    dr_act_batch, (b) the batched unfused launches, (c) N act_step calls;
    three repetitions of 50 steps each after a warm-up.  The committed
    dispatch sets must be consistent with the entry point's cap."""
    from dreamer_amd import _lib as L
    d, _ = _dreamer(gpu)
    assert d.ACT_BATCH_FUSED_N <= set(range(1, L.DR_ACT_MAX_ENVS + 1))
    assert not (d.ACT_BATCH_FUSED_N & d.ACT_BATCH_SEQUENTIAL_N)

    def per_step(fn, n=50):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    print("act_step_batch, us per step of N envs (min / max of 3 x 50 steps): fused | unfused | N x act_step")
    with torch.no_grad():
        for N in (1, 2, 4, 8, 16):
            frames, state, _, _ = _case(N, seed=N)
            state = tuple(t.to(gpu) for t in state)
            first = np.zeros(N, dtype=bool)
            row = []
            for path in ("fused", "unfused", "sequential"):
                d.act_batch_path = path
                ts = [per_step(lambda: d.act_step_batch(frames, state, first, deterministic=True)) for _ in range(3)]
                row.append(ts)
                assert all(np.isfinite(t) and t > 0 for t in ts)
            d.act_check()
            print(f"  N = {N:2d}: " + " | ".join(f"{min(ts):8.1f} / {max(ts):8.1f}" for ts in row)
                  + f"   dispatch: {'fused' if N in d.ACT_BATCH_FUSED_N else 'other'}")
    d.act_batch_path = None
