"""One-launch acting for vector observations: dr_act_vec (1 ... 16 rows in
one launch; act_step is its N = 1 call) and the Dreamer methods on top of it.

Weights are the default init under torch.manual_seed(0) at the FULL widths
plus observation_dims = [D], as in test_gpu_vector.py; the oracle side is
O.encode / O.observe_step / O.actor_act on (1, 1, D) observations (the vector
branch of oracle.encoder_logits).  The kernel's contract is row independence:
a row's outputs are the same bits for every n_env, row position and mix of
first flags, so the kernel tests compare rows with ``torch.equal`` against
Dreamer.act_step.  Every test that is about the kernel pins the one-launch
path with ``act_batch_path = "fused"`` and asserts that the per-N buffers of
a fused launch exist (the default dispatch follows the timing table,
DESIGN.md section 5b).  Against the oracle the bounds are
test_act_batch_matches_oracle's: latent indices exact (inputs tie-guarded),
|d| <= 1e-6 + 1e-4 |ref| on h', mu, sigma and the action, 1e-6 on the
straight-through latent values; between the fused and the unfused path
1e-6 + 1e-5 |ref| (test_gpu_act_batch._assert_rows_match_act_step's)."""
import time

import numpy as np
import pytest
import torch

from baseline_case import TieGuard
from formula import FULL
from gpu_helpers import close, cpu
from oracle import dreamer_oracle as O
from test_gpu_act_batch import SeededEnv

pytestmark = pytest.mark.gpu
R, C, A, HD = 32, 32, 3, 600
D_BENCH = 24  # bench.py's VEC_OBS_DIM
NAMES = ("a", "mu", "sigma", "z", "h")


def _dreamer(dev, D=D_BENCH, **over):
    from dreamer_amd import Dreamer
    cfg = dict(FULL)
    cfg.update(observation_dims=[D], **over)
    torch.manual_seed(0)
    return Dreamer(cfg, dev)


@pytest.fixture(scope="module")
def fused(gpu):
    """Dreamers by observation dim (built once each), pinned to the one-launch path."""
    made = {}

    def get(D=D_BENCH):
        if D not in made:
            d = _dreamer(gpu, D)
            d.act_batch_path = "fused"
            made[D] = (d, {k: v.detach().cpu().clone() for k, v in d.state_dict().items()})
        return made[D]
    return get


def _idx(z):
    return cpu(z).reshape(-1, C).argmax(-1)


def _case(N, seed, D=D_BENCH):
    """Observations, a random previous state and explicit noise for N rows."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(N, D, generator=g).numpy()
    z = torch.nn.functional.one_hot((torch.randn(N, 1, R, C, generator=g) * 2).argmax(-1), C).float()
    h = torch.randn(N, 1, HD, generator=g)
    a = torch.rand(N, 1, A, generator=g) * 2 - 1
    q = torch.empty(N * R, C).exponential_(generator=g)
    eps = torch.randn(N, A, generator=g)
    return obs, (z, h, a), q, eps


def _single(d, gpu, obs, state, first, q, eps, deterministic=False):
    """Dreamer.act_step on one row with that row's noise."""
    from dreamer_amd import hip
    with hip.noise_override(q=q.reshape(1, R, C).to(gpu), eps=eps.reshape(1, 1, A).to(gpu)):
        if first:
            out = d.act_step(obs, deterministic=deterministic)
        else:
            out = d.act_step(obs, *(t.to(gpu) for t in state), deterministic=deterministic)
    d.act_check()
    return tuple(cpu(t) for t in out)


def _batch(d, gpu, obs, state, first, q, eps, deterministic=False):
    from dreamer_amd import hip
    N = len(obs)
    with hip.noise_override(q=q.reshape(1, N * R, C).to(gpu), eps=eps.reshape(1, N, A).to(gpu)):
        out = d.act_step_batch(obs, None if state is None else tuple(t.to(gpu) for t in state), first,
                               deterministic=deterministic)
    d.act_check()
    return tuple(cpu(t) for t in out)


def _rows(q, e):
    return q[e * R:(e + 1) * R]


def _fused_ran(d, N):
    """The per-N buffers of a dr_act_vec launch exist and its status word is 0."""
    bufs = getattr(d, "_act_vec_bufs", {})
    assert N in bufs, f"no fused dr_act_vec launch was prepared for N = {N}"
    assert int(bufs[N]["status"].item()) == 0
    assert not getattr(d, "_act_vec_unsupported", False)


def _assert_rows_close(out, ref, what):
    """Two different paths (fused / unfused): indices exact, 1e-6 on the latent
    values, 1e-6 + 1e-5 |ref| on h', mu, sigma and the action."""
    a_b, mu_b, sg_b, z_b, h_b = out
    a_r, mu_r, sg_r, z_r, h_r = ref
    assert torch.equal(_idx(z_b), _idx(z_r)), f"{what}: latent groups differ"
    close(z_b, z_r, 0, 1e-6, f"{what}: latent values")
    close(h_b, h_r, 1e-5, 1e-6, f"{what}: h'")
    close(mu_b, mu_r, 1e-5, 1e-6, f"{what}: mu")
    close(sg_b, sg_r, 1e-5, 1e-6, f"{what}: sigma")
    close(a_b, a_r, 1e-5, 1e-6, f"{what}: action")


@pytest.mark.parametrize("D", [24, 67, 300])
def test_act_vec_matches_oracle(fused, gpu, D):
    """N = 5 rows over 4 env steps against the CPU oracle run per row, fresh
    tie-guarded q / eps per step.  Step 0 is all first; at step 2 rows 1 and 3
    start a new episode and are handed a NaN state, rows 0, 2 and 4 continue.
    D = 24 is the bench's width, 67 is no multiple of 4 and crosses one
    64-lane boundary, 300 takes more than one pass of the 4 x 64 register
    batch of encoder layer 0."""
    d, P = fused(D)
    N, n_steps = 5, 4
    g = torch.Generator().manual_seed(71 + D)
    st_o = [None] * N  # per row (z, h, a)
    st_f = None
    guarded = 0
    with torch.no_grad():
        for k in range(n_steps):
            obs = torch.randn(N, D, generator=g)
            q = torch.empty(N * R, C).exponential_(generator=g)
            eps = torch.randn(N, A, generator=g)
            first = np.ones(N, dtype=bool) if k == 0 else np.isin(np.arange(N), [1, 3]) & (k == 2)
            ref = []
            for e in range(N):
                ob = obs[e].view(1, 1, D)
                with TieGuard() as tg:  # widens near-tie margins in q (in place)
                    if first[e]:
                        h_o = torch.zeros(1, 1, HD)
                        z_o, _ = O.encode(h_o, ob, P, _rows(q, e), R, C)
                    else:
                        z_o, h_o, _ = O.observe_step(*st_o[e], ob, P, _rows(q, e), R, C)
                guarded += tg.guarded
                a_o, mu_o, sg_o = O.actor_act(h_o, z_o, P, eps[e].view(1, 1, A))
                st_o[e] = (z_o, h_o, a_o)
                ref.append((a_o, mu_o, sg_o, z_o, h_o))
            if st_f is not None and first.any():  # stale rows: nothing of them may reach a result
                st_f = tuple(t.clone() for t in st_f)
                for t in st_f:
                    t[torch.from_numpy(first)] = float("nan")
            a_f, mu_f, sg_f, z_f, h_f = _batch(d, gpu, obs.numpy(), st_f, first if k else None, q, eps)
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
    _fused_ran(d, N)
    print(f"dr_act_vec vs oracle, D = {D}: {N} rows x {n_steps} env steps, {guarded} tie-guarded groups")


@pytest.mark.parametrize("first", [True, False], ids=["first", "continuing"])
def test_act_vec_row_independence_bitwise(fused, gpu, first):
    """Row 3 of an N = 5 call, row 0 of an N = 1 call, row 15 of an N = 16
    call whose other rows carry the opposite flag, and act_step on the same
    observation, state and noise rows: the same bits."""
    d, _ = fused()
    obs5, state5, q5, eps5 = _case(5, seed=5)
    obs16, state16, q16, eps16 = _case(16, seed=16)
    e = 3
    obs16[15] = obs5[e]
    for t16, t5 in zip(state16, state5):
        t16[15] = t5[e]
    _rows(q16, 15)[...] = _rows(q5, e)
    eps16[15] = eps5[e]
    row_state = tuple(t[e:e + 1] for t in state5)
    with torch.no_grad():
        ref = _single(d, gpu, obs5[e], row_state, first, _rows(q5, e), eps5[e])
        out5 = _batch(d, gpu, obs5, None if first else state5, np.full(5, first), q5, eps5)
        out1 = _batch(d, gpu, obs5[e:e + 1], None if first else row_state, np.full(1, first), _rows(q5, e),
                      eps5[e:e + 1])
        f16 = np.full(16, not first)
        f16[15] = first
        out16 = _batch(d, gpu, obs16, state16, f16, q16, eps16)
    for N in (1, 5, 16):
        _fused_ran(d, N)
    for name, r, o5, o1, o16 in zip(NAMES, ref, out5, out1, out16):
        assert bool(torch.isfinite(r).all()), name
        assert torch.equal(o5[e], r[0]), f"{name}: row 3 of N = 5 differs from act_step"
        assert torch.equal(o1[0], r[0]), f"{name}: row 0 of N = 1 differs from act_step"
        assert torch.equal(o16[15], r[0]), f"{name}: row 15 of N = 16 differs from act_step"


@pytest.mark.parametrize("N", [2, 3, 8, 9, 16])
def test_act_vec_edge_sizes_bitwise(fused, gpu, N):
    """A mix of starting and continuing rows at N = 2, 3 (no power of two), 8,
    9 (two GRU chunks, an uneven 5 + 4 split over the grid halves) and 16
    (the cap): every row equals act_step bit for bit."""
    d, _ = fused()
    obs, state, q, eps = _case(N, seed=100 + N)
    first = (np.arange(N) % 3) == 1
    with torch.no_grad():
        out = _batch(d, gpu, obs, state, first, q, eps)
        for e in range(N):
            ref = _single(d, gpu, obs[e], tuple(t[e:e + 1] for t in state), bool(first[e]), _rows(q, e), eps[e])
            for name, r, o in zip(NAMES, ref, out):
                assert torch.equal(o[e], r[0]), f"N = {N}, row {e}, {name}"
    _fused_ran(d, N)


def test_act_vec_matches_unfused(fused, gpu):
    """The same N = 6 case through the one launch and through the batched
    unfused launches (act_batch_path = "unfused")."""
    d, _ = fused()
    N = 6
    obs, state, q, eps = _case(N, seed=6)
    first = (np.arange(N) % 3) == 1
    with torch.no_grad():
        out_f = _batch(d, gpu, obs, state, first, q, eps)
        _fused_ran(d, N)
        d.act_batch_path = "unfused"
        try:
            assert d._act_batch_route(N) == "unfused"
            out_u = _batch(d, gpu, obs, state, first, q, eps)
        finally:
            d.act_batch_path = "fused"
    for e in range(N):
        _assert_rows_close(tuple(t[e:e + 1] for t in out_u), tuple(t[e:e + 1] for t in out_f), f"row {e}")


def test_act_vec_noise_keys(fused, gpu):
    """Sixteen identical rows.  Deterministic with the same explicit q in every
    row: all rows bitwise equal.  Philox noise, sampling: row e is keyed row0 +
    e, so neither the sixteen actions nor the sixteen latent index vectors
    are all equal."""
    d, _ = fused()
    obs, _, q, eps = _case(1, seed=4)
    obs16 = np.repeat(obs, 16, axis=0)
    with torch.no_grad():
        out = _batch(d, gpu, obs16, None, None, q.repeat(16, 1), eps.repeat(16, 1), deterministic=True)
        for name, t in zip(NAMES, out):
            assert bool(torch.isfinite(t).all()), name
            assert all(torch.equal(t[e], t[0]) for e in range(1, 16)), f"{name}: identical rows differ"
        a, _, _, z, _ = d.act_step_batch(obs16, deterministic=False)
        d.act_check()
    _fused_ran(d, 16)
    zi = _idx(z).reshape(16, R)
    assert not all(torch.equal(zi[e], zi[0]) for e in range(1, 16)), "every row drew the same latent"
    assert not all(torch.equal(cpu(a)[e], cpu(a)[0]) for e in range(1, 16)), "every row drew the same action"


def test_act_vec_abi_edges(fused, gpu):
    """Calls the entry point rejects before any pointer is used, and what the
    host does with them: n_env = 0 (invalid), 17 (unsupported), pixel dims
    (invalid), obs_dim above the cap (unsupported; a Dreamer of that width
    acts through the unfused launches without raising); dr_act_batch on
    vector dims stays unsupported; N = 17 through act_step_batch runs unfused
    and matches per-row act_step."""
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    d, _ = fused()
    buf = torch.zeros(64, device=gpu)

    def rejects(entry, dims, n_env, code):
        with pytest.raises(L.HipError) as ei:
            L.call(entry, dims, d.world_model.packed(), d.agent.actor_struct(), n_env, *([L.ptr(buf)] * 5),
                   hip.explicit_noise(device=gpu), 0, *([L.ptr(buf)] * 5), None, None, L.ptr(buf), 256, hip.stream())
        assert ei.value.code == code, (entry, n_env, ei.value.code)

    dims = d.world_model.dims(d.agent)
    rejects("dr_act_vec", dims, 0, L.DR_E_INVALID)
    rejects("dr_act_vec", dims, L.DR_ACT_MAX_ENVS + 1, L.DR_E_UNSUPPORTED)
    rejects("dr_act_batch", dims, 2, L.DR_E_UNSUPPORTED)
    pixel = d.world_model.dims(d.agent)
    pixel.obs_dim, pixel.img_h, pixel.img_w, pixel.enc_depth = 0, 64, 64, 4
    rejects("dr_act_vec", pixel, 2, L.DR_E_INVALID)
    wide = d.world_model.dims(d.agent)
    wide.obs_dim = L.DR_ACT_VEC_MAX_OBS + 1
    rejects("dr_act_vec", wide, 2, L.DR_E_UNSUPPORTED)
    assert L.DR_ACT_VEC_MAX_OBS >= 512

    # a model above the observation cap: the one launch is tried once, then every step stays unfused
    dw = _dreamer(gpu, L.DR_ACT_VEC_MAX_OBS + 1)
    obs = np.random.default_rng(3).standard_normal((2, L.DR_ACT_VEC_MAX_OBS + 1)).astype(np.float32)
    with torch.no_grad():
        dw.act_batch_path = "fused"
        a, mu, sg, z, h = dw.act_step(obs[0])
        assert getattr(dw, "_act_vec_unsupported", False) and dw._act_batch_route(1) == "unfused"
        a2 = dw.act_step(obs[1], z, h, a)[0]
        ab = dw.act_step_batch(obs)[0]
        dw.act_check()
    assert not getattr(dw, "_act_vec_bufs", {})
    for t in (a, a2, ab):
        assert bool(torch.isfinite(t).all()) and bool((cpu(t).abs() <= 1).all())

    N = 17
    assert d._act_batch_route(N) == "unfused"
    obs, state, q, eps = _case(N, seed=17)
    first = (np.arange(N) % 4) == 2
    with torch.no_grad():
        out = _batch(d, gpu, obs, state, first, q, eps)
        assert N not in getattr(d, "_act_vec_bufs", {})  # no fused launch was prepared
        for e in range(N):
            ref = _single(d, gpu, obs[e], tuple(t[e:e + 1] for t in state), bool(first[e]), _rows(q, e), eps[e])
            _assert_rows_close(tuple(t[e:e + 1] for t in out), ref, f"N = 17 row {e}")


def test_act_vec_failure_paths(gpu, monkeypatch):
    """DREAMER_ACT_FORCE on dr_act_vec, N = 3.  =timeout (spin limit 0: every
    workgroup leaves through the bounded spin): every output of every row is
    NaN, act_check() raises and names dr_act_vec, and the next call without
    the variable is finite with status 0.  =nonresident: DR_E_UNSUPPORTED, the
    call lands on the unfused path and matches the fused rows."""
    d = _dreamer(gpu)
    d.act_batch_path = "fused"
    N = 3
    obs, state, q, eps = _case(N, seed=44)
    first = np.array([False, True, False])
    with torch.no_grad():
        monkeypatch.setenv("DREAMER_ACT_FORCE", "timeout")
        out = d.act_step_batch(obs, tuple(t.to(gpu) for t in state), first)
        with pytest.raises(RuntimeError, match="dr_act_vec: a grid barrier timed out"):
            d.act_check()
        for name, t in zip(NAMES, out):
            assert tuple(t.shape)[:2] == (N, 1)
            assert bool(torch.isnan(t).all()), f"{name} must be NaN in every row after a barrier timeout"
        monkeypatch.delenv("DREAMER_ACT_FORCE")
        out = d.act_step_batch(obs, tuple(t.to(gpu) for t in state), first)
        d.act_check()
        assert all(bool(torch.isfinite(t).all()) for t in out)
        _fused_ran(d, N)
        ref = _batch(d, gpu, obs, state, first, q, eps)
        monkeypatch.setenv("DREAMER_ACT_FORCE", "nonresident")
        out = _batch(d, gpu, obs, state, first, q, eps)
        assert getattr(d, "_act_vec_unsupported", False), "DR_E_UNSUPPORTED must switch to the unfused path"
        assert d._act_batch_route(N) == "unfused" and d._act_batch_route(1) == "unfused"
        monkeypatch.delenv("DREAMER_ACT_FORCE")
    for e in range(N):
        _assert_rows_close(tuple(t[e:e + 1] for t in out), tuple(t[e:e + 1] for t in ref), f"row {e}")


class SeededVecEnv(SeededEnv):
    """SeededEnv's scheme with vector observations: D floats, a function of (seed, t)."""

    def _obs(self):
        return np.random.default_rng([self.ep_seed, self.t]).standard_normal(D_BENCH).astype(np.float32)


def test_act_vec_methods_on_top(fused, gpu):
    """evaluate_agent_vec over 3 envs, 5 deterministic episodes and a shared
    explicit q == evaluate_agent on one env from the same starting seed: the
    same per-episode totals and mean, bitwise (the rows are the bits act_step
    gives).  rollout_policy_vec with the actor's policy fills 2 N S slots with
    finite actions in [-1, 1]."""
    from dreamer_amd import hip
    d, _ = fused()
    seed0 = 40
    q = torch.empty(R, C).exponential_(generator=torch.Generator().manual_seed(6)).repeat(3, 1).to(gpu)
    envs = [SeededVecEnv(), SeededVecEnv(), SeededVecEnv()]
    d.seed = seed0
    with hip.noise_override(q=q):
        mean_vec = d.evaluate_agent_vec(envs, eval_episodes=5)
    assert d.seed == seed0 + 5
    _fused_ran(d, 3)
    one = SeededVecEnv()
    d.seed = seed0
    with hip.noise_override(q=q):
        mean_one = d.evaluate_agent(one, eval_episodes=5)
    assert d.seed == seed0 + 5
    got = {}
    for env in envs:
        got.update(env.totals)
    assert sorted(got) == sorted(one.totals) == list(range(seed0 + 1, seed0 + 6))
    assert got == one.totals
    assert mean_vec.is_cuda and float(mean_vec) == float(mean_one)

    S, N = 8, 3
    d2 = _dreamer(gpu, sequence_length=S, buffer_size=128)
    d2.act_batch_path = "fused"
    envs = [SeededVecEnv(space_seed=20 + e) for e in range(N)]
    d2.rollout_policy_vec(envs, random_policy=False)
    d2.rollout_policy_vec(envs, random_policy=False)
    d2.act_check()
    _fused_ran(d2, N)
    n = 2 * N * S
    assert d2.buffer.size == n
    assert np.isfinite(d2.buffer.action_buffer[:n]).all() and np.isfinite(d2.buffer.reward_buffer[:n]).all()
    assert np.abs(d2.buffer.action_buffer[:n]).max() <= 1.0
    assert all(bool(torch.isfinite(t).all()) for t in (d2.vec_latent, d2.vec_hidden))


def test_act_vec_timing(gpu):
    """Prints the table the vector dispatch follows: per
    env step of N environments at D = 24, H2D of the observations included,
    (a) the one-launch dr_act_vec, (b) the batched unfused launches; three
    repetitions of 50 steps each after a warm-up.  The committed dispatch set
    must be consistent with the entry point's cap."""
    from dreamer_amd import _lib as L
    d = _dreamer(gpu)
    assert d.ACT_VEC_FUSED_N <= set(range(1, L.DR_ACT_MAX_ENVS + 1))

    def per_step(fn, n=50):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    print(f"act_step_batch, vector observations D = {D_BENCH}, us per step of N envs "
          "(min / max of 3 x 50 steps): fused dr_act_vec | unfused")
    with torch.no_grad():
        for N in (1, 2, 4, 8, 16):
            obs, state, _, _ = _case(N, seed=N)
            state = tuple(t.to(gpu) for t in state)
            first = np.zeros(N, dtype=bool)
            row = []
            for path in ("fused", "unfused"):
                d.act_batch_path = path
                ts = [per_step(lambda: d.act_step_batch(obs, state, first, deterministic=True)) for _ in range(3)]
                row.append(ts)
                assert all(np.isfinite(t) and t > 0 for t in ts)
            d.act_check()
            _fused_ran(d, N)
            print(f"  N = {N:2d}: " + " | ".join(f"{min(ts):8.1f} / {max(ts):8.1f}" for ts in row)
                  + f"   dispatch: {'fused' if N in d.ACT_VEC_FUSED_N else 'unfused'}")
        print("  stage timeline of one fused step, us since kernel start at the end of: GRU pre-activations + encoder "
              "layer 0, gates + encoder layer 1, latent_mapper.0, sampler, actor base_net.0, actor tail")
        d.act_batch_path = "fused"
        for N in (1, 16):
            obs, state, _, _ = _case(N, seed=N)
            d.act_step_batch(obs, tuple(t.to(gpu) for t in state), np.zeros(N, dtype=bool), deterministic=True)
            d.act_check()
            # workgroup 0's stage timestamps: 100 MHz ticks at workspace offset 0
            ts = d._act_vec_bufs[N]["ws"][:128].view(torch.int64).cpu().tolist()
            print(f"  N = {N:2d}: " + ", ".join(f"{(ts[i] - ts[0]) / 100.0:.1f}" for i in (1, 2, 3, 4, 5, 15)))
    d.act_batch_path = None
