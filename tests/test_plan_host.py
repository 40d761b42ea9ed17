"""Host-side checks of the planner that need no GPU: check_plan's accepted and
refused cases, Dreamer.plan's argument errors on a CPU model, the argument
checks of dr_plan_sample / dr_plan_update (which fail before any device work),
PlanResult.shifted against numpy, and plan_ref's f32 transcription against its
float64 version on the GPU tests' inputs (the accuracy bounds are not vacuous:
the yardstick is small, and non-zero where the formulas round)."""
import numpy as np
import pytest
import torch

import plan_ref as PRF
from formula import SMALL

GOOD = dict(E=2, N=16, N_pi=4, K=4, H=5, J=2, A=3)


def test_check_plan_accepts_and_rejects():
    from dreamer_amd import check_plan
    from dreamer_amd import _lib as L
    from dreamer_amd.plan import PLAN_MAX_ROWS
    check_plan(**GOOD)
    check_plan(1, 1, 0, 1, 1, 1)                                   # the smallest search
    check_plan(1, 8, 8, 8, 1, 1)                                   # N_pi = N = K
    check_plan(16, L.DR_PLAN_MAX_CANDIDATES, 0, 1, 1, 1)           # the row cap itself
    check_plan(**GOOD, temperature=0.0, momentum=0.0, std_min=0.0, std_max=0.0, std_init=0.0)
    check_plan(**GOOD, bootstrap="target")
    check_plan(**GOOD, bootstrap=None)
    assert PLAN_MAX_ROWS == 16 * L.DR_PLAN_MAX_CANDIDATES
    bad = [dict(K=17), dict(N_pi=17), dict(E=0), dict(N=0), dict(K=0), dict(H=0), dict(J=0), dict(N_pi=-1),
           dict(A=0), dict(temperature=-0.1), dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=1.5),
           dict(std_min=0.5, std_max=0.1), dict(std_min=-0.1), dict(std_init=-1.0), dict(bootstrap="online"),
           dict(temperature=float("nan")), dict(std_max=float("inf")),
           dict(N=L.DR_PLAN_MAX_CANDIDATES + 1, K=1),              # over one environment's LDS
           dict(E=17, N=L.DR_PLAN_MAX_CANDIDATES),                 # E * N over the stated cap
           dict(H=400, A=3),                                       # H * A over DR_PLAN_MAX_ELEMS
           dict(N=16.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            check_plan(**{**GOOD, **kw})


def test_plan_bad_arguments_raise_without_gpu():
    from dreamer_amd import Dreamer
    d = Dreamer(dict(SMALL), torch.device("cpu"))
    R, C = d.latent_state_dims
    E = 2
    z, h = torch.zeros(E, R * C), torch.zeros(E, d.hidden_state_dims)
    z4, h3 = torch.zeros(E, 1, R, C), torch.zeros(E, 1, d.hidden_state_dims)
    for kw in (dict(candidates=8, elites=9), dict(candidates=8, elites=2, policy_candidates=9),
               dict(candidates=4096, elites=2), dict(temperature=-1.0), dict(momentum=1.0),
               dict(std_min=1.0, std_max=0.5), dict(iterations=0), dict(horizon=0), dict(bootstrap="both"),
               dict(candidates=16.5, elites=2), dict(candidates=8, elites=2.5), dict(horizon=2.5),   # not truncated
               dict(candidates=8, elites=2, policy_candidates=1.5), dict(iterations=1.5),
               dict(candidates=8, elites=2, policy_candidates=0, mean_init=torch.zeros(E, 4, 3), horizon=5),
               dict(candidates=8, elites=2, policy_candidates=0, iterations=1, horizon=2,
                    noise=(torch.zeros(1, E, 8, 5), None))):
        for zz, hh in ((z, h), (z4, h3)):
            with pytest.raises(ValueError):
                d.plan(zz, hh, **kw)
    with pytest.raises(ValueError):
        d.plan(torch.zeros(E, 7), h)                                   # z of the wrong width
    with pytest.raises(ValueError):
        d.plan(z, torch.zeros(E, 5))                                   # h of the wrong width
    # good arguments get as far as the device check: the planner has no CPU path
    with pytest.raises(RuntimeError):
        d.plan(z, h, candidates=8, elites=2, policy_candidates=0, iterations=1)


def _code(L, want, name, *args):
    with pytest.raises(L.HipError) as e:
        L.call(name, *args)
    assert e.value.code == want, (name, args, e.value.code)


def test_plan_entry_points_refuse_bad_arguments_on_the_host():
    from dreamer_amd import _lib as L
    INV, UNS = L.DR_E_INVALID, L.DR_E_UNSUPPORTED
    p = 256  # a non-null address that is never dereferenced: the checks come before any launch
    nz = lambda eps=p, rng=None: L.dr_noise(None, eps, rng, 0, 0)
    # dr_plan_sample(E, N, N_pi, H, A, mean, std, policy_actions, noise, actions, stream)
    good = [2, 8, 2, 3, 2, p, p, p, nz(), p, None]
    for k, v in ((0, -1), (1, 0), (2, -1), (2, 9), (3, 0), (4, 0)):  # dims; N_pi < 0 and N_pi > N
        a = list(good)
        a[k] = v
        _code(L, INV, "dr_plan_sample", *a)
    for k in (5, 6, 9):  # each required pointer in turn
        a = list(good)
        a[k] = None
        _code(L, INV, "dr_plan_sample", *a)
    _code(L, INV, "dr_plan_sample", 2, 8, 2, 3, 2, p, p, None, nz(), p, None)   # N_pi > 0 without policy_actions
    _code(L, INV, "dr_plan_sample", 2, 8, 0, 3, 2, p, p, p, nz(), p, None)      # policy_actions with N_pi = 0
    _code(L, INV, "dr_plan_sample", 2, 8, 0, 3, 2, p, p, None, nz(None), p, None)  # neither eps nor an RNG state
    _code(L, UNS, "dr_plan_sample", 1, L.DR_PLAN_MAX_CANDIDATES + 1, 0, 3, 2, p, p, None, nz(), p, None)
    _code(L, UNS, "dr_plan_sample", 1, 8, 0, 513, 2, p, p, None, nz(), p, None)  # H * A = 1026
    L.call("dr_plan_sample", 0, 8, 2, 3, 2, p, p, p, nz(), p, None)             # E = 0: a no-op
    L.call("dr_plan_sample", 0, 8, 0, 3, 2, p, p, None, nz(None, p), p, None)
    # dr_plan_update(E, N, H, A, K, rewards, continues, v_last, gamma, temperature, momentum, std_min, std_max,
    #                actions, mean, std, scores, elite_idx, elite_w, n_elite, stream)
    good = [2, 8, 3, 2, 4, p, p, p, 0.99, 0.5, 0.1, 0.05, 2.0, p, p, p, p, p, p, p, None]
    for k, v in ((0, -1), (1, 0), (2, 0), (3, 0), (4, 0), (4, 9),          # dims; K = 0 and K > N
                 (9, -0.5), (10, 1.0), (10, -0.1), (11, -1.0), (11, 3.0)):  # temperature, momentum, std bounds
        a = list(good)
        a[k] = v
        _code(L, INV, "dr_plan_update", *a)
    for k in (5, 6, 13, 14, 15, 16, 17, 18, 19):  # each required pointer in turn (v_last may be NULL)
        a = list(good)
        a[k] = None
        _code(L, INV, "dr_plan_update", *a)
    a = list(good)
    a[1] = L.DR_PLAN_MAX_CANDIDATES + 1  # N = 2049
    _code(L, UNS, "dr_plan_update", *a)
    a = list(good)
    a[2], a[3] = 342, 3  # H * A = 1026
    _code(L, UNS, "dr_plan_update", *a)
    a = list(good)
    a[0] = 0
    L.call("dr_plan_update", *a)  # E = 0: a no-op
    a[7] = None
    L.call("dr_plan_update", *a)


def test_plan_result_shifted_matches_numpy():
    from dreamer_amd import PlanResult
    g = torch.Generator().manual_seed(3)
    for E, H, A in ((3, 5, 2), (1, 1, 3), (2, 2, 1)):
        mean = torch.randn(E, H, A, generator=g)
        z = torch.zeros(E)
        r = PlanResult(action=mean[:, 0], mean=mean, std=torch.ones(E, H, A), best_actions=mean, best_score=z,
                       score_mean=z[None], score_best=z[None], elite_score_mean=z[None], policy_score=z,
                       n_elite=torch.ones(1, E, dtype=torch.int32), ok=torch.ones(E, dtype=torch.bool),
                       scores=torch.zeros(E, 4))
        s = r.shifted()
        assert tuple(s.shape) == (E, H, A)
        assert np.array_equal(s.numpy(), PRF.shifted(mean.numpy()))
        for k in range(H):
            assert torch.equal(s[:, k], mean[:, min(k + 1, H - 1)])
        assert torch.equal(r.mean, mean)  # the result itself is left alone


def update_cases(E, N):
    """The (H, A, K, temperature, momentum) grid of the dr_plan_update test at one (E, N)."""
    for H in (1, 3):
        for A in (1, 3):
            for K in sorted({1, min(8, N), N}):
                for temperature in (0.0, 0.5):
                    for momentum in (0.0, 0.3):
                        yield H, A, K, temperature, momentum


def update_inputs(E, N, H, A, seed):
    """(rewards, continues, V_H, actions (E,N,H*A) in [-1, 1] with clamped entries, mean, std) of one case."""
    r, c, v = PRF.draw_update_inputs(E, N, H, seed)
    rng = np.random.default_rng(seed + 1)
    act = np.clip(rng.standard_normal((E, N, H * A)) * 0.7, -1, 1).astype(np.float32)
    mean = rng.uniform(-0.5, 0.5, (E, H * A)).astype(np.float32)
    std = rng.uniform(0.1, 1.0, (E, H * A)).astype(np.float32)
    return r, c, v, act, mean, std


@pytest.mark.parametrize("E,N", [(1, 5), (3, 5), (1, 64), (3, 64), (1, 130), (3, 130)])
def test_f32_transcription_tracks_float64(E, N):
    """On the inputs of the GPU test: the two versions agree on the elites
    exactly (the tie guard holds), and the f32 one is off by a few roundings --
    so 8 x its error is a bound that a wrong kernel would miss."""
    worst = dict(elite_w=0.0, mean=0.0, std=0.0, scores=0.0)
    for case, (H, A, K, temperature, momentum) in enumerate(update_cases(E, N)):
        r, c, v, act, mean, std = update_inputs(E, N, H, A, 1000 * N + 10 * E + H)
        G = PRF.scores(r, c, v, 0.99, np.float64).reshape(E, N)
        assert all(PRF.tie_gaps_ok(G[e]) for e in range(E))
        args = (r, c, v, 0.99, temperature, momentum, 0.05, 2.0, act, mean, std, K)
        r64, r32 = PRF.update(*args, np.float64), PRF.update(*args, np.float32)
        assert np.array_equal(r64["elite_idx"], r32["elite_idx"]) and np.array_equal(r64["n_elite"], r32["n_elite"])
        assert (r64["n_elite"] == K).all()
        for k in worst:
            worst[k] = max(worst[k], PRF.rel(r32[k], r64[k]))
    assert 0.0 < worst["scores"] <= 64 * PRF.U, worst
    for k in ("elite_w", "mean", "std"):
        assert worst[k] <= 1e-5, worst       # 8 x this stays under the rule's 1e-4 cap
    assert worst["mean"] > 0.0 and worst["std"] > 0.0, worst
    # the sampler is exact in both: one multiply, one add, a clamp
    rng = np.random.default_rng(N)
    eps = (3.0 * rng.standard_normal((E, N, 6))).astype(np.float32)
    mean, std = rng.uniform(-0.5, 0.5, (E, 6)).astype(np.float32), rng.uniform(0.1, 1, (E, 6)).astype(np.float32)
    a32, a64 = PRF.sample(mean, std, eps, None, 0, np.float32), PRF.sample(mean, std, eps, None, 0, np.float64)
    assert PRF.rel(a32, a64) <= 2 * PRF.U and (a32 == 1).any() and (a32 == -1).any()


# (N, K, H, A) at which dr_plan_update takes another path: 1, 2, 4 or 8 candidates per thread on either side of
# each threshold, elites staged through LDS in one piece or in several (K above 8192 // (H * A)), and 4
# elements of [H][A] per thread
PATH_CASES = [(256, 8, 3, 3), (257, 8, 3, 3), (512, 64, 3, 3), (513, 200, 15, 3), (1024, 8, 2, 2), (1025, 8, 2, 2),
              (2048, 64, 2, 2), (64, 20, 128, 8)]


def path_inputs(N, H, A, seed, E=2):
    r, c, v = PRF.spaced_update_inputs(E, N, H, seed)
    rng = np.random.default_rng(seed + 1)
    act = np.clip(rng.standard_normal((E, N, H * A)) * 0.7, -1, 1).astype(np.float32)
    mean = rng.uniform(-0.5, 0.5, (E, H * A)).astype(np.float32)
    std = rng.uniform(0.1, 1.0, (E, H * A)).astype(np.float32)
    return r, c, v, act, mean, std


@pytest.mark.parametrize("N,K,H,A", PATH_CASES)
def test_f32_transcription_tracks_float64_at_the_path_thresholds(N, K, H, A):
    E = 2
    r, c, v, act, mean, std = path_inputs(N, H, A, N + K)
    G = PRF.scores(r, c, v, 0.99, np.float64).reshape(E, N)
    assert all(PRF.tie_gaps_ok(G[e]) for e in range(E))
    if (N, K) == (513, 200) or H * A == 1024:   # these two do stage their elites in several pieces
        assert K > 8192 // (H * A)
    args = (r, c, v, 0.99, 0.5, 0.3, 0.05, 2.0, act, mean, std, K)
    r64, r32 = PRF.update(*args, np.float64), PRF.update(*args, np.float32)
    assert np.array_equal(r64["elite_idx"], r32["elite_idx"]) and (r64["n_elite"] == K).all()
    for k in ("elite_w", "mean", "std"):
        assert PRF.rel(r32[k], r64[k]) <= 1e-5, k
