"""Latent planning on the GPU (dr_plan_sample, dr_plan_update, Dreamer.plan,
plan_step, evaluate_planner).

The two kernels against tests/plan_ref.py: the sampler bit for bit against
numpy's f32 clip(mean + std * eps); the update's ranking exactly and its
weights and moments by the project's accuracy rule (8 x the error the f32
transcription of the same formulas makes against float64 on these inputs, at
least 4 * 2^-24, never more than 1e-4, relative to max(1, |ref|)).  The
one-call path against the composition of the separate entry points, bit for
bit.  Run on the MI355X box: pytest -m gpu.  Measured values: DESIGN section
5j."""
import numpy as np
import pytest
import torch

import plan_ref as PRF
from formula import FULL
from gpu_helpers import build
from test_plan_host import PATH_CASES, path_inputs, update_cases, update_inputs

pytestmark = pytest.mark.gpu
F32 = np.float32


def _api():
    from dreamer_amd import _lib as L
    from dreamer_amd import hip
    return L, hip.stream()


def _dev(a, gpu, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(gpu)


# ------------------------------------------------------------------ dr_plan_sample
def _sample(gpu, E, N, N_pi, H, A, mean, std, pol, eps=None, rng=None, row0=0, stream_id=0):
    """mean, std (E,H*A), pol (E,N_pi,H*A) or None, eps (E,N,H*A) numpy or None -> (E,N,H*A) numpy."""
    L, st = _api()
    md, sd = _dev(mean, gpu), _dev(std, gpu)
    pd = _dev(pol, gpu) if N_pi > 0 else None
    ed = _dev(eps, gpu) if eps is not None else None
    out = torch.full((E, N, H * A), float("nan"), device=gpu)
    nz = L.dr_noise(None, L.ptr(ed), None if rng is None else rng.data_ptr(), row0, stream_id)
    L.call("dr_plan_sample", E, N, N_pi, H, A, L.ptr(md), L.ptr(sd), L.ptr(pd), nz, L.ptr(out), st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _sample_inputs(E, N, H, A, seed):
    rng = np.random.default_rng(seed)
    HA = H * A
    mean = rng.uniform(-0.8, 0.8, (E, HA)).astype(F32)
    std = rng.uniform(0.05, 1.5, (E, HA)).astype(F32)
    eps = rng.standard_normal((E, N, HA)).astype(F32)
    eps.reshape(-1)[::7] *= 40.0          # far enough out to clamp on either side
    pol = rng.uniform(-1, 1, (E, N, HA)).astype(F32)
    return mean, std, eps, pol


@pytest.mark.parametrize("E", [1, 3])
def test_plan_sample_explicit_noise_is_numpy_bit_for_bit(E, gpu):
    lo = hi = 0
    for N in (5, 64, 130):
        for N_pi in (0, 2, N):
            for H in (1, 3):
                for A in (1, 3):
                    mean, std, eps, pol = _sample_inputs(E, N, H, A, 100 * N + 10 * H + A)
                    pol = pol[:, :N_pi]
                    got = _sample(gpu, E, N, N_pi, H, A, mean, std, pol, eps=eps)
                    want = PRF.sample(mean, std, eps, pol, N_pi, F32)
                    assert got.tobytes() == want.tobytes(), (E, N, N_pi, H, A)
                    assert got[:, :N_pi].tobytes() == pol.tobytes()  # the actor's rows are copies
                    lo += int((got[:, N_pi:] == -1).sum())
                    hi += int((got[:, N_pi:] == 1).sum())
    assert lo > 0 and hi > 0  # both clamps were exercised


def _rng_state(gpu, seed=1234, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=gpu)


def test_plan_sample_philox(gpu):
    L, st = _api()
    E, N, H, A = 3, 130, 3, 8
    n = E * N * H * A
    assert n >= 9000
    rng = np.random.default_rng(0)
    mean = rng.uniform(-0.5, 0.5, (E, H * A)).astype(F32)
    std = np.full((E, H * A), 1e-3, F32)
    state = _rng_state(gpu)
    a1 = _sample(gpu, E, N, 0, H, A, mean, std, None, rng=state, stream_id=5 << 17)
    a2 = _sample(gpu, E, N, 0, H, A, mean, std, None, rng=state, stream_id=5 << 17)
    assert a1.tobytes() == a2.tobytes()                                   # the same state: the same bits
    a3 = _sample(gpu, E, N, 0, H, A, mean, std, None, rng=state, stream_id=6 << 17)
    assert (a3 != a1).mean() > 0.99                                       # another stream: other draws
    L.call("dr_rng_advance", state.data_ptr(), 1, st)
    a4 = _sample(gpu, E, N, 0, H, A, mean, std, None, rng=state, stream_id=5 << 17)
    assert (a4 != a1).mean() > 0.99                                       # an advanced offset: other draws
    assert np.abs(a1).max() < 1.0                                         # nothing clamps at std = 1e-3
    x = (a1.astype(np.float64) - mean[:, None, :]) / 1e-3
    print(f"philox moments over n={n}: mean {x.mean():+.4f} (bound {5 / np.sqrt(n):.4f}), "
          f"var {x.var():.4f} (bound 1 +- {5 * np.sqrt(2 / n):.4f})")
    assert abs(x.mean()) <= 5 / np.sqrt(n)
    assert abs(x.var() - 1.0) <= 5 * np.sqrt(2 / n)
    # environment e of the E = 3 call is the E = 1 call at row0 = e
    L.call("dr_rng_advance", state.data_ptr(), 1, st)
    full = _sample(gpu, E, N, 0, H, A, mean, std, None, rng=state, stream_id=5 << 17)
    for e in range(E):
        one = _sample(gpu, 1, N, 0, H, A, mean[e:e + 1], std[e:e + 1], None, rng=state, row0=e, stream_id=5 << 17)
        assert one.tobytes() == full[e:e + 1].tobytes(), e


def test_plan_sample_environments_are_independent(gpu):
    E, N, N_pi, H, A = 3, 64, 2, 3, 3
    mean, std, eps, pol = _sample_inputs(E, N, H, A, 7)
    pol = pol[:, :N_pi]
    full = _sample(gpu, E, N, N_pi, H, A, mean, std, pol, eps=eps)
    for e in range(E):
        s = slice(e, e + 1)
        one = _sample(gpu, 1, N, N_pi, H, A, mean[s], std[s], pol[s], eps=eps[s])
        assert one.tobytes() == full[s].tobytes(), e


# ------------------------------------------------------------------ dr_plan_update
def _update(gpu, E, N, H, A, K, r, c, v, gamma, temperature, momentum, std_min, std_max, act, mean, std):
    """numpy in, dict of numpy out (mean / std are the updated copies)."""
    L, st = _api()
    rd, cd, ad = _dev(r, gpu), _dev(c, gpu), _dev(act, gpu)
    vd = _dev(v, gpu) if v is not None else None
    md, sd = _dev(mean, gpu), _dev(std, gpu)
    sc = torch.full((E, N), float("nan"), device=gpu)
    ei = torch.full((E, K), -7, dtype=torch.int32, device=gpu)
    ew = torch.full((E, K), float("nan"), device=gpu)
    ne = torch.full((E,), -7, dtype=torch.int32, device=gpu)
    L.call("dr_plan_update", E, N, H, A, K, L.ptr(rd), L.ptr(cd), L.ptr(vd), gamma, temperature, momentum, std_min,
           std_max, L.ptr(ad), L.ptr(md), L.ptr(sd), L.ptr(sc), L.ptr(ei), L.ptr(ew), L.ptr(ne), st)
    torch.cuda.synchronize()
    return dict(scores=sc.cpu().numpy(), elite_idx=ei.cpu().numpy().astype(np.int64), elite_w=ew.cpu().numpy(),
                n_elite=ne.cpu().numpy().astype(np.int64), mean=md.cpu().numpy(), std=sd.cpu().numpy())


def _lambda_returns_col0(gpu, r, c, v, gamma, seed=0):
    """Column 0 of dr_lambda_returns(B, H, r, c, V, gamma, 1) for a finite V whose column H is v."""
    L, st = _api()
    B, H = r.shape
    V = np.random.default_rng(seed).standard_normal((B, H + 1)).astype(F32) * 3
    V[:, H] = 0.0 if v is None else v
    rd, cd, Vd = _dev(r, gpu), _dev(c, gpu), _dev(V, gpu)
    R = torch.empty(B, H, device=gpu)
    L.call("dr_lambda_returns", B, H, L.ptr(rd), L.ptr(cd), L.ptr(Vd), gamma, 1.0, L.ptr(R), st)
    torch.cuda.synchronize()
    return R[:, 0].cpu().numpy()


@pytest.mark.parametrize("E,N", [(1, 5), (3, 5), (1, 64), (3, 64), (1, 130), (3, 130)])
def test_plan_update_against_float64(E, N, gpu):
    """Units: relative to max(1, |ref|).  Measured maxima (MI355X) and the
    yardsticks: DESIGN 5j."""
    worst = {k: [0.0, 0.0] for k in ("elite_w", "mean", "std")}   # [measured, yardstick]
    for H, A, K, temperature, momentum in update_cases(E, N):
        r, c, v, act, mean, std = update_inputs(E, N, H, A, 1000 * N + 10 * E + H)
        G = PRF.scores(r, c, v, 0.99, np.float64).reshape(E, N)
        assert all(PRF.tie_gaps_ok(G[e]) for e in range(E))      # the reference alone decides the elite set
        args = (r, c, v, 0.99, temperature, momentum, 0.05, 2.0, act, mean, std, K)
        r64, r32 = PRF.update(*args, np.float64), PRF.update(*args, F32)
        got = _update(gpu, E, N, H, A, K, r, c, v, 0.99, temperature, momentum, 0.05, 2.0, act, mean, std)
        what = (E, N, H, A, K, temperature, momentum)
        assert np.array_equal(got["elite_idx"], r64["elite_idx"]), what
        assert np.array_equal(got["n_elite"], r64["n_elite"]), what
        assert got["scores"].reshape(-1).tobytes() == _lambda_returns_col0(gpu, r, c, v, 0.99).tobytes(), what
        for k in worst:
            y, m = PRF.rel(r32[k], r64[k]), PRF.rel(got[k], r64[k])
            worst[k] = [max(worst[k][0], m), max(worst[k][1], y)]
            assert m <= PRF.bound(y), (what, k, m, y)
    print(f"plan_update E={E} N={N}: " + ", ".join(f"{k} measured {m:.3g} yardstick {y:.3g} bound {PRF.bound(y):.3g}"
                                                  for k, (m, y) in worst.items()))


@pytest.mark.parametrize("N,K,H,A", PATH_CASES)
def test_plan_update_at_the_path_thresholds(N, K, H, A, gpu):
    """1, 2, 4 or 8 candidates per thread on either side of each threshold, the
    elites staged through LDS in one piece or in several, up to 4 elements of
    [H][A] per thread: the same checks by the same rule."""
    E = 2
    r, c, v, act, mean, std = path_inputs(N, H, A, N + K)
    G = PRF.scores(r, c, v, 0.99, np.float64).reshape(E, N)
    assert all(PRF.tie_gaps_ok(G[e]) for e in range(E))
    args = (r, c, v, 0.99, 0.5, 0.3, 0.05, 2.0, act, mean, std, K)
    r64, r32 = PRF.update(*args, np.float64), PRF.update(*args, F32)
    got = _update(gpu, E, N, H, A, K, r, c, v, 0.99, 0.5, 0.3, 0.05, 2.0, act, mean, std)
    assert np.array_equal(got["elite_idx"], r64["elite_idx"]) and np.array_equal(got["n_elite"], r64["n_elite"])
    assert got["scores"].reshape(-1).tobytes() == _lambda_returns_col0(gpu, r, c, v, 0.99).tobytes()
    for k in ("elite_w", "mean", "std"):
        y, m = PRF.rel(r32[k], r64[k]), PRF.rel(got[k], r64[k])
        print(f"plan_update N={N} K={K} H={H} A={A}: {k} measured {m:.3g} yardstick {y:.3g} bound {PRF.bound(y):.3g}")
        assert m <= PRF.bound(y), (k, m, y)
    # environment 1 alone gives its bits of the two-environment call
    rows = slice(N, 2 * N)
    one = _update(gpu, 1, N, H, A, K, r[rows], c[rows], v[rows], 0.99, 0.5, 0.3, 0.05, 2.0, act[1:], mean[1:], std[1:])
    for k in got:
        assert one[k].tobytes() == got[k][1:].tobytes(), k


def test_plan_update_without_bootstrap(gpu):
    """v_last = NULL is V_H = 0: the bits of the call with a zero vector."""
    E, N, H, A, K = 2, 64, 3, 2, 8
    r, c, v, act, mean, std = update_inputs(E, N, H, A, 5)
    a = _update(gpu, E, N, H, A, K, r, c, None, 0.99, 0.5, 0.1, 0.05, 2.0, act, mean, std)
    b = _update(gpu, E, N, H, A, K, r, c, np.zeros_like(v), 0.99, 0.5, 0.1, 0.05, 2.0, act, mean, std)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["scores"].reshape(-1).tobytes() == _lambda_returns_col0(gpu, r, c, None, 0.99).tobytes()


@pytest.mark.parametrize("temperature", [0.0, 0.5])
def test_plan_update_exact_ties_rank_by_index(temperature, gpu):
    """Duplicated candidate rows score bit-identically: the lower index ranks
    first and elite_idx is exactly the stable order."""
    E, N, H, A = 2, 64, 3, 2
    r, c, v, act, mean, std = update_inputs(E, N, H, A, 11)
    r, c, v = (t.reshape(E, N, *t.shape[1:]).copy() for t in (r, c, v))
    for t in (r, c, v):
        t[:, 5] = t[:, 3]                     # rows 3 and 5 tie,
        t[:, N // 2:] = t[:, :N // 2]         # and every row of the upper half repeats one of the lower half
    r, c, v = r.reshape(E * N, H), c.reshape(E * N, H), v.reshape(E * N)
    for K in (1, 7, 8, N):
        got = _update(gpu, E, N, H, A, K, r, c, v, 0.99, temperature, 0.0, 0.05, 2.0, act, mean, std)
        sc = got["scores"]
        assert sc[:, N // 2:].tobytes() == sc[:, :N // 2].tobytes()
        for e in range(E):
            want = PRF.rank(sc[e], K)          # stable: ties by the lower index
            assert np.array_equal(got["elite_idx"][e], want), (K, e)
            assert got["n_elite"][e] == K
        ref = PRF.update(r, c, v, 0.99, temperature, 0.0, 0.05, 2.0, act, mean, std, K, np.float64, G=sc)
        assert np.array_equal(got["elite_idx"], ref["elite_idx"])
        for k in ("elite_w", "mean", "std"):
            assert PRF.rel(got[k], ref[k]) <= 1e-5, (K, k)


def test_plan_update_nonfinite_scores_are_never_elite(gpu):
    E, N, H, A, K = 2, 64, 3, 2, 8
    r, c, v, act, mean, std = update_inputs(E, N, H, A, 13)
    bad = {0: [0, 9, 63], 1: list(range(60))}   # env 1 keeps 4 finite rows: K' = 4 < K
    kinds = [np.nan, np.inf, -np.inf]
    for e, rows in bad.items():
        for i, n in enumerate(rows):
            r[e * N + n, i % H] = kinds[i % 3]
            c[e * N + n] = 1.0                    # (a zero continue would turn an Inf return's product into NaN)
    got = _update(gpu, E, N, H, A, K, r, c, v, 0.99, 0.5, 0.0, 0.05, 2.0, act, mean, std)
    sc = got["scores"]
    for e, rows in bad.items():
        assert not np.isfinite(sc[e, rows]).any()
        assert np.isfinite(np.delete(sc[e], rows)).all()
        ne = min(K, N - len(rows))
        assert got["n_elite"][e] == ne
        el = got["elite_idx"][e]
        assert not set(el[:ne]) & set(rows) and (el[ne:] == -1).all() and (got["elite_w"][e, ne:] == 0).all()
        assert np.array_equal(el[:ne], PRF.rank(sc[e], K))
        assert abs(got["elite_w"][e].sum() - 1.0) <= 1e-6
    # the raw value is reported: a NaN reward scores NaN, an Inf one +-Inf or NaN
    assert np.isnan(sc[0, 0]) and sc[0, 9] == np.inf and sc[0, 63] == -np.inf
    ref = PRF.update(r, c, v, 0.99, 0.5, 0.0, 0.05, 2.0, act, mean, std, K, np.float64)
    assert np.array_equal(got["elite_idx"], ref["elite_idx"])
    for k in ("elite_w", "mean", "std"):
        assert PRF.rel(got[k], ref[k]) <= 1e-5, k
    # every row non-finite: no elite, mean and std keep their bits
    r[:, 0] = np.nan
    got = _update(gpu, E, N, H, A, K, r, c, v, 0.99, 0.5, 0.3, 0.05, 2.0, act, mean, std)
    assert (got["n_elite"] == 0).all() and (got["elite_idx"] == -1).all() and (got["elite_w"] == 0).all()
    assert got["mean"].tobytes() == mean.tobytes() and got["std"].tobytes() == std.tobytes()
    assert np.isnan(got["scores"]).all()


def test_plan_update_environments_are_independent(gpu):
    E, N, H, A, K = 3, 130, 3, 3, 8
    r, c, v, act, mean, std = update_inputs(E, N, H, A, 17)
    full = _update(gpu, E, N, H, A, K, r, c, v, 0.99, 0.5, 0.3, 0.05, 2.0, act, mean, std)
    for e in range(E):
        s, rows = slice(e, e + 1), slice(e * N, (e + 1) * N)
        one = _update(gpu, 1, N, H, A, K, r[rows], c[rows], v[rows], 0.99, 0.5, 0.3, 0.05, 2.0, act[s], mean[s],
                      std[s])
        for k in full:
            assert one[k].tobytes() == full[k][s].tobytes(), (e, k)


@pytest.mark.parametrize("temperature", [0.0, 0.5])
def test_plan_kernels_loop_optimises(temperature, gpu):
    """The two kernels alone in a J = 6 loop on r_k = -|a_k - a*_k|^2 (torch
    forms the rewards), c = 1, V_H = 0, against plan_ref's float64 loop on the
    same eps.  Elite sets are not compared: this problem's scores come within
    1e-6 of a tie at the K boundary."""
    L, st = _api()
    E, N, K, H, A, J = 2, 64, 8, 3, 2, 6
    gamma, std_init, std_min, std_max = 0.99, 0.5, 0.05, 2.0
    for seed in range(20):                        # chosen on the CPU: the reference itself has to converge
        rng = np.random.default_rng(seed)
        a_star = rng.uniform(-0.8, 0.8, (E, H, A)).astype(F32)
        eps = rng.standard_normal((J, E, N, H * A)).astype(F32)
        _, before, after = PRF.cem_loop(a_star, eps, K, temperature, gamma, std_init, std_min, std_max, 0.0,
                                        np.float64)
        if after < 0.25 * before:
            break
    else:
        raise AssertionError("no seed converges in the reference")
    target = _dev(a_star, gpu)
    mean, std = torch.zeros(E, H * A, device=gpu), torch.full((E, H * A), std_init, device=gpu)
    cand = torch.empty(E, N, H, A, device=gpu)
    ones = torch.ones(E * N, H, device=gpu)
    sc, ei = torch.empty(E, N, device=gpu), torch.empty(E, K, dtype=torch.int32, device=gpu)
    ew, ne = torch.empty(E, K, device=gpu), torch.empty(E, dtype=torch.int32, device=gpu)
    epsd = _dev(eps, gpu)
    for j in range(J):
        nz = L.dr_noise(None, L.ptr(epsd[j]), None, 0, 0)
        L.call("dr_plan_sample", E, N, 0, H, A, L.ptr(mean), L.ptr(std), None, nz, L.ptr(cand), st)
        r = (-((cand - target[:, None]) ** 2).sum(-1)).reshape(E * N, H).contiguous()
        L.call("dr_plan_update", E, N, H, A, K, L.ptr(r), L.ptr(ones), None, gamma, temperature, 0.0, std_min,
               std_max, L.ptr(cand), L.ptr(mean), L.ptr(std), L.ptr(sc), L.ptr(ei), L.ptr(ew), L.ptr(ne), st)
    torch.cuda.synchronize()
    err = float((mean.cpu().numpy() - a_star.reshape(E, H * A)).__abs__().max())
    print(f"loop T={temperature}: seed {seed}, start {before:.3f}, reference {after:.4f}, gpu {err:.4f}")
    assert err <= 2 * after + std_min
    assert (ne.cpu().numpy() == K).all()


# ------------------------------------------------------------------ Dreamer.plan
def _states(dr, E, gpu, seed=0):
    """Belief states to plan from: random hiddens, one-hot latents."""
    R, C = dr.latent_state_dims
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(E, dr.hidden_state_dims, generator=g) * 0.5).to(gpu)
    z = torch.nn.functional.one_hot(torch.randn(E, R, C, generator=g).argmax(-1), C).float().reshape(E, R * C).to(gpu)
    return z, h


def _noise(dr, J, E, N, H, gpu, seed=0):
    R, C = dr.latent_state_dims
    g = torch.Generator().manual_seed(100 + seed)
    eps = torch.randn(J, E, N, H * dr.action_dims, generator=g)
    q = torch.empty(J, H, E * N * R, C).exponential_(generator=g)
    return eps.to(gpu), q.to(gpu)


def _launch_dims(dr):
    d = dr.world_model.dims(dr.agent)
    d.launch_form = 1
    return d


def _actor_sequences(dr, E, N, N_pi, H, z, h, eps0, q0):
    """dr_imagine_fwd's actions (E,N_pi,H,A) from the replicated states on the draws of candidates n < N_pi."""
    from dreamer_amd import hip
    L, st = _api()
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    dev = h.device
    B = E * N_pi
    d = _launch_dims(dr)
    zP, hP = z.repeat_interleave(N_pi, 0), h.repeat_interleave(N_pi, 0)
    eps = eps0.reshape(E, N, H, A)[:, :N_pi].permute(2, 0, 1, 3).reshape(H, B, A).contiguous()
    q = q0.reshape(H, E, N, R, C)[:, :, :N_pi].reshape(H, B * R, C).contiguous()
    lat, hid = torch.empty(B, H + 1, R, C, device=dev), torch.empty(B, H + 1, Hd, device=dev)
    act, mu, sg = (torch.empty(B, H, A, device=dev) for _ in range(3))
    rew, cont = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
    tape = torch.empty(L.query("dr_imagine_tape_bytes", d, B, H), dtype=torch.uint8, device=dev)
    ws = torch.empty(L.query("dr_imagine_workspace_bytes", d, B, H) + 256, dtype=torch.uint8, device=dev)
    L.call("dr_imagine_fwd", d, dr.world_model.packed(), dr.agent.actor_struct(), B, H, L.ptr(zP), L.ptr(hP),
           hip.explicit_noise(q=q, eps=eps, device=dev), 0, L.ptr(lat), L.ptr(hid), L.ptr(act), L.ptr(rew), L.ptr(cont),
           L.ptr(mu), L.ptr(sg), L.ptr(tape), L.ptr(ws), ws.numel(), st)
    return act.reshape(E, N_pi, H, A)


def _manual_round(dr, E, N, N_pi, K, H, z, h, mean, std, pol, eps_j, q_j, temperature, momentum, std_min, std_max,
                  target=False, bootstrap=True):
    """One iteration from the separate entry points: dr_plan_sample -> WorldModel._imagine_actions -> dr_critic_fwd
    (on contiguous copies of state H) -> dr_plan_update.  mean / std are updated in place."""
    L, st = _api()
    dev = h.device
    R, C = dr.latent_state_dims
    A, Hd = dr.action_dims, dr.hidden_state_dims
    B = E * N
    d = _launch_dims(dr)
    cand = torch.empty(E, N, H, A, device=dev)
    nz = L.dr_noise(None, L.ptr(eps_j), None, 0, 0)
    L.call("dr_plan_sample", E, N, N_pi, H, A, L.ptr(mean), L.ptr(std), L.ptr(pol), nz, L.ptr(cand), st)
    zB, hB = z.repeat_interleave(N, 0).contiguous(), h.repeat_interleave(N, 0).contiguous()
    lat, hid, rew, cont = dr.world_model._imagine_actions(d, B, H, zB, hB, cand.data_ptr(), H * A, A, q_j)
    v = None
    if bootstrap:
        hH, zH = hid[:, H].contiguous(), lat[:, H].reshape(B, R * C).contiguous()
        v = torch.empty(B, device=dev)
        ws = torch.empty(L.query("dr_critic_workspace_bytes", d, B, 0), dtype=torch.uint8, device=dev)
        L.call("dr_critic_fwd", d, dr.agent.critic_struct(target=target), B, L.ptr(hH), Hd, L.ptr(zH), R * C, None,
               L.ptr(v), None, L.ptr(ws), ws.numel(), st)
    sc = torch.empty(E, N, device=dev)
    ei, ew = torch.empty(E, K, dtype=torch.int32, device=dev), torch.empty(E, K, device=dev)
    ne = torch.empty(E, dtype=torch.int32, device=dev)
    L.call("dr_plan_update", E, N, H, A, K, L.ptr(rew), L.ptr(cont), L.ptr(v), float(dr.agent.gamma), temperature,
           momentum, std_min, std_max, L.ptr(cand), L.ptr(mean), L.ptr(std), L.ptr(sc), L.ptr(ei), L.ptr(ew),
           L.ptr(ne), st)
    return dict(cand=cand, scores=sc, elite_idx=ei, elite_w=ew, n_elite=ne, v=v)


def _same(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.numpy().tobytes() == b.numpy().tobytes(), what


def _check_against_rounds(res, rounds, mean, std, E, N, N_pi, K):
    """Every PlanResult field from the manual rounds' outputs (mean / std: the manual final ones)."""
    last = rounds[-1]
    _same(res.mean, mean, "mean")
    _same(res.std, std, "std")
    _same(res.action, mean[:, 0], "action")
    _same(res.scores, last["scores"], "scores")
    _same(res.candidates, last["cand"], "candidates")
    _same(res.elite_idx, last["elite_idx"], "elite_idx")
    _same(res.elite_w, last["elite_w"], "elite_w")
    _same(res.n_elite, torch.stack([r["n_elite"] for r in rounds]), "n_elite")
    assert bool(res.ok.all()) and res.ok.dtype == torch.bool and tuple(res.ok.shape) == (E,)
    sc = torch.stack([r["scores"] for r in rounds]).cpu()
    ei = torch.stack([r["elite_idx"] for r in rounds]).cpu().long()
    es = torch.gather(sc, -1, ei)
    _same(res.score_best, es[..., 0], "score_best")
    _same(res.best_score, es[-1, :, 0], "best_score")
    _same(res.best_actions, last["cand"].cpu()[torch.arange(E), ei[-1, :, 0]], "best_actions")
    assert torch.allclose(res.score_mean.cpu(), sc.mean(-1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(res.elite_score_mean.cpu(), es.mean(-1), rtol=1e-5, atol=1e-6)
    if N_pi > 0:
        assert torch.allclose(res.policy_score.cpu(), sc[-1, :, :N_pi].mean(-1), rtol=1e-5, atol=1e-6)
    else:
        assert bool(torch.isnan(res.policy_score).all())
    assert (es[..., :-1] >= es[..., 1:]).all()          # rank order
    assert tuple(res.shifted().shape) == tuple(mean.shape)


@pytest.mark.parametrize("N,K,N_pi,J", [(5, 3, 0, 1), (64, 8, 2, 1), (5, 3, 2, 2), (64, 8, 0, 2)])
def test_plan_matches_manual_composition(N, K, N_pi, J, gpu):
    """Dreamer.plan with explicit noise at SMALL, E = 3: every field is bit for
    bit J rounds of the separate entry points chained (E * N = 192 takes
    dr_imagine_actions' B >= 128 form); with policy_candidates > 0 rows n <
    N_pi of the candidates are dr_imagine_fwd's actions on the same draws."""
    dr, _ = build("small", gpu)
    E, H, A = 3, dr.horizon, dr.action_dims
    z, h = _states(dr, E, gpu)
    eps, q = _noise(dr, J, E, N, H, gpu, seed=N + J)
    kw = dict(temperature=0.5, momentum=0.1, std_min=0.05, std_max=2.0)
    with torch.no_grad():
        res = dr.plan(z, h, candidates=N, policy_candidates=N_pi, elites=K, iterations=J, std_init=0.5,
                      noise=(eps, q), **kw)
        pol = _actor_sequences(dr, E, N, N_pi, H, z, h, eps[0], q[0]) if N_pi > 0 else None
        mean, std = torch.zeros(E, H, A, device=gpu), torch.full((E, H, A), 0.5, device=gpu)
        rounds = [_manual_round(dr, E, N, N_pi, K, H, z, h, mean, std, pol, eps[j], q[j], **kw) for j in range(J)]
    torch.cuda.synchronize()
    _check_against_rounds(res, rounds, mean, std, E, N, N_pi, K)
    if N_pi > 0:
        _same(res.candidates[:, :N_pi], pol, "actor rows")
        assert float((pol[:, 0] - pol[:, 1]).abs().max()) > 0   # the sampling actor: distinct sequences
    # the (E,1,R,C) / (E,1,hidden) shapes act_step_batch returns are accepted and give the same bits
    R, C = dr.latent_state_dims
    with torch.no_grad():
        res4 = dr.plan(z.view(E, 1, R, C), h.view(E, 1, -1), candidates=N, policy_candidates=N_pi, elites=K,
                       iterations=J, std_init=0.5, noise=(eps, q), **kw)
    _same(res4.mean, res.mean, "mean from 4-d states")
    _same(res4.scores, res.scores, "scores from 4-d states")


def test_plan_bootstrap_variants(gpu):
    """bootstrap="target" values the end states with the target critic, None with 0 (and no critic launch)."""
    dr, _ = build("small", gpu)
    with torch.no_grad():
        for p in dr.agent.target_critic.parameters():   # make the two critics differ
            p.mul_(0.5)
    E, N, K, H, A = 2, 8, 3, dr.horizon, dr.action_dims
    z, h = _states(dr, E, gpu, seed=2)
    eps, q = _noise(dr, 1, E, N, H, gpu, seed=3)
    kw = dict(temperature=0.5, momentum=0.0, std_min=0.05, std_max=2.0)
    out = {}
    for name, mk in (("critic", dict()), ("target", dict(target=True)), (None, dict(bootstrap=False))):
        calls = []
        from dreamer_amd import _lib as L
        orig = L.call
        L.call = lambda n, *a, _o=orig: (calls.append(n), _o(n, *a))[1]
        try:
            with torch.no_grad():
                res = dr.plan(z, h, candidates=N, policy_candidates=0, elites=K, iterations=1, bootstrap=name,
                              noise=(eps, q), **kw)
        finally:
            L.call = orig
        assert calls.count("dr_critic_fwd") == (0 if name is None else 1)
        mean, std = torch.zeros(E, H, A, device=gpu), torch.full((E, H, A), 0.5, device=gpu)
        with torch.no_grad():
            rd = _manual_round(dr, E, N, 0, K, H, z, h, mean, std, None, eps[0], q[0], **kw, **mk)
        _same(res.scores, rd["scores"], f"scores bootstrap={name}")
        _same(res.mean, mean, f"mean bootstrap={name}")
        out[name] = res.scores.cpu()
    assert not torch.equal(out["critic"], out["target"]) and not torch.equal(out["critic"], out[None])


def test_plan_runs_in_launch_form(gpu, monkeypatch):
    """Every dr_imagine_fwd / dr_imagine_actions the planner issues is given
    dims with launch_form = 1, under which dr_persistent_kernels reports no
    persistent launch."""
    from dreamer_amd import _lib as L
    dr, _ = build("small", gpu)
    E, N, N_pi = 2, 8, 3
    z, h = _states(dr, E, gpu)
    seen = []
    orig = L.call

    def spy(name, *args):
        if name in ("dr_imagine_fwd", "dr_imagine_actions", "dr_critic_fwd"):
            d = args[0]
            B = args[3] if name == "dr_imagine_fwd" else args[2]
            seen.append((name, int(d.launch_form), L.query("dr_persistent_kernels", d, B, 1, dr.horizon), B))
        return orig(name, *args)

    monkeypatch.setattr(L, "call", spy)
    with torch.no_grad():
        dr.plan(z, h, candidates=N, policy_candidates=N_pi, elites=3, iterations=2)
    torch.cuda.synchronize()
    names = [s[0] for s in seen]
    assert names.count("dr_imagine_fwd") == 1 and names.count("dr_imagine_actions") == 2
    assert names.count("dr_critic_fwd") == 2
    assert all(lf == 1 and pk == 0 for _, lf, pk, _ in seen), seen
    assert [s[3] for s in seen if s[0] == "dr_imagine_fwd"] == [E * N_pi]
    assert float(dr.agent.fault_slot()) == 0.0


def test_plan_sample_false_is_reproducible_and_leaves_the_engine_rng(gpu):
    from dreamer_amd import hip
    dr, _ = build("small", gpu)
    E, N, H = 2, 16, dr.horizon
    z, h = _states(dr, E, gpu, seed=4)
    eps, _ = _noise(dr, 2, E, N, H, gpu, seed=5)
    before = hip.rng(gpu).state.clone()
    with torch.no_grad():
        a = dr.plan(z, h, candidates=N, policy_candidates=0, elites=4, iterations=2, sample=False, noise=(eps, None))
        b = dr.plan(z, h, candidates=N, policy_candidates=0, elites=4, iterations=2, sample=False, noise=(eps, None))
        c = dr.plan(z, h, candidates=N, policy_candidates=2, elites=4, iterations=2)   # all Philox
    torch.cuda.synchronize()
    for k in ("action", "mean", "std", "scores", "best_actions", "score_mean", "n_elite"):
        _same(getattr(a, k), getattr(b, k), k)
    assert torch.equal(hip.rng(gpu).state, before)        # the training run's {seed, offset}
    assert bool(torch.isfinite(c.mean).all()) and bool(c.ok.all())
    assert float(c.mean.abs().max()) <= 1.0 and float(c.std.min()) >= 0.05
    # the mode is q == 1: the same bits as explicit ones
    R, C = dr.latent_state_dims
    ones = torch.ones(2, H, E * N * R, C, device=gpu)
    with torch.no_grad():
        d = dr.plan(z, h, candidates=N, policy_candidates=0, elites=4, iterations=2, noise=(eps, ones))
    _same(a.scores, d.scores, "mode == explicit ones")


# ------------------------------------------------------------------ plan_step / evaluate_planner
class StubEnv:
    """A seeded environment whose frames, rewards and episode lengths depend on
    (seed, step) alone: what an episode returns is known without the agent."""

    def __init__(self, hw=(32, 32), vector=0):
        self.hw, self.vector = hw, vector
        self.seed, self.t = None, 0

    @staticmethod
    def length(seed):
        return 2 + seed % 2

    @staticmethod
    def reward(seed, t):
        return 0.25 * (seed % 5) + t

    def _frame(self):
        rng = np.random.default_rng(1000 * self.seed + self.t)
        if self.vector:
            return rng.standard_normal(self.vector).astype(np.float32)
        return rng.integers(0, 256, size=(*self.hw, 3), dtype=np.uint8)

    def reset(self, seed=None):
        self.seed, self.t = int(seed), 0
        return self._frame(), {}

    def step(self, action):
        assert np.all(np.isfinite(action)) and np.all(np.abs(action) <= 1.0)
        self.t += 1
        return self._frame(), self.reward(self.seed, self.t), self.t >= self.length(self.seed), False, {}


PLAN_KW = dict(candidates=8, policy_candidates=2, elites=3, iterations=1, horizon=2)


def test_plan_step_shapes_state_and_restart(gpu):
    from dreamer_amd import hip
    dr, _ = build("small", gpu)
    E, A = 2, dr.action_dims
    R, C = dr.latent_state_dims
    H, N = PLAN_KW["horizon"], PLAN_KW["candidates"]
    envs = [StubEnv() for _ in range(E)]
    frames = np.stack([env.reset(seed=3 + e)[0] for e, env in enumerate(envs)])
    # the filter's posterior draws, explicit, so a second act_step_batch gives the same states
    q_act = torch.empty(1, E * R, C).exponential_(generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad(), hip.noise_override(q=q_act):
        ref = dr.act_step_batch(frames, deterministic=True)
        act, state, res = dr.plan_step(frames, **PLAN_KW)    # (the planner's own draws: Philox)
    assert tuple(act.shape) == tuple(ref[0].shape) == (E, 1, A)
    assert tuple(state[0].shape) == tuple(ref[3].shape) == (E, 1, R, C)
    assert tuple(state[1].shape) == tuple(ref[4].shape) == (E, 1, dr.hidden_state_dims)
    _same(state[0], ref[3], "z'")
    _same(state[1], ref[4], "h'")
    assert state[2] is act and bool(res.ok.all())
    _same(act.view(E, A), res.action, "the planner's action")
    # the returned state feeds the next call; row 0 restarts (first), row 1 continues its plan
    frames2 = np.stack([env.step(act[e, 0].cpu().numpy())[0] for e, env in enumerate(envs)])
    first = np.array([True, False])
    eps, q = _noise(dr, 1, E, N, H, gpu, seed=9)
    with torch.no_grad(), hip.noise_override(q=q_act):
        act2, state2, res2 = dr.plan_step(frames2, state, first, res, noise=(eps, q), **PLAN_KW)
        a_ref, _, _, z2, h2 = dr.act_step_batch(frames2, state, first, deterministic=True)
        init = res.shifted().clone()
        init[0] = 0.0
        want = dr.plan(z2, h2, mean_init=init, noise=(eps, q), **PLAN_KW)
    _same(state2[0], z2, "z''")
    _same(state2[1], h2, "h''")
    _same(res2.mean, want.mean, "mean after a restart of row 0")
    _same(res2.scores, want.scores, "scores after a restart of row 0")
    _same(act2.view(E, A), want.action, "action")
    # an (E,H,A) mean is taken as given
    with torch.no_grad(), hip.noise_override(q=q_act):
        _, _, res3 = dr.plan_step(frames2, state, first, res.shifted(), noise=(eps, q), **PLAN_KW)
    _same(res3.mean, want.mean, "mean from a tensor plan_state")


def test_plan_step_falls_back_to_the_actor(gpu):
    """A head whose output bias is NaN makes every score NaN: no elite, ok is
    false, mean and std stay, and the action is the actor's deterministic one.
    The NaN sits in the continue head: sigmoid hands it on, whereas a NaN in
    the critic's (or the reward head's) logits is swallowed by symexp's clamp
    to +-20 (fminf / fmaxf drop a NaN) and comes out as a finite, saturated
    value -- such a critic does not show in `ok`."""
    from dreamer_amd import hip
    dr, _ = build("small", gpu)
    bias = dr.world_model.continue_predictor.logit_generator[6].bias
    with torch.no_grad():
        bias.fill_(float("nan"))
    E, A = 2, dr.action_dims
    R, C = dr.latent_state_dims
    frames = np.stack([StubEnv().reset(seed=5 + e)[0] for e in range(E)])
    q_act = torch.empty(1, E * R, C).exponential_(generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad(), hip.noise_override(q=q_act):
        a_ref = dr.act_step_batch(frames, deterministic=True)[0]
        act, state, res = dr.plan_step(frames, **PLAN_KW)
    assert not bool(res.ok.any()) and int(res.n_elite.sum()) == 0
    assert bool(torch.isnan(res.scores).all()) and bool(torch.isnan(res.best_score).all())
    assert bool((res.mean == 0).all()) and bool((res.std == 0.5).all())
    _same(act, a_ref, "the actor's action")
    assert bool(torch.isfinite(act).all())
    # with the head mended the same model plans
    with torch.no_grad():
        bias.fill_(0.0)
        act_t, _, res_t = dr.plan_step(frames, **PLAN_KW)
    assert bool(res_t.ok.all())
    _same(act_t.view(E, A), res_t.action, "planned action")


def test_plan_step_falls_back_row_by_row(gpu, monkeypatch):
    """One environment's hidden state is NaN (poisoned on the way out of the
    filter): its scores are NaN through the continue head, it has no elite and
    takes the actor's action, while the other row plans as it does beside a
    healthy neighbour."""
    from dreamer_amd import hip
    dr, _ = build("small", gpu)
    E, A = 2, dr.action_dims
    R, C = dr.latent_state_dims
    H, N = PLAN_KW["horizon"], PLAN_KW["candidates"]
    frames = np.stack([StubEnv().reset(seed=7 + e)[0] for e in range(E)])
    q_act = torch.empty(1, E * R, C).exponential_(generator=torch.Generator().manual_seed(8)).to(gpu)
    eps, q = _noise(dr, 1, E, N, H, gpu, seed=12)
    filt = dr.act_step_batch

    def poisoned(*args, **kw):
        out = filt(*args, **kw)
        out[4][0] = float("nan")
        return out

    with torch.no_grad(), hip.noise_override(q=q_act):
        a_ref, _, _, z2, h2 = filt(frames, deterministic=True)
        monkeypatch.setattr(dr, "act_step_batch", poisoned)
        act, state, res = dr.plan_step(frames, noise=(eps, q), **PLAN_KW)
        monkeypatch.undo()
        clean = dr.plan(z2, h2, noise=(eps, q), **PLAN_KW)   # the same call on the states as the filter left them
    assert res.ok.tolist() == [False, True] and res.n_elite[-1].tolist() == [0, PLAN_KW["elites"]]
    assert bool(torch.isnan(res.scores[0]).all()) and bool(torch.isfinite(res.scores[1]).all())
    assert bool((res.mean[0] == 0).all()) and bool((res.std[0] == 0.5).all())
    assert bool(torch.isnan(res.best_actions[0]).all()) and bool(torch.isfinite(res.best_actions[1]).all())
    _same(act[0], a_ref[0], "row 0: the actor's action")
    _same(act[1].view(A), res.action[1], "row 1: the planner's action")
    assert not torch.equal(act[1], a_ref[1])
    assert bool(clean.ok.all())
    _same(res.mean[1], clean.mean[1], "row 1 beside a NaN row")
    _same(res.scores[1], clean.scores[1], "row 1's scores")
    assert bool(torch.isfinite(act).all()) and state[2] is act


def test_plan_mean_init_layout(gpu):
    """A non-contiguous (E,H,A) mean_init (a permuted view) is read by value, not by memory order."""
    dr, _ = build("small", gpu)
    E, H, A, N = 2, dr.horizon, dr.action_dims, 8
    z, h = _states(dr, E, gpu, seed=3)
    eps, q = _noise(dr, 1, E, N, H, gpu, seed=4)
    base = (torch.rand(E, A, H, generator=torch.Generator().manual_seed(1)) - 0.5).to(gpu)
    view = base.permute(0, 2, 1)
    assert not view.is_contiguous()
    kw = dict(candidates=N, policy_candidates=0, elites=3, iterations=1, momentum=0.3, noise=(eps, q))
    with torch.no_grad():
        a = dr.plan(z, h, mean_init=view, **kw)
        b = dr.plan(z, h, mean_init=view.contiguous(), **kw)
    for k in ("mean", "std", "scores", "candidates"):
        _same(getattr(a, k), getattr(b, k), k)
    assert torch.equal(view, base.permute(0, 2, 1))   # the caller's tensor is left alone


def test_evaluate_planner_runs_episodes_in_order(gpu):
    dr, _ = build("small", gpu)
    seed0 = dr.seed
    envs = [StubEnv(), StubEnv()]
    with torch.no_grad():
        got = dr.evaluate_planner(envs, 3, **PLAN_KW)
    seeds = [seed0 + 1, seed0 + 2, seed0 + 3]               # in the order the episodes start
    totals = [sum(StubEnv.reward(s, t) for t in range(1, StubEnv.length(s) + 1)) for s in seeds]
    assert dr.seed == seed0 + 3
    assert abs(float(got) - float(np.mean(np.asarray(totals, np.float32)))) <= 1e-6
    assert got.device.type == "cuda" and got.dim() == 0


def test_plan_vector_observation_model(gpu):
    """A dims.obs_dim > 0 model (test_gpu_vector.py's config): the planner starts from a state, not a frame."""
    from dreamer_amd import Dreamer
    cfg = dict(FULL)
    cfg.update(observation_dims=[24])
    torch.manual_seed(0)
    dr = Dreamer(cfg, gpu)
    assert dr.world_model.dims(dr.agent).obs_dim == 24
    E, N, N_pi, K, H, A = 2, 8, 2, 3, 2, dr.action_dims
    z, h = _states(dr, E, gpu, seed=6)
    eps, q = _noise(dr, 1, E, N, H, gpu, seed=7)
    kw = dict(temperature=0.5, momentum=0.1, std_min=0.05, std_max=2.0)
    with torch.no_grad():
        res = dr.plan(z, h, horizon=H, candidates=N, policy_candidates=N_pi, elites=K, iterations=1, noise=(eps, q),
                      **kw)
        pol = _actor_sequences(dr, E, N, N_pi, H, z, h, eps[0], q[0])
        mean, std = torch.zeros(E, H, A, device=gpu), torch.full((E, H, A), 0.5, device=gpu)
        rounds = [_manual_round(dr, E, N, N_pi, K, H, z, h, mean, std, pol, eps[0], q[0], **kw)]
    torch.cuda.synchronize()
    _check_against_rounds(res, rounds, mean, std, E, N, N_pi, K)
    # and one env step from vector observations
    envs = [StubEnv(vector=24) for _ in range(E)]
    obs = np.stack([env.reset(seed=1 + e)[0] for e, env in enumerate(envs)])
    with torch.no_grad():
        act, state, r2 = dr.plan_step(obs, horizon=H, candidates=N, policy_candidates=N_pi, elites=K, iterations=1)
    assert tuple(act.shape) == (E, 1, A) and bool(r2.ok.all()) and bool(torch.isfinite(act).all())
