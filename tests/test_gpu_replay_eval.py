"""What the replay-window entry points share (dreamer_amd/replay_eval.py) and
the episode loop of evaluate_agent_vec / evaluate_planner: how many ad-hoc
Philox streams each call takes, that the evaluate_* methods put the random
state back when a batch raises, and the order in which the episode loop starts
and scores episodes.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

from formula import SMALL, replay_data
from gpu_helpers import build
from test_gpu_futures import _same
from test_gpu_plan import PLAN_KW, StubEnv

pytestmark = pytest.mark.gpu
B, S, TC, H, T, M = 2, 8, 3, 4, 6, 2


@pytest.fixture(scope="module")
def small(gpu):
    """One SMALL Dreamer with a filled ring (the tests below leave it as they found it)."""
    d, _ = build("small", gpu, B=B, H=H, S=S)
    d.buffer.load_arrays(*replay_data(64, tuple(SMALL["observation_dims"]), d.action_dims, seed=0))
    return d


def _exp(gen, *shape):
    return torch.empty(*shape).exponential_(generator=gen)


def test_adhoc_streams_taken_per_call(small, gpu):
    """The ad-hoc generator's counter advances once per stage that draws from
    Philox: open_loop and sample_futures scan + unroll, closed_loop trace +
    prior sample (the latter only with predict=True), agent_trace trace; a
    stage given explicit draws, or the mode, takes none."""
    from dreamer_amd import hip
    d = small
    R, C = d.latent_state_dims
    starts = np.array([0, 21])
    g = torch.Generator().manual_seed(5)
    q_ctx, q_h, q_hm, q_t = (t.to(gpu) for t in (_exp(g, TC, B * R, C), _exp(g, H, B * R, C),
                                                  _exp(g, H, B * M * R, C), _exp(g, T, B * R, C)))
    ol = dict(starts=starts, context=TC, horizon=H)
    tr = dict(starts=starts, length=T)
    cases = [
        ("open_loop", d.open_loop, ol, 2),
        ("open_loop sample=False", d.open_loop, dict(ol, sample=False), 0),
        ("open_loop noise", d.open_loop, dict(ol, noise=(q_ctx, q_h)), 0),
        ("sample_futures", d.sample_futures, dict(ol, samples=M), 2),
        ("sample_futures noise", d.sample_futures, dict(ol, samples=M, noise=(q_ctx, q_hm)), 0),
        ("closed_loop", d.closed_loop, tr, 2),
        ("closed_loop predict=False", d.closed_loop, dict(tr, predict=False), 1),
        ("closed_loop sample=False", d.closed_loop, dict(tr, sample=False), 0),
        ("closed_loop noise", d.closed_loop, dict(tr, noise=(q_t, q_t)), 0),
        ("agent_trace", d.agent_trace, tr, 1),
        ("agent_trace sample=False", d.agent_trace, dict(tr, sample=False), 0),
        ("agent_trace noise", d.agent_trace, dict(tr, noise=q_t), 0),
    ]
    ar = hip.adhoc(gpu)
    ar.reseed(12)  # counter 0: far from the 14-bit wrap
    got = {}
    with torch.no_grad():
        for name, fn, kw, _ in cases:
            before = ar.counter
            fn(**kw)
            got[name] = ar.counter - before
    torch.cuda.synchronize()
    print(got)
    assert got == {name: want for name, _, _, want in cases}


EVALUATE = [
    ("evaluate_world_model", "open_loop", dict(context=TC, horizon=H)),
    ("evaluate_filter", "closed_loop", dict(length=T)),
    ("evaluate_values", "agent_trace", dict(length=T)),
    ("evaluate_futures", "sample_futures", dict(context=TC, horizon=H, samples=M)),
]


@pytest.mark.parametrize("evaluate,inner,kw", EVALUATE, ids=[e[0] for e in EVALUATE])
def test_evaluate_restores_state_when_a_batch_raises(evaluate, inner, kw, small, gpu, monkeypatch):
    """The call inside evaluate_* raises on its second batch: np.random's state
    and training_state() are as found, though the first batch had moved both."""
    from dreamer_amd import hip
    d = small
    np.random.seed(3)
    hip.adhoc(gpu).reseed(12)
    real = getattr(d, inner)
    before_np, before = np.random.get_state(), d.training_state()
    seen = []

    def failing(*a, **k):
        if seen:
            # the first batch drew window starts and Philox streams
            now = np.random.get_state()
            assert now[2] != before_np[2] or not np.array_equal(now[1], before_np[1])
            assert hip.adhoc(gpu).counter != before["rng_adhoc_counter"]
            raise RuntimeError("second batch")
        seen.append(1)
        return real(*a, **k)

    monkeypatch.setattr(d, inner, failing)
    with pytest.raises(RuntimeError, match="second batch"):
        getattr(d, evaluate)(batches=3, **kw)
    after_np, after = np.random.get_state(), d.training_state()
    assert before_np[0] == after_np[0] and np.array_equal(before_np[1], after_np[1])
    assert before_np[2:] == after_np[2:]
    _same(before, after)


class LoggingEnv(StubEnv):
    """A StubEnv that writes its resets and its episodes' totals into a shared log."""

    def __init__(self, name, log):
        super().__init__()
        self.name, self.log = name, log

    def reset(self, seed=None):
        self.log.append([self.name, int(seed), 0.0, 0])  # env, seed, total, steps
        self.mine = self.log[-1]
        return super().reset(seed=seed)

    def step(self, action):
        out = super().step(action)
        self.mine[2] += out[1]
        self.mine[3] += 1
        return out


@pytest.mark.parametrize("entry", ["evaluate_agent_vec", "evaluate_planner"])
def test_episode_loop_order(entry, gpu):
    """2 envs, 5 episodes of lengths 2 and 3 in turn (StubEnv.length): the
    episodes are seeded seed + 1 .. seed + 5 in the order they start -- the
    first two together, then whichever env finishes takes the next seed, the
    lower row first when both finish in one step -- every episode runs to its
    end, and the result is the mean of the totals in that order."""
    d, _ = build("small", gpu)
    seed0, n = d.seed, 5
    log = []
    envs = [LoggingEnv(0, log), LoggingEnv(1, log)]
    with torch.no_grad():
        got = getattr(d, entry)(envs, n, **(PLAN_KW if entry == "evaluate_planner" else {}))
    # the schedule, written out: env e runs an episode of known length, then takes the next seed
    want, free_at, nxt = [], [0, 0], seed0 + 1
    while nxt <= seed0 + n:
        e = 0 if free_at[0] <= free_at[1] else 1
        want.append((free_at[e], e, nxt))
        free_at[e] += StubEnv.length(nxt)
        nxt += 1
    want = [(e, s) for _, e, s in sorted(want)]
    assert [(e, s) for e, s, _, _ in log] == want
    assert [s for _, s, _, _ in log] == list(range(seed0 + 1, seed0 + n + 1))
    assert len({StubEnv.length(s) for _, s, _, _ in log}) == 2  # unequal lengths
    for _, s, total, steps in log:
        assert steps == StubEnv.length(s)
        assert total == sum(StubEnv.reward(s, t) for t in range(1, steps + 1))
    assert d.seed == seed0 + n
    assert abs(float(got) - float(np.mean(np.asarray([t for _, _, t, _ in log], np.float32)))) <= 1e-6
    assert got.device.type == "cuda" and got.dim() == 0
