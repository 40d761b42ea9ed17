"""bench.py --dump-outputs: what dump_outputs writes for the timed path
(Dreamer.train_Agent): float32 .npy files, a fixed seeded sample where an
array is over its share of the size budget, and on the GPU the values the
caller of train_Agent() holds after the call."""
import os
import types

import numpy as np
import pytest
import torch

NAMES = {"losses", "actor_params", "critic_params", "target_critic_params", "latents", "hiddens", "actions",
         "rewards", "continues", "lambda_returns"}


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    flat = lambda n: types.SimpleNamespace(flat=r(n))
    eng = types.SimpleNamespace(latents=r(4, 3, 50), hiddens=r(4, 3, 70).double(), actions=r(4, 2, 3),
                                rewards=r(4, 2), continues=r(4, 2), R=r(4, 2))
    d = types.SimpleNamespace(_engine=eng, agent=types.SimpleNamespace(fa=flat(90), fc=flat(101), ft=flat(101)))
    # 1782 elements in all; with 1000 allowed, everything up to the 101 critic parameters is whole and
    # latents (600) and hiddens (840) share what is left: 329 each
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    bench.dump_outputs(str(tmp_path / "a"), d, (0.5, -1.25))
    bench.dump_outputs(str(tmp_path / "b"), d, (0.5, -1.25))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) == NAMES
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 4 * 1000
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
    assert a["losses"].tolist() == [0.5, -1.25]
    assert np.array_equal(a["actions"], eng.actions.numpy())
    assert np.array_equal(a["target_critic_params"], d.agent.ft.flat.numpy())
    assert a["latents"].shape == (329,) and a["hiddens"].shape == (329,)
    for k, src in (("latents", eng.latents), ("hiddens", eng.hiddens)):
        src = src.float().numpy().reshape(-1)
        idx = np.sort(np.random.default_rng(0).choice(src.size, size=329, replace=False))
        assert np.array_equal(a[k], src[idx]), k
    # nothing is sampled while the whole set fits
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1782)
    bench.dump_outputs(str(tmp_path / "c"), d, (0.5, -1.25))
    c = _load(tmp_path / "c")
    assert c["latents"].shape == (4, 3, 50) and c["hiddens"].shape == (4, 3, 70)


@pytest.mark.gpu
def test_dump_outputs_of_train_agent(gpu, tmp_path):
    import bench
    B = 16
    np.random.seed(1000)
    _, d = bench.make_dreamer(bench.CAR_RACER, gpu, B, 64, 15, 64, 1, 1, 0, None, "fp32")
    for _ in range(2):
        la, lc = d.train_Agent()
    torch.cuda.synchronize()
    bench.dump_outputs(str(tmp_path), d, (float(la), float(lc)))
    a = _load(tmp_path)
    assert set(a) == NAMES
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    assert a["losses"].tolist() == [np.float32(float(la)), np.float32(float(lc))]
    eng, ag = d._engine, d.agent
    for k, t in (("actor_params", ag.fa.flat), ("critic_params", ag.fc.flat), ("target_critic_params", ag.ft.flat),
                 ("latents", eng.latents), ("hiddens", eng.hiddens), ("actions", eng.actions),
                 ("rewards", eng.rewards), ("continues", eng.continues), ("lambda_returns", eng.R)):
        assert a[k].shape == tuple(t.shape) and np.array_equal(a[k], t.cpu().numpy()), k
    assert a["hiddens"].shape == (B, 16, 600) and np.abs(a["hiddens"]).max() > 0
    assert np.abs(a["lambda_returns"]).max() > 0 and np.abs(a["actions"]).max() > 0
