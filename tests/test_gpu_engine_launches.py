"""The launch order of one train_Agent epoch, per phase: the names of the library entry points the engine calls
(dreamer_amd._lib.call), in order, against a table.  The epoch exists as the sequential phases, the data-parallel
two-phase update and losses_and_grads(fork=True); all are compositions of the same launch methods, and
this holds them to one order.  The table is the recording made before the launch methods were introduced
(profiles/engine_launch_order_parent.txt).  The pipelined graphs are held bit for bit by
test_pipelined_epochs_match_sequential."""
import pytest
import torch

from conftest import load_fixture
from gpu_helpers import build
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu

ENCWARM = ["dr_replay_gather", "dr_encoder_features", "dr_observe_scan"]
UPDATE = ["dr_critic_fwd", "dr_update_S", "dr_actor_loss_grad", "dr_critic_loss_bwd", "dr_imagine_bwd"]
OPTIM = ["dr_ac_optimiser_step", "dr_rng_advance"]
SEQUENTIAL = {"encwarm": ENCWARM, "imagine": ["dr_imagine_fwd"], "returns": ["dr_critic_fwd", "dr_lambda_returns"],
              "update": UPDATE, "optim": OPTIM}
# the grouped heads pass: dr_heads_fwd behind the unroll, and no critic forward of its own in returns / update
GROUPED = dict(SEQUENTIAL, imagine=["dr_imagine_fwd", "dr_heads_fwd"], returns=["dr_lambda_returns"],
               update=UPDATE[1:])


def _trace(monkeypatch):
    """Every _lib.call from here on appends its entry-point name to the returned list before the real call."""
    from dreamer_amd import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return names


def _engine(which, gpu, world=None):
    """An eager engine over a loaded replay buffer: the small model of test_graph_replay_matches_eager (heads not
    grouped: B (H + 1) = 48 < 1024) or the full one at the grouped heads' test shape."""
    from dreamer_amd.engine import ImaginationEngine
    from formula import replay_data
    if which == "small":
        d, _ = build("small", gpu, load_fixture("small_epoch"), B=8, S=8, H=5)
        hw = (32, 32)
    else:
        d, _ = build("full", gpu, B=68, H=15)
        hw = (64, 64)
    fr, ac, rw, ct = replay_data(64, hw, 3, seed=3)
    d.buffer.load_arrays(fr, ac, O.symlog(torch.tensor(rw)).numpy(), ct)
    eng = ImaginationEngine(d, world=world, use_graph=False)
    eng.starts.copy_(torch.arange(eng.B) % 32)
    return eng


def _epoch(eng, names):
    """One epoch, phase by phase (no collectives): [(phase name, entry points called)]."""
    out = []
    for name, body, _ in eng.phases():
        del names[:]
        body()
        out.append((name, list(names)))
    torch.cuda.synchronize()
    return out


def test_sequential_phases(gpu, monkeypatch):
    eng = _engine("small", gpu)
    assert not eng.heads_fused
    got = _epoch(eng, _trace(monkeypatch))
    assert got == list(SEQUENTIAL.items())


def test_data_parallel_update_is_the_single_gpu_update_in_two_phases(gpu, monkeypatch):
    """_ph_critic's claim: the kernel order of losses_and_grads(fork=False) without the BPTT, which follows as the
    second phase.  The collectives between the phases are not run."""
    monkeypatch.setenv("DREAMER_PERSISTENT", "0")  # (with the persistent BPTT the update stays one phase)
    eng = _engine("small", gpu, world=(0, 1, None))
    got = _epoch(eng, _trace(monkeypatch))
    assert [n for n, _ in got] == ["encwarm", "imagine", "returns", "critic", "actor", "optim"]
    ph = dict(got)
    assert ph["critic"] + ph["actor"] == UPDATE
    for n in ("encwarm", "imagine", "returns", "optim"):
        assert ph[n] == SEQUENTIAL[n]


def test_grouped_heads(gpu, monkeypatch):
    eng = _engine("full", gpu)
    assert eng.heads_fused
    got = _epoch(eng, _trace(monkeypatch))
    assert got == list(GROUPED.items())
    ph = dict(got)
    assert "dr_critic_fwd" not in ph["returns"] + ph["update"]


def test_forked_update_issues_the_same_launches(gpu, monkeypatch):
    """losses_and_grads(fork=True), the two-stream form the parity tests call: the launches of fork=False, the
    critic backward (side stream) issued before update_S."""
    eng = _engine("small", gpu)
    names = _trace(monkeypatch)
    for name, body, _ in eng.phases():
        if name == "update":
            del names[:]
            eng.losses_and_grads(fork=True)
            got = list(names)
        else:
            body()
    torch.cuda.synchronize()
    assert sorted(got) == sorted(UPDATE)
    assert got.index("dr_critic_loss_bwd") < got.index("dr_update_S")
