"""Novelty of replay windows: ``Dreamer.novelty`` and ``evaluate_novelty`` (explore = "disagreement" or "entropy"),
and the k-nearest-neighbour read-outs ``Dreamer.knn`` / ``Dreamer.state_entropy`` (every mode).

A window b is S = sequence_length consecutive ring slots from starts[b].  The
posterior filter (warm_start_generator's, Dreamer.py:244-262, as closed_loop.py
runs it) gives a hidden state h_t per step; novelty[b][t] is the disagreement
of the ensemble's predictions on h_t (include/dreamer_hip.h, dr_disag_fwd):
high where the ensemble has seen too little data like it.  The front end is
replay_eval.py's.  The filter samples its posterior with the ad-hoc Philox
generator; numpy's state and that generator are put back before returning, so
a call never disturbs the training run (torch's generators are not drawn from).
With explore = "entropy" novelty[b][t] is the particle-entropy reward of h_t
among the B * length hidden states of the batch (dr_state_entropy_fwd, a state
never its own neighbour)."""
import torch

from . import _lib as L
from . import hip
from .replay_eval import check_window, preserved_rng, window_prologue


def novelty(dr, starts=None, batch_size=None, length=None):
    """(B, length) disagreement of the filter's hidden states; bit for bit
    dr.disagreement(dr.world_model.observe_sequence(frames, actions)[1]) on the
    same windows and draws."""
    ex = None if dr.explore == "entropy" and not dr._exploring() else dr._explorer()
    S, A = dr.sequence_length, dr.action_dims
    T = S if length is None else int(length)
    check_window(1 <= T <= S, "novelty needs 1 <= length <= sequence_length", T, S)
    with preserved_rng(dr.device), torch.no_grad():
        w = window_prologue(dr, starts, batch_size, T, lambda B, dev: (None,), lambda name: None)
        hid = dr.world_model._observe_trace(w.d, w.B, T, w.feat, w.act.data_ptr(), S * A, A, None, None, None,
                                            heads=False, prior=False)[1]
        return state_entropy(hid, dr.explore_knn) if ex is None else ex.disagreement(hid)


def evaluate_novelty(dr, batches=1, batch_size=None, length=None):
    """{"novelty": per-step mean over `batches` batches of windows (CPU floats), "mean": their mean}."""
    if dr.explore != "entropy" or dr._exploring():
        dr._explorer()
    if int(batches) < 1:
        raise ValueError("evaluate_novelty needs batches >= 1")
    acc = None
    with preserved_rng(dr.device):
        for _ in range(int(batches)):
            # each batch draws fresh windows and fresh posterior samples; novelty() alone would put both back
            starts = dr.buffer.sample_eval_starts(batch_size or dr.batch_size)
            cur = novelty(dr, starts=starts, length=length).mean(0)
            hip.adhoc(dr.device).noise()  # advance the ad-hoc stream id for the next batch
            acc = cur if acc is None else acc + cur
    curve = (acc / float(batches)).cpu()
    return {"novelty": curve.tolist(), "mean": float(curve.mean())}


def _rows(t, name, dtype=torch.float32):
    L.require_gpu(t)
    if t.dim() < 1 or t.shape[-1] < 1:
        raise ValueError(f"{name} must be a (..., D) tensor")
    return t.detach().to(dtype).reshape(-1, t.shape[-1]).contiguous()


def _groups(g, like, name):
    if g is None:
        return None
    L.require_gpu(g)
    if tuple(g.shape) != tuple(like.shape[:-1]):
        raise ValueError(f"{name} must have the rows' shape {tuple(like.shape[:-1])}, got {tuple(g.shape)}")
    return g.detach().to(torch.int32).reshape(-1).contiguous()


def _check_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= L.DR_KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1..{L.DR_KNN_MAX_K}, got {k!r}")


def knn(queries, bank=None, k=12, query_groups=None, bank_groups=None):
    """dr_knn on any device tensors (..., D): (dist (..., k) Euclidean, idx (..., k) int32 rows of the flattened
    bank).  bank = None: the queries among themselves with group = row index (no groups may be given then)."""
    _check_k(k)
    q = _rows(queries, "queries")
    if bank is None:
        if query_groups is not None or bank_groups is not None:
            raise ValueError("groups need a bank: with bank = None every row is its own group")
        b = q
        qg = bg = torch.arange(q.shape[0], dtype=torch.int32, device=q.device)
    else:
        b = _rows(bank, "bank")
        if b.shape[1] != q.shape[1]:
            raise ValueError(f"queries and bank differ in width: {q.shape[1]} vs {b.shape[1]}")
        qg, bg = _groups(query_groups, queries, "query_groups"), _groups(bank_groups, bank, "bank_groups")
    Mq, D = q.shape
    Nb = b.shape[0]
    if Mq < 1 or Nb < 1:
        raise ValueError("knn needs at least one query row and one bank row")
    d2 = torch.empty(Mq, k, device=q.device)
    idx = torch.empty(Mq, k, dtype=torch.int32, device=q.device)
    n = L.query("dr_knn_workspace_bytes", Mq, Nb, D, k)
    ws = hip.workspace(q.device).get("knn", n)
    L.call("dr_knn", D, k, Mq, L.ptr(q), D, L.ptr(qg), Nb, L.ptr(b), D, L.ptr(bg), L.ptr(d2), L.ptr(idx), L.ptr(ws),
           ws.numel(), hip.stream())
    lead = tuple(queries.shape[:-1])
    return d2.sqrt_().view(*lead, k), idx.view(*lead, k)


def state_entropy(hidden, k=12):
    """dr_state_entropy_fwd of the rows of a (..., D) device tensor among themselves (group = row index) -> (...)."""
    _check_k(k)
    h = _rows(hidden, "hidden")
    M, D = h.shape
    g = torch.arange(M, dtype=torch.int32, device=h.device)
    ent = torch.empty(M, device=h.device)
    n = L.query("dr_knn_workspace_bytes", M, M, D, k)
    ws = hip.workspace(h.device).get("knn", n)
    L.call("dr_state_entropy_fwd", D, k, M, L.ptr(h), D, L.ptr(g), M, L.ptr(h), D, L.ptr(g), None, None, L.ptr(ent),
           None, 0, 0, 0, 0, 0.0, 0.0, L.ptr(ws), ws.numel(), hip.stream())
    return ent.view(tuple(hidden.shape[:-1]))
