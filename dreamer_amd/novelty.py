"""Novelty of replay windows: ``Dreamer.novelty`` and ``evaluate_novelty`` (explore = "disagreement").

A window b is S = sequence_length consecutive ring slots from starts[b].  The
posterior filter (warm_start_generator's, Dreamer.py:244-262, as closed_loop.py
runs it) gives a hidden state h_t per step; novelty[b][t] is the disagreement
of the ensemble's predictions on h_t (include/dreamer_hip.h, dr_disag_fwd):
high where the ensemble has seen too little data like it.  The front end is
replay_eval.py's.  The filter samples its posterior with the ad-hoc Philox
generator; numpy's state and that generator are put back before returning, so
a call never disturbs the training run (torch's generators are not drawn from)."""
import torch

from . import hip
from .replay_eval import check_window, preserved_rng, window_prologue


def novelty(dr, starts=None, batch_size=None, length=None):
    """(B, length) disagreement of the filter's hidden states; bit for bit
    dr.disagreement(dr.world_model.observe_sequence(frames, actions)[1]) on the
    same windows and draws."""
    ex = dr._explorer()
    S, A = dr.sequence_length, dr.action_dims
    T = S if length is None else int(length)
    check_window(1 <= T <= S, "novelty needs 1 <= length <= sequence_length", T, S)
    with preserved_rng(dr.device), torch.no_grad():
        w = window_prologue(dr, starts, batch_size, T, lambda B, dev: (None,), lambda name: None)
        hid = dr.world_model._observe_trace(w.d, w.B, T, w.feat, w.act.data_ptr(), S * A, A, None, None, None,
                                            heads=False, prior=False)[1]
        return ex.disagreement(hid)


def evaluate_novelty(dr, batches=1, batch_size=None, length=None):
    """{"novelty": per-step mean over `batches` batches of windows (CPU floats), "mean": their mean}."""
    dr._explorer()
    if int(batches) < 1:
        raise ValueError("evaluate_novelty needs batches >= 1")
    acc = None
    with preserved_rng(dr.device):
        for _ in range(int(batches)):
            # each batch draws fresh windows and fresh posterior samples; novelty() alone would put both back
            starts = dr.buffer.sample_start_indices(batch_size or dr.batch_size)
            cur = novelty(dr, starts=starts, length=length).mean(0)
            hip.adhoc(dr.device).noise()  # advance the ad-hoc stream id for the next batch
            acc = cur if acc is None else acc + cur
    curve = (acc / float(batches)).cpu()
    return {"novelty": curve.tolist(), "mean": float(curve.mean())}
