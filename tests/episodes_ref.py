"""Numpy reference of episode-aware replay (include/dreamer_hip.h, "episode-aware
replay"): the stops and spans of a ring (a loop per slot and a
vectorised form), the masked weights, draw and probabilities on replay_ref's
definitions, a generator of rings with breaks and the ring cases the host and
GPU tests share.  Written from the definitions, independently of the kernels."""
import numpy as np

import replay_ref as RR


def newest_slot(cap, size, next_idx):
    """The slot written last (-1: none)."""
    if size == 0:
        return -1
    return size - 1 if size < cap else (next_idx - 1 + cap) % cap


def is_stop(cont, first, size, next_idx, j):
    cap = len(cont)
    if not np.float32(cont[j]) >= np.float32(0.5):  # a NaN is a stop
        return True
    if j + 1 < cap and first is not None and first[j + 1] != 0:
        return True
    return j == cap - 1 or j == newest_slot(cap, size, next_idx)


def spans(cont, first, size, next_idx):
    """span[i] = j* - i + 1 with j* the least stop >= i; 0 for i >= size.  A loop per slot: the stops one by
    one from the definition, then each slot's own search for the first stop at or behind it."""
    cap = len(cont)
    stop = np.array([is_stop(cont, first, size, next_idx, j) for j in range(cap)])
    out = np.zeros(cap, dtype=np.int32)
    for i in range(min(size, cap)):
        out[i] = int(np.argmax(stop[i:])) + 1  # slot cap - 1 is a stop: the search always finds one
    return out


def stops_fast(cont, first, size, next_idx):
    cap = len(cont)
    with np.errstate(invalid="ignore"):
        stop = ~(np.asarray(cont, dtype=np.float32) >= np.float32(0.5))
    if first is not None:
        stop[:-1] |= np.asarray(first)[1:] != 0
    stop[cap - 1] = True
    n = newest_slot(cap, size, next_idx)
    if n >= 0:
        stop[n] = True
    return stop


def spans_fast(cont, first, size, next_idx):
    cap = len(cont)
    i = np.arange(cap, dtype=np.int64)
    at = np.where(stops_fast(cont, first, size, next_idx), i, cap)  # slot cap - 1 is a stop: never cap below
    nxt = np.minimum.accumulate(at[::-1])[::-1]
    return np.where(i < size, nxt - i + 1, 0).astype(np.int32)


def weights(priority, span, S, p_floor):
    """w_i = replay_ref's floored priority (None: 1.0) where span[i] >= S, else 0; float64."""
    cap = len(span)
    w = np.ones(cap) if priority is None else RR.weights(priority, cap, 0, 1, p_floor)  # (S = 1, full: all valid)
    return np.where(np.asarray(span) >= S, w, 0.0)


def probabilities(priority, span, S, p_floor):
    w = weights(priority, span, S, p_floor)
    return w / np.cumsum(w)[-1]


def sample(priority, span, S, p_floor, u):
    """replay_ref.sample on the masked weights: (starts, prob, margin)."""
    w = weights(priority, span, S, p_floor)
    C = np.cumsum(w)
    W = C[-1]
    assert W > 0.0, "no valid start"
    t = np.asarray(u, dtype=np.float64) * W
    idx = np.searchsorted(C, t, side="right")
    last = int(np.nonzero(w > 0.0)[0][-1])
    starts = np.where(idx >= len(w), last, idx).astype(np.int64)
    hi = np.abs(C[np.minimum(idx, len(w) - 1)] - t)
    lo = np.where(idx > 0, np.abs(t - C[np.maximum(idx - 1, 0)]), np.inf)
    assert np.all(w[starts] > 0.0)
    return starts, w[starts] / W, np.minimum(hi, lo) / W


def broken_ring(g, cap, S):
    """(continues f32 [cap], first u8 [cap]): episodes laid end to end, lengths drawn from {S/2, S, S+1, 3S,
    10S, 40S}; the break behind an episode is continue = 0 on its last slot with probability 0.7, otherwise a
    first flag on the next slot.  (Lengths over a third of the ring are left out, so a small ring has breaks.)"""
    cont, first = np.ones(cap, dtype=np.float32), np.zeros(cap, dtype=np.uint8)
    lengths = [n for n in (max(1, S // 2), S, S + 1, 3 * S, 10 * S, 40 * S) if n <= cap // 3]
    end = -1
    while True:
        end += int(lengths[g.randint(len(lengths))])
        if end >= cap - 1:
            return cont, first
        if g.uniform() < 0.7:
            cont[end] = 0.0
        else:
            first[end + 1] = 1


def log_uniform(g, n, lo=0.04, hi=1e5):
    return np.exp(g.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


# name: (cap, size, next_idx, S, B); the first has no break
GEOMETRIES = {
    "cap64_partial": (64, 40, 40, 8, 256),
    "cap64_full": (64, 64, 20, 8, 256),
    "cap1024": (1024, 1024, 1000, 16, 256),
    "cap1025": (1025, 1025, 0, 16, 256),
    "cap3000": (3000, 3000, 1500, 8, 1024),
    "cap5000_one_break": (5000, 5000, 1, 16, 256),
    "cap10007": (10007, 10007, 5000, 16, 256),
    "cap131072": (131072, 131072, 70000, 64, 4096),
    "chunk_edge_breaks": (2500, 2500, 1500, 8, 256),
    "nan_continue": (3000, 3000, 700, 8, 256),
    "size_below_S": (64, 5, 5, 8, 256),
}
NAMES = list(GEOMETRIES)
DRAWABLE = [n for n in NAMES if n != "size_below_S"]  # a valid start exists


def case(name, breaks=True):
    """dict(cap, size, next_idx, S, B, cont, first, pri, u) of one named ring; breaks=False: the same geometry
    with no break in the data."""
    cap, size, next_idx, S, B = GEOMETRIES[name]
    g = np.random.RandomState(1000 + NAMES.index(name))
    cont, first = np.ones(cap, dtype=np.float32), np.zeros(cap, dtype=np.uint8)
    if breaks and name == "cap5000_one_break":
        cont[4500] = 0.0  # slots 1 .. 4500 are one stream: a span of 4500 over four chunks
    elif breaks and name == "chunk_edge_breaks":
        first[1024] = 1  # ends slot 1023 from the first byte of the next chunk
        cont[1024] = 0.0
        cont[next_idx - 1] = 0.0
    elif breaks and name == "nan_continue":
        cont, first = broken_ring(g, cap, S)
        cont[1234] = np.nan
    elif breaks and name != "cap64_partial":
        cont, first = broken_ring(g, cap, S)
    return dict(cap=cap, size=size, next_idx=next_idx, S=S, B=B, cont=cont, first=first,
                pri=log_uniform(g, cap), u=g.uniform(size=B))
