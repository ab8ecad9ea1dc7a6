"""A numpy model of packed recordings (include/syldet.h, "packed recordings"): the plan, the laid-out rows, and the events of
one recording -- the debounce loop of TrackDetector.swift:65-100 over that recording's own flags (test infrastructure)."""
import numpy as np


def clock(cfg):
    """(hop, need, T, first_index) of a configuration: need = gap + W samples make the first frame."""
    g = cfg.geometry()
    return int(g.hop), int(g.gap) + int(cfg.windowLength), int(cfg.timeRange), int(g.first_index)


def count_evals(S, hop, need, T):
    J = 0 if S < need else (S - need) // hop + 1
    return J - T + 1 if J >= T else 0


def plan(lengths, hop, need, T, C, channel_net=None, networks=None):
    """-> (slots [(row, offset, first_eval, n_evals, n_samples)] in the caller's order, row_samples, row_evals, fill)"""
    lengths = [int(n) for n in lengths]
    K = len(lengths)
    padded = [-(-n // hop) * hop for n in lengths]
    order = sorted(range(K), key=lambda k: (-padded[k], k))
    fills = [0] * C
    slots = [None] * K
    for k in order:
        rows = [c for c in range(C) if channel_net is None or channel_net[c] == networks[k]]
        row = min(rows, key=lambda c: (fills[c], c))
        slots[k] = (row, fills[row], fills[row] // hop, count_evals(lengths[k], hop, need, T), lengths[k])
        fills[row] += padded[k]
    row_samples = -(-(max(fills) if K else 0) // 8) * 8
    fill = sum(lengths) / (C * row_samples) if row_samples else 0.0
    return slots, row_samples, count_evals(row_samples, hop, need, T), fill


def rows(slots, row_samples, C, src, offsets, steps, sentinel=None, stride=None):
    """The rows the load call leaves: [C, stride] of src's dtype, `sentinel` where it must not write (beyond row_samples)."""
    stride = row_samples if stride is None else stride
    out = np.zeros((C, stride), src.dtype)
    if sentinel is not None:
        out[:, row_samples:] = sentinel
    for (row, offset, _, _, n), o, s in zip(slots, offsets, steps):
        out[row, offset:offset + n] = src[o:o + n * s:s][:n]
    return out


def events(flags, first_index, hop, debounce_frames):
    """-> (sample numbers, evaluations) of one recording's detections; flags: that recording's own, from its evaluation 0."""
    until = -1
    idx, ev = [], []
    for e in np.nonzero(np.asarray(flags))[0]:
        cur = first_index + int(e) * hop
        if until < cur:
            idx.append(cur)
            ev.append(int(e))
            until = cur + debounce_frames
    return np.asarray(idx, np.int64), np.asarray(ev, np.int64)
