"""Packed recordings' per-sample tracks in numpy (syldet_recordings_trace_device*, syldet_recordings_trigger*_device* of
include/syldet.h): per recording, the models of the calls for one recording -- trace_ref.closed_form / to_s16,
trigger_ref.closed_form and trigger_ref.onsets -- on the recording's own slice of the packed results, then scattered to
dst[offset[k] + i step[k]].  Nothing of a neighbour enters: the slice is [first_eval, first_eval + n_evals) of the recording's row."""
import numpy as np

import trace_ref
import trigger_ref


def own(slots, results, k):
    """recording k's part of packed results [C, row_evals, ...]"""
    row, _, first, n_evals, _ = slots[k]
    return np.asarray(results)[row, first:first + n_evals]


def layout(slots, steps=None, align=8):
    """Recordings.trackLayout: the recordings end to end in the caller's order, each from a multiple of `align` elements"""
    steps = [1] * len(slots) if steps is None else steps
    offsets, pos = [], 0
    for s, step in zip(slots, steps):
        pos = (pos + align - 1) // align * align
        offsets.append(pos)
        pos += (s[4] - 1) * step + 1 if s[4] > 0 else 0
    return np.asarray(offsets, np.int64), pos


def scatter(dst, per_recording, offsets, steps=None):
    """dst[offsets[k] + i steps[k]] = per_recording[k][i]; returns dst and the mask of the elements some recording owns"""
    owned = np.zeros(dst.size, bool)
    for k, x in enumerate(per_recording):
        step = 1 if steps is None else int(steps[k])
        at = int(offsets[k]) + np.arange(len(x), dtype=np.int64) * step
        dst[at] = x
        owned[at] = True
    return dst, owned


def trace_each(slots, outputs, thresholds_of_row, D, hop, k_out=0, s16=False):
    """-> one array a recording: trace_ref.closed_form of its own outputs over its own n_samples, by its row's thresholds"""
    out = []
    for k, s in enumerate(slots):
        tr = trace_ref.closed_form(own(slots, outputs, k), thresholds_of_row[s[0]], D, hop, s[4], k_out)
        out.append(trace_ref.to_s16(tr) if s16 else tr)
    return out


def trigger_each(slots, flags, D, hop, L, N, latency, s16=False):
    """-> one array a recording: trigger_ref.closed_form of its own flags, cut at its own n_samples"""
    out = []
    for k, s in enumerate(slots):
        t = trigger_ref.closed_form(own(slots, flags, k), D, hop, L, N, latency, s[4])
        out.append(trigger_ref.as_s16(t) if s16 else trigger_ref.as_f32(t))
    return out


def onsets_each(slots, flags, D, hop, L, N, latency):
    return [trigger_ref.onsets(own(slots, flags, k), D, hop, L, N, latency, s[4]) for k, s in enumerate(slots)]
