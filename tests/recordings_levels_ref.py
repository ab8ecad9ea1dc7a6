"""The level meters of packed recordings (syldet_recordings_levels_device*, syldet_recordings_output_levels_device) in numpy:
levels_ref.py applied to each recording alone, laid out by the prefix of syldet_recordings_levels_layout.  slots[k] = (row,
offset, first_eval, n_evals, n_samples), as recordings_ref.plan makes them."""
import numpy as np

import levels_ref


def layout(slots, L, P):
    """reading_first [K + 1]: recording k's readings are elements [first[k], first[k + 1]); a recording without samples has none"""
    first = np.zeros(len(slots) + 1, np.int64)
    for k, s in enumerate(slots):
        first[k + 1] = first[k] + levels_ref.levels_count(s[4], L, P)
    return first


def own_samples(slots, rows, k):
    """recording k's samples out of the packed rows [C, >= row_samples]"""
    row, offset, _, _, n = slots[k]
    return rows[row, offset:offset + n]


def input_each(slots, rows, L, P):
    """rows as the load wrote them (float32, or int16 meaning x / 32768) -> the flat table of mean squares, float64"""
    first = layout(slots, L, P)
    out = np.zeros(int(first[-1]), np.float64)
    for k in range(len(slots)):
        x = own_samples(slots, rows, k)
        if x.dtype == np.int16:
            x = x.astype(np.float32) * np.float32(1.0 / 32768.0)
        out[first[k]:first[k + 1]] = levels_ref.input_readings(x, L, P)
    return out


def output_each(slots, outputs, output, L, P, clock):
    """outputs [C, row_evals, n_out] of the packed run -> the flat table of output levels, float32.  clock: (window, overlap,
    timeRange) as levels_ref.count_evals takes them"""
    first = layout(slots, L, P)
    out = np.zeros(int(first[-1]), np.float32)
    for k, (row, _, first_eval, n_evals, n) in enumerate(slots):
        if n > 0:
            out[first[k]:first[k + 1]] = levels_ref.output_readings(outputs[row, first_eval:first_eval + n_evals], output, n, L, P, clock)[0]
    return out
