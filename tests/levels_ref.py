"""The two level meters of a ProcessorBase row (SyllableDetector/Processor.swift:111-113, :138, :158-184; SummaryStat.swift's
StatMax) restated in numpy, twice: the closed forms include/syldet.h states, and a literal replay -- a loop over callback
buffers, evaluations and timer reads -- as their witness.  The sum of squares is the library's own convention
(sum_squares_tree: vDSP_svesq's order is not specified)."""
import numpy as np


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def sum_squares_tree(x):
    """every square rounded to fp32 on its own; the squares added as a balanced binary tree in index order over next_pow2(n)
    slots, the slots past n holding +0; every addition rounded to fp32 (numpy's float32 arithmetic: no contraction)"""
    x = np.asarray(x, np.float32).reshape(-1)
    a = np.zeros(next_pow2(max(len(x), 1)), np.float32)
    with np.errstate(all="ignore"):
        a[:len(x)] = x * x
        while len(a) > 1:
            a = a[0::2] + a[1::2]
    return np.float32(a[0])


def sum_squares_sequential(x):
    s = np.float32(0)
    with np.errstate(all="ignore"):
        for v in np.asarray(x, np.float32).reshape(-1):
            s = np.float32(s + np.float32(v * v))
    return s


def sum_squares_tree_rows(rows):
    """sum_squares_tree of every row of [n, L] (L a power of two), at once"""
    a = np.asarray(rows, np.float32)
    with np.errstate(all="ignore"):
        a = a * a
        while a.shape[1] > 1:
            a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def stat_max(values):
    """StatMax, literally: the first value as it is, a later one only if it is greater; None if nothing was written"""
    cur = None
    for v in values:
        if cur is None:
            cur = v
        elif v > cur:
            cur = v
    return cur


def stat_max_closed(values):
    """the closed form: NaN if the first value is NaN, else the first of the greatest values that are not NaN"""
    v = np.asarray(values)
    if len(v) == 0:
        return None
    if np.isnan(v[0]):
        return v[0]
    live = v[~np.isnan(v)]
    return live[np.argmax(live)]


def geometry(window, overlap, time_range):
    """-> (gap, hop): CircularShortTimeFourierTransform.swift:66-73"""
    return (-overlap if overlap < 0 else 0), window - overlap


def count_evals(n_samples, window, overlap, time_range):
    """syldet_count_evals: frames J = (S - gap - W) / hop + 1, evaluations J - T + 1"""
    gap, hop = geometry(window, overlap, time_range)
    if n_samples < gap + window:
        return 0
    return max(0, (n_samples - gap - window) // hop + 1 - time_range + 1)


def levels_count(S, L, P):
    B = -(-S // L)
    return -(-B // P)


def buffer_mean_squares(samples, L):
    """Double(sum_squares_tree(buffer)) / Double(length) of every buffer of L samples; the last one may be short"""
    x = np.asarray(samples, np.float32).reshape(-1)
    S = len(x)
    B = -(-S // L)
    if B == 0:
        return np.zeros(0, np.float64)
    padded = np.zeros(B * L, np.float32)
    padded[:S] = x                                   # (padding to a longer power of two gives the same bits)
    sums = sum_squares_tree_rows(padded.reshape(B, L))
    length = np.full(B, L, np.float64)
    length[-1] = S - (B - 1) * L
    with np.errstate(all="ignore"):
        return sums.astype(np.float64) / length


def input_readings(samples, L, P):
    """in_ms [M] float64: the StatMax of the mean squares of the P buffers of every reading"""
    ms = buffer_mean_squares(samples, L)
    if len(ms) == 0:
        return ms
    P = min(P, len(ms))
    M = -(-len(ms) // P)
    # vectorised closed form: the groups' first values, and the greatest of the values that are not NaN (never negative)
    grid = np.full(M * P, np.nan)
    grid[:len(ms)] = ms
    grid = grid.reshape(M, P)
    first = grid[:, 0]
    best = np.where(np.isnan(grid), -1.0, grid).max(axis=1)
    return np.where(np.isnan(first), first, best)


def eval_ranges(S, n_evals, L, P, clock):
    """[(first, count)] of the evaluations of every reading: an evaluation belongs to the buffer whose arrival makes it available"""
    B = -(-S // L)
    if B == 0:
        return []
    P = min(P, B)
    M = -(-B // P)
    cut = [min(count_evals(min(m * P * L, S), *clock), n_evals) for m in range(M + 1)]
    return [(cut[m], cut[m + 1] - cut[m]) for m in range(M)]


def output_readings(outputs, k, S, L, P, clock, n_evals=None):
    """outputs [n_evals, n_out] of one channel -> (levels [M] float32, empty [M] bool): the StatMax of out[e][k] over every
    reading's evaluations, 0 for a reading without one"""
    o = np.asarray(outputs, np.float32)
    n_evals = len(o) if n_evals is None else n_evals
    rng = eval_ranges(S, n_evals, L, P, clock)
    lv = np.zeros(len(rng), np.float32)
    empty = np.zeros(len(rng), bool)
    for m, (first, count) in enumerate(rng):
        if count == 0:
            empty[m] = True
        else:
            lv[m] = stat_max_closed(o[first:first + count, k])
    return lv, empty


def replay(samples, L, P, clock, outputs=None, k=0):
    """The application, literally: callback buffers of L samples (the last one short) arrive one by one; each writes
    Double(sum) / Double(length) to the input statistic (Processor.swift:111-113) and then every evaluation processNewValue
    now has (syldet_count_evals of what was fed so far) writes Double(out[e][k]) to the output statistic (:136-138); the timer
    reads and resets both after every P buffers, and once more at the end if buffers remain.
    -> (input readings: mean squares or None, output readings: float64 or None)"""
    x = np.asarray(samples, np.float32).reshape(-1)
    S = len(x)
    stat_in, stat_out = [], []
    read_in, read_out = [], []
    fed = done = since = 0
    while fed < S:
        n = min(L, S - fed)
        with np.errstate(all="ignore"):
            stat_in.append(np.float64(sum_squares_tree(x[fed:fed + n])) / np.float64(n))
        fed += n
        if outputs is not None:
            have = min(count_evals(fed, *clock), len(outputs))
            while done < have:
                stat_out.append(np.float64(np.float32(outputs[done][k])))
                done += 1
        since += 1
        if since == P or fed == S:
            read_in.append(stat_max(stat_in))
            read_out.append(stat_max(stat_out))
            stat_in, stat_out, since = [], [], 0
    return read_in, read_out
