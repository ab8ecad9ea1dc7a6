"""The Simulator's output track (SyllableDetector/ViewControllerSimulator.swift:251-344) restated in numpy, twice: the closed
form the library's header states, and the reference's buffer-by-buffer loop (nextCount / nextValue) as its witness."""
import numpy as np


def geometry(window, overlap, time_range):
    """-> (D, hop, gap): the Simulator's nextCount (:251-254), its hold length windowLength - windowOverlap (:331), the gap"""
    D = window + (window - overlap) * (time_range - 1)
    if overlap < 0:
        D -= overlap
    return D, window - overlap, (-overlap if overlap < 0 else 0)


def count_evals(n_samples, window, overlap, time_range):
    """syldet_count_evals: frames J = (S - gap - W) / hop + 1, evaluations J - T + 1"""
    _, hop, gap = geometry(window, overlap, time_range)
    if n_samples < gap + window:
        return 0
    return max(0, (n_samples - gap - window) // hop + 1 - time_range + 1)


def values(outputs, thr, k=0):
    """v[e] = clamp01(out[e][k] / Float(thr[k])): an fp32 division, then the reference's two comparisons (:322-328)"""
    o = np.asarray(outputs, np.float32)[..., k]
    t = np.float32(np.asarray(thr, np.float64).reshape(-1)[k])            # Float(Double)
    with np.errstate(all="ignore"):
        q = (o / t).astype(np.float32)
        return np.where(q > 1, np.float32(1), np.where(q < 0, np.float32(0), q)).astype(np.float32)


def closed_form(outputs, thr, D, hop, n_samples, k=0):
    """outputs [n_evals, n_out] of one channel, thr [n_out] (Double) -> trace [n_samples] float32:
    0 for s < D, v[(s - D) / hop] for D <= s < D + n_evals hop, 0 beyond"""
    v = values(outputs, thr, k)
    s = np.arange(n_samples, dtype=np.int64)
    e = (s - D) // hop
    live = (s >= D) & (e < len(v))
    tr = np.zeros(n_samples, np.float32)
    tr[live] = v[e[live]]
    return tr


def closed_form_bank(outputs, thresholds, D, hop, n_samples, k=0):
    """outputs [C, n_evals, n_out]; thresholds: one list for every channel, or one per channel"""
    C = outputs.shape[0]
    per = thresholds if np.ndim(thresholds[0]) else [thresholds] * C
    return np.stack([closed_form(outputs[c], per[c], D, hop, n_samples, k) for c in range(C)]) if C else np.zeros((0, n_samples), np.float32)


def to_s16(v):
    """the library's 16-bit form: rint(v * 32767) in fp32, ties to even, NaN -> 0"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.rint(v * np.float32(32767))
    return np.where(np.isnan(v), np.float32(0), q).astype(np.int16)


def simulator_loop(v, window, overlap, time_range, n_samples, rng, max_buffer=3000):
    """The reference's loop over sample buffers of random sizes (:283-344): the leading nextCount samples of nextValue, then
    for every evaluation that processNewValue has (the rule of syldet_count_evals on what was fed so far) windowLength -
    windowOverlap samples of its value, a hold cut by a buffer's end carried over in nextCount / nextValue.  v: the clamped
    values of the evaluations in order.  Samples no branch writes stay NaN."""
    next_count, _, _ = geometry(window, overlap, time_range)
    next_value = np.float32(0)
    out = np.full(n_samples, np.nan, np.float32)
    fed = done = 0
    while fed < n_samples:
        n = int(min(n_samples - fed, rng.integers(1, max_buffer)))
        buf = np.full(n, np.nan, np.float32)
        fed += n                                                    # processSampleBuffer: the detector has the buffer now
        i = 0
        while 0 < next_count and i < n:
            buf[i] = next_value
            i += 1
            next_count -= 1
        while next_count == 0:
            if done >= count_evals(fed, window, overlap, time_range):   # processNewValue() == false
                break
            value = v[done]
            done += 1
            left = window - overlap
            while 0 < left and i < n:
                buf[i] = value
                i += 1
                left -= 1
            if 0 < left:
                next_count, next_value = left, value
                break
        out[fed - n:fed] = buf
    return out
