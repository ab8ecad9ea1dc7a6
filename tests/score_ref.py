"""A numpy model of threshold calibration (include/syldet.h, "threshold calibration"): one Python loop per threshold -- the flag
in double, the debounce loop of TrackDetector.swift:65-100, the class of every emitted detection -- and the generator of
synthetic outputs and labels the score tests share (test infrastructure)."""
import numpy as np

COLUMNS = 6     # detections, hits, false positives, repeats, sum of offsets, sum of squared offsets


def score(values, thresholds, labels, tolerance, first_index, hop, debounce_frames):
    """-> table [K, 6] int64 of one detector.  values: float32 [E]; labels: sorted sample numbers; all else Python ints."""
    values = np.asarray(values)
    assert values.dtype == np.float32 and values.ndim == 1
    v64 = values.astype(np.float64)
    labels = [int(t) for t in labels]
    m = int(tolerance)
    table = np.zeros((len(thresholds), COLUMNS), np.int64)
    for k, theta in enumerate(thresholds):
        with np.errstate(invalid="ignore"):
            fired = np.nonzero(v64 >= np.float64(theta))[0]          # NaN never fires
        until = -1
        hit = set()
        det = hits = stray = rep = s1 = s2 = 0
        for e in fired:
            idx = first_index + int(e) * hop
            if not until < idx:
                continue
            until = idx + debounce_frames
            det += 1
            j = _window(labels, m, idx)
            if j is None:
                stray += 1
            elif j in hit:
                rep += 1
            else:
                hit.add(j)
                hits += 1
                s1 += idx - labels[j]
                s2 += (idx - labels[j]) ** 2
        table[k] = (det, hits, stray, rep, s1, s2)
    return table


def _window(labels, m, idx):
    j = int(np.searchsorted(labels, idx - m))                        # the first label with t >= idx - m
    return j if j < len(labels) and labels[j] <= idx + m else None


def choose(tables, label_counts, cost):
    """-> (k, totals [K, 6], costs [K]): the tables summed over detectors, misses + cost (false positives + repeats), the lowest
    k of the smallest cost"""
    totals = np.asarray(tables, np.int64).reshape(len(label_counts), -1, COLUMNS).sum(axis=0)
    costs = (int(np.sum(label_counts)) - totals[:, 1]).astype(np.float64) + np.float64(cost) * (totals[:, 2] + totals[:, 3]).astype(np.float64)
    return int(np.argmin(costs)), totals, costs


def outputs(D, E, n_out, seed):
    rng = np.random.default_rng(seed)
    y = 0.05 + 0.25 * rng.random((D, E, n_out)); e = np.arange(E)
    for d in range(D):
        for o in range(n_out):
            for c in range(40, E + 3, 97):
                h, w = rng.uniform(0.2, 0.75), int(rng.integers(1, 5))
                y[d, np.abs(e - (c + int(rng.integers(-2, 3)))) < w, o] += h
            for c in rng.integers(0, E, size=E // 60 + 1):
                y[d, max(c - 1, 0):c + 2, o] += rng.uniform(0.1, 0.6)
    return y.astype(np.float32)


def labels(D, E, first_index, hop):
    """detector d: first_index + (40 + 97 j) hop + 17 (d + 1) for j < (E + 56) // 97; the last detector takes every second one"""
    out = []
    for d in range(D):
        t = [first_index + (40 + 97 * j) * hop + 17 * (d + 1) for j in range((E + 56) // 97)]
        out.append(np.asarray(t[::2] if d == D - 1 else t, np.int64))
    return out


def thresholds(K):
    return np.linspace(0.2, 1.0, K)


def debounces(hop):
    return [0, 2 * hop + 1, 9 * hop + 1]


def edge_values():
    """200 outputs that hold a value used as a threshold (three times), NaN (twice) and both infinities"""
    y = outputs(1, 200, 1, 7)[0, :, 0].copy()
    y[[5, 50, 120]] = np.float32(0.7)
    y[10], y[60], y[61], y[130] = np.nan, np.inf, -np.inf, np.nan
    return y


def edge_thresholds():
    """0.7f as a double and its neighbours in double, +-inf, beyond FLT_MAX on both sides, FLT_MAX itself"""
    x = np.float64(np.float32(0.7))
    return np.array([x, np.nextafter(x, 1.0), np.nextafter(x, 0.0), np.inf, -np.inf, 1e39, -1e39, 0.3, np.float64(np.finfo(np.float32).max)])
