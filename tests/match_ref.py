"""The numpy model of template matching, written from the words of include/syldet.h ("template matching"), not from the C++: the
score of position p is the cosine between the n frames from p on and the normalised template t^, taken as given, in float64; a
window that holds a NaN or an Inf scores NaN, one that is all zero +0.0.  The matches are comparisons of float32 scores; the
events Python integers."""
import numpy as np

U24 = 2.0 ** -24


def normalise(template):
    """t^ = float32(t / ||t||_2), norm and division in float64"""
    t = np.asarray(template, np.float32).astype(np.float64)
    return (t / np.sqrt((t * t).sum())).astype(np.float32)


def scores(t_hat, cols):
    """One detector.  t_hat [n, bins] float32, cols [U, bins] float32 -> (s64 [U] float64 with NaN in the last n - 1 positions and
    wherever the window is not finite, A [U] = sum |t^ x|, E [U] = sum x^2; A and E NaN where s64 is)."""
    t = np.asarray(t_hat, np.float32).astype(np.float64)
    x = np.asarray(cols, np.float32).astype(np.float64)
    n, bins = t.shape
    U = x.shape[0]
    s, A, E = (np.full(U, np.nan) for _ in range(3))
    P = U - n + 1
    if P <= 0:
        return s, A, E
    w = np.lib.stride_tricks.sliding_window_view(x, (n, bins))[:, 0]          # [P, n, bins]
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(w).all(axis=(1, 2))
        wz = np.where(fin[:, None, None], w, 0.0)
        dot = (wz * t).sum(axis=(1, 2))
        a = np.abs(wz * t).sum(axis=(1, 2))
        e = (wz * wz).sum(axis=(1, 2))
        val = np.where(e > 0, dot / np.sqrt(np.where(e > 0, e, 1.0)), 0.0)
    s[:P] = np.where(fin, val, np.nan)
    A[:P] = np.where(fin, a, np.nan)
    E[:P] = np.where(fin, e, np.nan)
    return s, A, E


def bar(n, bins, A, E):
    """the derived bound on |s32 - s64|: (1.5 M + 8) 2^-24 A / sqrt(E), M = n bins"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (1.5 * n * bins + 8) * U24 * A / np.sqrt(E)


def peaks(s, threshold, separation):
    """s [P] float32: one detector's positions -> the matching positions, ascending.  p matches iff s[p] is not NaN, s[p] >=
    threshold, s[q] < s[p] for every non-NaN q in [p - S, p) and s[q] <= s[p] for every non-NaN q in (p, p + S]."""
    s = np.asarray(s, np.float32).reshape(-1)
    P, S = s.size, int(separation)
    ok = ~np.isnan(s) & (s >= np.float32(threshold))
    for k in range(1, min(S, P - 1) + 1):              # (a comparison with a NaN is False: it suppresses nothing)
        ok[k:] &= ~(s[:-k] >= s[k:])
        ok[:-k] &= ~(s[k:] > s[:-k])
    return np.flatnonzero(ok)


def events(positions, origin, hop, anchor):
    return [int(origin) + (int(p) + int(anchor)) * int(hop) for p in positions]


def tables(s, threshold, separation, origin, hop, anchor, capacity):
    """one detector's row of the event tables: (events int64 [min(count, capacity)], count, scores float32)"""
    s = np.asarray(s, np.float32).reshape(-1)
    p = peaks(s, threshold, separation)
    k = min(p.size, int(capacity))
    return np.array(events(p[:k], origin, hop, anchor), np.int64), int(p.size), s[p[:k]]


def detector_positions(first, units, n):
    """the elements of a row's scores that hold one detector's positions"""
    return slice(int(first), int(first) + max(int(units) - n + 1, 0))
