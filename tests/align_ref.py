"""The numpy model of event-aligned windows, written from the words of include/syldet.h ("event-aligned windows"), not from the
C++: an event s of a detector anchors at unit u0 = floor((s - origin) / step); its window is the units u0 - before .. u0 + after;
an element whose unit lies in [0, U_d) of its own detector is present and is the source's, every other one is the fill.  The stack
statistics add a group's events in blocks of 256 consecutive ones, each block one after another from +0.0, the blocks one after
another from +0.0.  Python integers throughout (events reach +-(2^62 - 1)); the windows are made unit by unit."""
import numpy as np

COLUMNS, OUTPUTS, SAMPLES = 0, 1, 2
BLOCK = 256


def clock(cfg):
    """(hop, need = gap + W, T, first_index) of a configuration"""
    W, T = cfg.windowLength, cfg.timeRange
    gap = max(0, -cfg.windowOverlap)
    hop = gap + W - max(0, cfg.windowOverlap)
    need = gap + W
    return hop, need, T, (T - 1) * hop + need


def count_frames(cfg, n):
    hop, need, _, _ = clock(cfg)
    return 0 if n < need else (n - need) // hop + 1


def count_evals(cfg, n):
    J, T = count_frames(cfg, n), cfg.timeRange
    return J - T + 1 if J >= T else 0


def anchor(cfg, source):
    """(origin, step) of a source"""
    hop, need, _, first_index = clock(cfg)
    return {COLUMNS: (need, hop), OUTPUTS: (first_index, hop), SAMPLES: (0, 1)}[source]


def units_of(cfg, source, n_samples):
    """a detector's units: the frames, evaluations or samples its n_samples samples yield"""
    return {COLUMNS: count_frames(cfg, n_samples), OUTPUTS: count_evals(cfg, n_samples), SAMPLES: n_samples}[source]


def _two_d(units):
    """[U] or [U, width] (also with U = 0) -> [U, width] float32"""
    units = np.asarray(units, np.float32)
    return units[:, None] if units.ndim == 1 else units


def _flat(present):
    m = np.asarray(present, bool)
    return m.reshape(m.shape[0], int(np.prod(m.shape[1:])))


def window_units(s, origin, step, before, after):
    u0 = (int(s) - int(origin)) // int(step)         # Python's // is a floor, also for a negative numerator
    return range(u0 - before, u0 + after + 1)


def windows(units, events, origin, step, before, after, fill):
    """One detector.  units [U, width] float32: the detector's own units.  -> (windows [n_events, n, width] float32, present
    [n_events, n, width] bool)."""
    units = _two_d(units)
    U, width = units.shape
    n = before + after + 1
    out = np.full((len(events), n, width), fill, np.float32)
    present = np.zeros((len(events), n, width), bool)
    for j, s in enumerate(events):
        for i, u in enumerate(window_units(s, origin, step, before, after)):
            if 0 <= u < U:
                out[j, i] = units[u]
                present[j, i] = True
    return out, present


def detector_units(array, source, slot, cfg):
    """The units of one packed recording out of the packed array: row slot.row, from unit slot.first_eval (COLUMNS, OUTPUTS) or
    sample slot.offset (SAMPLES), as many as the recording's own samples yield.  -> [U, width]"""
    row, offset, first_eval, _, n_samples = slot
    U = units_of(cfg, source, n_samples)
    first = offset if source == SAMPLES else first_eval
    return _two_d(array[row, first:first + U])


def windows_each(per_detector_units, events, origin, step, before, after, fill):
    """Every detector in turn, detector d's j-th event at event_begin[d] + j.  -> (windows [N, n, width], present, event_begin)"""
    parts, masks, begin = [], [], [0]
    for units, ev in zip(per_detector_units, events):
        w, m = windows(units, list(ev), origin, step, before, after, fill)
        parts.append(w)
        masks.append(m)
        begin.append(begin[-1] + len(ev))
    width = _two_d(per_detector_units[0]).shape[1] if len(per_detector_units) else 1
    n = before + after + 1
    if not parts:
        return np.zeros((0, n, width), np.float32), np.zeros((0, n, width), bool), np.array(begin, np.int64)
    return np.concatenate(parts), np.concatenate(masks), np.array(begin, np.int64)


def stats_one(windows_, present):
    """One stack, its events in order: (count int64, sum float64, sumsq float64), each of a window's shape."""
    w = np.asarray(windows_, np.float32)
    shape = w.shape[1:]
    L = int(np.prod(shape))
    x = w.reshape(w.shape[0], L).astype(np.float64)
    m = np.asarray(present, bool).reshape(w.shape[0], L)
    count = m.sum(axis=0).astype(np.int64) if len(x) else np.zeros(L, np.int64)
    total, squares = np.zeros(L), np.zeros(L)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, len(x), BLOCK):
            bs, bq = np.zeros(L), np.zeros(L)
            for i in range(i0, min(i0 + BLOCK, len(x))):
                v = x[i]
                # an absent element adds nothing (s + 0.0 is s: s is never -0.0, it began as +0.0)
                bs = bs + np.where(m[i], v, 0.0)
                bq = bq + np.where(m[i], v * v, 0.0)
            total = total + bs
            squares = squares + bq
    return count.reshape(shape), total.reshape(shape), squares.reshape(shape)


def stats(windows_, present, event_begin, group, n_groups):
    """Every group: its events ordered by detector ascending, then event index ascending.  -> count, sum, sumsq [G, ...]"""
    w = np.asarray(windows_, np.float32)
    out = [[], [], []]
    for g in range(n_groups):
        idx = [i for d in range(len(group)) if group[d] == g for i in range(int(event_begin[d]), int(event_begin[d + 1]))]
        c, s, q = stats_one(w[idx], np.asarray(present)[idx])
        if not idx:
            c, s, q = (np.zeros(w.shape[1:], t) for t in (np.int64, np.float64, np.float64))
        for lst, v in zip(out, (c, s, q)):
            lst.append(v)
    return tuple(np.stack(v) for v in out)


def present_pairs(present):
    """[N, n, width] bool -> [N, 2] int64: each window's first present element and the number of present elements (a window's
    present elements are contiguous)"""
    m = _flat(present)
    pairs = np.zeros((len(m), 2), np.int64)
    for i, row in enumerate(m):
        idx = np.nonzero(row)[0]
        if idx.size:
            assert idx[-1] - idx[0] + 1 == idx.size
            pairs[i] = (idx[0], idx.size)
    return pairs


def states(present):
    """How many windows are wholly present, clipped on the left only, on the right only, on both sides, wholly absent."""
    m = _flat(present)
    whole = m.all(axis=1)
    none = ~m.any(axis=1)
    left = ~m[:, 0] & ~none
    right = ~m[:, -1] & ~none
    return {"whole": int(whole.sum()), "left": int((left & ~right).sum()), "right": int((right & ~left).sum()),
            "both": int((left & right).sum()), "absent": int(none.sum())}


def same(got, want, what=""):
    """NaN at the same places, the same bits everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype.kind != "f":
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d differ, the first at %s: got %r, want %r" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at %s, wanted at %s" % (what, np.argwhere(gn != wn)[:4].tolist(), int(wn.sum()))
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.argwhere((got.view(bits) != want.view(bits)) & ~gn)
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %s: got %r, want %r" % (
        what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
