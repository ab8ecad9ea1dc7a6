"""The numpy model of a bank of templates, written from the words of include/syldet.h ("template matching: a bank of templates") on
top of tests/match_ref.py: a class's score at a position is the greatest of its templates' scores there, the templates taken in
ascending k and the running value replaced only where the next is greater, so `which` is the lowest template of the class that
attains the maximum and -1 where the score is NaN; every class's tables are match_ref.tables of its own plane with its own
threshold."""
import numpy as np

import match_ref as ref


def class_table(classes, n_templates):
    """-> (class of each template int32 [K], C); None: template k is class k"""
    if classes is None:
        return np.arange(n_templates, dtype=np.int32), int(n_templates)
    c = np.asarray(classes, np.int32).reshape(-1)
    assert c.size == n_templates and sorted(set(c.tolist())) == list(range(int(c.max()) + 1))
    return c, int(c.max()) + 1


def classes(template_scores, classes=None):
    """template_scores [K, ...] float32 (any trailing shape) -> (class scores [C, ...] float32, which [C, ...] int32).  Comparisons
    only: a class score is one of its templates' scores, bit for bit."""
    s = np.asarray(template_scores, np.float32)
    cls, C = class_table(classes, s.shape[0])
    out = np.full((C,) + s.shape[1:], np.nan, np.float32)
    which = np.full((C,) + s.shape[1:], -1, np.int32)
    for k in range(s.shape[0]):                        # ascending k
        c = cls[k]
        with np.errstate(invalid="ignore"):
            take = np.where(which[c] < 0, ~np.isnan(s[k]), s[k] > out[c])
        out[c] = np.where(take, s[k], out[c])
        which[c] = np.where(take, k, which[c])
    return out, which


def scores(t_hats, cols, classes_=None):
    """One detector, float64: t_hats [K, n, bins], cols [U, bins] -> (class scores float64 [C, U], which [C, U])"""
    per = np.stack([ref.scores(t, cols)[0] for t in t_hats])
    cls, C = class_table(classes_, per.shape[0])
    out = np.full((C, per.shape[1]), np.nan)
    which = np.full((C, per.shape[1]), -1, np.int32)
    for k in range(per.shape[0]):
        c = cls[k]
        with np.errstate(invalid="ignore"):
            take = np.where(which[c] < 0, ~np.isnan(per[k]), per[k] > out[c])
        out[c] = np.where(take, per[k], out[c])
        which[c] = np.where(take, k, which[c])
    return out, which


def tables(class_scores, which, thresholds, separation, origin, hop, anchor, capacity):
    """one detector: class_scores [C, P] float32, which [C, P] or None -> a list with, a class, (events, count, event scores, event
    templates or None): match_ref.tables of the class's plane with the class's threshold; classes do not meet"""
    out = []
    for c in range(class_scores.shape[0]):
        ev, n, sc = ref.tables(class_scores[c], thresholds[c], separation, origin, hop, anchor, capacity)
        p = ref.peaks(class_scores[c], thresholds[c], separation)[:min(n, int(capacity))]
        out.append((ev, n, sc, None if which is None else np.asarray(which[c], np.int32)[p]))
    return out
