"""The numpy model of a ragged bank, written from the words of include/syldet.h ("template matching: a ragged bank") on top of
tests/match_ref.py and tests/match_bank_ref.py: template k has its own n_k frames and its own anchor a_k, the planes are indexed by
the ANCHOR frame -- element u of a detector of U frames holds template k's score of the window [u - a_k, u - a_k + n_k), which
exists iff 0 <= u - a_k and u - a_k + n_k <= U -- and a class's score is match_bank_ref.classes of its templates' shifted scores, a
NaN (no window, or a window that is not finite) never taken.  Every class's tables are match_ref.tables of its own plane with its
own threshold, its own separation and anchor 0."""
import numpy as np

import match_bank_ref as bref
import match_ref as ref


def anchors(lengths, anchor=None):
    """None: each template's last frame; one int: every template's; else one per template -> int array [K]"""
    n = np.asarray(lengths, np.int64).reshape(-1)
    if anchor is None:
        return n - 1
    a = np.asarray(anchor, np.int64).reshape(-1)
    a = np.full(n.size, a[0]) if a.size == 1 else a
    assert a.size == n.size and ((0 <= a) & (a < n)).all()
    return a


def to_anchor(s, n, a):
    """One detector's scores of one template indexed by the window's first frame, s [..., U] (position p at p, as the single
    matcher writes them) -> the same values indexed by the anchor frame: element u = p + a, NaN where no window exists."""
    s = np.asarray(s)
    U = s.shape[-1]
    out = np.full(s.shape, np.nan, s.dtype)
    P = U - int(n) + 1
    if P > 0:
        out[..., int(a):int(a) + P] = s[..., :P]
    return out


def classes(per_template, lengths, anchor=None, classes_=None):
    """per_template: a list with, a template, its single-matcher scores [..., U] float32 of ONE detector's frames (indexed by the
    window's first frame) -> (class planes [C, ..., U] float32, which [C, ..., U] int32) indexed by the anchor frame"""
    a = anchors(lengths, anchor)
    shifted = np.stack([to_anchor(np.asarray(s, np.float32), n, ak) for s, n, ak in zip(per_template, lengths, a)])
    return bref.classes(shifted, classes_)


def scores(t_hats, cols, anchor=None, classes_=None):
    """One detector, float64: t_hats a list of [n_k, bins], cols [U, bins] -> (class scores float64 [C, U], which [C, U], the
    templates' shifted scores [K, U]) indexed by the anchor frame"""
    lengths = [t.shape[0] for t in t_hats]
    a = anchors(lengths, anchor)
    per = np.stack([to_anchor(ref.scores(t, cols)[0], t.shape[0], ak) for t, ak in zip(t_hats, a)])
    cls, C = bref.class_table(classes_, per.shape[0])
    out = np.full((C, per.shape[1]), np.nan)
    which = np.full((C, per.shape[1]), -1, np.int32)
    for k in range(per.shape[0]):                       # ascending k, replaced only where greater
        c = cls[k]
        with np.errstate(invalid="ignore"):
            take = np.where(which[c] < 0, ~np.isnan(per[k]), per[k] > out[c])
        out[c] = np.where(take, per[k], out[c])
        which[c] = np.where(take, k, which[c])
    return out, which, per


def tables(class_scores, which, thresholds, separations, origin, hop, capacity):
    """one detector: class_scores [C, U] float32 -> a list with, a class, (events, count, event scores, event templates or None):
    the plane's index is the anchor frame, so the plane's own anchor is 0; separations: one, or one a class"""
    C = class_scores.shape[0]
    sep = np.asarray(separations).reshape(-1)
    sep = np.full(C, sep[0]) if sep.size == 1 else sep
    out = []
    for c in range(C):
        ev, n, sc = ref.tables(class_scores[c], thresholds[c], int(sep[c]), origin, hop, 0, capacity)
        p = ref.peaks(class_scores[c], thresholds[c], int(sep[c]))[:min(n, int(capacity))]
        out.append((ev, n, sc, None if which is None else np.asarray(which[c], np.int32)[p]))
    return out
