"""A ragged bank on the GPU (syldet_matcher_bank_create_ragged, syldet_match_bank_scores_device on its handle,
syldet_match_bank_peaks_each_device; include/syldet.h "template matching: a ragged bank").

No tolerance except in the one mixed case the header names: template k's plane of a ragged bank with identity classes has the bytes
of Matcher(template k).scores on the same columns shifted to the anchor index (the shipped single matcher, which
tests/test_match_gpu.py holds to the float64 model), NaN where no window exists; a class's plane the bytes of the model's ascending
maximum of those (tests/match_ragged_ref.py), `which` the model's; every class's event tables the bytes of syldet_match_peaks_host on
the downloaded plane with that class's threshold, that class's separation and anchor 0.  The kernel that ran and the number of
launches of a call are read from the profile.  The chain's threshold is the one tests/test_match_ragged_host.py fixed on the float64
model."""
import numpy as np
import pytest
import torch

import align_ref
import match_cases as mc
import match_ragged_cases as rc
import match_ragged_ref as rref
import match_ref as ref
import train_cases
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

TILE = 256
NAN, INF = np.float32(np.nan), np.float32(np.inf)
LENGTHS, CLASSES, ANCHORS = rc.LENGTHS, rc.CLASSES, rc.ANCHORS
_DETS = {}


def _det(bins, channels):
    key = (bins, channels)
    if key not in _DETS:
        cfg = {7: train_cases.small_net, 29: util.sample_net, 116: nets.config3}[bins]()
        assert cfg.geometry().bins == bins
        _DETS[key] = sd.SyllableDetector(cfg, channels=channels)
    return _DETS[key]


@pytest.fixture(scope="module", autouse=True)
def _detectors_closed_at_the_end():
    yield
    for d in _DETS.values():
        d.close()
    _DETS.clear()


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _columns(rng, J, bins, n=12):
    """three rows with NaN, Inf and all-zero windows where tests/test_match_bank_gpu.py places them for n = 12 -> (values [3, J, bins],
    the device tensor whose rows lie (J + 3) bins elements apart with NaN behind each)"""
    x = train_cases.columns(rng, J, bins, rows=3)
    if J >= 3 * n + 8:
        x[1, n + 2:2 * n + 4] = 0                                        # all-zero windows
        x[2, J - n - 1, bins - 1] = NAN
        x[2, n // 2, 0] = INF
    pad = np.full((3, J + 3, bins), NAN, np.float32)
    pad[:, :J] = x
    cols = torch.from_numpy(pad).cuda()[:, :J]
    assert J == 0 or cols.stride(0) > J * bins
    return x, cols


def _bank_scores(det, bank, cols, want_kernel):
    """scores and which into tensors with a sentinel behind each; the kernel's name, once, from the profile"""
    Cn, R, J = bank.nClasses, cols.shape[0], cols.shape[1]
    s_all = torch.full((Cn * R * J + 8,), 77.0, device="cuda")
    w_all = torch.full((Cn * R * J + 8,), 77, dtype=torch.int32, device="cuda")
    s, w = bank.scores(cols, which=True, out=(s_all[:Cn * R * J].view(Cn, R, J), w_all[:Cn * R * J].view(Cn, R, J)))
    torch.cuda.synchronize()
    assert (s_all[Cn * R * J:] == 77.0).all() and (w_all[Cn * R * J:] == 77).all()
    if J > 0:
        timings = det.lastTimings()
        assert [name for name, _ in timings] == [want_kernel], timings    # one call, one launch
    alone = bank.scores(cols)                                            # without which: the same scores
    assert _bytes(alone.cpu().numpy()) == _bytes(s.cpu().numpy())
    return s.cpu().numpy(), w.cpu().numpy()


def _single_planes(det, t, cols):
    """the shipped single matcher of every template on the same columns: a list of [rows, J], indexed by the window's first frame"""
    out = []
    for tk in t:
        with det.matcher(tk) as m:
            out.append(m.scores(cols).cpu().numpy())
    return out


def _shifted(per, lengths, anchor):
    a = rref.anchors(lengths, anchor)
    return np.stack([rref.to_anchor(s, n, ak) for s, n, ak in zip(per, lengths, a)])


# ---- 1. planes against the shipped single matchers ----
@pytest.mark.parametrize("anchor", [None, ANCHORS], ids=["last-frames", "anchors-0-3-16-4-0"])
@pytest.mark.parametrize("bins", [7, 29])
def test_a_ragged_banks_planes_have_the_shipped_matchers_bytes_at_the_anchor(bins, anchor):
    det = _det(bins, 3)
    rng = np.random.default_rng(9000 + bins)
    t = rc.random_templates(rng, LENGTHS, bins)
    a = rref.anchors(LENGTHS, anchor)
    kernel = "match_ragged_scores_mfma_kernel"
    with det.matcherBank(t, anchor=anchor) as ident, det.matcherBank(t, CLASSES, anchor) as bank:
        assert ident.ragged and bank.ragged and ident.shape == (3, 5, 5, 17, bins, 0) and bank.shape == (3, 5, 3, 17, bins, 0)
        assert ident.form == bank.form == "matrix"
        assert bank.lengths.tolist() == list(LENGTHS) and bank.anchors.tolist() == a.tolist() and bank.classes.tolist() == list(CLASSES)
        for k in range(5):
            with det.matcher(t[k]) as m:
                assert m.form == "matrix" and _bytes(bank.templates[k]) == _bytes(m.template) == _bytes(ident.templates[k])
        det.profile(True)
        holes = won = 0
        for J in (0, 11, 17, 257, 3 * TILE + 5):
            x, cols = _columns(rng, J, bins)
            per = _single_planes(det, t, cols)
            want = _shifted(per, LENGTHS, anchor)                         # [5, 3, J]
            s, w = _bank_scores(det, ident, cols, kernel)
            assert s.shape == (5, 3, J) and _bytes(s) == _bytes(want), (bins, J)
            assert ((w == -1) == np.isnan(want)).all() and ((w == np.arange(5)[:, None, None]) | np.isnan(want)).all()
            for k, n in enumerate(LENGTHS):                               # NaN on the first a_k and the last n_k - 1 - a_k elements
                lo, hi = min(int(a[k]), J), max(J - (n - 1 - int(a[k])), 0)
                assert np.isnan(s[k, :, :lo]).all() and np.isnan(s[k, :, hi:]).all()
                assert J < n or not np.isnan(s[k, 0, lo:hi]).any()
            if J == 17:
                assert (~np.isnan(s[2, 0])).sum() == 1 and not np.isnan(s[2, 0, int(a[2])])     # exactly one window
            want_s, want_w = rref.classes(per, LENGTHS, anchor, CLASSES)
            s, w = _bank_scores(det, bank, cols, kernel)
            assert s.shape == (3, 3, J) and _bytes(s) == _bytes(want_s) and _bytes(w) == _bytes(want_w), (bins, J)
            assert ((w == -1) == np.isnan(s)).all()
            holes += int((~np.isnan(s[0]) & np.isnan(want[[0, 1, 3]]).any(axis=0)).sum())
            if J >= 257:
                assert set(w[0][w[0] >= 0].tolist()) == {0, 1, 3}         # every exemplar of class 0 is the best somewhere
                won += 1
                zero = slice(int(a[4]) + 14, int(a[4]) + 17)              # row 1's frames 14 .. 27 are zero: three 12-frame windows
                assert (_bits(s[2, 1, zero]) == 0).all() and (w[2, 1, zero] == 4).all()
        det.profile(False)
        assert holes > 0 and won == 2      # a class is not NaN somewhere where one of its templates has no window or holds a NaN


# ---- 2. the plain form ----
def test_the_plain_form_has_the_plain_matchers_bytes():
    det = _det(116, 3)
    rng = np.random.default_rng(116)
    t = rc.random_templates(rng, LENGTHS, 116)
    with det.matcherBank(t, CLASSES, ANCHORS) as bank, det.matcherBank(t, anchor=ANCHORS) as ident:
        assert bank.ragged and bank.form == ident.form == "plain"
        det.profile(True)
        for J in (17, 257):
            x, cols = _columns(rng, J, 116)
            per = []
            for tk in t:
                with det.matcher(tk) as m:
                    assert m.form == "plain"
                    per.append(m.scores(cols).cpu().numpy())
            s, w = _bank_scores(det, ident, cols, "match_ragged_scores_plain_kernel")
            assert _bytes(s) == _bytes(_shifted(per, LENGTHS, ANCHORS)), J
            want_s, want_w = rref.classes(per, LENGTHS, ANCHORS, CLASSES)
            s, w = _bank_scores(det, bank, cols, "match_ragged_scores_plain_kernel")
            assert _bytes(s) == _bytes(want_s) and _bytes(w) == _bytes(want_w), J
        det.profile(False)


def test_a_mixed_bank_is_plain_and_its_short_template_stays_within_the_single_matchers_bound():
    """12 frames beside 100 at 29 bins: the bank's tile does not fit, so both templates take the plain form.  The 100-frame single
    matcher is plain too: bytes equal.  The 12-frame single matcher is matrix-form: its template's plane is held to the float64
    model within the bound tests/test_match_gpu.py uses for the single matcher, (1.5 M + 8) 2^-24 A / sqrt(E)."""
    det = _det(29, 3)
    rng = np.random.default_rng(12100)
    lengths = (12, 100)
    t = rc.random_templates(rng, lengths, 29)
    J = 257
    x, cols = _columns(rng, J, 29)
    with det.matcherBank(t) as bank, det.matcher(t[0]) as m0, det.matcher(t[1]) as m1:
        assert bank.ragged and bank.form == "plain" and m0.form == "matrix" and m1.form == "plain"
        det.profile(True)
        s, w = _bank_scores(det, bank, cols, "match_ragged_scores_plain_kernel")
        det.profile(False)
        assert _bytes(s[1]) == _bytes(rref.to_anchor(m1.scores(cols).cpu().numpy(), 100, 99))
        worst = 0.0
        for row in range(3):
            s64, A, E = (rref.to_anchor(v, 12, 11) for v in ref.scores(bank.templates[0], x[row]))
            got = s[0, row]
            assert np.array_equal(np.isnan(got), np.isnan(s64)), row
            ok = ~np.isnan(s64)
            zero = ok & (E == 0)
            assert (_bits(got[zero]) == 0).all()
            live = ok & ~zero
            err, bar = np.abs(got[live].astype(np.float64) - s64[live]), ref.bar(12, 29, A[live], E[live])
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (row, float((err / bar).max()))
        print("the 12-frame template in a plain ragged bank: max |s - s64| / bar = %.3f" % worst)


# ---- 3. equal lengths: the uniform bank, shifted ----
@pytest.mark.parametrize("a", [0, 11])
def test_an_equal_length_ragged_bank_is_the_uniform_bank_shifted(a):
    det, n, J = _det(29, 3), 12, 3 * TILE + 5
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    rng = np.random.default_rng(300 + a)
    t = (rng.standard_normal((5, n, 29)) * 2).astype(np.float32)
    x, cols = _columns(rng, J, 29)
    with det.matcherBank(t, CLASSES, anchor=a) as uni, det.matcherBank(list(t), CLASSES, anchor=a, ragged=True) as rag:
        assert not uni.ragged and rag.ragged and rag.shape == (3, 5, 3, n, 29, 0) and uni.shape == (3, 5, 3, n, 29, a)
        assert uni.lengths.tolist() == [n] * 5 and uni.anchors.tolist() == [a] * 5 == rag.anchors.tolist() and rag.lengths.tolist() == [n] * 5
        assert _bytes(np.stack(rag.templates)) == _bytes(uni.templates)
        su, wu = uni.scores(cols, which=True)
        sr, wr = rag.scores(cols, which=True)
        assert _bytes(sr.cpu().numpy()) == _bytes(rref.to_anchor(su.cpu().numpy(), n, a))
        shifted_w = np.full(wu.shape, -1, np.int32)
        shifted_w[..., a:a + J - n + 1] = wu.cpu().numpy()[..., :J - n + 1]
        assert _bytes(wr.cpu().numpy()) == _bytes(shifted_w)
        thr = [float(np.nanquantile(su[c].cpu().numpy(), q)) for c, q in enumerate((0.9, 0.97, 0.8))]
        tu = [v.cpu().numpy() for v in uni.peaks(su, thr, 12, capacity=32, which=wu)]
        tr = [v.cpu().numpy() for v in rag.peaks(sr, thr, 12, capacity=32, which=wr)]
        te = [v.cpu().numpy() for v in uni.peaks(su, thr, [12, 12, 12], capacity=32, which=wu)]      # _each on a uniform handle
        assert _bytes(tu[1]) == _bytes(tr[1]) == _bytes(te[1]) and tu[1].max() > 0
        for c in range(3):
            for d in range(3):
                k = min(int(tu[1][c, d]), 32)
                for table in (0, 2, 3):
                    assert _bytes(tu[table][c, d, :k]) == _bytes(tr[table][c, d, :k]) == _bytes(te[table][c, d, :k]), (a, c, d, table)
                assert ((tr[0][c, d, :k] - origin) % hop == 0).all()


# ---- 4. K = 64 ----
def test_sixty_four_templates_of_sixty_four_lengths():
    det, J = _det(7, 3), 257
    rng = np.random.default_rng(64)
    lengths = list(range(1, 65))
    classes = [k % 16 for k in range(64)]
    t = rc.random_templates(rng, lengths, 7)
    x, cols = _columns(rng, J, 7)
    per = _single_planes(det, t, cols)
    want_s, want_w = rref.classes(per, lengths, None, classes)
    det.profile(True)
    with det.matcherBank(t, classes) as bank:
        assert bank.ragged and bank.shape == (3, 64, 16, 64, 7, 0) and bank.form == "matrix"
        s, w = _bank_scores(det, bank, cols, "match_ragged_scores_mfma_kernel")
    det.profile(False)
    assert _bytes(s) == _bytes(want_s) and _bytes(w) == _bytes(want_w)
    assert len(set(w[w >= 0].tolist())) > 16


# ---- 5. packed recordings ----
def _frames_to_samples(f):
    return 100 if f == 0 else 256 + 132 * (f - 1)


@pytest.mark.parametrize("anchor", [None, ANCHORS], ids=["last-frames", "anchors-0-3-16-4-0"])
def test_a_packed_ragged_banks_planes_are_those_of_a_one_channel_handle(anchor):
    det, one = _det(29, 2), _det(29, 1)
    frames = [0, 1, 5, 16, 17, 300, 12, 700, 40]                         # shorter than the longest template (17); as long as the shortest (1)
    rec = det.recordings([_frames_to_samples(f) for f in frames])
    rng = np.random.default_rng(555)
    cols = [train_cases.columns(rng, f, 29) for f in frames]
    for k, c in enumerate(cols):                                         # the neighbours' border frames: huge and not finite
        if c.shape[0] >= 5 and k % 2:
            c[0] = np.float32(1e13)
            c[-1, 3] = NAN
        elif c.shape[0] >= 5:
            c[0, 1] = INF
            c[-1] = np.float32(3e12)
    where = []
    for k, (row, _, first, _, ns) in enumerate(rec.slots):
        assert det.countFrames(ns) == frames[k] or frames[k] == 0
        where.append((row, first))
    assert len({w[0] for w in where}) == 2
    J = det.countFrames(rec.rowSamples)
    t = rc.random_templates(rng, LENGTHS, 29)
    try:
        with one.matcherBank(t, CLASSES, anchor) as b1, rec.matcherBank(t, CLASSES, anchor) as bp:
            assert bp.ragged and bp.shape == (len(frames), 5, 3, 17, 29, 0) and bp.form == b1.form == "matrix"
            got = {}
            for name, outside in (("zeros", 0.0), ("NaN", NAN), ("1e30", np.float32(1e30))):
                a = np.full((2, J, 29), outside, np.float32)
                own = np.zeros((2, J), bool)
                for f, c, (row, first) in zip(frames, cols, where):
                    a[row, first:first + f] = c
                    own[row, first:first + f] = True
                assert (~own).sum() > 0
                s, w = bp.scores(torch.from_numpy(a).cuda(), which=True)
                got[name] = (s.cpu().numpy(), w.cpu().numpy())
            for name, (s, w) in got.items():
                assert _bytes(s) == _bytes(got["zeros"][0]) and _bytes(w) == _bytes(got["zeros"][1]), name
            s, w = got["zeros"]
            assert np.isnan(s[:, ~own]).all() and (w[:, ~own] == -1).all()    # everything outside recordings
            live = 0
            for k, (f, c, (row, first)) in enumerate(zip(frames, cols, where)):
                if f == 0:
                    continue
                s1, w1 = b1.scores(torch.from_numpy(c[None]).cuda(), which=True)
                assert _bytes(s[:, row, first:first + f]) == _bytes(s1.cpu().numpy()[:, 0]), (k, f)
                assert _bytes(w[:, row, first:first + f]) == _bytes(w1.cpu().numpy()[:, 0]), (k, f)
                live += int((~np.isnan(s[:, row, first:first + f])).sum())
                if f == 1:
                    assert w[0, row, first] == 0 and np.isnan(s[1:, row, first]).all()      # the 1-frame template alone fits
                if f == 16:
                    assert np.isnan(s[1, row, first:first + f]).all()                       # class 1 is the 17-frame template
            assert live > 1000
            # the packed bank's tables: each class the host's on its detectors' stretches
            origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
            thr, sep = [0.1, 0.0, 0.2], [0, 3, 40]
            ds, dw = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
            ev, cnt, es, et = (v.cpu().numpy() for v in bp.peaks(ds, thr, sep, capacity=16, which=dw))
            for c in range(3):
                for d, (f, (row, first)) in enumerate(zip(frames, where)):
                    e1, n1, s1 = sd.matchPeaksHost(s[c, row, first:first + f], thr[c], sep[c], origin, hop, 0, capacity=16)
                    assert cnt[c, d] == n1 and _bytes(ev[c, d, :len(e1)]) == _bytes(e1) and _bytes(es[c, d, :len(e1)]) == _bytes(s1), (c, d)
                    assert (et[c, d, :len(e1)] == w[c, row, first + (e1 - origin) // hop]).all()
            assert cnt[:, 0].max() == 0 and cnt[0, 7] > 16
            with pytest.raises(sd.SyllableDetectorError) as e:
                bp.scores(torch.zeros((2, J - 1, 29), device="cuda"))
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT
    finally:
        rec.close()


# ---- 6. peaks: a separation a class ----
def test_every_classs_tables_are_the_hosts_with_its_own_separation():
    det, J = _det(7, 3), 2048 + 300                                      # more than one step of the peaks kernel
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    rng = np.random.default_rng(606)
    t = rc.random_templates(rng, LENGTHS, 7)
    s = (rng.integers(0, 40, (3, 3, J)) / 40).astype(np.float32)        # few values: plateaus and ties
    s[rng.uniform(size=s.shape) < 0.05] = NAN
    s[:, :, :3] = NAN
    s[2, 1] = NAN                                                         # a detector without a score
    w = rng.integers(0, 5, s.shape).astype(np.int32)
    w[np.isnan(s)] = -1
    thr, sep, cap = [0.5, 0.6, -INF], [0, 3, 40], 200
    ds, dw = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
    det.profile(True)
    with det.matcherBank(t, CLASSES, ANCHORS) as bank:
        ev, cnt, es, et = bank.peaks(ds, thr, sep, capacity=cap, which=dw)
        torch.cuda.synchronize()
        timings = det.lastTimings()
        assert [name for name, _ in timings] == ["match_bank_peaks_each_kernel"], timings
        ev, cnt, es, et = ev.cpu().numpy(), cnt.cpu().numpy(), es.cpu().numpy(), et.cpu().numpy()
        assert ev.shape == (3, 3, cap) == es.shape == et.shape and cnt.shape == (3, 3)
        for c in range(3):
            for d in range(3):
                e1, n1, s1 = sd.matchPeaksHost(s[c, d], thr[c], sep[c], origin, hop, 0, capacity=cap)
                k = len(e1)
                assert cnt[c, d] == n1 and k == min(n1, cap), (c, d)
                assert _bytes(ev[c, d, :k]) == _bytes(e1) and _bytes(es[c, d, :k]) == _bytes(s1), (c, d)
                u = (ev[c, d, :k] - origin) // hop
                assert ((ev[c, d, :k] - origin) % hop == 0).all() and (np.diff(u) > 0).all() and (u >= 0).all() and (u < J).all()
                assert (et[c, d, :k] == w[c, d, u]).all() and (et[c, d, :k] >= 0).all()
        assert cnt[0].min() > cap and cnt[2, 1] == 0 and 0 < cnt[2, 0] <= cap and cnt[1].max() > cnt[2].max()
        # the shared separation on a ragged handle: the existing kernel, the same tables as _each with equal separations
        one = [v.cpu().numpy() for v in bank.peaks(ds, thr, 3, capacity=cap, which=dw)]
        torch.cuda.synchronize()
        assert [name for name, _ in det.lastTimings()] == ["match_bank_peaks_kernel"]
        each = [v.cpu().numpy() for v in bank.peaks(ds, thr, [3, 3, 3], capacity=cap, which=dw)]
        assert _bytes(one[1]) == _bytes(each[1]) and _bytes(one[1][1]) == _bytes(cnt[1])
        for c in range(3):
            for d in range(3):
                k = min(int(one[1][c, d]), cap)
                for table in (0, 2, 3):
                    assert _bytes(one[table][c, d, :k]) == _bytes(each[table][c, d, :k])
    det.profile(False)


# ---- 7. refusals on a device ----
def test_the_ragged_banks_refusals_on_a_device_leave_sentinels_in_place():
    det = _det(7, 3)
    good = [np.ones((3, 7), np.float32), np.ones((2, 7), np.float32) * 2]
    for bad in (dict(anchor=2), dict(anchor=[0, 2]), dict(anchor=[-1, 0]), dict(templates=[np.ones((3, 6), np.float32), np.ones((2, 6), np.float32)]),
                dict(templates=[good[0], np.zeros((2, 7), np.float32)]), dict(templates=[good[0], np.full((2, 7), NAN, np.float32)]),
                dict(templates=[good[0], np.ones((4682, 7), np.float32)]), dict(classes=[0, 2]), dict(classes=[1, 1]),
                dict(templates=[np.ones((1 + k % 3, 7), np.float32) for k in range(65)], classes=[0] * 65),
                dict(templates=[np.ones((1 + k % 3, 7), np.float32) for k in range(17)])):
        kw = dict(templates=good, classes=None, anchor=None)
        kw.update(bad)
        with pytest.raises(sd.SyllableDetectorError) as e:
            det.matcherBank(**kw)
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad
    with pytest.raises(ValueError):
        det.matcherBank(good, anchor=[0, 1, 1])
    with pytest.raises(ValueError):
        det.matcherBank([good[0], np.ones((2, 6), np.float32)])
    with pytest.raises(ValueError):
        det.matcherBank(np.ones((2, 3, 7), np.float32), ragged=True)
    with det.matcherBank(good, [1, 0], anchor=[2, 0]) as bank:
        assert bank.ragged and bank.shape == (3, 2, 2, 3, 7, 0) and bank.anchors.tolist() == [2, 0] and bank.lengths.tolist() == [3, 2]
        assert [tk.shape for tk in bank.templates] == [(3, 7), (2, 7)] and abs(float((bank.templates[1] ** 2).sum()) - 1) < 1e-6
        J = 40
        s = torch.full((2, 3, J), 77.0, device="cuda")
        w = torch.full((2, 3, J), 77, dtype=torch.int32, device="cuda")
        ev = torch.full((2, 3, 4), 77, dtype=torch.int64, device="cuda")
        cnt = torch.full((2, 3), 77, dtype=torch.int64, device="cuda")
        es = torch.full((2, 3, 4), 77.0, device="cuda")
        et = torch.full((2, 3, 4), 77, dtype=torch.int32, device="cuda")
        cols = torch.zeros((3, J, 7), device="cuda")
        thr = np.array([0.5, 0.5], np.float32)
        fp, ip = (lambda v: v.ctypes.data_as(_abi.c_float_p)), (lambda v: v.ctypes.data_as(_abi.c_int32_p))
        lib = _abi.lib
        assert lib.syldet_match_bank_scores_device(bank._h, cols.data_ptr(), -1, 0, s.data_ptr(), w.data_ptr(), None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.syldet_match_bank_scores_device(bank._h, cols.data_ptr(), J, J * 7 - 1, s.data_ptr(), w.data_ptr(), None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.syldet_match_bank_scores_device(bank._h, None, J, 0, s.data_ptr(), w.data_ptr(), None) == _abi.ERR_INVALID_ARGUMENT
        each = lambda thr_=fp(thr), sep_=ip(np.array([1, 2], np.int32)), cap=4, which=w.data_ptr(), J_=J: lib.syldet_match_bank_peaks_each_device(
            bank._h, s.data_ptr(), which, J_, thr_, sep_, ev.data_ptr(), cap, cnt.data_ptr(), es.data_ptr(), et.data_ptr(), None)
        for bad in (dict(sep_=None), dict(thr_=None), dict(sep_=ip(np.array([1, 4097], np.int32))), dict(sep_=ip(np.array([-1, 0], np.int32))),
                    dict(thr_=fp(np.array([0.5, NAN], np.float32))), dict(cap=-1), dict(which=None), dict(J_=-1)):
            assert each(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        torch.cuda.synchronize()
        for v in (s, w, ev, cnt, es, et):
            assert (v == 77).all()
        assert each() == 0                                                # ... and the call they were refusals of works
        torch.cuda.synchronize()
        assert (cnt.cpu().numpy() == 1).all()                             # (77.0 everywhere: of a plateau the earliest position matches)
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.matcherBank(object(), good)
    assert e.value.status == _abi.ERR_UNSUPPORTED


# ---- 8. the chain: two exemplars of different lengths -> MatcherBank.find -> Trainer.targets ----
def test_the_chain_from_exemplars_of_different_lengths_to_targets():
    cfg = train_cases.sample_wide(16, 4, "SatLin", "PureLin")
    origin, hop = align_ref.anchor(cfg, align_ref.COLUMNS)
    x = np.stack([mc.planted(seed)[0] for seed in mc.SEEDS])
    ex, anc = rc.exemplars()
    with sd.SyllableDetector(cfg, channels=2) as det:
        cols = det.spectrogram(torch.from_numpy(x).cuda())
        U = cols.shape[1]
        with det.matcherBank(ex, [0, 0], anchor=anc) as bank:
            assert bank.ragged and bank.form == "matrix" and bank.lengths.tolist() == [12, 10] and bank.anchors.tolist() == [11, 9]
            events, ev_scores, ev_templates = bank.find(cols, rc.THRESHOLD, rc.SEPARATION)
        assert len(events) == 1 and len(events[0]) == 2
        for d, seed in enumerate(mc.SEEDS):
            u = (events[0][d] - origin) // hop                           # the plane's index IS the anchor frame
            assert ((events[0][d] - origin) % hop == 0).all() and rc.found_once(u, mc.planted(seed)[1], U), (seed, u.tolist())
            assert (ev_scores[0][d] >= rc.THRESHOLD).all() and set(ev_templates[0][d].tolist()) <= {0, 1}
        assert set(np.concatenate(ev_templates[0]).tolist()) == {0, 1}    # each exemplar is the better one somewhere
        # the events, unchanged, are the labels of output 0
        E = det.countEvaluations(x.shape[1])
        first = align_ref.clock(cfg)[3]
        with det.trainer() as tr:
            tg, wt = tr.targets(events[0], 0, 1.0, 0.0, labelOutputs=[np.zeros(len(e), np.int32) for e in events[0]], n_evals=E)
            tg, wt = tg.cpu().numpy(), wt.cpu().numpy()
            for d in range(2):
                e = (events[0][d] - first) // hop
                assert ((events[0][d] - first) % hop == 0).all() and (e >= 0).all() and (e < E).all()
                assert (tg[d, e, 0] == 1).all() and (wt[d, e] == 1).all() and tg[d].sum() == len(e) == tg[d, :, 0].sum()
