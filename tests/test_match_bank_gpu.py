"""A bank of templates on the GPU (syldet_match_bank_scores_device, syldet_match_bank_peaks_device; include/syldet.h "template
matching: a bank of templates").

No tolerance anywhere: template k's plane of a bank with identity classes has the bytes of Matcher(template k).scores on the same
columns (the shipped single matcher, which tests/test_match_gpu.py holds to the float64 model), a class's plane the bytes of the
model's ascending maximum of those single-matcher outputs (tests/match_bank_ref.py), `which` the model's with -1 exactly on the NaN
positions, and every class's event tables the bytes of Matcher.peaks on that plane with that class's threshold.  The form that ran
and the number of kernels a call launched are read from the profile.  The chain's threshold is the one
tests/test_match_bank_host.py fixed on the float64 model."""
import numpy as np
import pytest
import torch

import align_ref
import match_bank_cases as bc
import match_bank_ref as bref
import match_cases as mc
import train_cases
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

TILE = 256
NAN, INF = np.float32(np.nan), np.float32(np.inf)
CLASSES = (0, 0, 1, 0, 2)
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


def _columns(rng, J, n, bins):
    """three rows with NaN, Inf and all-zero windows where tests/test_match_gpu.py places them -> (values [3, J, bins], the device
    tensor whose rows lie (J + 3) bins elements apart with NaN behind each)"""
    x = train_cases.columns(rng, J, bins, rows=3)
    if J >= 3 * n + 8:
        x[1, n + 2:2 * n + 4] = 0                                        # three all-zero windows
        x[2, J - n - 1, bins - 1] = NAN
        x[2, n // 2, 0] = INF
    pad = np.full((3, J + 3, bins), NAN, np.float32)
    pad[:, :J] = x
    cols = torch.from_numpy(pad).cuda()[:, :J]
    assert J == 0 or cols.stride(0) > J * bins
    return x, cols


def _bank_scores(det, bank, cols, want_kernel):
    """scores and which into tensors with a sentinel behind each; the kernel's name from the profile"""
    Cn, R, J = bank.nClasses, cols.shape[0], cols.shape[1]
    s_all = torch.full((Cn * R * J + 8,), 77.0, device="cuda")
    w_all = torch.full((Cn * R * J + 8,), 77, dtype=torch.int32, device="cuda")
    s, w = bank.scores(cols, which=True, out=(s_all[:Cn * R * J].view(Cn, R, J), w_all[:Cn * R * J].view(Cn, R, J)))
    torch.cuda.synchronize()
    assert (s_all[Cn * R * J:] == 77.0).all() and (w_all[Cn * R * J:] == 77).all()
    if J > 0:
        timings = det.lastTimings()
        assert [name for name, _ in timings] == [want_kernel], timings
    alone = bank.scores(cols)                                            # without which: the same scores
    assert _bytes(alone.cpu().numpy()) == _bytes(s.cpu().numpy())
    return s.cpu().numpy(), w.cpu().numpy()


@pytest.mark.parametrize("n", [1, 12, 17])
@pytest.mark.parametrize("bins", [7, 29, 116])
def test_a_banks_planes_have_the_shipped_matchers_bytes(bins, n):
    det = _det(bins, 3)
    rng = np.random.default_rng(7000 + 100 * bins + n)
    t = bc.random_templates(rng, 5, n, bins)
    form = "plain" if bins == 116 else "matrix"
    kernel = "match_bank_scores_%s_kernel" % ("plain" if bins == 116 else "mfma")
    singles = [det.matcher(t[k]) for k in range(5)]
    try:
        with det.matcherBank(t) as ident, det.matcherBank(t, CLASSES) as bank:
            assert ident.shape == (3, 5, 5, n, bins, n - 1) and bank.shape == (3, 5, 3, n, bins, n - 1)
            assert ident.form == bank.form == singles[0].form == form
            assert bank.classes.tolist() == list(CLASSES) and ident.classes.tolist() == [0, 1, 2, 3, 4]
            for k in range(5):
                assert _bytes(bank.templates[k]) == _bytes(singles[k].template) == _bytes(ident.templates[k])
            det.profile(True)
            for J in (n - 1, n, 257, 3 * TILE + 5):
                x, cols = _columns(rng, J, n, bins)
                per = np.stack([m.scores(cols).cpu().numpy() for m in singles])                  # [5, 3, J]: the shipped matcher
                s, w = _bank_scores(det, ident, cols, kernel)
                assert s.shape == (5, 3, J) and _bytes(s) == _bytes(per), (bins, n, J)
                assert ((w == np.arange(5)[:, None, None]) | np.isnan(per)).all() and ((w == -1) == np.isnan(per)).all()
                want_s, want_w = bref.classes(per, CLASSES)
                s, w = _bank_scores(det, bank, cols, kernel)
                assert s.shape == (3, 3, J) and _bytes(s) == _bytes(want_s), (bins, n, J)
                assert _bytes(w) == _bytes(want_w) and ((w == -1) == np.isnan(per[0])[None]).all()
                assert (np.isnan(per) == np.isnan(per[0])).all()                                # NaN for every template or for none
                if J >= 3 * n + 8:
                    zero = slice(n + 2, n + 5)
                    assert (s[:, 1, zero].view(np.uint32) == 0).all() and (w[0, 1, zero] == 0).all() and (w[2, 1, zero] == 4).all()
                    assert np.isnan(s[:, 2, J - 2 * n:J - n]).all() and np.isnan(s[:, 2, :n // 2 + 1]).all()
                    assert len(set(w[0][w[0] >= 0].tolist())) == 3                              # every exemplar of class 0 is the best somewhere
                assert np.isnan(s[:, :, max(J - n + 1, 0):]).all()
            det.profile(False)
    finally:
        for m in singles:
            m.close()


@pytest.mark.parametrize("K", [1, 64])
def test_one_template_and_sixty_four(K):
    det, n, J = _det(29, 3), 12, 257
    rng = np.random.default_rng(K)
    t = bc.random_templates(rng, K, n, 29)
    classes = None if K == 1 else [k % 16 for k in range(K)]
    x, cols = _columns(rng, J, n, 29)
    per = []
    for k in range(K):
        with det.matcher(t[k]) as m:
            per.append(m.scores(cols).cpu().numpy())
    per = np.stack(per)
    want_s, want_w = bref.classes(per, classes)
    det.profile(True)
    with det.matcherBank(t, classes) as bank:
        assert bank.shape == (3, K, 1 if K == 1 else 16, n, 29, n - 1)
        s, w = _bank_scores(det, bank, cols, "match_bank_scores_mfma_kernel")
    det.profile(False)
    assert _bytes(s) == _bytes(want_s) and _bytes(w) == _bytes(want_w)
    if K == 64:
        assert len(set(w[w >= 0].tolist())) > 16


def test_a_tie_goes_to_the_lower_template():
    det, n, J = _det(29, 3), 12, 3 * TILE + 5
    rng = np.random.default_rng(13)
    t = bc.random_templates(rng, 5, n, 29)
    t[3] = t[1]
    classes = [0, 1, 0, 1, 1]
    x, cols = _columns(rng, J, n, 29)
    with det.matcherBank(t, classes) as bank, det.matcher(t[1]) as m1:
        s, w = bank.scores(cols, which=True)
        s, w = s.cpu().numpy(), w.cpu().numpy()
        one = m1.scores(cols).cpu().numpy()
    assert not (w == 3).any() and (w[1] == 1).sum() > 100 and (w[1] == 4).sum() > 100
    at = w[1] == 1
    assert _bytes(s[1][at]) == _bytes(one[at])


# ---- the packed plan: 7 recordings on 2 rows (as tests/test_match_gpu.py builds it) ----
def _frames_to_samples(f):
    return 100 if f == 0 else 256 + 132 * (f - 1)


def _plan(n):
    det = _det(29, 2)
    frames = [0, 5, n, n + 1, 300, 40 + n, 700]
    rec = det.recordings([_frames_to_samples(f) for f in frames])
    rng = np.random.default_rng(50 + n)
    cols = [train_cases.columns(rng, f, 29) for f in frames]
    where = []
    for k, (row, _, first, _, ns) in enumerate(rec.slots):
        assert det.countFrames(ns) == frames[k] or frames[k] == 0
        where.append((row, first))
    assert len({w[0] for w in where}) == 2
    return det, rec, frames, cols, where


def _packed(det, rec, frames, cols, where, outside):
    J = det.countFrames(rec.rowSamples)
    a = np.full((2, J, 29), outside, np.float32)
    own = np.zeros((2, J), bool)
    for f, c, (row, first) in zip(frames, cols, where):
        a[row, first:first + f] = c
        own[row, first:first + f] = True
    assert (~own).sum() > 0                                              # there are frames between recordings or behind them
    return a


@pytest.mark.parametrize("n", [12, 91])
def test_a_packed_banks_planes_are_those_of_a_one_channel_handle(n):
    det, rec, frames, cols, where = _plan(n)
    one = _det(29, 1)
    rng = np.random.default_rng(n)
    t = bc.random_templates(rng, 5, n, 29)
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    try:
        with one.matcherBank(t, CLASSES) as b1, rec.matcherBank(t, CLASSES) as bp, rec.matcher(t[2]) as single:
            assert bp.shape == (7, 5, 3, n, 29, n - 1) and b1.form == bp.form == "matrix"
            s4, w4 = b1.scores(torch.from_numpy(cols[4][None]).cuda(), which=True)
            s4, w4 = s4.cpu().numpy()[:, 0], w4.cpu().numpy()[:, 0]
            got = {}
            for name, outside in (("zeros", 0.0), ("NaN", NAN), ("1e30", np.float32(1e30))):
                a = torch.from_numpy(_packed(det, rec, frames, cols, where, outside)).cuda()
                s, w = bp.scores(a, which=True)
                got[name] = (s.cpu().numpy(), w.cpu().numpy())
            row, first = where[4]
            for name, (s, w) in got.items():
                assert _bytes(s[:, row, first:first + frames[4]]) == _bytes(s4), name
                assert _bytes(w[:, row, first:first + frames[4]]) == _bytes(w4), name
                assert _bytes(s) == _bytes(got["zeros"][0]) and _bytes(w) == _bytes(got["zeros"][1]), name
            s, w = got["zeros"]
            J = s.shape[2]
            mine = np.zeros((2, J), bool)
            for f, (r, fi) in zip(frames, where):
                mine[r, fi:fi + max(f - n + 1, 0)] = True
            assert (np.isnan(s) == ~mine[None]).all() and ((w == -1) == ~mine[None]).all()
            # class 1 is template 2 alone: the packed single matcher's plane
            assert _bytes(s[1]) == _bytes(single.scores(torch.from_numpy(_packed(det, rec, frames, cols, where, 0.0)).cuda()).cpu().numpy())
            # the packed bank's tables: each class the single matcher's on that plane
            thr = [float(np.nanquantile(s[c], q)) for c, q in enumerate((0.5, 0.7, 0.6))]
            ds, dw = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
            ev, cnt, es, et = (a.cpu().numpy() for a in bp.peaks(ds, thr, 12, capacity=64, which=dw))
            for c in range(3):
                e1, c1, s1 = (a.cpu().numpy() for a in single.peaks(ds[c].contiguous(), thr[c], 12, capacity=64))
                assert _bytes(cnt[c]) == _bytes(c1) and cnt[c][0] == 0 and cnt[c][6] > 3
                for d in range(7):
                    k = min(int(c1[d]), 64)
                    assert _bytes(ev[c, d, :k]) == _bytes(e1[d, :k]) and _bytes(es[c, d, :k]) == _bytes(s1[d, :k])
                    p = (ev[c, d, :k] - origin) // hop - (n - 1)
                    assert (et[c, d, :k] == w[c, where[d][0], where[d][1] + p]).all()
            with pytest.raises(sd.SyllableDetectorError) as e:
                bp.scores(torch.zeros((2, J - 1, 29), device="cuda"))
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT
    finally:
        rec.close()


# ---- peaks ----
@pytest.mark.parametrize("S", [0, 1, 12, 4096])
def test_every_classs_tables_are_the_single_matchers_on_its_plane(S):
    det, n, J = _det(7, 3), 3, 2048 + 300                                # more than one step of the peaks kernel
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    rng = np.random.default_rng(100 + S)
    t = bc.random_templates(rng, 5, n, 7)
    s = (rng.integers(0, 40, (3, 3, J)) / 40).astype(np.float32)        # few values: plateaus and ties
    s[rng.uniform(size=s.shape) < 0.05] = NAN
    s[:, :, J - n + 1:] = NAN
    s[2, 1] = NAN                                                         # a detector without a score
    w = rng.integers(0, 5, s.shape).astype(np.int32)
    w[np.isnan(s)] = -1
    thr = [0.9, 0.5, -INF]                                                # a threshold a class
    ds, dw = torch.from_numpy(s).cuda(), torch.from_numpy(w).cuda()
    det.profile(True)
    with det.matcherBank(t, CLASSES, anchor=1) as bank, det.matcher(t[0], anchor=1) as single:
        want = [[a.cpu().numpy() for a in single.peaks(ds[c], thr[c], S, capacity=J)] for c in range(3)]
        most = max(int(x[1].max()) for x in want)
        assert most >= 1
        for cap in (most - 1, most + 3):                                  # below the largest count (0 at S = 4096); above every count
            want = [[a.cpu().numpy() for a in single.peaks(ds[c], thr[c], S, capacity=cap)] for c in range(3)]
            ev, cnt, es, et = bank.peaks(ds, thr, S, capacity=cap, which=dw)
            torch.cuda.synchronize()
            timings = det.lastTimings()
            assert [name for name, _ in timings] == ["match_bank_peaks_kernel"], timings
            ev, cnt, es, et = ev.cpu().numpy(), cnt.cpu().numpy(), es.cpu().numpy(), et.cpu().numpy()
            assert ev.shape == (3, 3, cap) and cnt.shape == (3, 3) and es.shape == ev.shape == et.shape
            for c in range(3):
                e1, c1, s1 = want[c]
                assert _bytes(cnt[c]) == _bytes(c1), (S, cap, c)
                for d in range(3):
                    k = min(int(c1[d]), cap)
                    assert _bytes(ev[c, d, :k]) == _bytes(e1[d, :k]) and _bytes(es[c, d, :k]) == _bytes(s1[d, :k]), (S, cap, c, d)
                    p = (ev[c, d, :k] - origin) // hop - 1
                    assert ((ev[c, d, :k] - origin) % hop == 0).all() and (et[c, d, :k] == w[c, d, p]).all() and (et[c, d, :k] >= 0).all()
            assert cnt[2, 1] == 0 and (cnt.max() > cap) == (cap < most)
        # a scalar threshold is every class's; without which there are no event templates, and none may be asked for
        ev, cnt, es, et = bank.peaks(ds, 0.5, S, capacity=8, withScores=False)
        assert es is None and et is None
        assert _bytes(cnt.cpu().numpy()) == _bytes(np.stack([single.peaks(ds[c], 0.5, S, capacity=8)[1].cpu().numpy() for c in range(3)]))
        table = torch.zeros((3, 3, 8), dtype=torch.int32, device="cuda")
        st = _abi.lib.syldet_match_bank_peaks_device(bank._h, ds.data_ptr(), None, J, np.array(thr, np.float32).ctypes.data_as(_abi.c_float_p), S,
                                                     ev.data_ptr(), 8, cnt.data_ptr(), None, table.data_ptr(), None)
        assert st == _abi.ERR_INVALID_ARGUMENT
        for bad in (dict(thresholds=[0.5, float("nan"), 0.5]), dict(separation=-1), dict(separation=4097), dict(capacity=-1)):
            kw = dict(thresholds=thr, separation=1, capacity=4)
            kw.update(bad)
            with pytest.raises(sd.SyllableDetectorError) as e:
                bank.peaks(ds, **kw)
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad
        with pytest.raises(ValueError):
            bank.peaks(ds, [0.5, 0.5], 1)
    det.profile(False)


def test_the_banks_refusals_on_a_device():
    det = _det(7, 3)
    t = np.ones((3, 2, 7), np.float32)
    t[1] *= 2
    for bad in (dict(anchor=2), dict(templates=np.ones((3, 2, 6), np.float32)), dict(templates=np.zeros((3, 2, 7), np.float32)),
                dict(templates=np.concatenate([t[:2], np.zeros((1, 2, 7), np.float32)])), dict(templates=np.full((3, 2, 7), NAN, np.float32)),
                dict(templates=np.ones((65, 2, 7), np.float32), classes=[0] * 65), dict(templates=np.ones((17, 2, 7), np.float32)),
                dict(classes=[0, 2, 0]), dict(classes=[0, -1, 1]), dict(templates=np.ones((1, 4682, 7), np.float32))):
        kw = dict(templates=t, classes=None, anchor=None)
        kw.update(bad)
        with pytest.raises(sd.SyllableDetectorError) as e:
            det.matcherBank(**kw)
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad
    with pytest.raises(ValueError):
        det.matcherBank(t[0])
    with det.matcherBank(t, [1, 0, 1], anchor=0) as bank:
        assert bank.shape == (3, 3, 2, 2, 7, 0) and bank.classes.tolist() == [1, 0, 1]
        assert _bytes(bank.templates[0]) == _bytes(bank.templates[1])    # each normalised on its own
        s = bank.scores(torch.zeros((3, 0, 7), device="cuda"))
        assert tuple(s.shape) == (2, 3, 0)
        with pytest.raises(ValueError):
            bank.scores(torch.zeros((3, 5, 6), device="cuda"))


# ---- the chain: two exemplars -> MatcherBank.find -> Trainer.targets ----
def test_the_chain_from_a_class_of_exemplars_to_targets():
    cfg = train_cases.sample_wide(16, 4, "SatLin", "PureLin")
    origin, hop = align_ref.anchor(cfg, align_ref.COLUMNS)
    x = np.stack([mc.planted(seed)[0] for seed in mc.SEEDS])
    n = mc.N
    # class 0: one exemplar (seed 5's second syllable); class 1: the two exemplars whose threshold the host test fixed
    t = np.concatenate([bc.exemplar_of(5)[None], bc.exemplars()])
    with sd.SyllableDetector(cfg, channels=2) as det:
        cols = det.spectrogram(torch.from_numpy(x).cuda())
        P = cols.shape[1] - n + 1
        with det.matcherBank(t, [0, 1, 1]) as bank:
            assert bank.form == "matrix"
            events, ev_scores, ev_templates = bank.find(cols, bc.THRESHOLD, bc.SEPARATION)
        assert len(events) == 2 and len(events[1]) == 2
        for d, seed in enumerate(mc.SEEDS):
            p = (events[1][d] - origin) // hop - (n - 1)
            assert ((events[1][d] - origin) % hop == 0).all() and mc.found_once(p, mc.planted(seed)[1], P), (seed, p.tolist())
            assert (ev_scores[1][d] >= bc.THRESHOLD).all() and set(ev_templates[1][d].tolist()) <= {1, 2} and (ev_templates[0][d] == 0).all()
            assert len(events[0][d]) > 0
        # a class's events, unchanged, are the labels of that class's output
        E = det.countEvaluations(x.shape[1])
        first = align_ref.clock(cfg)[3]
        with det.trainer() as tr:
            for c in range(2):
                tg, wt = tr.targets(events[c], 0, 1.0, 0.0, labelOutputs=[np.full(len(e), c, np.int32) for e in events[c]], n_evals=E)
                tg, wt = tg.cpu().numpy(), wt.cpu().numpy()
                for d in range(2):
                    e = (events[c][d] - first) // hop
                    assert ((events[c][d] - first) % hop == 0).all() and (e >= 0).all() and (e < E).all()
                    assert (tg[d, e, c] == 1).all() and (wt[d, e] == 1).all() and tg[d].sum() == len(e) == tg[d, :, c].sum()


def test_one_call_is_one_launch():
    det, n, J = _det(29, 3), 12, 600
    rng = np.random.default_rng(5)
    t = bc.random_templates(rng, 5, n, 29)
    x, cols = _columns(rng, J, n, 29)
    det.profile(True)
    with det.matcherBank(t, CLASSES) as bank:
        s, w = bank.scores(cols, which=True)
        torch.cuda.synchronize()
        assert [name for name, _ in det.lastTimings()] == ["match_bank_scores_mfma_kernel"]
        bank.peaks(s, [0.1, 0.2, 0.3], 12, which=w)
        torch.cuda.synchronize()
        assert [name for name, _ in det.lastTimings()] == ["match_bank_peaks_kernel"]
    det.profile(False)
