"""Template matching on the GPU (syldet_match_scores_device, syldet_match_peaks_device; include/syldet.h "template matching").

Scores: every position within (1.5 M + 8) 2^-24 A / sqrt(E) of the float64 model of tests/match_ref.py (M = n bins, A = sum |t^ x|;
the bar is derived: M rounded products in any order are within M u A, the energy within M u E and so M u / 2 behind the root, three
more roundings and second order in the 8), NaN exactly where the convention has it, +0.0 exactly on all-zero windows -- for 7, 29
and 116 bins, n in {1, 3, 12, 16, 17, 91}, rows of n - 1 to three tiles + 5 frames, three rows with a stride above the minimum,
templates with negative values and columns over six decades; the form that ran is read from the profile's kernel name.  Position
independence and "nothing outside a window is read": bit identity.  Peaks: the device's tables equal the model on the device's own
scores to the last element.  The chain: exemplar -> Matcher.find -> Aligner.windows / Trainer.targets."""
import numpy as np
import pytest
import torch

import align_ref
import match_cases as mc
import match_ref as ref
import train_cases
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets
from test_match_host import peak_cases

pytestmark = pytest.mark.gpu

TILE = 256
NAN, INF = np.float32(np.nan), np.float32(np.inf)
_DETS = {}


def _config(bins):
    return {7: train_cases.small_net, 29: util.sample_net, 116: nets.config3}[bins]()


def _det(bins, channels):
    key = (bins, channels)
    if key not in _DETS:
        cfg = _config(bins)
        assert cfg.geometry().bins == bins
        _DETS[key] = sd.SyllableDetector(cfg, channels=channels)
    return _DETS[key]


@pytest.fixture(scope="module", autouse=True)
def _detectors_closed_at_the_end():
    yield
    for d in _DETS.values():
        d.close()
    _DETS.clear()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_scores(got, t_hat, cols, what):
    """one detector: got [U] float32 against the model of cols [U, bins]; -> the largest error over its bar"""
    n, bins = t_hat.shape
    s, A, E = ref.scores(t_hat, cols)
    assert np.array_equal(np.isnan(got), np.isnan(s)), what
    ok = ~np.isnan(s)
    zero = ok & (E == 0)
    assert (_bits(got[zero]) == 0).all(), what                           # +0.0
    live = ok & ~zero
    if not live.any():
        return 0.0
    err, bar = np.abs(got[live].astype(np.float64) - s[live]), ref.bar(n, bins, A[live], E[live])
    print("%s: max |s - s64| / bar = %.3f over %d positions" % (what, float((err / bar).max()), int(live.sum())))
    assert (err <= bar).all(), (what, float((err / bar).max()))
    return float((err / bar).max())


@pytest.mark.parametrize("n", [1, 3, 12, 16, 17, 91])
@pytest.mark.parametrize("bins", [7, 29, 116])
def test_scores_lie_within_the_derived_bar_of_the_float64_model(bins, n):
    det = _det(bins, 3)
    rng = np.random.default_rng(1000 * bins + n)
    t = (rng.standard_normal((n, bins)) * 2).astype(np.float32)
    assert (t < 0).any() or n * bins < 4
    with det.matcher(t) as m:
        assert m.shape == (3, n, bins, n - 1) and m.template.tobytes() == ref.normalise(t).tobytes()
        assert m.form == ("plain" if bins == 116 else "matrix")          # (116 bins: the staged tile is above 64 KB of LDS)
        det.profile(True)
        for J in (n - 1, n, n + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
            x = train_cases.columns(rng, J, bins, rows=3)
            if J >= 3 * n + 8:
                x[1, n + 2:2 * n + 4] = 0                                # three all-zero windows
                x[2, J - n - 1, bins - 1] = NAN
                x[2, n // 2, 0] = INF
            pad = np.full((3, J + 3, bins), NAN, np.float32)             # rows (J + 3) bins elements apart, NaN behind each row
            pad[:, :J] = x
            cols = torch.from_numpy(pad).cuda()[:, :J]
            assert J == 0 or cols.stride(0) > J * bins
            sentinel = torch.full((3 * J + 8,), 77.0, device="cuda")
            out = sentinel[:3 * J].view(3, J)
            got = m.scores(cols, out=out)
            torch.cuda.synchronize()
            assert (sentinel[3 * J:] == 77.0).all()
            got = got.cpu().numpy()
            if J > 0:
                name = det.lastTimings()[0][0]
                assert name == ("match_scores_plain_kernel" if bins == 116 else "match_scores_mfma_kernel"), name
            for c in range(3):
                _check_scores(got[c], m.template, x[c], "bins %d n %d frames %d row %d" % (bins, n, J, c))
            if J >= 3 * n + 8:
                assert (_bits(got[1, n + 2:n + 5]) == 0).all() and np.isnan(got[2, J - 2 * n:J - n]).all() and np.isnan(got[2, :n // 2 + 1]).all()
            assert np.isnan(got[:, max(J - n + 1, 0):]).all()
        det.profile(False)


# ---- the packed plan: 7 recordings on 2 rows ----
def _frames_to_samples(f):
    return 100 if f == 0 else 256 + 132 * (f - 1)


def _plan(n):
    """-> (det, rec, frames of the 7 recordings, their columns, (row, first) of each); two are shorter than the template, one is
    exactly n frames long, one n + 1; recording 4 (300 frames) is the one that is also scored alone"""
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
    for f, c, (row, first) in zip(frames, cols, where):
        a[row, first:first + f] = c
    own = np.zeros((2, J), bool)
    for f, (row, first) in zip(frames, where):
        own[row, first:first + f] = True
    assert (~own).sum() > 0                                              # there are frames between recordings or behind them
    return a


@pytest.mark.parametrize("n", [12, 91])
def test_a_score_has_the_same_bits_wherever_its_window_lies(n):
    det, rec, frames, cols, where = _plan(n)
    one = _det(29, 1)
    rng = np.random.default_rng(n)
    t = (rng.standard_normal((n, 29))).astype(np.float32)
    try:
        with one.matcher(t) as m1, rec.matcher(t) as mp:
            assert mp.shape == (7, n, 29, n - 1) and m1.form == mp.form == "matrix"
            alone = [m1.scores(torch.from_numpy(c[None]).cuda()).cpu().numpy()[0] for c in cols]
            for k, f in enumerate(frames):
                _check_scores(alone[k], m1.template, cols[k], "recording %d alone" % k)
            # the packed plan, with zeros and with poison in every frame that is no recording's
            got = {}
            for name, outside in (("zeros", 0.0), ("NaN", NAN), ("Inf", INF), ("1e30", np.float32(1e30))):
                a = _packed(det, rec, frames, cols, where, outside)
                got[name] = mp.scores(torch.from_numpy(a).cuda()).cpu().numpy()
            J = got["zeros"].shape[1]
            mine = np.zeros((2, J), bool)
            for k, (f, (row, first)) in enumerate(zip(frames, where)):
                sl = ref.detector_positions(first, f, n)
                mine[row, sl] = True
                for name, g in got.items():
                    assert _bits(g[row, first:first + f]).tobytes() == _bits(alone[k]).tobytes(), (name, k)
            assert mine.sum() == sum(max(f - n + 1, 0) for f in frames)
            for name, g in got.items():
                assert np.isnan(g[~mine]).all() and not np.isnan(g[mine]).any(), name       # NaN exactly where no window begins
            # recording 4 shifted by 1, 5 and 16 frames within a one-channel row, other frames in front of and behind it
            for shift in (1, 5, 16):
                row = np.concatenate([train_cases.columns(rng, shift, 29), cols[4], train_cases.columns(rng, 7, 29)])
                g = m1.scores(torch.from_numpy(row[None]).cuda()).cpu().numpy()[0]
                P = frames[4] - n + 1
                assert _bits(g[shift:shift + P]).tobytes() == _bits(alone[4][:P]).tobytes(), shift
            # one NaN and one Inf inside recording 6: exactly the windows that hold them are NaN, every other score keeps its bits
            dirty = [c.copy() for c in cols]
            dirty[6][100, 3], dirty[6][400, 28] = NAN, INF
            g = mp.scores(torch.from_numpy(_packed(det, rec, frames, dirty, where, 0.0)).cuda()).cpu().numpy()
            hit = np.zeros((2, J), bool)
            row, first = where[6]
            for at in (100, 400):
                hit[row, first + max(at - n + 1, 0):first + at + 1] = True
            hit &= mine
            assert hit.sum() == 2 * n and np.isnan(g[hit]).all()
            assert _bits(g[mine & ~hit]).tobytes() == _bits(got["zeros"][mine & ~hit]).tobytes() and np.isnan(g[~mine]).all()
            # the statuses of the packed form: the rows' frames, nothing else
            with pytest.raises(sd.SyllableDetectorError) as e:
                mp.scores(torch.zeros((2, J - 1, 29), device="cuda"))
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT
    finally:
        rec.close()


# ---- peaks ----
def _device_tables(m, scores, thr, S, cap):
    ev, cnt, es = m.peaks(torch.from_numpy(np.ascontiguousarray(scores)).cuda(), thr, S, capacity=cap)
    torch.cuda.synchronize()
    return ev.cpu().numpy(), cnt.cpu().numpy(), es.cpu().numpy()


def _same_tables(got, want_rows, cap, what):
    ev, cnt, es = got
    for d, (w_ev, w_n, w_sc) in enumerate(want_rows):
        k = min(w_n, cap)
        assert cnt[d] == w_n and ev[d, :k].tolist() == w_ev.tolist() and _bits(es[d, :k]).tobytes() == _bits(w_sc).tobytes(), (what, d)


def test_the_devices_peaks_equal_the_model_on_every_host_case():
    det = _det(7, 3)
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    with det.matcher(np.ones((1, 7), np.float32)) as m:                  # n = 1: a row's positions are its frames
        for name, s, thr, S, cap in peak_cases():
            rows = np.stack([s, s[::-1], np.full_like(s, NAN)])
            got = _device_tables(m, rows, thr, S, cap)
            _same_tables(got, [ref.tables(r, thr, S, origin, hop, 0, cap) for r in rows], cap, name)
            again = _device_tables(m, rows, thr, S, cap)
            for a, b in zip(got, again):                                 # the same call twice: the same bits (within the counts)
                for d in range(3):
                    k = min(int(got[1][d]), cap)
                    assert a[d].tobytes() == b[d].tobytes() if a.ndim == 1 else a[d, :k].tobytes() == b[d, :k].tobytes(), name
        # without event scores, and an anchor other than the default
        ev, cnt, es = m.peaks(torch.from_numpy(peak_cases()[0][1][None].repeat(3, 0)).cuda(), 0.0, 1, capacity=8, withScores=False)
        assert es is None and cnt.cpu().tolist() == [4, 4, 4]
        for bad in (dict(threshold=float("nan")), dict(separation=-1), dict(separation=4097), dict(capacity=-1)):
            kw = dict(threshold=0.0, separation=1, capacity=4)
            kw.update(bad)
            with pytest.raises(sd.SyllableDetectorError) as e:
                m.peaks(torch.zeros((3, 5), device="cuda"), **kw)
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad
    t = np.ones((3, 7), np.float32)
    with det.matcher(t, anchor=1) as m:
        assert m.shape == (3, 3, 7, 1)
        s = np.full((3, 12), NAN, np.float32)
        s[:, :10] = [0.1, 0.9, 0.2, 0.3, 0.8, 0.1, 0.1, 0.7, 0.2, 0.95]
        got = _device_tables(m, s, 0.5, 2, 8)
        _same_tables(got, [ref.tables(r[:10], 0.5, 2, origin, hop, 1, 8) for r in s], 8, "anchor 1")
        assert got[0][0, 0] == origin + (1 + 1) * hop
    for bad in (dict(anchor=3), dict(template=np.ones((3, 6), np.float32)), dict(template=np.zeros((3, 7), np.float32)),
                dict(template=np.full((3, 7), NAN, np.float32)), dict(template=np.ones((4682, 7), np.float32))):
        kw = dict(template=t, anchor=None)
        kw.update(bad)
        with pytest.raises(sd.SyllableDetectorError) as e:
            det.matcher(**kw)
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad


@pytest.mark.parametrize("S", [0, 12, 300, 4096])
def test_peaks_of_a_packed_plan_never_reach_into_the_neighbour(S):
    n = 12
    det, rec, frames, cols, where = _plan(n)
    origin, hop = align_ref.anchor(det.config, align_ref.COLUMNS)
    rng = np.random.default_rng(S)
    try:
        with rec.matcher(rng.standard_normal((n, 29)).astype(np.float32), anchor=4) as mp:
            a = _packed(det, rec, frames, cols, where, NAN)
            s = mp.scores(torch.from_numpy(a).cuda())
            thr = float(np.nanquantile(s.cpu().numpy(), 0.6))
            for scores in (s.cpu().numpy(), None):
                if scores is None:
                    # a ramp over each row: every recording's last position is its largest, and the next recording's first ones,
                    # a few frames on, are larger still -- they must not suppress it
                    J = s.shape[1]
                    scores = np.tile(np.arange(J, dtype=np.float32) / J, (2, 1))
                    thr = -1.0
                cap = 16 if S == 0 else 1024
                got = _device_tables(mp, scores, thr, S, cap)
                want = [ref.tables(scores[row, ref.detector_positions(first, f, n)], thr, S, origin, hop, 4, cap) for f, (row, first) in zip(frames, where)]
                _same_tables(got, want, cap, S)
                assert got[1][0] == 0 and got[1][1] == 0                  # shorter than the template: no position
                if thr == -1.0:
                    assert got[1][2] == 1                                 # exactly n frames: its one position
                if S > 0 and thr == -1.0:
                    assert all(c == (1 if f >= n else 0) for c, f in zip(got[1], frames))
                    for k, f in enumerate(frames):
                        if f >= n:
                            assert got[0][k, min(got[1][k], cap) - 1] == origin + (f - n + 4) * hop
    finally:
        rec.close()


# ---- the chain: exemplar -> matches -> windows and targets ----
def test_the_chain_from_an_exemplar_to_windows_and_targets():
    det = _det(29, 2)
    cfg = det.config
    origin, hop = align_ref.anchor(cfg, align_ref.COLUMNS)
    x = np.stack([mc.planted(seed)[0] for seed in mc.SEEDS])
    cols = det.spectrogram(torch.from_numpy(x).cuda())
    n = mc.N
    with det.matcher(mc.exemplar()) as m:
        assert m.form == "matrix"
        events, ev_scores = m.find(cols, mc.THRESHOLD, mc.SEPARATION)
        host = cols.cpu().numpy()
        P = host.shape[1] - n + 1
        for d, seed in enumerate(mc.SEEDS):
            p = (events[d] - origin) // hop - (n - 1)
            assert ((events[d] - origin) % hop == 0).all() and mc.found_once(p, mc.planted(seed)[1], P), (seed, p.tolist())
            assert (ev_scores[d] >= mc.THRESHOLD).all()
        s = m.scores(cols)
        table, counts, _ = m.peaks(s, mc.THRESHOLD, mc.SEPARATION, capacity=64)
        assert counts.cpu().tolist() == [len(e) for e in events]
        # the table as it is into the aligner: each window is the bit copy of the matched frames
        with det.aligner("columns", n - 1, 0) as al:
            w = al.windows(cols, table, counts=counts).cpu().numpy()
            at = 0
            for d in range(2):
                for e in events[d]:
                    p = (int(e) - origin) // hop - (n - 1)
                    assert w[at].tobytes() == host[d, p:p + n].tobytes()
                    at += 1
            assert at == w.shape[0] > 40
        # ... and into the trainer: every event selects an evaluation with target 1
        E = det.countEvaluations(x.shape[1])
        with det.trainer() as tr:
            tg, wt = tr.targets(events, 0, 1.0, 0.0, n_evals=E)
            tg, wt = tg.cpu().numpy(), wt.cpu().numpy()
            first = align_ref.clock(cfg)[3]
            for d in range(2):
                e = (events[d] - first) // hop
                assert ((events[d] - first) % hop == 0).all() and (e >= 0).all() and (e < E).all()
                assert (tg[d, e, 0] == 1).all() and (wt[d, e] == 1).all() and tg[d].sum() == len(e)
