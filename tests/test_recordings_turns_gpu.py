"""Packed recordings on the GPU: the five kept tables of one handle take turns (the plain load's sources, the converting load's
tables, the tracks' destination layout and last_seen prefix, the level meters' reading prefix).  One Recordings, ten calls, each
with a key that differs from the previous use of its table; every result against the numpy models (recordings_ref,
recordings_tracks_ref, recordings_levels_ref) bit for bit, never against another run of the library.  The converting load's rows
against the converter's model as tests/test_recordings_sinc_gpu.py holds it: copies and the +0 around the recordings bit for bit,
converted samples against the fp64 model of sinc_ref.py within the converter's own bound (that model has no bits to compare).
Then, with profiling on, two keys that were used before: their calls launch what a call with the kept key launches."""
import numpy as np
import pytest
import torch

import recordings_levels_ref as lref
import recordings_ref as ref
import recordings_tracks_ref as tref
import util
import syllable_detector_swift_amd as sd
from test_recordings_sinc_gpu import Q, RATE, check_model, make_sources, n_in_for, take

pytestmark = pytest.mark.gpu

C = 2
# none; one sample short of the first evaluation and exactly it; two that make the rows longer than one tile of 8192; a short one
LENGTHS = [0, 1443, 1444, 5280, 9000, 333]
RATES = [48000.0, 22050.0, 48000.0, 44100.0, 96000.0, 24414.0625]      # (22050 makes odd lengths only; 44100: a copy)
SENTINEL = -7


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(_bits(got), _bits(want)), what


def test_the_five_tables_take_turns_on_one_handle():
    cfg = util.sample_net()
    hop, _, _, D = ref.clock(cfg)
    assert hop == 132
    K = len(LENGTHS)
    rng = np.random.default_rng(5)
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(LENGTHS) as rec:
        slots, S, E = rec.slots, rec.rowSamples, rec.rowEvaluations
        assert [s[3] for s in slots][:3] == [0, 0, 1] and 8192 < S <= 2 * 8192 and E > 0         # rows of two tiles
        # sources A and B of the plain load: other values, other offsets, other steps
        steps_a, steps_b = [1] * K, [2, 1, 3, 1, 2, 3]
        src_a, off_a = make_sources(LENGTHS, steps_a, np.float32, 0)
        src_b, off_b = make_sources(LENGTHS, steps_b, np.float32, 5)
        src_b = src_b[::-1].copy()
        d_a, d_b = torch.from_numpy(src_a).cuda(), torch.from_numpy(src_b).cuda()
        rows_a, rows_b = ref.rows(slots, S, C, src_a, off_a, steps_a), ref.rows(slots, S, C, src_b, off_b, steps_b)
        assert not np.array_equal(rows_a, rows_b)
        # the converting load's sources: lengths at other rates that make the planned lengths
        n_in = [n_in_for(n, r) for n, r in zip(LENGTHS, RATES)]
        steps_s = [1, 2, 1, 1, 1, 3]
        src_s, off_s = make_sources(n_in, steps_s, np.float32, 1)
        # the run's results, made here: outputs around the threshold, every fifth flag set
        thr = float(cfg.thresholds[0])
        outh = (rng.standard_normal((C, E, 1)) * 1.5 * thr).astype(np.float32)
        flh = (rng.random((C, E)) < 0.2).astype(np.uint8)
        out, fl = torch.from_numpy(outh).cuda(), torch.from_numpy(flh).cuda()
        thr_rows = [cfg.thresholds] * C
        # destination layouts A and B of the tracks
        lay_a = rec.trackLayout()
        st_b = np.array([2, 1, 3, 2, 1, 2], np.int32)
        lay_b = rec.trackLayout(st_b, align=1)
        assert not np.array_equal(lay_a[0], lay_b[0])

        def track(per_recording, lay, steps=None):
            return tref.scatter(np.full(lay[1], SENTINEL, np.int16), per_recording, lay[0], steps)[0]

        def dest(lay):
            return torch.full((lay[1],), SENTINEL, dtype=torch.int16, device="cuda")

        want_trace = track(tref.trace_each(slots, outh, thr_rows, D, hop, 0, True), lay_a)
        assert (want_trace > 0).any()

        # 1. plain load, sources A
        _same(rec.load(d_a, off_a, steps_a), rows_a, "1: plain load, sources A")
        # 2. converting load
        got = rec.loadSinc(torch.from_numpy(src_s).cuda(), off_s, n_in, RATES, steps_s, *Q).cpu().numpy()
        want, converted, exact = np.zeros((C, S), np.float32), [], np.ones((C, S), bool)
        for k, (row, offset, _, _, n) in enumerate(slots):
            x = take(src_s, off_s[k], n_in[k], steps_s[k])
            if RATES[k] == RATE:
                want[row, offset:offset + n] = x
            elif n > 0:
                exact[row, offset:offset + n] = False
                converted.append((k, x))
        assert len(converted) == 4
        assert np.array_equal(_bits(got)[exact], _bits(want)[exact]), "2: converting load, the copy and the +0 around the recordings"
        check_model(got, rec, converted, RATES, Q, "2: converting load")
        # 3. plain load, sources B
        d_rows = rec.load(d_b, off_b, steps_b)
        _same(d_rows, rows_b, "3: plain load, sources B")
        # 4. trace, layout A
        _same(rec.trace(out, 0, np.int16, lay_a[0], None, out=dest(lay_a)), want_trace, "4: trace, layout A")
        # 5. trigger track, layout B, L = 8
        want = track(tref.trigger_each(slots, flh, D, hop, 8, 44, 0, True), lay_b, st_b)
        assert ((want != 0) & (want != SENTINEL)).any()
        _same(rec.triggerTrack(fl, 8, 44, 0, np.int16, lay_b[0], st_b, out=dest(lay_b)), want, "5: trigger track, layout B, L 8")
        # 6. levels, L = 32, P = 1
        _same(rec.levels(d_rows, 32, 1), lref.input_each(slots, rows_b, 32, 1), "6: levels (32, 1)")
        # 7. trigger onsets, L = 32
        idx, cnt = rec.triggerOnsets(fl, 32, 44, 0)
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        model = tref.onsets_each(slots, flh, D, hop, 32, 44, 0)
        assert sum(len(m) for m in model) > 0
        for k in range(K):
            assert int(cnt[k]) == len(model[k]) <= idx.shape[1] and np.array_equal(idx[k, :len(model[k])], model[k]), "7: onsets, recording %d" % k
        # 8. levels, L = 8, P = 3
        _same(rec.levels(d_rows, 8, 3), lref.input_each(slots, rows_b, 8, 3), "8: levels (8, 3)")
        det.profile(True)
        try:
            # 9. plain load, sources A again: the load is none of the profile's calls, with the kept sources or with others
            got = rec.load(d_a, off_a, steps_a)
            torch.cuda.synchronize()
            assert util.launched(det) == []
            _same(got, rows_a, "9: plain load, sources A again")
            # 10. trace, layout A again: the one kernel of a trace with the kept layout
            got = rec.trace(out, 0, np.int16, lay_a[0], None, out=dest(lay_a))
            torch.cuda.synchronize()
            assert util.launched(det) == ["recordings_trace_kernel"]
            _same(got, want_trace, "10: trace, layout A again")
        finally:
            det.profile(False)
