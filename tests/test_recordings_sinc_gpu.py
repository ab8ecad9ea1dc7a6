"""Packed recordings at other rates on the GPU (syldet_recordings_load_sinc_device*, recordings_load_sinc_kernel): the rows the
converting load lays out against the SHIPPED whole-recording converter given each recording alone -- the same 32-bit patterns,
for fp32 and int16 sources -- and, as an anchor that does not share its code, against the fp64 model of tests/sinc_ref.py within
the converter's own bound T 2^-24 A + 2^-21 X (tests/test_sinc_gpu.py's check, imported).  Recordings at the network's rate are
exact copies, every other element of [0, row_samples) is +0, what lies behind row_samples is left alone.  Then downstream: each
recording's outputs and flags out of the packed run are those of converting it alone and running it alone, and runRecordings with
rates gives what the loop over convertRate, run and detections gives.  Last, the statuses that need a handle: each comes back
before the device is touched (the rows keep their sentinels)."""
import math

import numpy as np
import pytest
import torch

import recordings_ref as ref
import sinc_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth
from test_sinc_gpu import check_against_model

pytestmark = pytest.mark.gpu

RATE = 44100.0
Q = (8, 12.0, 0.9)
SENTINEL = 12345.0
# the output lengths: none; one; shorter than H (every tap cut at both ends); exactly one workgroup's block; a block and one;
# several blocks; many blocks
N_OUT = [0, 1, 37, 1024, 1025, 5000, 9001]
# two assignments of rates to them (22050 -> 44100 makes odd lengths only; 44100 is the network's rate: a copy)
RATES_A = [48000.0, 96000.0, 24414.0625, 48000.0, 22050.0, 44100.0, 96000.0]
RATES_B = [44100.0, 22050.0, 48000.0, 96000.0, 24414.0625, 48000.0, 22050.0]


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def n_in_for(n_out, ri, ro=RATE):
    """a source length whose length at the network's rate is n_out"""
    if n_out == 0:
        return 0
    n = int((n_out - 1) * ri / ro) + 1
    for cand in range(max(n - 3, 1), n + 4):
        if sinc_ref.count(cand, ri, ro) == n_out:
            return cand
    raise AssertionError("no source length at %g Hz makes %d samples" % (ri, n_out))


def make_sources(n_in, steps, dtype, first):
    """-> (src, offsets): a 1-D source of non-zero values; recording k has n_in[k] samples `steps[k]` apart from offsets[k], the
    first at `first`, the next at the other parity every second time"""
    rng = np.random.default_rng(11)
    offsets, pos = [], first
    for k, (n, s) in enumerate(zip(n_in, steps)):
        offsets.append(pos)
        pos += n * s + (k % 2)
    size = pos + 8
    if dtype == np.int16:
        src = rng.integers(1, 32767, size=size).astype(np.int16) * rng.choice([-1, 1], size=size).astype(np.int16)
    else:
        src = (rng.uniform(0.1, 1.0, size=size) * rng.choice([-1.0, 1.0], size=size)).astype(np.float32)
    return src, offsets


def take(src, offset, n, step):
    return src[offset:offset + n * step:step][:n].copy()        # (a copy: one sample of a strided slice keeps the slice's stride)


def alone(x, ri, quality):
    """the shipped converter on recording x alone, one contiguous row -> float32 [n_out] (the reference of the bit contract)"""
    if x.size == 0:
        return np.zeros(0, np.float32)
    got = sd.convertRate(torch.from_numpy(x[None, :]).cuda(), ri, RATE, "sinc", *quality)
    torch.cuda.synchronize()
    return got[0].cpu().numpy()


def widen(x):
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x


def expected_rows(rec, C, stride, src, offsets, n_in, steps, rates, quality):
    """rows [C, stride] as the contract states them, and per converted recording (k, its values) for the model's check"""
    want = np.full((C, stride), SENTINEL, np.float32)
    want[:, :rec.rowSamples] = 0.0                              # +0
    converted = []
    for k, (row, offset, _, _, n) in enumerate(rec.slots):
        x = take(src, offsets[k], n_in[k], steps[k])
        if rates[k] == RATE:
            assert n == n_in[k]
            want[row, offset:offset + n] = widen(x)             # a copy, int16 as x * 2^-15 exactly
        else:
            y = alone(x, rates[k], quality)
            assert y.size == n
            want[row, offset:offset + n] = y
            converted.append((k, x))
    return want, converted


def load(rec, src, offsets, n_in, rates, steps, quality, out):
    got = rec.loadSinc(torch.from_numpy(src).cuda(), offsets, n_in, rates, steps, *quality, out=out)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy()


def rows_buffer(C, rec, aligned):
    """rows of `stride` > rowSamples elements full of sentinels, their base 16-byte aligned or one element off (an odd stride)"""
    stride = rec.rowSamples + (16 if aligned else 9)
    big = torch.full((C, stride + (8 if aligned else 1)), SENTINEL, dtype=torch.float32, device="cuda")
    out = big[:, :stride] if aligned else big[:, 1:]
    assert (out.data_ptr() % 16 == 0 and (out.stride(0) * 4) % 16 == 0) == aligned
    return big, out, stride


def check_model(rows, rec, converted, rates, quality, label):
    for k, x in converted:
        row, offset, _, _, n = rec.slots[k]
        model = sinc_ref.convert(widen(x), rates[k], RATE, *quality)
        check_against_model(rows[row:row + 1, offset:offset + n], [model], "%s, recording %d (%g Hz, %d outputs)" % (label, k, rates[k], n))


@pytest.mark.parametrize("layout", ["planar", "interleaved-odd"])
@pytest.mark.parametrize("hop", [132, 131])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_rows_hold_the_converters_bits(dtype, hop, layout):
    """K = 7 on C = 3.  planar: step 1, rows of whole 16 bytes (base and stride), rates A.  interleaved-odd: steps 1, 2 and 3,
    source offsets of both parities from an odd one on, rows whose base is one element off a whole 16 bytes and whose stride is
    odd, rates B.  (Two tracks of ONE file: test_two_tracks_of_one_interleaved_file.)"""
    cfg = util.sample_net() if hop == 132 else _hop131(util.sample_net())
    assert ref.clock(cfg)[0] == hop
    planar = layout == "planar"
    rates = RATES_A if planar else RATES_B
    n_in = [n_in_for(n, r) for n, r in zip(N_OUT, rates)]
    steps = [1] * 7 if planar else [2, 3, 2, 1, 2, 3, 2]
    src, offsets = make_sources(n_in, steps, dtype, 0 if planar else 1)
    if not planar:
        assert any(o % 2 for o in offsets)
    C = 3
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(sd.recordingLengths(n_in, rates, RATE)) as rec:
        assert [s[4] for s in rec.slots] == N_OUT
        big, out, stride = rows_buffer(C, rec, planar)
        want, converted = expected_rows(rec, C, stride, src, offsets, n_in, steps, rates, Q)
        assert len(converted) == 6                              # all but the one at the network's rate
        got = load(rec, src, offsets, n_in, rates, steps, Q, out)
        # checks 1, 3, 4: the converter's bits, exact copies, +0 (its sign too) elsewhere, the sentinels behind row_samples
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        rest = big.cpu().numpy()
        assert (rest[:, stride:] == SENTINEL).all() if planar else (rest[:, 0] == SENTINEL).all()
        # check 2: the independent anchor
        check_model(got, rec, converted, rates, Q, "%s, hop %d, %s" % (layout, hop, np.dtype(dtype).name))
        # check 5: the same layout again (a launch only) gives the same bits
        out.fill_(SENTINEL)
        assert np.array_equal(load(rec, src, offsets, n_in, rates, steps, Q, out).view(np.uint32), want.view(np.uint32))


def test_two_tracks_of_one_interleaved_file():
    """A two-track file as its WAV stores it: both tracks are recordings of step 2, one element apart -- and a mono file behind
    it at an odd offset."""
    cfg = util.sample_net()
    n_in = [6000, 6000, 2500]
    rates = [48000.0, 48000.0, 22050.0]
    steps = [2, 2, 1]
    offsets = [0, 1, 2 * 6000 + 1]
    for dtype in (np.float32, np.int16):
        src, _ = make_sources([2 * 6000 + 1 + 2500], [1], dtype, 0)
        with sd.SyllableDetector(cfg, channels=2) as det, det.recordings(sd.recordingLengths(n_in, rates, RATE)) as rec:
            big, out, stride = rows_buffer(2, rec, True)
            want, converted = expected_rows(rec, 2, stride, src, offsets, n_in, steps, rates, Q)
            got = load(rec, src, offsets, n_in, rates, steps, Q, out)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            assert len(converted) == 3


def test_a_row_without_a_recording_and_the_default_quality():
    """C = 4 > K = 2: two rows hold no recording and are +0 throughout.  The defaults (32, 12, 0.9): the 64 KiB table, H = 38.7."""
    cfg = util.sample_net()
    rates = [48000.0, 24414.0625]
    n_in = [n_in_for(2500, rates[0]), n_in_for(1025, rates[1])]
    src, offsets = make_sources(n_in, [1, 1], np.float32, 1)
    quality = sinc_ref.DEFAULTS
    with sd.SyllableDetector(cfg, channels=4) as det, det.recordings(sd.recordingLengths(n_in, rates, RATE)) as rec:
        assert sorted(s[0] for s in rec.slots) == [0, 1]
        big, out, stride = rows_buffer(4, rec, False)
        want, converted = expected_rows(rec, 4, stride, src, offsets, n_in, [1, 1], rates, quality)
        got = rec.loadSinc(torch.from_numpy(src).cuda(), offsets, n_in, rates, out=out)          # (no quality: the defaults)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[2:, :rec.rowSamples].view(np.uint32) == 0).all()
        check_model(got, rec, converted, rates, quality, "defaults")


def test_a_workgroup_that_stages_more_than_once():
    """8 : 1 (352.8 kHz): the 1024 outputs of a workgroup read 8192 inputs and the filter's reach, three stretches of 4000."""
    cfg = util.sample_net()
    rates = [352800.0, 44100.0]
    n_in = [n_in_for(1500, rates[0]), 700]
    src, offsets = make_sources(n_in, [1, 1], np.float32, 0)
    with sd.SyllableDetector(cfg, channels=1) as det, det.recordings(sd.recordingLengths(n_in, rates, RATE)) as rec:
        big, out, stride = rows_buffer(1, rec, True)
        want, converted = expected_rows(rec, 1, stride, src, offsets, n_in, [1, 1], rates, Q)
        got = load(rec, src, offsets, n_in, rates, [1, 1], Q, out)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        check_model(got, rec, converted, rates, Q, "352800 -> 44100")


def test_a_changed_layout_gives_the_new_layouts_bits():
    """check 6: the same handle, then other rates (with other source lengths that make the planned lengths), another quality,
    other offsets -- each a new layout: the rows are the new layout's, nothing of the old tables is left."""
    cfg = util.sample_net()
    C = 3
    n_in = [n_in_for(n, r) for n, r in zip(N_OUT, RATES_A)]
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(N_OUT) as rec:
        big, out, stride = rows_buffer(C, rec, True)
        src, offsets = make_sources(n_in, [1] * 7, np.float32, 0)
        first = load(rec, src, offsets, n_in, RATES_A, [1] * 7, Q, out).copy()
        # recording 1 (one output) from 96 to 48 kHz, recording 2 (37 outputs) from 24414.0625 to 22050 Hz
        rates2 = list(RATES_A)
        rates2[1], rates2[2] = 48000.0, 22050.0
        n_in2 = [n_in_for(n, r) for n, r in zip(N_OUT, rates2)]
        assert n_in2[2] != n_in[2]
        want, _ = expected_rows(rec, C, stride, src, offsets, n_in2, [1] * 7, rates2, Q)
        got = load(rec, src, offsets, n_in2, rates2, [1] * 7, Q, out)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(got.view(np.uint32), first.view(np.uint32))
        # another quality alone
        q2 = (12, 9.0, 0.85)
        want, _ = expected_rows(rec, C, stride, src, offsets, n_in2, [1] * 7, rates2, q2)
        assert np.array_equal(load(rec, src, offsets, n_in2, rates2, [1] * 7, q2, out).view(np.uint32), want.view(np.uint32))
        # ... and back to the first layout, from other offsets
        src3, offsets3 = make_sources(n_in, [1] * 7, np.float32, 3)
        want, _ = expected_rows(rec, C, stride, src3, offsets3, n_in, [1] * 7, RATES_A, Q)
        assert np.array_equal(load(rec, src3, offsets3, n_in, RATES_A, [1] * 7, Q, out).view(np.uint32), want.view(np.uint32))
        # a plain load in between keeps its own sources: the converting load after it is still the kept layout's
        plain = rec.load(torch.from_numpy(src3).cuda(), offsets3)
        torch.cuda.synchronize()
        assert np.array_equal(plain.cpu().numpy(), ref.rows(rec.slots, rec.rowSamples, C, src3, offsets3, [1] * 7))
        assert np.array_equal(load(rec, src3, offsets3, n_in, RATES_A, [1] * 7, Q, out).view(np.uint32), want.view(np.uint32))


# ---- downstream ----
# lengths at the network's rate (the sample network's first evaluation needs 1444 samples): one without samples, one shorter than
# a window, one of exactly one evaluation, longer ones
RUN_OUT = [20003, 0, 100, 1444, 5281, 7777, 12001]
RUN_RATES = [48000.0, 96000.0, 48000.0, 24414.0625, 22050.0, 44100.0, 96000.0]


@pytest.mark.parametrize("route", ["fold", "generic"])
def test_each_recording_has_the_values_of_converting_and_running_it_alone(route):
    """check 7, after _check_values / _alone of tests/test_recordings_gpu.py"""
    cfg = util.sample_net()
    engine = _abi.ENGINE_AUTO if route == "fold" else _abi.ENGINE_GENERIC
    n_in = [n_in_for(n, r) for n, r in zip(RUN_OUT, RUN_RATES)]
    rng = np.random.default_rng(9)
    recs = [(synth.channel(n, 40 + k, fs=r) * np.float32(rng.uniform(0.2, 1.0))).astype(np.float32) for k, (n, r) in enumerate(zip(n_in, RUN_RATES))]
    offsets = np.cumsum([0] + [x.size + 3 for x in recs])[:-1]
    src = np.zeros(int(offsets[-1]) + recs[-1].size + 8, np.float32)
    for o, x in zip(offsets, recs):
        src[o:o + x.size] = x
    with sd.SyllableDetector(cfg, channels=3, engine=engine) as det, sd.SyllableDetector(cfg, channels=1, engine=engine) as one, \
            det.recordings(sd.recordingLengths(n_in, RUN_RATES, RATE)) as rec:
        rows = rec.loadSinc(torch.from_numpy(src).cuda(), offsets, n_in, RUN_RATES, None, *Q)
        out, fl = det.run(rows)
        torch.cuda.synchronize()
        if route == "fold":
            assert det.lastFusedForm()[0] == 2                  # the symmetric-fold kernel ran
        assert out.shape[1] == rec.rowEvaluations
        seen = 0
        for k, x in enumerate(recs):
            n_evals = rec.slots[k][3]
            if n_evals == 0:
                continue
            t = torch.from_numpy(x[None, :]).cuda()
            y = t if RUN_RATES[k] == RATE else sd.convertRate(t, RUN_RATES[k], RATE, "sinc", *Q)
            assert y.shape[1] == RUN_OUT[k]
            o1, f1 = one.run(y.contiguous())
            torch.cuda.synchronize()
            assert o1.shape[1] == n_evals
            assert torch.equal(rec.view(out, k), o1[0]), "recording %d: outputs differ from converting and running it alone" % k
            assert torch.equal(rec.view(fl, k), f1[0]), "recording %d: flags differ from converting and running it alone" % k
            seen += 1
        assert seen >= 5


def _quantise(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def _to_rate(x, rate):
    """a 44.1 kHz signal at another rate, by linear interpolation on the host (test material: it only has to hold syllables)"""
    if rate == RATE:
        return x
    n = int((x.size - 1) * rate / RATE) + 1
    return np.interp(np.arange(n) * (RATE / rate), np.arange(x.size), x).astype(np.float32)


@pytest.mark.parametrize("s16", [False, True])
def test_run_recordings_with_rates(s16):
    """check 8: per recording what the loop `convertRate sinc, run, detections` returns"""
    cfg = util.sample_net()
    tmpl = util.template()
    # a mono file at 48 kHz, a stereo one at 22.05 kHz, a mono one at the network's rate (copied), a mono one at 96 kHz, one
    # without frames
    rates = [48000.0, 22050.0, 44100.0, 96000.0, 48000.0]
    arrays = [_to_rate(synth.syllable_channel(30011, tmpl, seed=30), rates[0]),
              np.stack([_to_rate(synth.syllable_channel(22222, tmpl, seed=40 + t), rates[1]) for t in range(2)], axis=1),
              synth.syllable_channel(14000, tmpl, seed=32), _to_rate(synth.syllable_channel(9000, tmpl, seed=33), rates[3]),
              np.zeros((0, 2), np.float32)]
    if s16:
        arrays = [_quantise(a) for a in arrays]
    tracks = [(arrays[0], rates[0]), (arrays[1][:, 0], rates[1]), (arrays[1][:, 1], rates[1]), (arrays[2], rates[2]), (arrays[3], rates[3]),
              (arrays[4][:, 0], rates[4]), (arrays[4][:, 1], rates[4])]
    hop, _, _, first = ref.clock(cfg)
    for debounce in (0.0, 0.05):
        with sd.SyllableDetector(cfg, channels=3) as det, sd.SyllableDetector(cfg, channels=1) as one:
            got = det.runRecordings(arrays, debounce, rates=rates, resample="sinc", zeroCrossings=Q[0], beta=Q[1], rolloff=Q[2])
            assert len(got) == len(tracks)
            total = 0
            for (gi, gv), (x, r) in zip(got, tracks):
                x = np.ascontiguousarray(x)
                if one.countEvaluations(sinc_ref.count(x.size, r, RATE)) <= 0:
                    assert gi.size == 0 and gv.shape == (0, 1)
                    continue
                t = torch.from_numpy(x[None, :]).cuda()
                if r != RATE:
                    o1, f1 = one.run(sd.convertRate(t, r, RATE, "sinc", *Q))
                else:
                    o1, f1 = (one.runPCM16 if s16 else one.run)(t)
                torch.cuda.synchronize()
                mi, me = ref.events(f1[0].cpu().numpy(), first, hop, int(debounce * cfg.samplingRate))
                assert np.array_equal(gi, mi) and np.array_equal(gv.view(np.uint32), o1[0].cpu().numpy()[me].view(np.uint32))
                total += gi.size
            assert total >= 3
    with sd.SyllableDetector(cfg, channels=2) as det:
        # without rates: exactly what it did before (the plain load, int16 rows for int16 arrays)
        plain = det.runRecordings(arrays[:1], 0.05)
        same = det.runRecordings(arrays[:1], 0.05, rates=[RATE], resample="sinc")
        assert np.array_equal(plain[0][0], same[0][0]) and np.array_equal(plain[0][1].view(np.uint32), same[0][1].view(np.uint32))


# ---- the statuses that need a handle: each before the device is touched ----
def test_refused_arguments_leave_the_rows_alone():
    cfg = util.sample_net()
    bad, unsupported = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_UNSUPPORTED
    rates = [48000.0, 44100.0, 22050.0]
    n_in = [3000, 2000, 1001]
    lengths = sd.recordingLengths(n_in, rates, RATE)
    with sd.SyllableDetector(cfg, channels=2) as det, det.recordings(lengths) as rec:
        src = torch.ones(8000, dtype=torch.float32, device="cuda")
        src16 = torch.ones(8000, dtype=torch.int16, device="cuda")
        rows = torch.full((2, rec.rowSamples), SENTINEL, dtype=torch.float32, device="cuda")
        off = np.array([0, 3000, 5000], np.int64)

        def call(fn=_abi.lib.syldet_recordings_load_sinc_device, s=src, offsets=off, steps=None, n=n_in, r=rates, q=Q, out=rows, stride=None,
                 null=()):
            offsets, n, r = np.asarray(offsets, np.int64), np.asarray(n, np.int64), np.asarray(r, np.float64)
            steps = None if steps is None else np.asarray(steps, np.int32)
            st = fn(rec._h, None if "src" in null else s.data_ptr(), None if "offsets" in null else offsets.ctypes.data_as(_abi.c_int64_p),
                    None if steps is None else steps.ctypes.data_as(_abi.c_int32_p), None if "n" in null else n.ctypes.data_as(_abi.c_int64_p),
                    None if "r" in null else r.ctypes.data_as(_abi.c_double_p), q[0], q[1], q[2], None if "rows" in null else out.data_ptr(),
                    rec.rowSamples if stride is None else stride, None)
            torch.cuda.synchronize()
            return st

        for fn, s in ((_abi.lib.syldet_recordings_load_sinc_device, src), (_abi.lib.syldet_recordings_load_sinc_device_s16, src16)):
            # the plain load's checks
            for what in ("src", "offsets", "n", "r", "rows"):
                assert call(fn, s, null=(what,)) == bad
            assert call(fn, s, stride=rec.rowSamples - 1) == bad
            assert call(fn, s, offsets=[0, -1, 5000]) == bad and "recording 1" in _abi.last_error()
            assert call(fn, s, steps=[1, 1, 0]) == bad and "recording 2" in _abi.last_error()
            # lengths and rates
            assert call(fn, s, n=[3000, -1, 1001]) == bad and "src_samples[1]" in _abi.last_error()
            for v in (0.0, -48000.0, math.nan, math.inf):
                assert call(fn, s, r=[48000.0, 44100.0, v]) == bad and "src_rate[2]" in _abi.last_error()
            # the quality: the converter's statuses
            for q in ((3, 12.0, 0.9), (65, 12.0, 0.9), (8, -0.5, 0.9), (8, 20.5, 0.9), (8, math.nan, 0.9), (8, 12.0, 0.0), (8, 12.0, 1.5)):
                assert call(fn, s, q=q) == bad
            # a rate the converter does not take, a filter too wide: unsupported, the recording named
            assert call(fn, s, n=[3000, 2000, 1], r=[48000.0, 44100.0, 44100.0 * 16.5]) == unsupported and "(recording 2)" in _abi.last_error()
            assert call(fn, s, n=[1, 2000, 1001], r=[44100.0 / 16.5, 44100.0, 22050.0]) == unsupported and "(recording 0)" in _abi.last_error()
            assert call(fn, s, q=(64, 12.0, 0.0005)) == unsupported and "(recording 0)" in _abi.last_error()
            # a length that differs from the plan's names its recording
            assert call(fn, s, n=[3000, 2000, 1002]) == bad and "recording 2" in _abi.last_error() and "1002" in _abi.last_error()
            assert call(fn, s, n=[3000, 1999, 1001]) == bad and "recording 1" in _abi.last_error()
            assert call(fn, s, r=[44100.0, 44100.0, 22050.0]) == bad and "recording 0" in _abi.last_error()
        assert (rows == SENTINEL).all(), "a refused call wrote to the rows"
        assert call() == _abi.OK
        assert not (rows == SENTINEL).any()
        with pytest.raises(ValueError):
            rec.loadSinc(src, [0, 3000, 7500], n_in, rates)       # outside the source
        with pytest.raises(ValueError):
            rec.loadSinc(src, off, n_in, rates, out=torch.empty((2, rec.rowSamples), dtype=torch.int16, device="cuda"))   # rows are fp32
