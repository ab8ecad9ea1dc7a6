"""Packed recordings from the files' own bytes on the GPU (syldet_recordings_load_pcm_device, recordings_load_pcm_kernel;
syldet_recordings_load_sinc_pcm_device, recordings_load_sinc_kernel<uint8_t>).  The reference of every check is the parent's own
call on the float32 the numpy model (tests/pcm_ref.py) makes of the same bytes: Recordings.load for the plain form,
Recordings.loadSinc for the converting one -- the same 32-bit patterns, +0 in pads and empty rows, sentinels behind rowSamples kept.
Six formats, contiguous and as one track of a 2- or 3-track file, S24 and U8 at every byte address mod 4, hops 132 and 131, rows
of whole 16 bytes and rows one element off.  Then downstream (each recording's outputs and flags are those of its decoded float32
run alone, on the fold kernel and the generic engine), runRecordings on a list of mixed dtypes, the profile, and the refusals."""
import numpy as np
import pytest
import torch

import pcm_ref
import recordings_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth
from test_recordings_sinc_gpu import n_in_for, rows_buffer, RATE, Q, SENTINEL

pytestmark = pytest.mark.gpu

# none; one; fewer than a group's worth; an eighth of a tile; odd ends; one past a kRecTile (8192) edge; more than a tile
LENGTHS = [0, 1, 37, 1024, 1025, 5000, 8193, 9001]
K, C = 8, 3


def _cfg(hop):
    base = util.sample_net()
    cfg = base if hop == 132 else nets.variant(base, windowOverlap=base.windowLength - 131)
    assert ref.clock(cfg)[0] == hop
    return cfg


U8, S16, S24, S32, F32, F64 = pcm_ref.FORMATS
# recording k of layout `case`: (format, tracks of its file).  Over the three layouts every format is contiguous in one of the five
# long recordings and one track of a 2- or 3-track file in another.
LAYOUTS = [[(F64, 1), (S24, 1), (F32, 3), (U8, 1), (S16, 2), (S24, 3), (S32, 1), (F32, 2)],
           [(S24, 2), (F32, 1), (U8, 1), (F64, 1), (U8, 2), (S16, 1), (S24, 2), (S32, 3)],
           [(S32, 2), (S16, 1), (F64, 3), (F32, 1), (F64, 2), (S24, 1), (U8, 3), (S16, 3)]]


def formats_and_tracks(case):
    return LAYOUTS[case % 3]


def _coverage():
    long_ones = {ft for layout in LAYOUTS for n, ft in zip(LENGTHS, layout) if n >= 1024}
    return all((f, 1) in long_ones and ((f, 2) in long_ones or (f, 3) in long_ones) for f in pcm_ref.FORMATS)


assert _coverage(), "every format is contiguous and interleaved in a long recording"


def no_f64_nans(raw, fmt):
    """(the contract's reference decodes F64 NaNs through numpy, whose payload rule is not the device's: none in these sources)"""
    if fmt == pcm_ref.F64:
        x = raw.view("<f8")
        x[np.isnan(x)] = 0.25
    return raw


def make_bytes(lengths, layout, seed, shift=0):
    """-> (src uint8, byte offsets, byte steps, formats): every recording one track of a file of its own, the other tracks random
    bytes; S16 / S32 / F32 / F64 files start at a multiple of their size, and the files of U8 and S24 at addresses that go through
    0, 1, 2, 3 (mod 4) (+ shift).  The source ends with the last file's last byte."""
    rng = np.random.default_rng(seed)
    parts, offsets, steps, formats, pos = [], [], [], [], 0
    free = shift
    for k, (n, (fmt, tracks)) in enumerate(zip(lengths, layout)):
        size = pcm_ref.BYTES[fmt]
        if fmt in (pcm_ref.U8, pcm_ref.S24):
            start = pos + (free - pos) % 4
            free += 1
        else:
            start = -(-pos // size) * size
        parts.append(rng.integers(0, 256, size=start - pos, dtype=np.uint8))
        t = k % tracks
        tr = [no_f64_nans(pcm_ref.samples(fmt, n, rng, special=(i == t)), fmt) for i in range(tracks)]
        parts.append(pcm_ref.interleave(tr, fmt))
        offsets.append(start + t * size)
        steps.append(tracks * size)
        formats.append(fmt)
        pos = start + n * tracks * size
    src = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    assert src.size == pos
    return src, offsets, steps, formats


def decoded(src, offsets, steps, formats, lengths):
    """-> (float32 source, element offsets): the model's float32 of every recording, end to end, three elements between two"""
    parts, at, pos = [], [], 0
    for o, s, f, n in zip(offsets, steps, formats, lengths):
        x = pcm_ref.decode(src, f, n, s, o)
        at.append(pos)
        parts.append(x)
        parts.append(np.zeros(3, np.float32))
        pos += n + 3
    return np.concatenate(parts), at


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.zeros(0, dtype=torch.from_numpy(a).dtype, device="cuda")


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("hop", [132, 131])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_rows_hold_the_bits_of_load_on_the_decoded_float32(case, hop):
    """hop 132: rows of whole 16 bytes (16 bytes a store); hop 131: rows whose base is one element off and whose stride is odd (one
    element a store), and the addresses of U8 and S24 files shifted by 2."""
    aligned = hop == 132
    layout = formats_and_tracks(case)
    src, offsets, steps, formats = make_bytes(LENGTHS, layout, 7 + case, 0 if aligned else 2)
    f32, at = decoded(src, offsets, steps, formats, LENGTHS)
    with sd.SyllableDetector(_cfg(hop), channels=C) as det, det.recordings(LENGTHS) as rec:
        big, out, stride = rows_buffer(C, rec, aligned)
        want = rec.load(dev(f32), at)
        torch.cuda.synchronize()
        assert np.array_equal(want.cpu().numpy().view(np.uint32), ref.rows(rec.slots, rec.rowSamples, C, f32, at, [1] * K).view(np.uint32))
        d_src = dev(src)
        for _ in range(2):                                        # (the second time: the kept layout, a launch only)
            out.fill_(SENTINEL)
            got = rec.loadPCM(d_src, offsets, steps, formats, out=out)
            torch.cuda.synchronize()
            assert got is out
            assert np.array_equal(bits(out[:, :rec.rowSamples]), bits(want)), "layout %d, hop %d" % (case, hop)
            rest = big.cpu().numpy()
            assert (out[:, rec.rowSamples:] == SENTINEL).all() and ((rest[:, stride:] == SENTINEL).all() if aligned else (rest[:, 0] == SENTINEL).all())
        # NaNs with their payloads came through
        k = formats.index(pcm_ref.F32)
        if LENGTHS[k] >= 2:
            row, offset = rec.slots[k][:2]
            assert bits(out[row, offset:offset + 2]).tolist() == [0x7FC12345, 0xFFA00001]


def test_u8_and_s24_at_every_address():
    """Eight contiguous recordings of U8 and of S24 whose first bytes lie at 0, 1, 2, 3 (mod 4), twice: the 4- and 12-byte reads
    where the address allows them, byte by byte elsewhere; lengths that end inside a group of four."""
    lengths = [4099, 4098, 4097, 4100, 1025, 1026, 1027, 5001]
    for fmt in (pcm_ref.U8, pcm_ref.S24):
        src, offsets, steps, formats = make_bytes(lengths, [(fmt, 1)] * K, 21)
        assert sorted(o % 4 for o in offsets) == [0, 0, 1, 1, 2, 2, 3, 3]
        f32, at = decoded(src, offsets, steps, formats, lengths)
        with sd.SyllableDetector(_cfg(132), channels=C) as det, det.recordings(lengths) as rec:
            want = rec.load(dev(f32), at)
            got = rec.loadPCM(dev(src), offsets, None, formats)      # (no steps: contiguous)
            torch.cuda.synchronize()
            assert np.array_equal(bits(got), bits(want)), pcm_ref.NAMES[fmt]


def test_a_row_without_a_recording():
    """C = 3 > K = 2: one row holds no recording and is +0 throughout."""
    lengths = [5000, 1025]
    src, offsets, steps, formats = make_bytes(lengths, [(pcm_ref.S24, 2), (pcm_ref.F64, 1)], 5)
    f32, at = decoded(src, offsets, steps, formats, lengths)
    with sd.SyllableDetector(_cfg(132), channels=C) as det, det.recordings(lengths) as rec:
        assert sorted(s[0] for s in rec.slots) == [0, 1]
        big, out, stride = rows_buffer(C, rec, True)
        want = rec.load(dev(f32), at)
        rec.loadPCM(dev(src), offsets, steps, formats, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out[:, :rec.rowSamples]), bits(want)) and (bits(out[2, :rec.rowSamples]) == 0).all()
        assert (out[:, rec.rowSamples:] == SENTINEL).all()


def test_a_changed_layout_and_calls_that_take_turns():
    """One handle: a layout, another layout (other formats at other places), then the four old calls and the two new ones in turn,
    each with sources of its own -- every call writes its own bits."""
    rates = [48000.0, 96000.0, 24414.0625, 48000.0, 22050.0, 44100.0, 22050.0, 96000.0]       # (22050 -> 44100 makes odd lengths only)
    n_in = [n_in_for(n, r) for n, r in zip(LENGTHS, rates)]
    a = make_bytes(LENGTHS, formats_and_tracks(0), 31)
    b = make_bytes(LENGTHS, formats_and_tracks(1), 32, 1)
    s = make_bytes(n_in, formats_and_tracks(2), 33)
    fa, at_a = decoded(*a, LENGTHS)
    fb, at_b = decoded(*b, LENGTHS)
    fs, at_s = decoded(*s, n_in)
    rng = np.random.default_rng(34)
    i16 = rng.integers(-32768, 32768, size=fa.size, dtype=np.int16)
    i16s = rng.integers(-32768, 32768, size=fs.size, dtype=np.int16)
    with sd.SyllableDetector(_cfg(132), channels=C) as det, det.recordings(LENGTHS) as rec, det.recordings(LENGTHS) as other:
        # the references, on a handle of their own
        want_a, want_b = other.load(dev(fa), at_a).clone(), other.load(dev(fb), at_b).clone()
        want_16 = other.load(dev(i16), at_a).clone()
        want_s = other.loadSinc(dev(fs), at_s, n_in, rates, None, *Q).clone()
        torch.cuda.synchronize()
        assert not np.array_equal(bits(want_a), bits(want_b))
        d_a, d_b, d_s, d_fa, d_fs, d_16, d_16s = dev(a[0]), dev(b[0]), dev(s[0]), dev(fa), dev(fs), dev(i16), dev(i16s)
        for _ in range(2):
            calls = [(lambda: rec.loadPCM(d_a, *a[1:]), want_a), (lambda: rec.loadPCM(d_b, *b[1:]), want_b),
                     (lambda: rec.load(d_fa, at_a), want_a), (lambda: rec.loadPCM(d_b, *b[1:]), want_b),
                     (lambda: rec.load(d_16, at_a), want_16), (lambda: rec.loadPCM(d_a, *a[1:]), want_a),
                     (lambda: rec.loadSincPCM(d_s, *s[1:], n_in, rates, *Q), want_s), (lambda: rec.loadPCM(d_a, *a[1:]), want_a),
                     (lambda: rec.loadSinc(d_fs, at_s, n_in, rates, None, *Q), want_s), (lambda: rec.loadSincPCM(d_s, *s[1:], n_in, rates, *Q), want_s),
                     (lambda: rec.loadSinc(d_16s, at_s, n_in, rates, None, *Q), None),
                     (lambda: rec.loadSincPCM(d_s, *s[1:], n_in, rates, *Q), want_s)]
            for i, (call, want) in enumerate(calls):
                got = call()
                torch.cuda.synchronize()
                if want is not None:
                    assert got.dtype == want.dtype and np.array_equal(got.cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8)), "call %d" % i


@pytest.mark.parametrize("hop", [132, 131])
def test_the_converting_load_holds_the_bits_of_load_sinc_on_the_decoded_float32(hop):
    """K = 8 on C = 3: every format, contiguous and interleaved; the rates of tests/test_recordings_sinc_gpu.py (44100: a copy) and
    one recording at 352800 Hz whose workgroup stages more than once (1024 outputs read 8192 inputs and the filter's reach, three
    stretches of 4000)."""
    rates = [48000.0, 96000.0, 24414.0625, 22050.0, 44100.0, 352800.0, 48000.0, 44100.0]
    n_out = [0, 1, 37, 1025, 1024, 1500, 5000, 2049]
    n_in = [n_in_for(n, r) for n, r in zip(n_out, rates)]
    aligned = hop == 132
    for case in (0, 1):
        src, offsets, steps, formats = make_bytes(n_in, formats_and_tracks(case + (0 if aligned else 1)), 41 + case, case)
        f32, at = decoded(src, offsets, steps, formats, n_in)
        with sd.SyllableDetector(_cfg(hop), channels=C) as det, det.recordings(sd.recordingLengths(n_in, rates, RATE)) as rec:
            assert [s[4] for s in rec.slots] == n_out
            big, out, stride = rows_buffer(C, rec, aligned)
            want = rec.loadSinc(dev(f32), at, n_in, rates, None, *Q)
            torch.cuda.synchronize()
            d_src = dev(src)
            for _ in range(2):
                out.fill_(SENTINEL)
                rec.loadSincPCM(d_src, offsets, steps, formats, n_in, rates, *Q, out=out)
                torch.cuda.synchronize()
                assert np.array_equal(bits(out[:, :rec.rowSamples]), bits(want)), "layout %d, hop %d" % (case, hop)
                assert (out[:, rec.rowSamples:] == SENTINEL).all()
            # a recording at the network's rate is decoded and copied
            for k in (4, 7):
                row, offset, _, _, n = rec.slots[k]
                assert np.array_equal(bits(out[row, offset:offset + n]), pcm_ref.decode(src, formats[k], n, steps[k], offsets[k]).view(np.uint32))


# ---- downstream ----
def quantise(x, fmt):
    """a float32 signal in [-1, 1) as the bytes of the format"""
    x = np.asarray(x, np.float64)
    if fmt == pcm_ref.U8:
        return (np.clip(np.round(x * 128.0), -128, 127) + 128).astype(np.uint8)
    if fmt == pcm_ref.S16:
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == pcm_ref.S24:
        v = np.clip(np.round(x * 8388608.0), -8388608, 8388607).astype("<i4")
        return v.view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()
    if fmt == pcm_ref.S32:
        return np.clip(np.round(x * 2147483648.0), -2147483648, 2147483647).astype("<i4").view(np.uint8)
    return x.astype("<f4" if fmt == pcm_ref.F32 else "<f8").view(np.uint8)


RUN_LENGTHS = [20003, 0, 100, 1444, 5281, 7777, 12001, 9000]


@pytest.mark.parametrize("route", ["fold", "generic"])
def test_each_recording_has_the_values_of_its_decoded_float32_run_alone(route):
    cfg = util.sample_net()
    engine = _abi.ENGINE_AUTO if route == "fold" else _abi.ENGINE_GENERIC
    rng = np.random.default_rng(9)
    layout = formats_and_tracks(1)
    parts, offsets, steps, formats, pos = [], [], [], [], 0
    for k, (n, (fmt, tracks)) in enumerate(zip(RUN_LENGTHS, layout)):
        size = pcm_ref.BYTES[fmt]
        start = -(-pos // 8) * 8
        parts.append(np.zeros(start - pos, np.uint8))
        tr = [quantise(synth.channel(n, 40 + k + 10 * t) * np.float32(rng.uniform(0.2, 1.0)), fmt) for t in range(tracks)]
        parts.append(pcm_ref.interleave(tr, fmt))
        offsets.append(start + (k % tracks) * size)
        steps.append(tracks * size)
        formats.append(fmt)
        pos = start + n * tracks * size
    src = np.concatenate(parts)
    with sd.SyllableDetector(cfg, channels=C, engine=engine) as det, sd.SyllableDetector(cfg, channels=1, engine=engine) as one, \
            det.recordings(RUN_LENGTHS) as rec:
        rows = rec.loadPCM(dev(src), offsets, steps, formats)
        out, fl = det.run(rows)
        torch.cuda.synchronize()
        if route == "fold":
            assert det.lastFusedForm()[0] == 2                  # the symmetric-fold kernel ran
        seen = 0
        for k, n in enumerate(RUN_LENGTHS):
            n_evals = rec.slots[k][3]
            if n_evals == 0:
                continue
            x = pcm_ref.decode(src, formats[k], n, steps[k], offsets[k])
            o1, f1 = one.run(dev(x[None, :]))
            torch.cuda.synchronize()
            assert o1.shape[1] == n_evals
            assert torch.equal(rec.view(out, k), o1[0]), "recording %d: outputs differ from its decoded float32 run alone" % k
            assert torch.equal(rec.view(fl, k), f1[0]), "recording %d: flags differ from its decoded float32 run alone" % k
            seen += 1
        assert seen >= 6


def _to_rate(x, rate):
    if rate == RATE:
        return x
    n = int((x.size - 1) * rate / RATE) + 1
    return np.interp(np.arange(n) * (RATE / rate), np.arange(x.size), x).astype(np.float32)


def _as_dtype(x, kind):
    """a float32 array [frames] or [frames, tracks] as runRecordings takes it in the format, and the float32 it means"""
    fmt = {"u8": pcm_ref.U8, "s16": pcm_ref.S16, "s24": pcm_ref.S24, "s32": pcm_ref.S32, "f32": pcm_ref.F32, "f64": pcm_ref.F64}[kind]
    raw = quantise(np.ascontiguousarray(x).reshape(-1), fmt)
    means = pcm_ref.decode(raw, fmt).reshape(x.shape)
    if kind == "s24":
        return sd.PCM24(raw.reshape(x.shape + (3,))), means
    dtype = {"u8": np.uint8, "s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[kind]
    return raw.view(dtype).reshape(x.shape), means


def _same_results(a, b):
    assert len(a) == len(b)
    for (ai, av), (bi, bv) in zip(a, b):
        assert np.array_equal(ai, bi) and np.array_equal(av.view(np.uint32), bv.view(np.uint32))
    return sum(ai.size for ai, _ in a)


def test_run_recordings_on_a_list_of_mixed_dtypes():
    cfg = util.sample_net()
    tmpl = util.template()
    kinds = ["s24", "s16", "f32", "u8", "f64", "s32", "s24"]
    sig = [synth.syllable_channel(30011, tmpl, seed=30), np.stack([synth.syllable_channel(22222, tmpl, seed=40 + t) for t in range(2)], axis=1),
           synth.syllable_channel(14000, tmpl, seed=32), synth.syllable_channel(9000, tmpl, seed=33), synth.syllable_channel(12001, tmpl, seed=34),
           np.zeros((0, 2), np.float32), np.stack([synth.syllable_channel(8000, tmpl, seed=50 + t) for t in range(3)], axis=1)]
    pairs = [_as_dtype(np.asarray(x, np.float32) * np.float32(0.9), k) for x, k in zip(sig, kinds)]
    arrays, means = [p[0] for p in pairs], [p[1] for p in pairs]
    with sd.SyllableDetector(cfg, channels=C) as det:
        for debounce in (0.0, 0.05):
            got = det.runRecordings(arrays, debounce)
            want = det.runRecordings(means, debounce)
            assert _same_results(got, want) >= 3 and len(got) == 1 + 2 + 1 + 1 + 1 + 2 + 3
        # the other products of the same run
        got = det.runRecordings(arrays, 0.05, tracks=("trace", "ttl"), levels=(32, None))
        want = det.runRecordings(means, 0.05, tracks=("trace", "ttl"), levels=(32, None))
        _same_results(got[0], want[0])
        for name in ("trace", "ttl"):
            assert all(np.array_equal(x, y) for x, y in zip(got[1][name], want[1][name]))
        for name in ("input", "output"):
            assert all(np.array_equal(x, y) for x, y in zip(got[2][name], want[2][name]))
        # with rates: loadSincPCM
        rates = [48000.0, 22050.0, 44100.0, 96000.0, 44100.0, 44100.0, 24414.0625]
        pairs = [_as_dtype(_to_rate_tracks(np.asarray(x, np.float32) * np.float32(0.9), r), k) for x, k, r in zip(sig, kinds, rates)]
        got = det.runRecordings([p[0] for p in pairs], 0.05, rates=rates, resample="sinc", zeroCrossings=Q[0], beta=Q[1], rolloff=Q[2])
        want = det.runRecordings([p[1] for p in pairs], 0.05, rates=rates, resample="sinc", zeroCrossings=Q[0], beta=Q[1], rolloff=Q[2])
        assert _same_results(got, want) >= 3


def _to_rate_tracks(x, rate):
    return _to_rate(x, rate) if x.ndim == 1 else np.stack([_to_rate(x[:, t], rate) for t in range(x.shape[1])], axis=1).reshape(-1, x.shape[1])


def test_lists_of_one_dtype_take_the_path_they_took(monkeypatch):
    """all int16: int16 rows through load and runPCM16, as ever; all float32: load and run; one uint8 array among them: loadPCM."""
    cfg = util.sample_net()
    tmpl = util.template()
    x = [synth.syllable_channel(9000, tmpl, seed=60 + i) for i in range(2)]
    x16 = [np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16) for v in x]
    seen = []
    for name in ("load", "loadPCM", "loadSinc", "loadSincPCM"):
        real = getattr(sd.Recordings, name)
        monkeypatch.setattr(sd.Recordings, name, lambda self, src, *a, _real=real, _name=name, **kw: (seen.append((_name, src.dtype)), _real(self, src, *a, **kw))[1])
    with sd.SyllableDetector(cfg, channels=2) as det:
        for name in ("run", "runPCM16"):
            real = getattr(det, name)
            monkeypatch.setattr(det, name, lambda rows, _real=real, _name=name: (seen.append((_name, rows.dtype)), _real(rows))[1])
        a = det.runRecordings(x16, 0.05)
        assert seen == [("load", torch.int16), ("runPCM16", torch.int16)]
        del seen[:]
        det.runRecordings(x, 0.05)
        assert seen == [("load", torch.float32), ("run", torch.float32)]
        del seen[:]
        b = det.runRecordings([x16[0], x16[1].astype(np.int32) * 65536], 0.05)
        assert seen == [("loadPCM", torch.uint8), ("run", torch.float32)]
        # (fp32 rows of x * 2^-15 against int16 rows: the same detections; the outputs agree to the engines' own tolerance)
        assert all(np.array_equal(ai, bi) for (ai, _), (bi, _) in zip(a, b))


def test_the_launch_is_listed_under_profiling():
    src, offsets, steps, formats = make_bytes(LENGTHS, formats_and_tracks(0), 3)
    with sd.SyllableDetector(_cfg(132), channels=C) as det, det.recordings(LENGTHS) as rec:
        d_src = dev(src)
        det.profile(True)
        try:
            for _ in range(2):
                rec.loadPCM(d_src, offsets, steps, formats)
            torch.cuda.synchronize()
            names = det.lastTimings()
            assert [n for n, _ in names] == ["recordings_load_pcm_kernel"] and all(ms > 0 for _, ms in names)
        finally:
            det.profile(False)


def test_refused_arguments_leave_the_rows_alone():
    bad = _abi.ERR_INVALID_ARGUMENT
    lengths = [3000, 2000, 1001, 500]
    formats = [sd.PCM_S24, sd.PCM_S16, sd.PCM_F64, sd.PCM_U8]
    steps = [3, 4, 8, 1]
    offsets = [1, 9002, 17008, 25016]                              # ends: 9001, 17002, 25016, 25516
    total = 25516
    with sd.SyllableDetector(util.sample_net(), channels=2) as det, det.recordings(lengths) as rec:
        src = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        rows = torch.full((2, rec.rowSamples), SENTINEL, dtype=torch.float32, device="cuda")
        rates = [RATE] * 4

        def call(sinc=False, s=src, nbytes=total, off=offsets, stp=steps, fmt=formats, n=lengths, r=rates, q=Q, out=rows, stride=None, null=(), base=0):
            off, n, r = np.asarray(off, np.int64), np.asarray(n, np.int64), np.asarray(r, np.float64)
            stp, fmt = None if stp is None else np.asarray(stp, np.int32), np.asarray(fmt, np.int32)
            head = (rec._h, None if "src" in null else s.data_ptr() + base, nbytes, None if "off" in null else off.ctypes.data_as(_abi.c_int64_p),
                    None if stp is None else stp.ctypes.data_as(_abi.c_int32_p), None if "fmt" in null else fmt.ctypes.data_as(_abi.c_int32_p))
            tail = (None if "rows" in null else out.data_ptr(), rec.rowSamples if stride is None else stride, None)
            if sinc:
                st = _abi.lib.syldet_recordings_load_sinc_pcm_device(*head, None if "n" in null else n.ctypes.data_as(_abi.c_int64_p),
                                                                     None if "r" in null else r.ctypes.data_as(_abi.c_double_p), q[0], q[1], q[2], *tail)
            else:
                st = _abi.lib.syldet_recordings_load_pcm_device(*head, *tail)
            torch.cuda.synchronize()
            return st

        for sinc in (False, True):
            # the plain load's checks first
            for what in ("src", "off", "fmt", "rows") + (("n", "r") if sinc else ()):
                assert call(sinc, null=(what,)) == bad and "NULL" in _abi.last_error()
            assert call(sinc, stride=rec.rowSamples - 1) == bad
            assert call(sinc, off=[1, -2, 17008, 25016], fmt=[0, 0, 0, 0]) == bad and "recording 1" in _abi.last_error()
            assert call(sinc, stp=[3, 4, 0, 1], fmt=[0, 0, 0, 0]) == bad and "recording 2" in _abi.last_error()
            # then the byte source's
            assert call(sinc, fmt=[sd.PCM_S24, sd.PCM_S16, 9, sd.PCM_U8]) == bad and "recording 2" in _abi.last_error() and "format" in _abi.last_error()
            assert call(sinc, stp=[2, 4, 8, 1]) == bad and "recording 0" in _abi.last_error() and "step" in _abi.last_error()
            assert call(sinc, off=[1, 9003, 17008, 25016]) == bad and "recording 1" in _abi.last_error() and "multiple" in _abi.last_error()
            assert call(sinc, stp=[3, 4, 12, 1]) == bad and "recording 2" in _abi.last_error() and "multiple" in _abi.last_error()
            assert call(sinc, base=1) == bad and "recording 1" in _abi.last_error() and "multiple" in _abi.last_error()
            assert call(sinc, nbytes=total - 1) == bad and "recording 3" in _abi.last_error() and "src_bytes" in _abi.last_error()
            assert call(sinc, nbytes=25015) == bad and "recording 2" in _abi.last_error()
        # ... and only then the converting load's own: a negative length reads nothing and is refused as load_sinc refuses it
        assert call(True, n=[3000, -1, 1001, 500]) == bad and "src_samples[1]" in _abi.last_error()
        assert call(True, q=(3, 12.0, 0.9)) == bad
        assert call(True, n=[3000, 2000, 1002, 500], nbytes=total + 64) == bad and "recording 2" in _abi.last_error() and "1002" in _abi.last_error()
        assert (rows == SENTINEL).all(), "a refused call wrote to the rows"
        assert call() == _abi.OK and not (rows[:, :100] == SENTINEL).any()
        rows.fill_(SENTINEL)
        assert call(True) == _abi.OK and not (rows[:, :100] == SENTINEL).any()
        # the Python layer
        with pytest.raises(sd.SyllableDetectorError) as ei:
            rec.loadPCM(src[:total - 1].contiguous(), offsets, steps, formats)
        assert ei.value.status == bad
        with pytest.raises(ValueError):
            rec.loadPCM(torch.zeros(total, dtype=torch.int16, device="cuda"), offsets, steps, formats)
        with pytest.raises(ValueError):
            rec.loadPCM(src, offsets, steps, formats, out=torch.empty((2, rec.rowSamples), dtype=torch.int16, device="cuda"))
        with pytest.raises(ValueError):
            rec.loadPCM(src, offsets[:3], steps, formats)
