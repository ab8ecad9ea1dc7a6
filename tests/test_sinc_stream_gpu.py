"""The streaming band-limited resampler (syldet_sinc_resampler_*, ResamplerSinc) on the GPU.  The contract has no tolerance: however
a recording is cut into pushes, the concatenated outputs are syldet_convert_rate_sinc_device's on the same rows, bit for bit -- that
call is the reference of every comparison here (tests/test_sinc_gpu.py holds it to the fp64 model), and equality is torch.equal.
Output buffers are filled with a sentinel; after every call everything it had no business writing is checked."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import sinc_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi
from test_sinc_gpu import DEFAULTS, RATIOS, SENTINEL, device_convert, strided

pytestmark = pytest.mark.gpu

LIB = _abi.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _abi.ERR_INVALID_ARGUMENT
CASES = [(ri, ro, DEFAULTS) for ri, ro in RATIOS] + [(48000.0, 44100.0, (8, 6.0, 0.8)), (48000.0, 44100.0, (64, 12.0, 0.9))]
PARTITIONS = {"one push": lambda n: [n],
              "ragged": lambda n: [0, 1, 1, 7, 64, 0, 500, 1, 1023, 1024, n - 2621],
              "callbacks of 32": lambda n: [32] * (n // 32) + ([n % 32] if n % 32 else []),
              "300 single samples": lambda n: [1] * 300 + [n - 300]}


def pushes_of(size, n):
    return [size] * (n // size) + ([n % size] if n % size else [])


class Handle:
    def __init__(self, ri, ro, channels, quality=DEFAULTS):
        self.ri, self.ro, self.channels, self.quality = ri, ro, channels, quality
        self.h = _abi.Handle()
        Z, beta, rho = quality
        assert LIB.syldet_sinc_resampler_create(ri, ro, channels, 0, Z, beta, rho, C.byref(self.h)) == _abi.OK, _abi.last_error()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        LIB.syldet_sinc_resampler_destroy(self.h)
        return False

    def position(self):
        n, m, f = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
        assert LIB.syldet_sinc_resampler_position(self.h, C.byref(n), C.byref(m), C.byref(f)) == _abi.OK
        return n.value, m.value, f.value

    def ready(self, n):
        return LIB.syldet_sinc_ready(n, self.ri, self.ro, self.quality[0], self.quality[2])


class Sink:
    """The output rows of one stream: [C, total + 5] sentinels, out_stride apart; every call writes behind what is there."""

    def __init__(self, channels, total, pad=5):
        self.total, self.stride = total, total + pad
        self.buf = torch.full((channels, self.stride), SENTINEL, dtype=torch.float32, device="cuda")

    def at(self, m):
        return self.buf.data_ptr() + 4 * m

    def untouched_from(self, m):
        torch.cuda.synchronize()
        return bool((self.buf[:, m:] == SENTINEL).all())


def push(hd, sink, rows, check=True):
    """One push of rows [C, n] (a view: float32 or int16, rows stride(0) apart) with every per-push check of the contract."""
    n = rows.shape[1]
    N0, M0, fin = hd.position()
    want = LIB.syldet_sinc_resampler_count(hd.h, n)
    got = C.c_int64(-1)
    fn = LIB.syldet_sinc_resample_device_s16 if rows.dtype == torch.int16 else LIB.syldet_sinc_resample_device
    st = fn(hd.h, rows.data_ptr() if n else None, n, rows.stride(0), sink.at(M0) if want else None, sink.stride, C.byref(got),
            torch.cuda.current_stream().cuda_stream)
    assert st == _abi.OK, _abi.last_error()
    assert got.value == want and want >= 0
    N1, M1, fin = hd.position()
    assert (N1, M1, fin) == (N0 + n, M0 + want, 0)
    assert M1 == hd.ready(N1)
    if check:
        assert sink.untouched_from(M1), "wrote behind its outputs"
    return want


def flush(hd, sink):
    N0, M0, _ = hd.position()
    want = LIB.syldet_sinc_resampler_flush_count(hd.h)
    got = C.c_int64(-1)
    st = LIB.syldet_sinc_resampler_flush_device(hd.h, sink.at(M0) if want else None, sink.stride, C.byref(got), torch.cuda.current_stream().cuda_stream)
    assert st == _abi.OK, _abi.last_error()
    assert got.value == want
    assert hd.position() == (N0, M0 + want, 1)
    assert M0 + want == LIB.syldet_convert_rate_count(N0, hd.ri, hd.ro) == sink.total
    assert sink.untouched_from(sink.total), "wrote behind the rows"
    return want


def stream(rows, ri, ro, quality, partition, kinds=None, hd=None, check=True):
    """rows: a view [C, n], or {dtype: view} of the same samples with kinds[j] naming push j's -> the concatenated outputs."""
    views = rows if isinstance(rows, dict) else {rows.dtype: rows}
    first = next(iter(views.values()))
    Cn, n = first.shape
    assert sum(partition) == n
    sink = Sink(Cn, sinc_ref.count(n, ri, ro))
    own = hd is None
    hd = Handle(ri, ro, Cn, quality) if own else hd
    try:
        pos = 0
        for j, size in enumerate(partition):
            v = views[kinds[j % len(kinds)]] if kinds else first
            push(hd, sink, v[:, pos:pos + size], check)
            pos += size
        flush(hd, sink)
    finally:
        if own:
            LIB.syldet_sinc_resampler_destroy(hd.h)
    return sink.buf[:, :sink.total]


@functools.lru_cache(maxsize=None)
def rows_of(ri, ro, n, channels=3, seed=0):
    x = np.random.default_rng([seed, n, int(ri), int(ro)]).uniform(-1.0, 1.0, (channels, n)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def whole(ri, ro, n, quality, channels=3, seed=0):
    """The whole-recording call's outputs on the case's rows (on the device, made once, never written)."""
    got, st = device_convert(strided(rows_of(ri, ro, n, channels, seed), n + 7), ri, ro, quality)
    assert st == _abi.OK
    return got.clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("partition", list(PARTITIONS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%g-%g-Z%d" % (c[0], c[1], c[2][0]))
def test_any_partition_gives_the_whole_recordings_bits(case, partition):
    ri, ro, quality = case
    n = 3000
    rows = strided(rows_of(ri, ro, n), n + 11)
    got = stream(rows, ri, ro, quality, PARTITIONS[partition](n))
    assert same_bits(got, whole(ri, ro, n, quality)), (case, partition)


def test_pushes_shorter_than_the_filter_throughout():
    """16 : 1 at Z = 64: H = 1137.8 input samples, pushes of 100 -- no push alone completes an output's taps; 1 : 16: one input
    makes 16 outputs, several workgroups a push."""
    q = (64, 12.0, 0.9)
    for ri, ro, n in ((16.0, 1.0, 8192), (1.0, 16.0, 600)):
        rows = strided(rows_of(ri, ro, n), n + 3)
        got = stream(rows, ri, ro, q, pushes_of(100, n))
        assert same_bits(got, whole(ri, ro, n, q)), (ri, ro)


@pytest.mark.parametrize("rates", RATIOS)
def test_rows_shorter_than_the_filter(rates):
    ri, ro = rates
    for n in (1, 2, 40):
        got = stream(strided(rows_of(ri, ro, n), n + 7), ri, ro, DEFAULTS, [n])
        assert same_bits(got, whole(ri, ro, n, DEFAULTS)), (rates, n)
    with Handle(ri, ro, 3) as hd:                            # a flush on an empty stream emits 0
        sink = Sink(3, 0)
        assert flush(hd, sink) == 0 and hd.position() == (0, 0, 1)


def test_late_positions():
    """n_in = 2^24 + 1000 in pushes of 2^20 + 17: by then the absolute indices are past what an fp32 position could hold."""
    ri, ro, n = 48000.0, 44100.0, 2 ** 24 + 1000
    x = torch.from_numpy(np.random.default_rng(24).uniform(-1.0, 1.0, (1, n)).astype(np.float32)).cuda()
    want, st = device_convert(x, ri, ro)
    assert st == _abi.OK
    got = stream(x, ri, ro, DEFAULTS, pushes_of(2 ** 20 + 17, n))
    assert same_bits(got, want)


def test_int16_pushes_and_alternating_pushes():
    ri, ro, n = 48000.0, 44100.0, 3000
    q16 = np.random.default_rng(16).integers(-32768, 32768, (3, n)).astype(np.int16)
    q16[0, :4] = [-32768, 32767, 0, -1]
    as_float = (q16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    r16, r32 = strided(q16, n + 1, 1), strided(as_float, n + 4)
    want, st = device_convert(r32, ri, ro)
    assert st == _abi.OK
    assert same_bits(device_convert(r16, ri, ro)[0], want)
    part = PARTITIONS["ragged"](n)
    all32 = stream(r32, ri, ro, DEFAULTS, part)
    all16 = stream(r16, ri, ro, DEFAULTS, part)
    assert same_bits(all32, want) and same_bits(all16, all32)
    views = {torch.int16: r16, torch.float32: r32}
    for kinds in ([torch.int16, torch.float32], [torch.float32, torch.int16, torch.int16]):
        assert same_bits(stream(views, ri, ro, DEFAULTS, pushes_of(32, n), kinds=kinds, check=False), want), kinds


def test_independence_of_channels_strides_handles_and_runs():
    ri, ro, n = 48000.0, 44100.0, 3000
    x = rows_of(ri, ro, n)
    want = whole(ri, ro, n, DEFAULTS)
    part = PARTITIONS["ragged"](n)
    alone = stream(torch.from_numpy(x[2:3].copy()).cuda(), ri, ro, DEFAULTS, part)
    assert same_bits(alone[0], want[2])
    for stride in (n, n + 13, 4096):
        assert same_bits(stream(strided(x, stride), ri, ro, DEFAULTS, part)[2], alone[0]), stride
    # two handles of different ratios pushed alternately on one stream
    ri2, ro2 = 44100.0, 48000.0
    x2 = rows_of(ri2, ro2, n)
    a, b = strided(x, n + 5), strided(x2, n + 9)
    with Handle(ri, ro, 3) as ha, Handle(ri2, ro2, 3) as hb:
        sa, sb = Sink(3, sinc_ref.count(n, ri, ro)), Sink(3, sinc_ref.count(n, ri2, ro2))
        for pos in range(0, n, 250):
            push(ha, sa, a[:, pos:pos + 250], check=False)
            push(hb, sb, b[:, pos:pos + 250], check=False)
        flush(ha, sa)
        flush(hb, sb)
        assert same_bits(sa.buf[:, :sa.total], want) and same_bits(sb.buf[:, :sb.total], whole(ri2, ro2, n, DEFAULTS))
        # reset after a flush, then the same pushes: the same bits (a second run)
        assert LIB.syldet_sinc_resampler_reset(ha.h) == _abi.OK and ha.position() == (0, 0, 0)
        again = stream(a, ri, ro, DEFAULTS, part, hd=ha)
        assert same_bits(again, want)
    assert same_bits(stream(a, ri, ro, DEFAULTS, part), want)


def test_refused_calls_leave_the_stream_as_it_was():
    ri, ro, n = 48000.0, 44100.0, 3000
    rows = strided(rows_of(ri, ro, n), n + 7)
    want = whole(ri, ro, n, DEFAULTS)
    s = torch.cuda.current_stream().cuda_stream
    for fn, kind in ((LIB.syldet_sinc_resample_device, np.float32), (LIB.syldet_sinc_resample_device_s16, np.int16)):
        with Handle(ri, ro, 3) as hd:
            sink = Sink(3, sinc_ref.count(n, ri, ro))
            other = strided(np.zeros((3, 600), kind), 607)    # the refused calls' rows: the right type, never read
            push(hd, sink, rows[:, :1000])
            pos = hd.position()
            count = LIB.syldet_sinc_resampler_count(hd.h, 500)
            assert count > 1
            got = C.c_int64(-1)
            refused = [(other.data_ptr(), -1, 607, sink.at(pos[1]), sink.stride),              # a negative n_in
                       (None, 500, 607, sink.at(pos[1]), sink.stride),                         # a NULL input with n_in > 0
                       (other.data_ptr(), 500, 607, None, sink.stride),                        # a NULL output when something is emitted
                       (other.data_ptr(), 500, 607, sink.at(pos[1]), count - 1),               # an out_stride below the count
                       (other.data_ptr(), 500, 499, sink.at(pos[1]), sink.stride)]             # an in_stride below the row
            for d_in, n_in, in_stride, d_out, out_stride in refused:
                got.value = -1
                assert fn(hd.h, d_in, n_in, in_stride, d_out, out_stride, C.byref(got), s) == INV
                assert got.value == 0 and hd.position() == pos and sink.untouched_from(pos[1])
            got.value = -1
            assert LIB.syldet_sinc_resampler_flush_device(hd.h, None, sink.stride, C.byref(got), s) == INV      # the flush owes outputs
            assert got.value == 0 and hd.position() == pos
            # a push of nothing is legal, with no buffers at all
            assert fn(hd.h, None, 0, 0, None, 0, C.byref(got), s) == _abi.OK and got.value == 0 and hd.position() == pos
            # the stream continues and ends with the right bits
            push(hd, sink, rows[:, 1000:2000])
            push(hd, sink, rows[:, 2000:])
            flush(hd, sink)
            assert same_bits(sink.buf[:, :sink.total], want)
            # a push after the flush
            done = hd.position()
            got.value = -1
            assert fn(hd.h, other.data_ptr(), 100, 607, sink.at(0), sink.stride, C.byref(got), s) == INV
            assert got.value == 0 and hd.position() == done and same_bits(sink.buf[:, :sink.total], want)
            assert LIB.syldet_sinc_resampler_count(hd.h, 100) == 0 and LIB.syldet_sinc_resampler_flush_count(hd.h) == 0
            assert LIB.syldet_sinc_resampler_flush_device(hd.h, None, 0, C.byref(got), s) == _abi.OK and got.value == 0      # nothing owed


def test_the_python_class_reproduces_convertRate():
    ri, ro, n = 48000.0, 44100.0, 3000
    x = rows_of(ri, ro, n)
    rows = torch.from_numpy(x.copy()).cuda()
    want = sd.convertRate(rows, ri, ro, method="sinc")
    assert same_bits(want, whole(ri, ro, n, DEFAULTS))
    cuts = [0, 32, 33, 1500, 1500, n]
    with sd.ResamplerSinc(ri, ro, channels=3) as r:
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            expect = r.countOutput(b - a)
            parts.append(r.resampleVector(rows[:, a:b]))
            assert parts[-1].shape == (3, expect)
        assert r.position == (n, sd.sincReady(n, ri, ro), False)
        parts.append(r.flush())
        assert r.position == (n, want.shape[1], True)
        assert same_bits(torch.cat(parts, dim=1), want)
        with pytest.raises(sd.SyllableDetectorError):
            r.resampleVector(rows[:, :10])                   # finished
        r.reset()
        host = [r.resampleArray(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [r.flushArray()]
        assert np.array_equal(np.concatenate(host, axis=1).view(np.int32), want.cpu().numpy().view(np.int32))
    # one channel as a vector, another quality, int16
    q = (8, 6.0, 0.8)
    q16 = torch.from_numpy(np.random.default_rng(3).integers(-32768, 32768, (n,)).astype(np.int16)).cuda()
    want16 = sd.convertRate(q16, ri, ro, "sinc", *q)
    with sd.ResamplerSinc(ri, ro, zeroCrossings=q[0], beta=q[1], rolloff=q[2]) as r:
        parts = [r.resampleVector(q16[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [r.flush().reshape(-1)]
        assert same_bits(torch.cat(parts), want16)
    with pytest.raises(sd.SyllableDetectorError):
        sd.ResamplerSinc(ri, ro, zeroCrossings=2)


def test_live_input_through_the_resampler_into_the_detector():
    """Two seconds of one channel at 48 kHz through ResamplerSinc (Z = 8) in 32-frame pushes into appendAudioData / processAll:
    the outputs and flags of `run` on convertRate(..., "sinc", zeroCrossings=8) of the whole row, bit for bit.  (The streaming and
    the batch path of the detector are equal on this network: tests/test_parity_gpu.py.)"""
    from syllable_detector_swift_amd import synth
    cfg = util.sample_net()
    ri, ro = 48000.0, 44100.0
    at_net = synth.syllable_channel(88400, util.template(), seed=11)
    x = sd.convertRate(torch.from_numpy(at_net).cuda(), ro, ri, "sinc").contiguous()      # the "device" signal at 48 kHz
    x = x[:96000]
    whole_row = sd.convertRate(x, ri, ro, "sinc", zeroCrossings=8)
    with sd.SyllableDetector(cfg, channels=1) as det, sd.ResamplerSinc(ri, ro, zeroCrossings=8) as r:
        parts = [r.resampleVector(x[pos:pos + 32]) for pos in range(0, x.shape[0], 32)]
        parts.append(r.flush().reshape(-1))
        assert same_bits(torch.cat(parts), whole_row)
        sizes = [int(p.shape[0]) for p in parts]
        host = torch.cat(parts).cpu().numpy()
        outs, flags, pos = [], [], 0
        for j, size in enumerate(sizes):
            det.appendAudioData(host[pos:pos + size])
            pos += size
            if j % 128 == 127 or j == len(sizes) - 1:
                det.processAll()
                while det.processNewValue():
                    outs.append(det.lastOutputs)
                    flags.append(det.lastDetected)
        want_out, want_fl = det.run(whole_row.reshape(1, -1))
        torch.cuda.synchronize()
        want_out, want_fl = want_out.cpu().numpy()[0], want_fl.cpu().numpy()[0]
    got = np.array(outs, np.float32).reshape(-1, want_out.shape[1])
    assert got.shape == want_out.shape and want_out.shape[0] > 600
    assert np.array_equal(got.view(np.int32), want_out.astype(np.float32).view(np.int32))
    assert np.array_equal(np.array(flags, bool), want_fl.astype(bool)) and want_fl.sum() > 0


def test_cpp_mirror_program(tmp_path):
    """tests/cpp/resampler_sinc_test.cpp: syldetxx::ResamplerSinc, one row in three pushes, against the C call."""
    lib = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
    exe = str(tmp_path / "resampler_sinc_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "resampler_sinc_test.cpp"), "-o", exe, "-L" + lib, "-lsyldet", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
