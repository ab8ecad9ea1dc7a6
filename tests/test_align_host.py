"""Event-aligned windows, the host side (no GPU): csrc/align_span.hpp alone under ASan and UBSan (a program of its own,
tests/cpp/align_span_test.cpp), the entry points under ABI 1, syldet_align_host and syldet_align_stats_host against the numpy model
of tests/align_ref.py for the three sources' anchor rules, and every status that needs no device.  No tolerance anywhere: the
contract is bit identity, NaN at the same places."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_aligner_create", "syldet_aligner_destroy", "syldet_aligner_shape", "syldet_align_anchor", "syldet_align_device",
       "syldet_align_stats_device", "syldet_align_host", "syldet_align_stats_host")
LENGTHS = [0, 255, 256, 387, 388, 1443, 1444, 1575, 1576, 5000, 12001, 30011]
LIMIT = 2 ** 62 - 1


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _events(cfg, n, seed):
    """the events of a recording of n samples: the grid of the issue, and 20 seeded random ones, unsorted and with repeats"""
    hop, need, T, first = ref.clock(cfg)
    last = first + max(ref.count_evals(cfg, n) - 1, 0) * hop
    rng = np.random.default_rng(seed)
    rnd = rng.integers(-1000, n + 1001, 20)
    rnd[15:] = rnd[:5]
    return [-5000, -1, 0, need - 1, need, first - 1, first, first + hop - 1, first + hop, last, n - 1, n, n + 10 ** 6, LIMIT, -LIMIT] + [int(v) for v in rnd]


def test_the_span_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "align_span_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "align_span_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    section = header[header.index("---- event-aligned windows"):]
    for word in ('"align_windows_kernel"', '"align_stats_kernel"', '"align_combine_kernel"', "align_span.hpp", "floor((s - origin) / step)",
                 "SYLDET_ALIGN_BLOCK"):
        assert word in section, word
    for name, value in (("COLUMNS", 0), ("OUTPUTS", 1), ("SAMPLES", 2)):
        assert re.search(r"#define SYLDET_ALIGN_%s +%d\b" % (name, value), header) and getattr(sd, "ALIGN_" + name) == value == getattr(ref, name)
    assert re.search(r"#define SYLDET_ALIGN_MAX_WINDOW +1048576\b", header) and _abi.ALIGN_MAX_WINDOW == 1 << 20
    assert re.search(r"#define SYLDET_ALIGN_BLOCK +256\b", header) and _abi.ALIGN_BLOCK == 256 == ref.BLOCK
    # the packed rows' columns are stated where the packed rows are
    packed = header[header.index("---- packed recordings: many recordings"):header.index("---- packed recordings at other rates")]
    assert "syldet_spectrogram_device on the" in packed and "syldet_count_frames(h, n_k)" in packed
    for name in ("aligner", "spectrogram", "columnsView"):
        assert callable(getattr(sd.Recordings, name))
    assert callable(sd.SyllableDetector.aligner) and callable(sd.Aligner.windows) and callable(sd.Aligner.stats)
    assert callable(sd.alignHost) and callable(sd.alignStatsHost)


@pytest.mark.parametrize("hop", [132, 131])
@pytest.mark.parametrize("source", [ref.COLUMNS, ref.OUTPUTS, ref.SAMPLES], ids=["columns", "outputs", "samples"])
def test_the_host_windows_equal_the_model(source, hop):
    cfg = util.sample_net() if hop == 132 else _hop131(util.sample_net())
    assert ref.clock(cfg)[0] == hop
    T = cfg.timeRange
    origin, step = ref.anchor(cfg, source)
    width = {ref.COLUMNS: 30, ref.OUTPUTS: 1, ref.SAMPLES: 1}[source]
    pairs = [(0, 0), (T - 1, 0), (0, 5), (7, 9), (300, 300)] + ([(0, 3), (1, 2), (2, 1), (3, 0)] if source == ref.SAMPLES else [])
    seen = dict.fromkeys(("whole", "left", "right", "both", "absent"), 0)
    for k, n in enumerate(LENGTHS):
        U = ref.units_of(cfg, source, n)
        units = np.random.default_rng(10 * k + source).standard_normal((U, width)).astype(np.float32)
        events = _events(cfg, n, 77 + k)
        for before, after in pairs:
            for fill in (np.float32(-7.0), np.float32(np.nan)):
                want, mask = ref.windows(units, events, origin, step, before, after, fill)
                got, present = sd.alignHost(units, events, before, after, origin, step, fill)
                ref.same(got, want, "source %d, n %d, (%d, %d)" % (source, n, before, after))
                assert np.array_equal(present, ref.present_pairs(mask))
            for key, v in ref.states(mask).items():
                seen[key] += v
    assert all(v > 0 for v in seen.values()), seen


def test_the_host_statistics_equal_the_model():
    rng = np.random.default_rng(5)
    L = 37
    for n_events in (0, 1, 255, 256, 257, 513):
        w = rng.standard_normal((n_events, L)).astype(np.float32) * np.float32(1e3)
        first = rng.integers(0, L + 1, n_events)
        count = np.array([rng.integers(0, L - f + 1) for f in first], np.int64)
        present = np.stack([first, count], axis=1).astype(np.int64).reshape(-1, 2)
        mask = (np.arange(L)[None, :] >= first[:, None]) & (np.arange(L)[None, :] < (first + count)[:, None])
        for fill in (np.float32(np.nan), np.float32(0.0)):
            x = np.where(mask, w, fill).astype(np.float32)
            if n_events > 3:
                x[3, :] = np.where(mask[3], np.float32(np.nan), x[3])    # a NaN inside the present part reaches the sums, at its positions
            got = sd.alignStatsHost(x, present)
            want = ref.stats_one(x, mask)
            for g, v, name in zip(got, want, ("count", "sum", "sumsq")):
                ref.same(g, v, "%s of %d events" % (name, n_events))
            assert np.array_equal(got[0], mask.sum(axis=0))
            if n_events > 3:
                assert np.array_equal(np.isnan(got[1]), mask[3]) and np.array_equal(np.isnan(got[2]), mask[3])
    # the tree is not the plain sum: values chosen so that the order of the additions shows
    x = np.ones((513, 1), np.float32)
    x[0] = np.float32(2.0 ** 60)
    pres = np.tile(np.array([[0, 1]], np.int64), (513, 1))
    got = sd.alignStatsHost(x, pres)[1][0]
    assert got == ref.stats_one(x, np.ones((513, 1), bool))[1][0] == 2.0 ** 60 + 256.0    # block 0 loses its ones, block 1 keeps 256 of them


def test_the_statuses_that_need_no_device():
    f = np.zeros(8, np.float32)
    ev = np.zeros(2, np.int64)
    out = np.zeros(64, np.float32)
    pres = np.zeros(4, np.int64)
    fp, ep, op, pp = (a.ctypes.data_as(t) for a, t in ((f, _abi.c_float_p), (ev, _abi.c_int64_p), (out, _abi.c_float_p), (pres, _abi.c_int64_p)))
    ok = lambda **kw: LIB.syldet_align_host(*[kw.get(k, v) for k, v in (("src", fp), ("n", 8), ("width", 1), ("origin", 0), ("step", 1), ("before", 1),
                                                                        ("after", 1), ("events", ep), ("n_events", 2), ("fill", 0.0), ("windows", op),
                                                                        ("present", pp))])
    assert ok() == 0 and ok(present=None) == 0 and ok(n=0, src=None) == 0 and ok(n_events=0, events=None, windows=None) == 0
    for bad in (dict(before=-1), dict(after=-1), dict(width=0), dict(step=0), dict(origin=-1), dict(origin=2 ** 32), dict(step=2 ** 31), dict(n=-1),
                dict(n_events=-1), dict(src=None), dict(events=None), dict(windows=None), dict(before=2 ** 20, after=0), dict(before=2 ** 19, after=2 ** 19),
                dict(width=4, before=2 ** 17, after=2 ** 17)):
        assert ok(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
    assert "limit" in _abi.last_error()
    assert ok(before=2 ** 19, after=2 ** 19 - 1, n_events=0) == 0         # exactly 2^20 elements
    cnt, s, q = np.zeros(4, np.int64), np.zeros(4), np.zeros(4)
    cp, sp, qp = cnt.ctypes.data_as(_abi.c_int64_p), s.ctypes.data_as(_abi.c_double_p), q.ctypes.data_as(_abi.c_double_p)
    assert LIB.syldet_align_stats_host(fp, pp, 2, 4, cp, sp, qp) == 0
    for args in ((None, pp, 2, 4, cp, sp, qp), (fp, None, 2, 4, cp, sp, qp), (fp, pp, -1, 4, cp, sp, qp), (fp, pp, 2, 0, cp, sp, qp),
                 (fp, pp, 2, 2 ** 20 + 1, cp, sp, qp), (fp, pp, 2, 4, None, sp, qp), (fp, pp, 2, 4, cp, None, qp), (fp, pp, 2, 4, cp, sp, None)):
        assert LIB.syldet_align_stats_host(*args) == _abi.ERR_INVALID_ARGUMENT, args
    pres[:] = (3, 2, 0, 0)                                                # a present span that leaves the window
    assert LIB.syldet_align_stats_host(fp, pp, 2, 4, cp, sp, qp) == _abi.ERR_INVALID_ARGUMENT
    # the calls on handles: NULL before anything else
    h = _abi.Handle()
    assert LIB.syldet_aligner_create(None, None, 0, 1, 1, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h
    assert LIB.syldet_aligner_create(None, None, 0, 1, 1, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_aligner_shape(None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_align_anchor(None, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_align_device(None, None, 0, 0, None, 0, ep, 0.0, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_align_stats_device(None, None, ep, None, 1, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_aligner_destroy(None) == 0
    # the bindings: a sharded bank has no aligner; the Python layer's own argument errors
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.aligner(object(), "columns", 1, 1)
    assert e.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sd.alignHost(np.zeros((4, 2), np.float64), [0], 1, 1, 0, 1)
    with pytest.raises(sd.SyllableDetectorError):
        sd.alignHost(np.zeros((4, 2), np.float32), [0], -1, 1, 0, 1)
    with pytest.raises(ValueError):
        sd.alignStatsHost(np.zeros((3, 4), np.float32), np.zeros((2, 2), np.int64))
