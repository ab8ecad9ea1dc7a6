"""Template matching, the host side (no GPU): the numpy model of tests/match_ref.py against brute-force loops on tiny arrays;
csrc/match_peaks.hpp alone under ASan and UBSan (a program of its own, tests/cpp/match_peaks_test.cpp); syldet_match_peaks_host
against the model to the last event; syldet_match_scores_host within the derived bar of the float64 model; the normalised
template; detection quality on the model alone (which fixes the fixture and threshold the GPU tests reuse); the entry points
under ABI 1; and every status that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref
import train_cases
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_matcher_create", "syldet_matcher_destroy", "syldet_matcher_shape", "syldet_matcher_template", "syldet_match_scores_device",
       "syldet_match_peaks_device", "syldet_match_normalize_host", "syldet_match_scores_host", "syldet_match_peaks_host")
NAN, INF = float("nan"), float("inf")


def peak_cases():
    """(name, scores float32, threshold, S, capacity): what the issue lists, shared with the GPU test"""
    rng = np.random.default_rng(7)
    out = []
    plateau = np.array([0.1, 0.5, 0.5, 0.5, 0.2, 0.5, 0.1, 0.5, 0.5, 0.0, 0.0, 0.5], np.float32)
    for S in (0, 1, 2, 3, 4, 11, 12, 4096):
        out.append(("plateaus S=%d" % S, plateau, 0.0, S, 64))
    ten = rng.uniform(0, 1, 10).astype(np.float32)
    out.append(("S=4096 on 10 positions", ten, 0.0, 4096, 64))
    out.append(("S=0", ten, 0.5, 0, 64))
    runs = rng.uniform(0, 1, 300).astype(np.float32)
    runs[0:3] = NAN
    runs[40:90] = NAN
    runs[100] = NAN
    runs[297:] = NAN
    for S in (1, 7, 64):
        out.append(("NaN runs S=%d" % S, runs, 0.3, S, 512))
    out.append(("all NaN", np.full(17, NAN, np.float32), -INF, 3, 8))
    low = np.array([-INF, NAN, -INF, -1.0, NAN, -INF, 0.0, -0.0, NAN], np.float32)
    for S in (0, 1, 2, 5):
        out.append(("threshold -inf S=%d" % S, low, -INF, S, 64))
    many = rng.integers(0, 4, 5000).astype(np.float32)
    out.append(("capacity below the count", many, 1.0, 2, 5))
    out.append(("capacity 0", many, 1.0, 2, 0))
    ends = np.array([0.9, 0.1, 0.2, 0.1, 0.3, 0.95], np.float32)
    for S in (1, 3, 5, 6):
        out.append(("a peak at both ends S=%d" % S, ends, 0.5, S, 8))
    out.append(("one position", np.array([0.4], np.float32), 0.4, 9, 8))
    out.append(("no position", np.zeros(0, np.float32), 0.0, 9, 8))
    long = rng.integers(0, 50, 6000).astype(np.float32) / 50
    long[rng.integers(0, 6000, 300)] = NAN
    for S in (1, 5, 100, 1000, 4096):
        out.append(("6000 positions S=%d" % S, long, 0.5, S, 6000))
    return out


def _brute_peaks(s, threshold, S):
    out = []
    for p in range(len(s)):
        if np.isnan(s[p]) or not s[p] >= np.float32(threshold):
            continue
        ok = True
        for q in range(max(0, p - S), min(len(s), p + S + 1)):
            if q == p or np.isnan(s[q]):
                continue
            if (q < p and not s[q] < s[p]) or (q > p and not s[q] <= s[p]):
                ok = False
        if ok:
            out.append(p)
    return out


def test_the_model_is_the_brute_force_loop_on_tiny_arrays():
    rng = np.random.default_rng(1)
    for n, bins, U in ((1, 1, 5), (2, 3, 7), (3, 2, 3), (3, 2, 2), (4, 5, 12)):
        t = ref.normalise(rng.standard_normal((n, bins)))
        assert abs(float((t.astype(np.float64) ** 2).sum()) - 1) < 1e-6
        x = train_cases.columns(rng, U, bins)
        if U > 5:
            x[1] = 0
            x[U - 2, 0] = NAN
        if U == 12:
            x[2:6] = 0                                                    # an all-zero window (n = 4)
        s, A, E = ref.scores(t, x)
        for p in range(U):
            w = x[p:p + n].astype(np.float64)
            if p + n > U or not np.isfinite(w).all():
                assert np.isnan(s[p]) and np.isnan(A[p]) and np.isnan(E[p])
                continue
            dot = sum(float(t[j, b]) * w[j, b] for j in range(n) for b in range(bins))
            e = sum(w[j, b] ** 2 for j in range(n) for b in range(bins))
            want = dot / np.sqrt(e) if e > 0 else 0.0
            assert s[p] == pytest.approx(want, rel=1e-13, abs=1e-300) and E[p] == pytest.approx(e, rel=1e-13)
            assert A[p] == pytest.approx(sum(abs(float(t[j, b]) * w[j, b]) for j in range(n) for b in range(bins)), rel=1e-13)
        if U == 12:
            assert s[2] == 0.0 and not np.signbit(s[2])
    for name, s, thr, S, _ in peak_cases():
        if s.size <= 300:
            assert ref.peaks(s, thr, S).tolist() == _brute_peaks(s, thr, S), name
    assert ref.events([0, 5], 256, 132, 11) == [256 + 11 * 132, 256 + 16 * 132]


def test_the_peaks_rule_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "match_peaks_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "match_peaks_test.cpp"),
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
    section = header[header.index("---- template matching"):]
    for word in ('"match_scores_mfma_kernel"', '"match_scores_plain_kernel"', '"match_peaks_kernel"', "match_peaks.hpp", "v_mfma_f32_16x16x4_f32",
                 "A SCORE IS A FUNCTION OF ITS WINDOW'S VALUES AND t^ ALONE", "E == 0 gives +0.0", "earliest position of a tie wins"):
        assert word in section, word
    assert re.search(r"#define SYLDET_MATCH_MAX_TEMPLATE +32768\b", header) and _abi.MATCH_MAX_TEMPLATE == 32768
    assert re.search(r"#define SYLDET_MATCH_MAX_SEPARATION +4096\b", header) and _abi.MATCH_MAX_SEPARATION == 4096
    assert callable(sd.SyllableDetector.matcher) and callable(sd.Recordings.matcher)
    for name in ("scores", "peaks", "find"):
        assert callable(getattr(sd.Matcher, name)), name


@pytest.mark.parametrize("case", peak_cases(), ids=lambda c: c[0])
def test_the_host_peaks_equal_the_model_to_the_last_event(case):
    _, s, thr, S, cap = case
    for origin, hop, anchor in ((256, 132, 11), (0, 1, 0), (300, 131, 3)):
        want_ev, want_n, want_sc = ref.tables(s, thr, S, origin, hop, anchor, cap)
        ev, n, sc = sd.matchPeaksHost(s, thr, S, origin, hop, anchor, capacity=cap)
        assert n == want_n and ev.tolist() == want_ev.tolist() and sc.tobytes() == want_sc.tobytes()
        assert (np.diff(ev) > 0).all()


def test_the_cases_hold_what_they_are_for():
    seen = {name: ref.tables(s, thr, S, 0, 1, 0, cap) for name, s, thr, S, cap in peak_cases()}
    assert seen["plateaus S=1"][0].tolist() == [1, 5, 7, 11]                 # the earliest of a tie within S wins
    assert seen["plateaus S=2"][0].tolist() == [1, 11] and seen["plateaus S=0"][1] == 12
    assert seen["S=4096 on 10 positions"][1] == 1 and seen["all NaN"][1] == 0
    assert seen["capacity below the count"][1] > 5 == len(seen["capacity below the count"][0]) and seen["capacity 0"][1] > 0
    assert seen["a peak at both ends S=1"][0].tolist() == [0, 5] and seen["a peak at both ends S=5"][0].tolist() == [5]
    assert seen["threshold -inf S=0"][1] == 6 and seen["threshold -inf S=1"][0].tolist() == [0, 3, 6]          # (a NaN neither matches nor suppresses; -0.0 ties with +0.0)


@pytest.mark.parametrize("bins,n", [(7, 1), (7, 3), (29, 12), (29, 91), (116, 17), (1, 16)])
def test_the_host_scores_lie_within_the_bar_of_the_model(bins, n):
    rng = np.random.default_rng(bins * 100 + n)
    U, at = 3 * n + 60, 2 * n + 20
    x = train_cases.columns(rng, U, bins)
    x[5:5 + n + 2] = 0                                                    # three all-zero windows
    x[at, bins // 2] = NAN
    x[U - 3, 0] = INF
    t = sd.matchNormalizeHost((rng.standard_normal((n, bins)) * 3).astype(np.float32))        # negative values too
    got = sd.matchScoresHost(t, x)
    s, A, E = ref.scores(t, x)
    assert np.array_equal(np.isnan(got), np.isnan(s))
    assert np.isnan(got[U - n + 1:]).all() and np.isnan(got[at - n + 1:at + 1]).all() and not np.isnan(got[[at - n, at + 1]]).any()
    ok = ~np.isnan(s)
    zero = ok & (E == 0)
    assert zero.sum() >= 3 and (got[zero] == 0).all() and not np.signbit(got[zero]).any()
    live = ok & ~zero
    err, bar = np.abs(got[live].astype(np.float64) - s[live]), ref.bar(n, bins, A[live], E[live])
    assert live.sum() > 10 and (err <= bar).all(), float((err / bar).max())


def test_the_normalised_template():
    rng = np.random.default_rng(3)
    t = (rng.standard_normal((5, 7)) * 1e-3).astype(np.float32)
    assert sd.matchNormalizeHost(t).tobytes() == ref.normalise(t).tobytes()
    assert sd.matchNormalizeHost(t * 1e6).tobytes() == ref.normalise(t * np.float32(1e6)).tobytes()


def test_detection_quality_on_the_model_alone():
    """the experiment of the issue: a 12-frame exemplar from seed 1's second planted syllable finds, at threshold 0.77 and separation
    12, every planted syllable of seeds 2 and 3 once within one frame, and nothing else"""
    t = ref.normalise(mc.exemplar())
    for seed in mc.SEEDS:
        cols, frames = mc.columns64(seed).astype(np.float32), mc.planted(seed)[1]
        s = ref.scores(t, cols)[0]
        P = cols.shape[0] - mc.N + 1
        s32 = s[:P].astype(np.float32)
        p = ref.peaks(s32, mc.THRESHOLD, mc.SEPARATION)
        assert len(frames) >= 20 and mc.found_once(p, frames, P), (seed, p.tolist(), frames.tolist())
        # ... with room on either side of the threshold
        away = np.ones(P, bool)
        for f in frames:
            away[max(f - 12, 0):f + 13] = False
        assert s32[away].max() < 0.70 and min(s32[max(f - 2, 0):f + 3].max() for f in frames if f < P) > 0.84


def test_the_statuses_that_need_no_device():
    t = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    that = np.full((2, 3), 5.0, np.float32)
    x = np.ones((6, 3), np.float32)
    sc = np.full(6, 7.0, np.float32)
    ev, evs, cnt = np.full(4, -1, np.int64), np.full(4, 9.0, np.float32), C.c_int64(-5)
    fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
    # the template
    norm = lambda **kw: LIB.syldet_match_normalize_host(*[kw.get(k, v) for k, v in (("t", fp(t)), ("n", 2), ("bins", 3), ("out", fp(that)))])
    bad_nan, bad_inf, zero = t.copy(), t.copy(), np.zeros((2, 3), np.float32)
    bad_nan[1, 1], bad_inf[0, 2] = NAN, INF
    for bad in (dict(t=None), dict(out=None), dict(n=0), dict(bins=0), dict(n=-1), dict(n=32768, bins=2), dict(n=32769, bins=1), dict(t=fp(bad_nan)),
                dict(t=fp(bad_inf)), dict(t=fp(zero))):
        assert norm(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert (that == 5.0).all(), bad
    assert norm() == 0 and that.tobytes() == ref.normalise(t).tobytes()
    # the scores
    score = lambda **kw: LIB.syldet_match_scores_host(*[kw.get(k, v) for k, v in (("t", fp(that)), ("n", 2), ("bins", 3), ("x", fp(x)), ("U", 6), ("out", fp(sc)))])
    for bad in (dict(t=None), dict(x=None), dict(out=None), dict(n=0), dict(bins=0), dict(U=-1), dict(n=32768, bins=2)):
        assert score(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert (sc == 7.0).all(), bad
    assert score(U=0, x=None, out=None) == 0 and score() == 0 and np.isnan(sc[5]) and not np.isnan(sc[:5]).any()
    # the peaks
    names = (("s", fp(sc)), ("P", 5), ("thr", 0.0), ("S", 2), ("origin", 256), ("hop", 132), ("anchor", 1), ("ev", ev.ctypes.data_as(_abi.c_int64_p)), ("cap", 4),
             ("cnt", C.byref(cnt)), ("evs", fp(evs)))
    peaks = lambda **kw: LIB.syldet_match_peaks_host(*[kw.get(k, v) for k, v in names])
    for bad in (dict(s=None), dict(ev=None), dict(cnt=None), dict(P=-1), dict(thr=NAN), dict(S=-1), dict(S=4097), dict(cap=-1), dict(hop=0), dict(hop=2 ** 31),
                dict(origin=-1), dict(origin=2 ** 32), dict(anchor=-1), dict(anchor=32768), dict(P=2 ** 31)):
        assert peaks(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert (ev == -1).all() and (evs == 9.0).all() and cnt.value == -5, bad
    assert peaks(evs=None) == 0 and cnt.value >= 1 and peaks(cap=0, ev=None, evs=None) == 0 and peaks(P=0, s=None) == 0 and cnt.value == 0
    assert peaks(thr=-INF, S=4096) == 0 and peaks(thr=INF, S=0) == 0
    # the calls on handles: NULL before anything else
    h = _abi.Handle()
    assert LIB.syldet_matcher_create(None, None, fp(t), 2, 3, -1, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h
    assert LIB.syldet_matcher_create(None, None, fp(t), 2, 3, -1, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_shape(None, None, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_template(None, fp(that)) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_match_scores_device(None, None, 0, 0, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_match_peaks_device(None, None, 0, 0.0, 0, None, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_destroy(None) == 0
    # the bindings: a sharded bank has no matcher; the Python layer's own argument errors
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.matcher(object(), t)
    assert e.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sd.matchScoresHost(t, np.ones((4, 2), np.float32))
    with pytest.raises(sd.SyllableDetectorError):
        sd.matchPeaksHost(sc, NAN, 1, 0, 1, 0)
