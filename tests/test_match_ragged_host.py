"""A ragged bank, the host side (no GPU): the numpy model of tests/match_ragged_ref.py against a brute-force loop on tiny arrays;
csrc/match_ragged.hpp alone under ASan and UBSan (a program of its own, tests/cpp/match_ragged_test.cpp: the plan, the two read
bounds, the window rule); the entry points under ABI 1; every refusal that needs no device, with the outputs untouched; and, on the
float64 model alone, the gap in which the threshold of the class of two exemplars of different lengths is fixed for the GPU tests."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import match_ragged_cases as rc
import match_ragged_ref as rref
import match_ref as ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_matcher_bank_create_ragged", "syldet_matcher_bank_lengths", "syldet_match_bank_peaks_each_device")
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_model_is_the_brute_force_loop_on_tiny_arrays():
    rng = np.random.default_rng(21)
    bins = 3
    for U in (0, 1, 4, 5, 9, 23):
        x = np.abs(rng.standard_normal((U, bins))).astype(np.float32)
        if U >= 9:
            x[6, 1] = NAN                                                 # the 1- and 2-frame windows miss it where the 5-frame one holds it
        if U >= 23:
            x[15, 0] = INF
            x[18:21] = 0
        for lengths, anchor, classes in (((1, 5, 2, 5), None, (0, 0, 1, 1)), ((1, 5, 2, 5), (0, 2, 1, 0), (0, 0, 1, 1)), ((3, 3), 1, None),
                                         ((5,), 0, None), ((2, 4, 4), (1, 0, 3), (0, 0, 0))):
            t = [ref.normalise(rng.standard_normal((n, bins))) for n in lengths]
            a = rref.anchors(lengths, anchor)
            s, w, per = rref.scores(t, x, anchor, classes)
            cls = list(range(len(lengths))) if classes is None else classes
            assert s.shape == (max(cls) + 1, U) and w.shape == s.shape and per.shape == (len(lengths), U)
            for u in range(U):
                best = {}
                for k, n in enumerate(lengths):
                    lo = u - a[k]
                    if lo < 0 or lo + n > U:                              # the window leaves the detector, in front or behind
                        assert np.isnan(per[k, u])
                        continue
                    win = x[lo:lo + n].astype(np.float64)
                    if not np.isfinite(win).all():
                        assert np.isnan(per[k, u])
                        continue
                    e = (win * win).sum()
                    v = 0.0 if e == 0 else (win * t[k].astype(np.float64)).sum() / np.sqrt(e)
                    assert abs(per[k, u] - v) < 1e-12
                    if cls[k] not in best or per[k, u] > per[best[cls[k]], u]:
                        best[cls[k]] = k
                for c in range(s.shape[0]):
                    assert w[c, u] == best.get(c, -1), (U, lengths, u, c)
                    assert np.isnan(s[c, u]) if c not in best else s[c, u] == per[best[c], u]
            # the float32 path the GPU tests take: single-matcher scores (indexed by the window's first frame) shifted, then the classes
            by_start = [ref.scores(tk, x)[0].astype(np.float32) for tk in t]
            s32, w32 = rref.classes(by_start, lengths, anchor, classes)
            assert s32.dtype == np.float32 and (np.isnan(s32) == np.isnan(s)).all() and (w32 == -1).tolist() == np.isnan(s).tolist()
    # somewhere a class is not NaN where one of its templates has no window, and where one of its templates holds a NaN
    x = np.abs(rng.standard_normal((9, bins))).astype(np.float32)
    x[6, 1] = NAN
    t = [ref.normalise(rng.standard_normal((n, bins))) for n in (1, 5)]
    s, w, per = rref.scores(t, x, None, (0, 0))
    assert np.isnan(per[1, :4]).all() and not np.isnan(s[0, :4]).any() and (w[0, :4] == 0).all()
    assert np.isnan(per[1, 7]) and np.isnan(per[0, 6]) and w[0, 7] == 0 and w[0, 6] == -1
    # the tables: a separation a class, the plane's own anchor 0
    planes = np.array([[0.1, 0.9, 0.2, 0.8, NAN], [0.5, 0.6, 0.5, 0.7, 0.7]], np.float32)
    wh = np.array([[0, 2, 0, 2, -1], [1, 1, 1, 1, 1]], np.int32)
    tb = rref.tables(planes, wh, [0.5, 0.4], [1, 0], 256, 132, 8)
    assert tb[0][0].tolist() == [256 + 132, 256 + 3 * 132] and tb[0][3].tolist() == [2, 2]
    assert tb[1][0].tolist() == [256 + k * 132 for k in range(5)] and tb[1][1] == 5
    assert rref.tables(planes, wh, [0.5, 0.4], 4, 256, 132, 8)[1][0].tolist() == [256 + 3 * 132]


def test_the_plan_and_the_window_rule_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "match_ragged_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "match_ragged_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.stdout, r.stderr)


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    bank = header[header.index("---- template matching: a bank of templates"):header.index("---- template matching: a ragged bank")]
    assert "NOT HERE: templates of different lengths" not in bank
    section = header[header.index("---- template matching: a ragged bank"):]
    for word in ('"match_ragged_scores_mfma_kernel"', '"match_ragged_scores_plain_kernel"', '"match_bank_peaks_each_kernel"', "match_ragged.hpp",
                 "INDEXED BY THE ANCHOR FRAME", "ON BOTH SIDES", "LOWEST k", "255 + a_max + r_max", "templates of different lengths",
                 "within one .npy file", "sharded banks"):
        assert word in section, word
    source = inspect.getsource(sd.MatcherBank.__init__)
    for name in ("self.ragged", "self.lengths", "self.anchors"):
        assert name in source, name


def test_the_refusals_that_need_no_device():
    fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
    ip = lambda a: a.ctypes.data_as(_abi.c_int32_p)
    t = np.ones(3 * 3 + 2 * 3, np.float32)
    n = np.array([3, 2], np.int32)
    h = _abi.Handle()
    # NULL before anything else, then the counts, the lengths and the anchors, all before the bank is looked at: a handle that is
    # not NULL but is never read (the calls below are refused in front of it)
    fake = C.cast(C.create_string_buffer(64), _abi.Handle)
    create = lambda hh=fake, tt=fp(t), K=2, nn=ip(n), bins=3, anc=None, cls=None, Cn=0, out=C.byref(h): LIB.syldet_matcher_bank_create_ragged(
        hh, None, tt, K, nn, bins, anc, cls, Cn, out)
    big = np.array([3, 32768 // 3 + 1], np.int32)
    for bad in (dict(hh=None), dict(out=None), dict(nn=None), dict(tt=None), dict(K=0), dict(K=65), dict(Cn=1), dict(Cn=17),
                dict(nn=ip(np.array([3, 0], np.int32))), dict(nn=ip(np.array([-1, 2], np.int32))), dict(nn=ip(big)), dict(bins=0),
                dict(anc=ip(np.array([3, 0], np.int32))), dict(anc=ip(np.array([0, 2], np.int32))), dict(anc=ip(np.array([-1, 0], np.int32))),
                dict(cls=ip(np.array([0, 2], np.int32)), Cn=2), dict(cls=ip(np.array([1, 1], np.int32)), Cn=2), dict(cls=ip(np.array([0, -1], np.int32)), Cn=1)):
        assert create(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert not h, bad
    ln, an, rg = np.full(2, 9, np.int32), np.full(2, 9, np.int32), C.c_int32(9)
    assert LIB.syldet_matcher_bank_lengths(None, ip(ln), ip(an), C.byref(rg)) == _abi.ERR_INVALID_ARGUMENT
    assert (ln == 9).all() and (an == 9).all() and rg.value == 9
    thr, sep = np.zeros(2, np.float32), np.zeros(2, np.int32)
    assert LIB.syldet_match_bank_peaks_each_device(None, None, None, 0, fp(thr), ip(sep), None, 0, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    # the bindings: a sharded bank has no ragged bank either; the Python layer's own argument errors
    parts = [np.ones((3, 3), np.float32), np.ones((2, 3), np.float32)]
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.matcherBank(object(), parts)
    assert e.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.matcherBank(object(), parts, None, [2, 1], ragged=True)
    assert e.value.status == _abi.ERR_UNSUPPORTED


def test_two_exemplars_of_different_lengths_on_the_model_alone():
    """The class of two exemplars -- all 12 frames of seed 1's second planted syllable and the last 10 of seed 4's, both anchored at
    the syllable's frame 11 -- on the float64 model over seeds 2 and 3: within one frame of frame 11 of every planted syllable the
    class scores at least 0.876 (0.8797 and 0.8766 are the two seeds' lowest), more than 12 frames from all of them at most 0.674
    (0.6731, 0.6720).  The threshold, 0.77, lies in that gap with 0.09 on either side."""
    ex, anc = rc.exemplars()
    assert [e.shape for e in ex] == [(12, 29), (10, 29)] and anc == [11, 9]
    t = [ref.normalise(e) for e in ex]
    for seed in mc.SEEDS:
        cols, frames = mc.columns64(seed).astype(np.float32), mc.planted(seed)[1]
        s, w, per = rref.scores(t, cols, anc, [0, 0])
        U = cols.shape[0]
        s32 = s[0].astype(np.float32)
        assert np.isnan(s32[:9]).all() and not np.isnan(s32[9:]).any()    # the shorter exemplar's first window; anchors are last frames
        assert np.isnan(per[0, :11]).all() and not np.isnan(per[0, 11:]).any()
        away = np.ones(U, bool)
        for f in frames:
            away[max(f + rc.MARK - 12, 0):f + rc.MARK + 13] = False
        near = min(s32[f + rc.MARK - 1:f + rc.MARK + 2].max() for f in frames if f + mc.N <= U)
        other = np.nanmax(s32[away])
        print("seed %d: lowest class score near a planted syllable %.4f, highest elsewhere %.4f" % (seed, near, other))
        assert other + 0.09 < rc.THRESHOLD < near - 0.09
        p = ref.peaks(s32, rc.THRESHOLD, rc.SEPARATION)
        assert len(frames) >= 20 and rc.found_once(p, frames, U), (seed, p.tolist(), frames.tolist())
        assert set(w[0][p].tolist()) == {0, 1}                            # each exemplar is the better one somewhere
