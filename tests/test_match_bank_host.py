"""A bank of templates, the host side (no GPU): the numpy model of tests/match_bank_ref.py against brute-force loops on tiny arrays;
csrc/match_classes.hpp alone under ASan and UBSan (a program of its own, tests/cpp/match_classes_test.cpp);
syldet_match_classes_host against the model to the last bit and index; the entry points under ABI 1; every refusal that needs no
device; and, on the float64 model alone, the gap in which the two-exemplar class's threshold is fixed for the GPU tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import match_bank_cases as bc
import match_bank_ref as bref
import match_cases as mc
import match_ref as ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_matcher_bank_create", "syldet_matcher_bank_destroy", "syldet_matcher_bank_shape", "syldet_matcher_bank_templates",
       "syldet_match_bank_scores_device", "syldet_match_bank_peaks_device", "syldet_match_classes_host")
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def class_cases():
    """(name, template scores [K, P] float32, classes or None)"""
    rng = np.random.default_rng(11)
    out = []
    s = rng.uniform(-1, 1, (5, 40)).astype(np.float32)
    s[:, 3] = NAN                                                         # a position without a window: NaN for every template
    s[:, 7] = 0.0                                                         # silence: +0.0 for every template
    s[:, 9] = NAN
    out.append(("identity classes", s, None))
    out.append(("classes (0, 0, 1, 0, 2)", s, [0, 0, 1, 0, 2]))
    dup = s.copy()
    dup[3] = dup[1]                                                       # a duplicated template in a class: which is the lower k
    out.append(("templates 1 and 3 the same", dup, [0, 1, 0, 1, 1]))
    few = rng.integers(0, 3, (8, 200)).astype(np.float32) / 2             # few values: ties everywhere
    few[:, rng.integers(0, 200, 30)] = NAN
    out.append(("ties", few, [1, 0, 1, 1, 0, 2, 2, 0]))
    out.append(("one template", s[:1], None))
    out.append(("one class", s, [0] * 5))
    out.append(("all NaN", np.full((3, 6), NAN, np.float32), [0, 1, 0]))
    out.append(("all +0.0", np.zeros((3, 6), np.float32), [1, 0, 0]))
    out.append(("infinities", np.array([[-INF, INF, -INF], [INF, INF, -INF]], np.float32), [0, 0]))
    big = rng.uniform(0, 1, (64, 9)).astype(np.float32)
    out.append(("64 templates in 16 classes", big, [k % 16 for k in range(64)]))
    out.append(("no position", np.zeros((2, 0), np.float32), None))
    return out


def test_the_model_is_the_brute_force_loop_on_tiny_arrays():
    for name, s, cls in class_cases():
        table, Cn = bref.class_table(cls, s.shape[0])
        got, which = bref.classes(s, cls)
        assert got.shape == (Cn, s.shape[1]) and which.shape == got.shape, name
        for c in range(Cn):
            for p in range(s.shape[1]):
                best = -1
                for k in range(s.shape[0]):
                    if table[k] != c or np.isnan(s[k, p]):
                        continue
                    if best < 0 or s[k, p] > s[best, p]:
                        best = k
                assert which[c, p] == best, (name, c, p)
                if best < 0:
                    assert np.isnan(got[c, p]), (name, c, p)
                else:
                    assert _bits(got[c, p]) == _bits(s[best, p]), (name, c, p)
    # the float64 scores of a bank: each class the maximum of its templates' model scores
    rng = np.random.default_rng(2)
    t = np.stack([ref.normalise(rng.standard_normal((3, 4))) for _ in range(3)])
    x = np.abs(rng.standard_normal((12, 4))).astype(np.float32)
    x[5, 1] = NAN
    s, w = bref.scores(t, x, [0, 1, 0])
    per = np.stack([ref.scores(tk, x)[0] for tk in t])
    ok = ~np.isnan(per[0])
    assert (np.isnan(per) == np.isnan(per[0])).all() and ok.sum() == 7 and (w[:, ~ok] == -1).all() and np.isnan(s[:, ~ok]).all()
    assert (s[0, ok] == np.maximum(per[0, ok], per[2, ok])).all() and (s[1, ok] == per[1, ok]).all() and (w[1, ok] == 1).all()
    assert set(w[0, ok].tolist()) <= {0, 2}
    # the per-class tables: match_ref.tables of every plane with its own threshold, which gathered at the matches
    planes = np.array([[0.1, 0.9, 0.2, 0.8, NAN], [0.5, 0.5, 0.5, 0.1, 0.7]], np.float32)
    wh = np.array([[0, 2, 0, 2, -1], [1, 1, 1, 1, 1]], np.int32)
    tb = bref.tables(planes, wh, [0.85, 0.4], 1, 256, 132, 2, 8)
    assert tb[0][0].tolist() == [256 + 3 * 132] and tb[0][1] == 1 and tb[0][3].tolist() == [2]
    assert tb[1][0].tolist() == [256 + 2 * 132, 256 + 6 * 132] and tb[1][3].tolist() == [1, 1]


def test_the_class_rule_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "match_classes_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "match_classes_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


@pytest.mark.parametrize("case", class_cases(), ids=lambda c: c[0])
def test_the_host_classes_equal_the_model_to_the_last_bit_and_index(case):
    name, s, cls = case
    want, want_w = bref.classes(s, cls)
    got, which = sd.matchClassesHost(s, cls)
    assert got.shape == want.shape and _bits(got).tobytes() == _bits(want).tobytes() and which.tobytes() == want_w.tobytes()
    assert ((which == -1) == np.isnan(got)).all()
    if name == "templates 1 and 3 the same":
        assert not (which == 3).any() and (which == 1).any()
    if name == "all NaN":
        assert (which == -1).all()
    if name == "all +0.0":
        assert (_bits(got) == 0).all() and which.tolist() == [[1] * 6, [0] * 6]


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    section = header[header.index("---- template matching: a bank of templates"):]
    for word in ('"match_bank_scores_mfma_kernel"', '"match_bank_scores_plain_kernel"', '"match_bank_peaks_kernel"', "match_classes.hpp",
                 "WITH THE SAME BITS", "LOWEST k", "CLASSES DO NOT SUPPRESS EACH OTHER", "templates of different lengths", "sharded banks"):
        assert word in section, word
    assert re.search(r"#define SYLDET_MATCH_MAX_TEMPLATES +64\b", header) and _abi.MATCH_MAX_TEMPLATES == 64
    assert re.search(r"#define SYLDET_MATCH_MAX_CLASSES +16\b", header) and _abi.MATCH_MAX_CLASSES == 16
    assert callable(sd.SyllableDetector.matcherBank) and callable(sd.Recordings.matcherBank)
    for name in ("scores", "peaks", "find", "close", "__enter__", "__exit__"):
        assert callable(getattr(sd.MatcherBank, name)), name


def test_the_refusals_that_need_no_device():
    fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
    ip = lambda a: a.ctypes.data_as(_abi.c_int32_p)
    s = np.arange(12, dtype=np.float32).reshape(3, 4)
    cls = np.array([0, 1, 0], np.int32)
    out, which = np.full((2, 4), 5.0, np.float32), np.full((2, 4), 9, np.int32)
    names = (("s", fp(s)), ("P", 4), ("K", 3), ("cls", ip(cls)), ("C", 2), ("out", fp(out)), ("which", ip(which)))
    call = lambda **kw: LIB.syldet_match_classes_host(*[kw.get(k, v) for k, v in names])
    gap, low, high = np.array([0, 2, 0], np.int32), np.array([0, -1, 1], np.int32), np.array([0, 2, 1], np.int32)
    for bad in (dict(s=None), dict(out=None), dict(P=-1), dict(K=0), dict(K=65), dict(C=0), dict(C=17), dict(cls=ip(gap), C=3), dict(cls=ip(low)),
                dict(cls=ip(high)), dict(cls=None, C=2), dict(cls=None, K=17, C=17), dict(cls=None, K=17, C=0)):
        assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert (out == 5.0).all() and (which == 9).all(), bad
    assert call(which=None) == 0 and (out == [[8, 9, 10, 11], [4, 5, 6, 7]]).all() and (which == 9).all()
    assert call() == 0 and which.tolist() == [[2] * 4, [1] * 4]
    assert call(P=0, s=None, out=None, which=None) == 0
    out3 = np.zeros((3, 4), np.float32)
    assert call(cls=None, C=0, out=fp(out3), which=None) == 0 and call(cls=None, C=3, out=fp(out3), which=None) == 0 and (out3 == s).all()
    # the calls on handles: NULL before anything else; the counts before the bank is looked at
    t = np.ones((2, 2, 3), np.float32)
    h = _abi.Handle()
    assert LIB.syldet_matcher_bank_create(None, None, fp(t), 2, 2, 3, -1, None, 0, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h
    assert LIB.syldet_matcher_bank_create(None, None, fp(t), 2, 2, 3, -1, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_bank_shape(None, None, None, None, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_bank_templates(None, fp(t), None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_match_bank_scores_device(None, None, 0, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_match_bank_peaks_device(None, None, None, 0, fp(out), 0, None, 0, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_matcher_bank_destroy(None) == 0
    # the bindings: a sharded bank has no bank of templates; the Python layer's own argument errors
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.matcherBank(object(), t)
    assert e.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sd.matchClassesHost(s, [0, 1])
    with pytest.raises(ValueError):
        sd.matchClassesHost(s[0])
    with pytest.raises(sd.SyllableDetectorError):
        sd.matchClassesHost(s, [0, 2, 0])


def test_two_exemplars_of_the_planted_syllable_on_the_model_alone():
    """The class of two exemplars -- the second planted syllable of seed 1 and the second of seed 4 -- on the float64 model over
    seeds 2 and 3: within one frame of every planted syllable the class scores at least 0.885 (0.8939 and 0.8857 are the two
    seeds' lowest), more than 12 frames from all of them at most 0.671 (0.6670, 0.6701).  The bank's threshold, 0.77, lies in that
    gap with 0.09 on either side; the first pair of exemplars tried has the gap, so none from another seed was needed."""
    t = np.stack([ref.normalise(e) for e in bc.exemplars()])
    for seed in mc.SEEDS:
        cols, frames = mc.columns64(seed).astype(np.float32), mc.planted(seed)[1]
        s, w = bref.scores(t, cols, [0, 0])
        P = cols.shape[0] - mc.N + 1
        s32, w = s[0, :P].astype(np.float32), w[0, :P]
        away = np.ones(P, bool)
        for f in frames:
            away[max(f - 12, 0):f + 13] = False
        near = min(s32[max(f - 1, 0):f + 2].max() for f in frames if f < P)
        other = s32[away].max()
        print("seed %d: lowest class score near a planted syllable %.4f, highest elsewhere %.4f" % (seed, near, other))
        assert other + 0.09 < bc.THRESHOLD < near - 0.09
        p = ref.peaks(s32, bc.THRESHOLD, bc.SEPARATION)
        assert len(frames) >= 20 and mc.found_once(p, frames, P), (seed, p.tolist(), frames.tolist())
        assert set(w[p].tolist()) == {0, 1}                               # each exemplar is the better one somewhere
