"""Threshold calibration on the host (no GPU): the syldet_score* functions are declared, exported and bound; syldet_score_host
equals the numpy model (tests/score_ref.py) over evaluation counts around the wave's 64, strides, threshold counts around a
group's 64 and three debounces; the flag is the double comparison at the threshold's edge, at +-inf and beyond FLT_MAX, and NaN
never fires; label edges; syldet_score_choose; the statuses that need no device; the per-threshold step under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
NEW = ["syldet_scorer_create", "syldet_scorer_destroy", "syldet_scorer_shape", "syldet_score_device", "syldet_score_host", "syldet_score_choose"]
HOP = 132
D = 3


def _first_index():
    g = util.sample_net().geometry()
    assert int(g.hop) == HOP
    return int(g.first_index)


def test_the_score_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    for i, col in enumerate(["DETECTIONS", "HITS", "FALSE_POSITIVES", "REPEATS", "SUM_OFFSET", "SUM_OFFSET_SQUARED", "COLUMNS"]):
        assert re.search(r"#define SYLDET_SCORE_%s\s+%d\b" % (col, i), header), col
    assert lib.syldet_abi_version() == 1                     # nothing existing changed
    assert sd.scoreHost is not None and sd.chooseThreshold is not None and sd.Scorer is not None


@pytest.fixture(scope="module")
def model_1000():
    """the generator's outputs at E = 1000 and the model's tables per (debounce, K = 130): [D][K][6]"""
    first = _first_index()
    y = ref.outputs(D, 1000, 1, 1000)
    lab = ref.labels(D, 1000, first, HOP)
    thr = ref.thresholds(130)
    return y, lab, {deb: np.stack([ref.score(y[d, :, 0], thr, lab[d], 3 * HOP, first, HOP, deb) for d in range(D)]) for deb in ref.debounces(HOP)}


def test_the_models_tables_are_not_vacuous(model_1000):
    _, lab, tables = model_1000
    for deb in (0, 2 * HOP + 1):
        t = tables[deb]
        for col in (_abi.SCORE_HITS, _abi.SCORE_FALSE_POSITIVES, _abi.SCORE_REPEATS):
            assert (t[:, :, col] > 0).any(), (deb, col)
    rises = np.diff(tables[9 * HOP + 1][:, :, _abi.SCORE_HITS], axis=1) > 0
    assert rises.any(axis=1).any(), "no detector's hits ever rise with the threshold: debounce would be a histogram"
    for t in tables.values():
        assert (t[:, :, 0] == t[:, :, 1] + t[:, :, 2] + t[:, :, 3]).all()
        assert (t[:, :, 1] <= np.array([len(x) for x in lab])[:, None]).all()


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 1000])
def test_score_host_equals_the_model(E, model_1000):
    first = _first_index()
    for stride in (1, 3):
        y = ref.outputs(D, E, stride, E) if E else np.zeros((D, 0, stride), np.float32)    # (the generator draws from [0, E))
        lab = ref.labels(D, E, first, HOP)
        for K in (1, 64, 65, 130):
            thr = ref.thresholds(K)
            for deb in ref.debounces(HOP):
                for d in range(D):
                    got = sd.scoreHost(y[d, :, stride - 1], thr, lab[d], 3 * HOP, first, HOP, deb)
                    if E == 1000 and stride == 1 and K == 130:
                        want = model_1000[2][deb][d]                    # (the tables the conditions above were asserted on)
                        assert np.array_equal(y, model_1000[0])
                    else:
                        want = ref.score(y[d, :, stride - 1], thr, lab[d], 3 * HOP, first, HOP, deb)
                    assert got.dtype == np.int64 and got.shape == (K, 6)
                    assert np.array_equal(got, want), (E, stride, K, deb, d)


def test_the_flag_is_the_double_comparison_at_every_edge():
    first = _first_index()
    y, thr = ref.edge_values(), ref.edge_thresholds()
    for deb in (0, 2 * HOP + 1):
        want = ref.score(y, thr, [], 0, first, HOP, deb)
        assert np.array_equal(sd.scoreHost(y, thr, [], 0, first, HOP, deb), want)
    n = ref.score(y, thr, [], 0, first, HOP, 0)[:, 0]
    assert n[0] == n[2] and n[1] == n[0] - 3                  # the three evaluations at exactly 0.7 fire at it and below it, not above
    assert n[3] == 1 and n[5] == 1                           # +inf and 1e39: the one +inf output
    assert n[4] == 200 - 2 and n[6] == 200 - 3               # -inf: everything but the NaNs; -1e39: not the -inf either


def test_label_edges():
    first = _first_index()
    y = ref.outputs(1, 300, 1, 3)[0, :, 0]
    thr = ref.thresholds(5)
    end = first + 300 * HOP
    at = first + 40 * HOP                                    # the generator's first syllable
    for labels, m in [([], 3 * HOP), ([-5000, at, end + 10 * HOP], 3 * HOP), ([-1, at], 0), ([at, at + 1], 0), ([at - HOP, at + HOP + 1], HOP),
                      ([at], 1 << 20)]:
        for deb in (0, 2 * HOP + 1):
            want = ref.score(y, thr, labels, m, first, HOP, deb)
            assert np.array_equal(sd.scoreHost(y, thr, labels, m, first, HOP, deb), want), (labels, m, deb)
    # tolerance 0 hits only on the label's own sample: the evaluation at `at` + 1 sample is a false positive
    assert ref.score(np.float32([1.0]), [0.5], [first], 0, first, HOP, 0)[0].tolist() == [1, 1, 0, 0, 0, 0]
    assert sd.scoreHost(np.float32([1.0]), [0.5], [first + 1], 0, first, HOP, 0)[0].tolist() == [1, 0, 1, 0, 0, 0]
    # neighbours at 2 m + 1 are accepted, at 2 m refused, and the error names the label
    bad = _abi.ERR_INVALID_ARGUMENT
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.scoreHost(y, thr, [at, at + 2 * HOP], HOP, first, HOP, 0)
    assert ei.value.status == bad and "detector 0, label 1" in _abi.last_error()
    for labels in ([at, at], [at + 1, at]):                   # not strictly sorted
        with pytest.raises(sd.SyllableDetectorError):
            sd.scoreHost(y, thr, labels, 0, first, HOP, 0)


def test_choose_against_the_model(model_1000):
    _, lab, tables = model_1000
    counts = [len(x) for x in lab]
    for deb, t in tables.items():
        for cost in (0.0, 1.0, 2.5):
            k, totals, costs = sd.chooseThreshold(t, counts, cost)
            wk, wt, wc = ref.choose(t, counts, cost)
            assert k == wk and np.array_equal(totals, wt) and np.array_equal(costs, wc), (deb, cost)
    # ties go to the lowest index: with cost 0 every threshold that hits all labels costs 0
    t = np.zeros((2, 4, 6), np.int64)
    t[:, 1:3, 1] = 2
    t[:, 1:3, 0] = 2
    t[0, 1, 2] = 5
    t[0, 1, 0] += 5
    assert sd.chooseThreshold(t, [2, 2], 0.0)[0] == 1 and sd.chooseThreshold(t, [2, 2], 1.0)[0] == 2
    assert sd.chooseThreshold(t, [2, 2], 1.0)[2].tolist() == [4.0, 5.0, 0.0, 4.0]
    assert sd.chooseThreshold(t[0], [2], 2.5)[2].tolist() == [2.0, 12.5, 0.0, 2.0]
    assert sd.chooseThreshold(np.zeros((1, 3, 6), np.int64), [0], 1.0)[0] == 0


def test_statuses_without_a_device():
    lib = _abi.lib
    bad = _abi.ERR_INVALID_ARGUMENT
    v = np.zeros(8, np.float32)
    thr = np.array([0.5, 0.6])
    nan = np.array([0.5, np.nan])
    many = np.zeros(4097)
    lab = np.array([10, 2000], np.int64)
    tab = np.zeros((4097, 6), np.int64)
    pv, pt, pl, pn = v.ctypes.data_as(_abi.c_float_p), thr.ctypes.data_as(_abi.c_double_p), lab.ctypes.data_as(_abi.c_int64_p), tab.ctypes.data_as(_abi.c_int64_p)
    host = lib.syldet_score_host
    assert host(pv, 8, 1, pt, 2, pl, 2, 5, 100, 132, 0, pn) == 0
    assert host(None, 8, 1, pt, 2, pl, 2, 5, 100, 132, 0, pn) == bad
    assert host(None, 0, 1, pt, 2, None, 0, 5, 100, 132, 0, pn) == 0                     # nothing to read
    assert host(pv, 8, 1, None, 2, pl, 2, 5, 100, 132, 0, pn) == bad
    assert host(pv, 8, 1, pt, 2, None, 2, 5, 100, 132, 0, pn) == bad
    assert host(pv, 8, 1, pt, 2, pl, 2, 5, 100, 132, 0, None) == bad
    assert host(pv, 8, 1, pt, 0, pl, 2, 5, 100, 132, 0, pn) == bad                       # K = 0
    assert host(pv, 8, 1, many.ctypes.data_as(_abi.c_double_p), 4097, pl, 2, 5, 100, 132, 0, pn) == bad
    assert host(pv, 8, 1, many.ctypes.data_as(_abi.c_double_p), 4096, pl, 2, 5, 100, 132, 0, pn) == 0
    assert host(pv, 8, 1, nan.ctypes.data_as(_abi.c_double_p), 2, pl, 2, 5, 100, 132, 0, pn) == bad
    assert "thresholds[1] is NaN" in _abi.last_error()
    assert host(pv, 8, 1, pt, 2, pl, 2, -1, 100, 132, 0, pn) == bad                      # negative tolerance
    assert host(pv, 8, 1, pt, 2, pl, 2, (1 << 20) + 1, 100, 132, 0, pn) == bad
    assert host(pv, -1, 1, pt, 2, pl, 2, 5, 100, 132, 0, pn) == bad
    assert host(pv, 8, 0, pt, 2, pl, 2, 5, 100, 132, 0, pn) == bad
    assert host(pv, 8, 1, pt, 2, pl, 2, 5, 100, 0, 0, pn) == bad                         # hop 0
    best = C.c_int32(-7)
    n = np.array([2], np.int64)
    pc = n.ctypes.data_as(_abi.c_int64_p)
    choose = lib.syldet_score_choose
    assert choose(pn, 1, 2, pc, 1.0, C.byref(best), None, None) == 0 and best.value == 0
    assert choose(None, 1, 2, pc, 1.0, C.byref(best), None, None) == bad
    assert choose(pn, 1, 2, None, 1.0, C.byref(best), None, None) == bad
    assert choose(pn, 1, 2, pc, 1.0, None, None, None) == bad
    assert choose(pn, 1, 0, pc, 1.0, C.byref(best), None, None) == bad
    assert choose(pn, 1, 4097, pc, 1.0, C.byref(best), None, None) == bad
    assert choose(pn, -1, 2, pc, 1.0, C.byref(best), None, None) == bad
    assert choose(pn, 1, 2, pc, float("nan"), C.byref(best), None, None) == bad
    out = _abi.Handle(5)
    begin = np.zeros(2, np.int64)
    assert lib.syldet_scorer_create(None, None, pt, 2, pl, begin.ctypes.data_as(_abi.c_int64_p), 5, 0.0, C.byref(out)) == bad
    assert not out.value                                                                  # *out is cleared
    assert lib.syldet_scorer_create(None, None, pt, 2, pl, begin.ctypes.data_as(_abi.c_int64_p), 5, 0.0, None) == bad
    assert lib.syldet_scorer_destroy(None) == 0
    assert lib.syldet_scorer_shape(None, None, None, None) == bad
    assert lib.syldet_score_device(None, 1, 8, 0, 1, None) == bad
    assert lib.syldet_abi_version() == 1
    with pytest.raises(ValueError):
        sd.scoreHost(np.zeros(4, np.float64), [0.5], [], 0, 0, 1, 0)
    with pytest.raises(ValueError):
        sd.chooseThreshold(np.zeros((2, 3, 6), np.int64), [1], 1.0)


def test_the_header_still_compiles_as_strict_c99(tmp_path):
    c = tmp_path / "score.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    float v[2] = {0.9f, 0.1f}; double th[1] = {0.5}; int64_t lab[1] = {3}, table[SYLDET_SCORE_COLUMNS], n[1] = {1}; int32_t best = -1;\n"
                 "    syldet_scorer_t *s = NULL;\n"
                 "    if (syldet_score_host(v, 2, 1, th, 1, lab, 1, 4, 0, 10, 0, table)) return 1;\n"
                 "    if (table[SYLDET_SCORE_HITS] != 1 || table[SYLDET_SCORE_SUM_OFFSET] != -3 || table[SYLDET_SCORE_SUM_OFFSET_SQUARED] != 9) return 2;\n"
                 "    if (syldet_score_choose(table, 1, 1, n, 1.0, &best, NULL, NULL) || best != 0) return 3;\n"
                 "    if (syldet_scorer_create(NULL, NULL, th, 1, lab, n, 4, 0.0, &s) != SYLDET_ERR_INVALID_ARGUMENT || s) return 4;\n"
                 "    if (syldet_score_device(NULL, v, 2, 0, table, NULL) != SYLDET_ERR_INVALID_ARGUMENT || syldet_scorer_shape(NULL, NULL, NULL, NULL) == 0) return 5;\n"
                 "    return syldet_scorer_destroy(NULL);\n"
                 "}\n")
    exe = tmp_path / "score"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + LIB, "-lsyldet", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_step_on_hand_worked_cases_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "score_scan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "score_scan_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.returncode, r.stdout, r.stderr)
    # the library's host function and the kernel are that header's
    for name in ("syldet_score.cpp", "kernels_score.hip"):
        text = open(os.path.join(ROOT, "syllable_detector_swift_amd", "csrc", name)).read()
        assert "score_cursor_start(" in text and "score_visit(" in text, name
