"""The level meters on the host (no GPU): the entry points are declared, exported and bound and refuse a NULL handle; the header
and the C++ mirror compile; syldet_levels_count is the formula; syldet_sum_squares is the tree of levels_ref bit for bit (and
not the sequential sum); the closed forms the header states are the literal replay of buffers, evaluations and timer reads; the
tool's usage errors for --levels; the built kernels load 16 bytes a lane."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import levels_ref
import util
import wavutil
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
CLI = os.path.join(LIB, "syllable-detector-cli")
NEW = ["syldet_levels_count", "syldet_sum_squares", "syldet_levels_eval_range", "syldet_levels_device", "syldet_levels_device_s16",
       "syldet_levels_interleaved_device", "syldet_levels_interleaved_device_s16", "syldet_output_levels_device", "syldet_levels",
       "syldet_levels_s16", "syldet_output_levels", "syldet_meters_enable", "syldet_input_level", "syldet_output_level"]


def test_the_levels_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert lib.syldet_abi_version() == 1                     # nothing existing changed


def test_null_handle_is_refused_by_every_levels_entry_point():
    lib = _abi.lib
    x32, x16 = np.zeros(64, np.float32), np.zeros(64, np.int16)
    ms, lv = np.full(8, 7.0), np.full(8, 7.0, np.float32)
    first, count, has = C.c_int64(5), C.c_int64(5), C.c_int32(5)
    v = C.c_double(5.0)
    bad = _abi.ERR_INVALID_ARGUMENT
    assert lib.syldet_levels_eval_range(None, 64, 0, 32, 1, 0, C.byref(first), C.byref(count)) == bad
    assert lib.syldet_levels_device(None, x32.ctypes.data, 64, 64, 32, 1, ms.ctypes.data, None) == bad
    assert lib.syldet_levels_device_s16(None, x16.ctypes.data, 64, 64, 32, 1, ms.ctypes.data, None) == bad
    assert lib.syldet_levels_interleaved_device(None, x32.ctypes.data, 64, 1, 32, 1, ms.ctypes.data, None) == bad
    assert lib.syldet_levels_interleaved_device_s16(None, x16.ctypes.data, 64, 1, 32, 1, ms.ctypes.data, None) == bad
    assert lib.syldet_output_levels_device(None, x32.ctypes.data, 8, 0, 64, 32, 1, lv.ctypes.data, None) == bad
    assert lib.syldet_levels(None, x32.ctypes.data_as(_abi.c_float_p), 64, 64, 32, 1, ms.ctypes.data_as(_abi.c_double_p)) == bad
    assert lib.syldet_levels_s16(None, x16.ctypes.data_as(_abi.c_int16_p), 64, 64, 32, 1, ms.ctypes.data_as(_abi.c_double_p)) == bad
    assert lib.syldet_output_levels(None, x32.ctypes.data_as(_abi.c_float_p), 8, 0, 64, 32, 1, lv.ctypes.data_as(_abi.c_float_p)) == bad
    assert lib.syldet_meters_enable(None, 1) == bad
    assert lib.syldet_input_level(None, 0, C.byref(v), C.byref(has)) == bad
    assert lib.syldet_output_level(None, 0, C.byref(v), C.byref(has)) == bad
    assert (ms == 7.0).all() and (lv == 7.0).all() and (first.value, count.value, has.value, v.value) == (5, 5, 5, 5.0)


def test_header_declarations_compile_as_c99_and_the_cpp_mirror_has_the_methods(tmp_path):
    c = tmp_path / "levels.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    float x[8] = {0}, lv[2]; int16_t q[8] = {0}; double ms[2], v; int32_t has; int64_t a, b;\n"
                 "    int st = syldet_levels(NULL, x, 8, 8, 8, 1, ms) + syldet_levels_s16(NULL, q, 8, 8, 8, 1, ms) +\n"
                 "             syldet_output_levels(NULL, x, 1, 0, 8, 8, 1, lv) + syldet_levels_device(NULL, x, 8, 8, 8, 1, ms, NULL) +\n"
                 "             syldet_levels_device_s16(NULL, q, 8, 8, 8, 1, ms, NULL) + syldet_levels_interleaved_device(NULL, x, 8, 1, 8, 1, ms, NULL) +\n"
                 "             syldet_levels_interleaved_device_s16(NULL, q, 8, 1, 8, 1, ms, NULL) +\n"
                 "             syldet_output_levels_device(NULL, x, 1, 0, 8, 8, 1, lv, NULL) + syldet_levels_eval_range(NULL, 8, 1, 8, 1, 0, &a, &b) +\n"
                 "             syldet_meters_enable(NULL, 1) + syldet_input_level(NULL, 0, &v, &has) + syldet_output_level(NULL, 0, &v, &has);\n"
                 "    x[0] = 3.0f; x[1] = 4.0f;\n"
                 "    if (syldet_sum_squares(x, 8) != 25.0f || syldet_levels_count(100, 32, 3) != 2) return 2;\n"
                 "    return st == 12 * SYLDET_ERR_INVALID_ARGUMENT ? 0 : 1;\n"
                 "}\n")
    exe = tmp_path / "levels"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + LIB, "-lsyldet", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    cpp = tmp_path / "levels.cpp"
    cpp.write_text('#include "syldet.hpp"\n'
                   "void f(syldetxx::SyllableDetectorBank &b, const float *x, const int16_t *q, double *ms, float *lv) {\n"
                   "    std::optional<double> in = b.getInputForChannel(0), out = b.getOutputForChannel(1);\n"
                   "    b.enableMeters(); b.enableMeters(false);\n"
                   "    std::vector<double> r = b.levels(x, 64, 32, 1); r = b.levelsPCM16(q, 64, 32, 1);\n"
                   "    std::vector<float> o = b.outputLevels(x, 4, 64, 32, 1); o = b.outputLevels(x, 4, 64, 32, 1, 1);\n"
                   "    b.levelsDevice(x, 64, 64, 32, 1, ms, nullptr); b.levelsDevicePCM16(q, 64, 64, 32, 1, ms, nullptr);\n"
                   "    b.levelsInterleavedDevice(x, 64, 32, 1, ms, nullptr); b.levelsInterleavedDevicePCM16(q, 64, 32, 1, ms, nullptr);\n"
                   "    b.outputLevelsDevice(x, 4, 0, 64, 32, 1, lv, nullptr);\n"
                   "    (void)in; (void)out; (void)syldetxx::SyllableDetectorBank::levelsCount(64, 32, 1);\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(cpp)], check=True)


def test_levels_count_is_the_formula():
    lib = _abi.lib
    for S, L, P in [(5, 8, 1), (5, 32, 7), (0, 32, 1), (0, 8, 10 ** 6), (64, 32, 1), (64, 32, 2), (64, 32, 3), (65, 32, 2), (4096 * 5, 4096, 2),
                    (200003, 8, 1), (200003, 32, 137), (200003, 4096, 5), (200003, 32, 10 ** 6), (1 << 40, 32, 137)]:
        assert lib.syldet_levels_count(S, L, P) == levels_ref.levels_count(S, L, P), (S, L, P)
    assert lib.syldet_levels_count(5, 8, 1) == 1 and lib.syldet_levels_count(0, 32, 1) == 0      # S < L: one short buffer; S = 0: none
    assert lib.syldet_levels_count(200003, 32, 10 ** 6) == 1                                    # P > B: one reading
    for L in (0, 12, 8192, 4, -32):
        assert lib.syldet_levels_count(100, L, 1) == -1, L
    assert lib.syldet_levels_count(100, 32, 0) == -1 and lib.syldet_levels_count(100, 32, -3) == -1
    assert lib.syldet_levels_count(-1, 32, 1) == -1


def _lib_sum(x):
    x = np.ascontiguousarray(x, np.float32)
    return np.float32(_abi.lib.syldet_sum_squares(x.ctypes.data_as(_abi.c_float_p), len(x)))


def _same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def test_sum_squares_is_the_tree_bit_for_bit():
    rng = np.random.default_rng(20250117)
    lengths = list(range(0, 71)) + [4095, 4096, 4097]
    for n in lengths:
        for level in (1e-20, 1e-4, 1.0, 3e4, 1e15):
            x = (rng.standard_normal(n) * level).astype(np.float32)
            assert _same_bits(_lib_sum(x), levels_ref.sum_squares_tree(x)), (n, level)
        # planted values: NaN, +-Inf, subnormals, at random places
        x = rng.standard_normal(n).astype(np.float32)
        for val in (np.nan, np.inf, -np.inf, 1e-42, -3e-45):
            if n:
                y = x.copy()
                y[rng.integers(0, n)] = val
                assert _same_bits(_lib_sum(y), levels_ref.sum_squares_tree(y)), (n, val)
        if n:
            y = (x * 1e-22).astype(np.float32)                          # every square subnormal or zero
            assert _same_bits(_lib_sum(y), levels_ref.sum_squares_tree(y)), n
    assert _lib_sum(np.zeros(0, np.float32)) == 0 and _abi.lib.syldet_sum_squares(None, 5) == 0
    # padding to a longer power of two gives the same bits
    x = rng.standard_normal(37).astype(np.float32)
    assert _same_bits(_lib_sum(x), _lib_sum(np.concatenate([x, np.zeros(4096 - 37, np.float32)])))


def test_the_tree_is_not_the_sequential_sum():
    x = np.random.default_rng(7).standard_normal(32).astype(np.float32)
    tree, seq = levels_ref.sum_squares_tree(x), levels_ref.sum_squares_sequential(x)
    assert not _same_bits(tree, seq)                                    # this vector tells the orders apart ...
    assert _same_bits(_lib_sum(x), tree)                                # ... and the library has the tree's
    differ = sum(not _same_bits(levels_ref.sum_squares_tree(v), levels_ref.sum_squares_sequential(v))
                 for v in np.random.default_rng(8).standard_normal((200, 32)).astype(np.float32))
    assert differ > 100, differ


def test_stat_max_closed_form_is_the_literal_loop():
    rng = np.random.default_rng(5)
    for trial in range(2000):
        n = int(rng.integers(1, 12))
        v = rng.standard_normal(n).astype(np.float32 if trial % 2 else np.float64)
        for val in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            if rng.random() < 0.3:
                v[rng.integers(0, n)] = val
        a, b = levels_ref.stat_max(list(v)), levels_ref.stat_max_closed(v)
        assert np.asarray(a, v.dtype).tobytes() == np.asarray(b, v.dtype).tobytes(), (trial, v)     # -0 in front of +0 stays
    assert levels_ref.stat_max([]) is None and levels_ref.stat_max_closed(np.zeros(0)) is None


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_the_closed_forms_are_the_replay():
    """420 seeded geometries: L 8 .. 4096, P 1 .. beyond the buffer count, windows 64 .. 256, overlaps -40 .. W - 1 (gaps
    included), timeRange 1 .. 12, lengths around every boundary (S < L, S < gap + W, exactly one evaluation, many), NaN and
    +-Inf planted in samples and outputs."""
    rng = np.random.default_rng(20250118)
    seen = {"short": 0, "below_first_eval": 0, "one_eval": 0, "P_beyond": 0, "nan_first": 0, "empty_reading": 0, "cut": 0}
    for trial in range(420):
        L = int(rng.choice([8, 16, 32, 64, 256, 4096]))
        W = int(rng.choice([64, 128, 200, 256]))
        ov = int(rng.integers(-40, W))
        T = 1 if trial % 9 == 0 else int(rng.integers(1, 13))
        clock = (W, ov, T)
        gap, hop = levels_ref.geometry(*clock)
        need = gap + W + (T - 1) * hop                                  # samples of one evaluation
        kind = trial % 6
        if kind == 0:
            S = int(rng.integers(1, L))                                 # S < L
        elif kind == 1:
            S = int(rng.integers(1, gap + W))                           # no frame
        elif kind == 2:
            S = need + int(rng.integers(0, hop))                        # exactly one evaluation
        else:
            S = int(rng.integers(1, 40 * max(L, hop) + need))
        B = -(-S // L)
        P = int(rng.choice([1, 2, 3, 5, 137, B, B + 1, 10 ** 6])) if trial % 4 else int(rng.integers(1, B + 2))
        x = (rng.standard_normal(S) * 10.0 ** rng.integers(-6, 3)).astype(np.float32)
        for val in (np.nan, np.inf, -np.inf, 0.0):
            for _ in range(int(rng.integers(0, 3))):
                x[rng.integers(0, S)] = val
        if trial % 5 == 0:
            x[:min(S, L)] = np.nan if trial % 10 == 0 else x[:min(S, L)]
            x[0] = np.nan                                               # a reading whose first buffer is NaN
        E = levels_ref.count_evals(S, *clock)
        n_evals = E if trial % 7 else int(rng.integers(0, E + 1))       # fewer outputs than the clock's cut the ranges
        out = rng.standard_normal((n_evals, 2)).astype(np.float32)
        for val in (np.nan, np.inf, -np.inf, -0.0, 0.0):
            for _ in range(int(rng.integers(0, 3))):
                if n_evals:
                    out[rng.integers(0, n_evals), rng.integers(0, 2)] = val
        k = trial % 2
        want_in, want_out = levels_ref.replay(x, L, P, clock, out, k)
        got_in = levels_ref.input_readings(x, L, P)
        got_out, empty = levels_ref.output_readings(out, k, S, L, P, clock)
        M = levels_ref.levels_count(S, L, P)
        assert len(want_in) == len(got_in) == len(got_out) == M, trial
        assert None not in want_in                                      # input readings are never empty
        assert np.array_equal(_bits64(want_in), _bits64(got_in)), (trial, L, P, S)
        assert [w is None for w in want_out] == list(empty), (trial, L, P, S, clock)
        # the fp32 -> Double conversion is exact: compare as Double, bit for bit; an empty reading is the table's ?? 0.0
        assert np.array_equal(_bits64([0.0 if w is None else w for w in want_out]), _bits64(got_out.astype(np.float64))), (trial, L, P, S, clock)
        ranges = levels_ref.eval_ranges(S, n_evals, L, P, clock)
        assert ranges[0][0] == 0 and sum(c for _, c in ranges) == n_evals and all(ranges[m][0] + ranges[m][1] == ranges[m + 1][0] for m in range(M - 1))
        seen["short"] += S < L
        seen["below_first_eval"] += E == 0
        seen["one_eval"] += E == 1
        seen["P_beyond"] += P > B
        seen["nan_first"] += bool(np.isnan(got_in).any())
        seen["empty_reading"] += bool(empty.any())
        seen["cut"] += n_evals < E
    assert min(seen.values()) >= 10, seen


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def net_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("levelsnet") / "net.txt")
    open(p, "w").write(util.sample_net().toText())
    return p


def test_the_tools_usage_errors_for_levels(tmp_path, net_file):
    assert os.path.exists(CLI), "syllable-detector-cli has not been built"
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((100, 2), np.int16), 44100, "pcm16")
    out = str(tmp_path / "levels.tsv")
    cases = [["-n", net_file, "--levels", out],                                     # no -a
             ["-n", net_file, "-a", a, "-a", a, "--levels", out],                   # more than one -a
             ["-n", net_file, "-a", a, "--levels"],                                 # a missing value
             ["-n", net_file, "-a", a, "--levels", out, "--levels-buffer"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-period"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-buffer", "12"],   # not a power of two
             ["-n", net_file, "-a", a, "--levels", out, "--levels-buffer", "4"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-buffer", "8192"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-buffer", "many"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-period", "0"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-period", "-0.1"],
             ["-n", net_file, "-a", a, "--levels", out, "--levels-period", "soon"],
             ["-n", net_file, "-a", a, "--levels-buffer", "32"],                    # options of a table nobody asked for
             ["-n", net_file, "-a", a, "--levels-period", "0.1"]]
    for args in cases:
        r = run_cli(*args)
        assert r.returncode == 64, (args, r.returncode, r.stderr)
        assert "Path to trained network file." in r.stdout, args      # every usage error prints the usage text
        assert not os.path.exists(out), args
    assert "power of two" in run_cli(*cases[5]).stderr
    u = run_cli("-h").stdout
    assert "--levels <out.tsv>" in u and "--levels-buffer <L>" in u and "--levels-period <seconds>" in u


def test_probe_ignores_the_levels_options(tmp_path):
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((123, 2), np.int16), 22050, "pcm16")
    plain = run_cli("--probe", "-a", a)
    out = str(tmp_path / "levels.tsv")
    r = run_cli("--probe", "-a", a, "--levels", out, "--levels-buffer", "64", "--levels-period", "0.5")
    assert plain.returncode == 0 and (r.returncode, r.stdout, r.stderr) == (0, plain.stdout, plain.stderr)
    assert not os.path.exists(out)


def _kernel_body(text, fragment):
    """the instructions of the one kernel whose mangled name holds `fragment`: from its label to its .Lfunc_end"""
    labels = re.findall(r"^(_Z\w*%s\w*):" % fragment, text, re.M)
    assert len(labels) == 1, (fragment, labels)
    start = text.index("\n" + labels[0] + ":")
    return text[start:text.index(".Lfunc_end", start)]


def test_the_built_levels_kernels_load_sixteen_bytes_a_lane():
    """the ISA the build wrote (--save-temps) for the file that holds levels_in_kernel: both instantiations read the aligned rows
    with global_load_dwordx4, hold no fused multiply-add, and take the tree's first lane exchanges as DPP operands"""
    files = [f for f in glob.glob(os.path.join(LIB, "obj", "isa", "*-hip-amdgcn-*.s")) if "levels_in_kernel" in open(f).read()]
    assert len(files) == 1, files
    text = open(files[0]).read()
    for name in ("levels_in_kernelIfE", "levels_in_kernelIsE"):
        body = _kernel_body(text, name)
        assert len(re.findall(r"^\s*global_load_dwordx4\b", body, re.M)) == 8, name     # eight loads in flight a lane
        # squares and additions round on their own: no multiply-add between registers (the literal-constant forms v_fmamk / v_fmaak
        # belong to the compiler's expansion of the 64-bit integer division by buffers_per_reading)
        assert not re.search(r"\bv_(pk_)?fmac?_f32\b", body), name
        assert "row_half_mirror" in body and "quad_perm" in body, name
