"""The TTL trigger track on the host (no GPU): the syldet_trigger* functions are declared, exported and bound and refuse a NULL
handle; the header and the C++ mirror compile; the closed form the header states is the rig's callback loop, and its onset rule
gives the track's rising edges; b(e) is the rule of syldet_levels_eval_range; syldet_trigger_width is Int(seconds * rate); the
monostable's arm and render under ASan + UBSan; the tool's new usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import levels_ref
import trigger_ref
import util
import wavutil
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
CLI = os.path.join(LIB, "syllable-detector-cli")
NEW = ["syldet_trigger_width", "syldet_trigger_device", "syldet_trigger_device_s16", "syldet_trigger_interleaved_device_s16",
       "syldet_trigger_mux_device_s16", "syldet_trigger_onsets_device", "syldet_trigger", "syldet_trigger_s16", "syldet_trigger_onsets",
       "syldet_trigger_arm", "syldet_trigger_render", "syldet_trigger_rehearse_device", "syldet_trigger_rehearse_device_s16",
       "syldet_deinterleave_device_s16"]


def test_the_trigger_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert lib.syldet_abi_version() == 1                     # nothing existing changed


def test_null_handle_is_refused_by_every_trigger_entry_point():
    lib = _abi.lib
    fl = np.zeros(8, np.uint8)
    t32, t16, a16 = np.zeros(64, np.float32), np.zeros(128, np.int16), np.zeros(64, np.int16)
    idx, cnt = np.zeros(8, np.int64), np.zeros(1, np.int64)
    pf = fl.ctypes.data_as(_abi.c_uint8_p)
    bad = _abi.ERR_INVALID_ARGUMENT
    assert lib.syldet_trigger_device(None, fl.ctypes.data, 8, 32, 44, 0, t32.ctypes.data, 64, 64, None) == bad
    assert lib.syldet_trigger_device_s16(None, fl.ctypes.data, 8, 32, 44, 0, t16.ctypes.data, 64, 64, None) == bad
    assert lib.syldet_trigger_interleaved_device_s16(None, fl.ctypes.data, 8, 32, 44, 0, t16.ctypes.data, 64, None) == bad
    assert lib.syldet_trigger_mux_device_s16(None, fl.ctypes.data, 8, 32, 44, 0, a16.ctypes.data, 64, t16.ctypes.data, 64, None) == bad
    assert lib.syldet_trigger_onsets_device(None, fl.ctypes.data, 8, 32, 44, 0, 64, idx.ctypes.data, 8, cnt.ctypes.data, None) == bad
    assert lib.syldet_trigger(None, pf, 8, 32, 44, 0, t32.ctypes.data_as(_abi.c_float_p), 64, 64) == bad
    assert lib.syldet_trigger_s16(None, pf, 8, 32, 44, 0, t16.ctypes.data_as(_abi.c_int16_p), 64, 64) == bad
    assert lib.syldet_trigger_onsets(None, pf, 8, 32, 44, 0, 64, idx.ctypes.data_as(_abi.c_int64_p), 8, cnt.ctypes.data_as(_abi.c_int64_p)) == bad
    assert lib.syldet_trigger_rehearse_device(None, fl.ctypes.data, 8, 32, 44, 0, t32.ctypes.data, 64, 64, idx.ctypes.data, 8, cnt.ctypes.data, None) == bad
    assert lib.syldet_trigger_rehearse_device_s16(None, fl.ctypes.data, 8, 32, 44, 0, t16.ctypes.data, 64, 64, idx.ctypes.data, 8, cnt.ctypes.data, None) == bad
    assert lib.syldet_deinterleave_device_s16(None, 10, 2, 2, t16.ctypes.data, 10, None) == bad
    assert lib.syldet_deinterleave_device_s16(a16.ctypes.data, 10, 2, 3, t16.ctypes.data, 10, None) == bad     # more channels than the frames hold
    assert lib.syldet_deinterleave_device_s16(None, 0, 2, 2, None, 0, None) == 0                                # nothing to do
    assert lib.syldet_trigger_arm(None, 0, 44) == bad
    assert lib.syldet_trigger_render(None, 0, t32.ctypes.data_as(_abi.c_float_p), 32) == bad
    assert not t32.any() and not t16.any() and not idx.any() and not cnt.any()


def test_header_declarations_compile_as_c99_and_the_cpp_mirror_has_the_methods(tmp_path):
    c = tmp_path / "trigger.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    uint8_t f[4] = {0}; float t[8]; int16_t q[16], a[8] = {0}; int64_t i[4], n[1];\n"
                 "    int st = syldet_trigger(NULL, f, 4, 8, 1, 0, t, 8, 8) + syldet_trigger_s16(NULL, f, 4, 8, 1, 0, q, 8, 8) +\n"
                 "             syldet_trigger_onsets(NULL, f, 4, 8, 1, 0, 8, i, 4, n) +\n"
                 "             syldet_trigger_device(NULL, f, 4, 8, 1, 0, t, 8, 8, NULL) + syldet_trigger_device_s16(NULL, f, 4, 8, 1, 0, q, 8, 8, NULL) +\n"
                 "             syldet_trigger_interleaved_device_s16(NULL, f, 4, 8, 1, 0, q, 8, NULL) +\n"
                 "             syldet_trigger_mux_device_s16(NULL, f, 4, 8, 1, 0, a, 8, q, 8, NULL) +\n"
                 "             syldet_trigger_onsets_device(NULL, f, 4, 8, 1, 0, 8, i, 4, n, NULL) +\n"
                 "             syldet_trigger_arm(NULL, 0, 44) + syldet_trigger_render(NULL, 0, t, 8);\n"
                 "    if (syldet_trigger_width(0.001, 44100.0) != 44 || syldet_trigger_width(0.0, 44100.0) != -1) return 2;\n"
                 "    return st == 10 * SYLDET_ERR_INVALID_ARGUMENT ? 0 : 1;\n"
                 "}\n")
    exe = tmp_path / "trigger"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + LIB, "-lsyldet", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    cpp = tmp_path / "trigger.cpp"
    cpp.write_text('#include "syldet.hpp"\n'
                   "void f(syldetxx::SyllableDetectorBank &b, const uint8_t *fl, float *t, int16_t *q, const int16_t *a, int64_t *i) {\n"
                   "    std::vector<float> v = b.triggerTrack(fl, 4, 8, 44); v = b.triggerTrack(fl, 4, 8, 44, 32, 221);\n"
                   "    std::vector<int16_t> s = b.triggerTrackPCM16(fl, 4, 8, 44);\n"
                   "    std::vector<int64_t> o = b.triggerOnsets(fl, 4, 8, 44, 0);\n"
                   "    int64_t w = syldetxx::SyllableDetectorBank::triggerWidth(0.001, 44100.0); (void)w;\n"
                   "    b.triggerDevice(fl, 4, 32, 44, 0, t, 8, 8, nullptr); b.triggerDevicePCM16(fl, 4, 32, 44, 0, q, 8, 8, nullptr);\n"
                   "    b.triggerInterleavedDevicePCM16(fl, 4, 32, 44, 0, q, 8, nullptr);\n"
                   "    b.triggerMuxDevicePCM16(fl, 4, 32, 44, 0, a, 8, q, 8, nullptr);\n"
                   "    b.triggerOnsetsDevice(fl, 4, 32, 44, 0, 8, i, 4, i, nullptr);\n"
                   "    b.armTrigger(0, 44); b.renderTrigger(0, t, 8);\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(cpp)], check=True)


def test_the_swift_shim_and_the_cpp_mirror_have_methods_of_the_same_names():
    hpp = open(os.path.join(ROOT, "include", "syldet.hpp")).read()
    swift = open(os.path.join(ROOT, "swift", "SyllableDetector.swift")).read()
    for name in ("triggerWidth", "triggerTrack", "triggerTrackPCM16", "triggerOnsets", "triggerDevice", "triggerDevicePCM16",
                 "triggerInterleavedDevicePCM16", "triggerMuxDevicePCM16", "triggerOnsetsDevice", "armTrigger", "renderTrigger"):
        assert re.search(r"\b%s\(" % name, hpp), name
        assert re.search(r"func %s\(" % name, swift), name
    # no status of the C ABI is dropped in the shim's trigger methods
    for call in re.findall(r"^.*syldet_trigger_(?!width)\w+\(handle.*$", swift, re.M):
        assert "checkTrigger(" in call or "st = " in call, call


def _planted(rng, E, density):
    if density == "none":
        return np.zeros(E, np.uint8)
    if density == "all":
        return np.ones(E, np.uint8)
    p = 0.02 if density == "sparse" else 0.6
    return (rng.random(E) < p).astype(np.uint8)


def test_the_closed_form_is_the_rigs_callback_loop_and_the_onsets_are_its_rising_edges():
    """252 seeded geometries: windows 64 .. 256, overlaps -40 .. W - 1 (gaps included), timeRange 1 .. 12, L in {8, 32, 256},
    every width of {1, L - 1, L, L + 1, 44, 20 L, 5000} and latency of {0, 1, 221} and flag density of {none, sparse, dense, all}
    in turn.  The loop renders buffer after buffer with renderOutput's arithmetic and equals the closed form in every sample; the
    onset rule gives exactly the samples where the closed-form track rises."""
    rng = np.random.default_rng(20241018)
    seen = {"gap": 0, "t1": 0, "below_D": 0, "retriggered": 0, "abut": 0, "pulse_cut_by_the_end": 0, "onset_beyond_the_end": 0,
            "several_evals_a_buffer": 0, "no_onset": 0, "many_onsets": 0}
    widths = lambda L: [1, L - 1, L, L + 1, 44, 20 * L, 5000]
    trial = 0
    for L in (8, 32, 256):
        for wi in range(7):
            for lat in (0, 1, 221):
                for density in ("none", "sparse", "dense", "all"):
                    N = widths(L)[wi]
                    W = int(rng.choice([64, 128, 200, 256]))
                    ov = int(rng.integers(-40, W)) if trial % 5 else W - int(rng.integers(1, 4))
                    T = 1 if trial % 9 == 0 else int(rng.integers(1, 13))
                    D, hop, gap = trigger_ref.geometry(W, ov, T)
                    S = int(rng.integers(0, D)) if trial % 11 == 0 else int(rng.integers(D, D + min(40 * hop, 6000) + 3 * L))
                    E = trigger_ref.count_evals(S, W, ov, T)
                    flags = _planted(rng, E, density)
                    want = trigger_ref.closed_form(flags, D, hop, L, N, lat, S)
                    got = trigger_ref.rig_loop(flags, W, ov, T, L, N, lat, S)
                    case = "trial %d (W %d, overlap %d, T %d, S %d, L %d, N %d, latency %d, %s)" % (trial, W, ov, T, S, L, N, lat, density)
                    assert np.array_equal(got, want), case
                    on = trigger_ref.onsets(flags, D, hop, L, N, lat, S)
                    assert np.array_equal(on, trigger_ref.rising_edges(want)), case
                    sb = trigger_ref.seen_buffers(flags, D, hop, L)
                    gaps = np.diff(sb) if len(sb) > 1 else np.zeros(0, np.int64)
                    seen["gap"] += ov < 0
                    seen["t1"] += T == 1
                    seen["below_D"] += S < D
                    seen["retriggered"] += bool(((gaps * L < N)).any())
                    seen["abut"] += bool((gaps * L == N).any())
                    seen["pulse_cut_by_the_end"] += bool(len(want) and want[-1])
                    seen["onset_beyond_the_end"] += bool(len(sb) and (sb[-1] + 1) * L + lat >= S)
                    seen["several_evals_a_buffer"] += hop < L
                    seen["no_onset"] += len(on) == 0
                    seen["many_onsets"] += len(on) >= 3
                    trial += 1
    assert trial == 252 and min(seen.values()) >= 5, seen


def test_the_reference_functions_on_hand_made_flags():
    # D 5, hop 4, L 8: evaluations become available at samples 5, 9, 13, 17, ...: buffers 0, 1, 1, 2, 2, 3, ...
    assert list(trigger_ref.buffer_of(np.arange(6), 5, 4, 8)) == [0, 1, 1, 2, 2, 3]
    f = np.array([1, 0, 0, 0, 0, 0], np.uint8)
    tr = trigger_ref.closed_form(f, 5, 4, 8, 3, 0, 40)
    assert list(np.nonzero(tr)[0]) == [8, 9, 10]                                          # the render buffer behind buffer 0
    assert list(np.nonzero(trigger_ref.closed_form(f, 5, 4, 8, 3, 2, 40))[0]) == [10, 11, 12]    # ... two samples of latency later
    f = np.array([1, 0, 0, 1, 0, 0], np.uint8)                                            # buffers 0 and 2: t = 8 and 24
    assert list(trigger_ref.onsets(f, 5, 4, 8, 16, 0, 100)) == [8]                        # 8 + 16 = 24: the pulses abut, one pulse
    assert trigger_ref.closed_form(f, 5, 4, 8, 16, 0, 100).sum() == 32
    assert list(trigger_ref.onsets(f, 5, 4, 8, 15, 0, 100)) == [8, 24]                    # a miss by one sample: two
    assert trigger_ref.closed_form(f, 5, 4, 8, 15, 0, 100)[23] == 0
    assert list(trigger_ref.onsets(f, 5, 4, 8, 15, 0, 24)) == [8]                         # an onset at n_samples is not reported
    assert list(trigger_ref.as_s16([0, 1])) == [0, 32767] and list(trigger_ref.as_f32([0, 1])) == [0.0, 1.0]


def test_b_of_e_is_the_rule_of_levels_eval_range():
    """with one buffer a reading, reading m of syldet_levels_eval_range's rule (tests/levels_ref.py holds the numpy form to the
    library on the device; tests/test_trigger_gpu.py asks the library itself) holds exactly the evaluations with b(e) = m"""
    rng = np.random.default_rng(5)
    for trial in range(200):
        W = int(rng.choice([64, 128, 200, 256]))
        ov = int(rng.integers(-40, W))
        T = int(rng.integers(1, 13))
        L = int(rng.choice([8, 32, 256]))
        D, hop, _ = trigger_ref.geometry(W, ov, T)
        S = int(rng.integers(D, D + 30 * hop + 2 * L))
        E = trigger_ref.count_evals(S, W, ov, T)
        b = trigger_ref.buffer_of(np.arange(E), D, hop, L)
        for m, (first, count) in enumerate(levels_ref.eval_ranges(S, E, L, 1, (W, ov, T))):
            assert list(np.nonzero(b == m)[0]) == list(range(first, first + count)), (trial, m)


def test_trigger_width_is_int_of_seconds_times_rate():
    w = _abi.lib.syldet_trigger_width
    for seconds, rate in [(0.001, 44100.0), (0.001, 48000.0), (0.001, 22050.0), (0.005, 44100.0), (1.0, 44100.0), (0.0015, 44100.0),
                          (0.1, 3.0), (0.3, 10.0), (0.7, 10.0), (1e-3, 1e3), (2.5e-5, 96000.0), (1.0 / 3.0, 48000.0), (380.0, 44100.0)]:
        n = int(seconds * rate)                                                    # exact and inexact products alike: the Double product, truncated
        assert w(seconds, rate) == (n if n >= 1 else -1), (seconds, rate)
    assert w(0.001, 44100.0) == 44 and w(0.3, 10.0) == 3 and w(0.7, 10.0) == 7 and w(0.1, 3.0) == -1
    for seconds, rate in [(0.0, 44100.0), (-0.001, 44100.0), (1e-6, 44100.0), (float("nan"), 44100.0), (0.001, float("inf")),
                          (float("inf"), 1.0), (0.001, float("nan")), (1e300, 1e300)]:
        assert w(seconds, rate) == -1, (seconds, rate)


def test_arm_and_render_literally_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "pulse"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "trigger_pulse_test.cpp"),
                    "-o", str(exe), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.returncode, r.stdout, r.stderr)
    # the library's two functions are that header's
    api = open(os.path.join(ROOT, "syllable_detector_swift_amd", "csrc", "syldet_trigger.cpp")).read()
    assert "trigger_pulse_arm(" in api and "trigger_pulse_render(" in api


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def net_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ttlnet") / "net.txt")
    open(p, "w").write(util.sample_net().toText())
    return p


def test_the_tools_usage_errors_for_ttl(tmp_path, net_file):
    assert os.path.exists(CLI), "syllable-detector-cli has not been built"
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((100, 2), np.int16), 44100, "pcm16")
    out, tsv = str(tmp_path / "ttl.wav"), str(tmp_path / "on.tsv")
    base = ["-n", net_file, "-a", a, "--ttl", out]
    cases = [["-n", net_file, "--ttl", out],                                         # no -a
             ["-n", net_file, "-a", a, "-a", a, "--ttl", out],                       # more than one -a
             ["-n", net_file, "-a", a, "-a", a, "--ttl-onsets", tsv],
             ["-n", net_file, "-a", a, "--ttl"],                                     # a missing value
             base + ["--ttl-width"], base + ["--ttl-steps"], base + ["--ttl-buffer"], base + ["--ttl-latency"], base + ["--ttl-onsets"],
             base + ["--ttl-width", "0"], base + ["--ttl-width", "-0.001"], base + ["--ttl-width", "wide"], base + ["--ttl-width", "nan"],
             base + ["--ttl-width", "1e-6"],                                         # shorter than one sample at 44100 Hz
             base + ["--ttl-width", "400"],                                          # more than 2^24 samples
             base + ["--ttl-steps", "0"], base + ["--ttl-steps", "2.5"], base + ["--ttl-steps", "20", "--ttl-buffer", "4096", "--ttl-steps", "5000"],
             base + ["--ttl-buffer", "33"], base + ["--ttl-buffer", "4"], base + ["--ttl-buffer", "8192"],
             base + ["--ttl-latency", "-1"], base + ["--ttl-latency", "soon"], base + ["--ttl-latency", "400"],
             base + ["--ttl-width", "0.001", "--ttl-steps", "20"],                   # two widths
             ["-n", net_file, "-a", a, "--ttl-mux"],                                 # options for a track nobody asked for
             ["-n", net_file, "-a", a, "--ttl-width", "0.001"], ["-n", net_file, "-a", a, "--ttl-steps", "20"],
             ["-n", net_file, "-a", a, "--ttl-buffer", "32"], ["-n", net_file, "-a", a, "--ttl-latency", "0"]]
    for args in cases:
        r = run_cli(*args)
        assert r.returncode == 64, (args, r.returncode, r.stderr)
        assert "Path to trained network file." in r.stdout, args       # every usage error prints the usage text
        assert not os.path.exists(out) and not os.path.exists(tsv), args
    assert "--ttl-mux needs --ttl" in run_cli("-n", net_file, "-a", a, "--ttl-mux").stderr
    assert "give one" in run_cli(*(base + ["--ttl-width", "0.001", "--ttl-steps", "20"])).stderr
    u = run_cli("-h").stdout
    for opt in ("--ttl <out.wav>", "--ttl-mux", "--ttl-width <seconds>", "--ttl-steps <n>", "--ttl-buffer <L>", "--ttl-latency <seconds>",
                "--ttl-onsets <out.tsv>"):
        assert opt in u, opt


def test_probe_ignores_the_ttl_options(tmp_path):
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((123, 2), np.int16), 22050, "pcm16")
    plain = run_cli("--probe", "-a", a)
    out = str(tmp_path / "ttl.wav")
    r = run_cli("--probe", "-a", a, "--ttl", out, "--ttl-steps", "20")
    assert plain.returncode == 0 and (r.returncode, r.stdout, r.stderr) == (0, plain.stdout, plain.stderr)
    assert not os.path.exists(out)
