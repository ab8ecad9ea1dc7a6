"""The Simulator's output track on the host (no GPU): the five syldet_trace* functions are declared, exported and bound and refuse
a NULL handle; the header and the C++ mirror compile; the closed form the header states is the reference's buffer loop; the
tool's WAV writer round-trips; the tool's new usage errors; the built kernel stores 16 bytes a lane."""
import ctypes as C
import glob
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import trace_ref
import util
import wavutil
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
CLI = os.path.join(LIB, "syllable-detector-cli")
NEW = ["syldet_trace_device", "syldet_trace_device_s16", "syldet_trace_interleaved_device_s16", "syldet_trace", "syldet_trace_s16"]


def test_the_trace_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert lib.syldet_abi_version() == 1                     # nothing existing changed


def test_null_handle_is_refused_by_every_trace_entry_point():
    lib = _abi.lib
    out = np.zeros(8, np.float32)
    t32, t16 = np.zeros(64, np.float32), np.zeros(64, np.int16)
    po = out.ctypes.data_as(_abi.c_float_p)
    bad = _abi.ERR_INVALID_ARGUMENT
    assert lib.syldet_trace_device(None, out.ctypes.data, 8, 0, t32.ctypes.data, 64, 64, None) == bad
    assert lib.syldet_trace_device_s16(None, out.ctypes.data, 8, 0, t16.ctypes.data, 64, 64, None) == bad
    assert lib.syldet_trace_interleaved_device_s16(None, out.ctypes.data, 8, 0, t16.ctypes.data, 64, None) == bad
    assert lib.syldet_trace(None, po, 8, 0, t32.ctypes.data_as(_abi.c_float_p), 64, 64) == bad
    assert lib.syldet_trace_s16(None, po, 8, 0, t16.ctypes.data_as(_abi.c_int16_p), 64, 64) == bad
    assert not t32.any() and not t16.any()


def test_header_declarations_compile_as_c99_and_the_cpp_mirror_has_the_methods(tmp_path):
    c = tmp_path / "trace.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    float o[4] = {0}, t[8]; int16_t q[8];\n"
                 "    int st = syldet_trace(NULL, o, 4, 0, t, 8, 8) + syldet_trace_s16(NULL, o, 4, 0, q, 8, 8) +\n"
                 "             syldet_trace_device(NULL, o, 4, 0, t, 8, 8, NULL) + syldet_trace_device_s16(NULL, o, 4, 0, q, 8, 8, NULL) +\n"
                 "             syldet_trace_interleaved_device_s16(NULL, o, 4, 0, q, 8, NULL);\n"
                 "    return st == 5 * SYLDET_ERR_INVALID_ARGUMENT ? 0 : 1;\n"
                 "}\n")
    exe = tmp_path / "trace"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + LIB, "-lsyldet", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    cpp = tmp_path / "trace.cpp"
    cpp.write_text('#include "syldet.hpp"\n'
                   "void f(syldetxx::SyllableDetectorBank &b, const float *o, float *t, int16_t *q) {\n"
                   "    std::vector<float> v = b.trace(o, 4, 8); v = b.trace(o, 4, 8, 1);\n"
                   "    b.traceDevice(o, 4, 0, t, 8, 8, nullptr); b.traceDevicePCM16(o, 4, 0, q, 8, 8, nullptr);\n"
                   "    b.traceInterleavedDevicePCM16(o, 4, 0, q, 8, nullptr);\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(cpp)], check=True)


def test_the_closed_form_is_the_simulators_buffer_loop():
    """400 seeded geometries: windows 64 .. 256, overlaps -40 .. W - 1 (gaps included), timeRange 1 .. 12, lengths from 0 (below
    D) to 40 hops behind it (so most end inside a hold), buffers cut at random.  The loop writes every sample of every buffer
    and equals the closed form in every sample."""
    rng = np.random.default_rng(20240521)
    seen = {"gap": 0, "t1": 0, "below_D": 0, "inside_hold": 0}
    for trial in range(400):
        W = int(rng.choice([64, 128, 200, 256]))
        ov = int(rng.integers(-40, W))
        T = 1 if trial % 9 == 0 else int(rng.integers(1, 13))
        D, hop, gap = trace_ref.geometry(W, ov, T)
        S = int(rng.integers(0, D)) if trial % 11 == 0 else int(rng.integers(0, 40 * hop + D))
        E = trace_ref.count_evals(S, W, ov, T)
        assert S <= max(D, D + E * hop)                            # the holds of S samples' evaluations reach S: nothing lies behind them
        out = (rng.random((E, 2)) * 1.6 - 0.3).astype(np.float32)  # below 0, inside, above the threshold
        thr = [0.71, 0.9]
        want = trace_ref.closed_form(out, thr, D, hop, S, k=trial % 2)
        got = trace_ref.simulator_loop(trace_ref.values(out, thr, trial % 2), W, ov, T, S, rng)
        assert not np.isnan(got).any(), "trial %d: the loop left a sample unwritten" % trial
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), "trial %d (W %d, overlap %d, T %d, S %d)" % (trial, W, ov, T, S)
        seen["gap"] += ov < 0
        seen["t1"] += T == 1
        seen["below_D"] += S < D
        seen["inside_hold"] += S > D and (S - D) % hop != 0
    assert min(seen.values()) >= 10, seen


def test_the_reference_functions_on_hand_made_values():
    out = np.array([[np.nan], [np.inf], [-np.inf], [-0.25], [0.5], [2.0], [0.0]], np.float32)
    v = trace_ref.values(out, [0.5])
    assert np.isnan(v[0]) and list(v[1:]) == [1, 0, 0, 1, 1, 0]
    assert list(trace_ref.values(out, [-0.5])[1:]) == [0, 1, 0.5, 0, 0, 0]      # a negative threshold flips the sign before the clamp
    z = trace_ref.values(out, [0.0])                                              # x / 0: 1 or 0 by its sign, 0 / 0 stays NaN
    assert np.isnan(z[0]) and list(z[1:6]) == [1, 0, 0, 1, 1] and np.isnan(z[6])
    q = trace_ref.to_s16(np.array([0, 1, np.nan, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767], np.float32))
    assert list(q[:3]) == [0, 32767, 0]
    tr = trace_ref.closed_form(out, [0.5], D=3, hop=2, n_samples=20)
    assert not tr[:3].any() and not tr[3 + 7 * 2:].any() and list(tr[9:17]) == [0, 0, 1, 1, 1, 1, 0, 0]


@pytest.fixture(scope="module")
def wav_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavdrv")
    src = d / "wr.cpp"
    # writes argv[3] frames of argv[2] tracks (sample (f, c) = the low 16 bits of 7919 f + 131 c - 20000) to argv[1], reads the file
    # back with the tool's own readers and compares
    src.write_text('#include "wav.hpp"\n#include <cstdlib>\n'
                   "int main(int argc, char **argv) {\n"
                   "    if (argc < 4) return 9;\n"
                   "    const int ch = std::atoi(argv[2]); const long long n = std::atoll(argv[3]);\n"
                   "    std::vector<int16_t> x((size_t)n * ch);\n"
                   "    for (long long f = 0; f < n; f++) for (int c = 0; c < ch; c++) x[(size_t)f * ch + c] = (int16_t)(uint16_t)(7919 * f + 131 * c - 20000);\n"
                   "    std::string e;\n"
                   "    if (!wav::write_s16(argv[1], 44100.0, ch, n, x.data(), e)) return 2;\n"
                   "    wav::Info i; std::vector<int16_t> y;\n"
                   "    if (!wav::read_s16(argv[1], i, y, e)) return 3;\n"
                   "    if (i.channels != ch || i.frames != n || i.rate != 44100.0 || i.bits != 16 || i.format != 1 || i.data_offset != 44) return 4;\n"
                   "    if (y != x) return 5;\n"
                   "    if (wav::write_s16(argv[1], 44100.0, 0, n, x.data(), e)) return 6;\n"
                   "    if (wav::write_s16(argv[1], 44100.0, 2, (1ll << 30), x.data(), e) || e.find(\"4 GiB\") == std::string::npos) return 7;\n"
                   "    return wav::write_s16(argv[1], 44100.0, ch, n, x.data(), e) ? 0 : 8;\n"
                   "}\n")
    exe = d / "wr"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "cli"),
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("channels,frames", [(1, 1000), (2, 4097), (7, 333), (1, 0), (7, 0)])
def test_wav_write_s16_round_trip(tmp_path, wav_driver, channels, frames):
    p = str(tmp_path / "w.wav")
    assert subprocess.run([wav_driver, p, str(channels), str(frames)]).returncode == 0
    assert os.path.getsize(p) == 44 + 2 * channels * frames            # the canonical header, nothing behind the samples
    with wave.open(p, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (channels, 2, 44100, frames)
        got = np.frombuffer(w.readframes(frames), "<i2").reshape(frames, channels)
    f, c = np.meshgrid(np.arange(frames, dtype=np.int64), np.arange(channels, dtype=np.int64), indexing="ij")
    want = ((7919 * f + 131 * c - 20000) & 0xFFFF).astype(np.uint16).view(np.int16)
    assert np.array_equal(got, want)


def run_cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def net_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("tracenet") / "net.txt")
    open(p, "w").write(util.sample_net().toText())
    return p


def test_the_tools_usage_errors_for_simulate(tmp_path, net_file):
    assert os.path.exists(CLI), "syllable-detector-cli has not been built"
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((100, 2), np.int16), 44100, "pcm16")
    out = str(tmp_path / "sim.wav")
    cases = [["-n", net_file, "--simulate", out],                                   # no -a
             ["-n", net_file, "-a", a, "-a", a, "--simulate", out],                 # more than one -a
             ["-n", net_file, "-a", a, "--simulate"],                               # a missing value
             ["-n", net_file, "-a", a, "--simulate", out, "--simulate-output"],
             ["-n", net_file, "-a", a, "--simulate", out, "--simulate-output", "-1"],
             ["-n", net_file, "-a", a, "--simulate", out, "--simulate-output", "one"],
             ["-n", net_file, "-a", a, "--simulate-output", "0"],                   # an output for a track nobody asked for
             ["-n", net_file, "-a", a, "--simulate", out, "--simulate-output", "1"]]   # the example network has one output
    for args in cases:
        r = run_cli(*args)
        assert r.returncode == 64, (args, r.returncode, r.stderr)
        assert "Path to trained network file." in r.stdout, args      # every usage error prints the usage text
        assert not os.path.exists(out), args
    assert "the network has 1 output(s)" in run_cli(*cases[-1]).stderr
    u = run_cli("-h").stdout
    assert "--simulate <out.wav>" in u and "--simulate-output <k>" in u


def test_probe_ignores_the_simulate_options(tmp_path):
    a = str(tmp_path / "a.wav")
    wavutil.write_wav(a, np.zeros((123, 2), np.int16), 22050, "pcm16")
    plain = run_cli("--probe", "-a", a)
    out = str(tmp_path / "sim.wav")
    r = run_cli("--probe", "-a", a, "--simulate", out, "--simulate-output", "5")
    assert plain.returncode == 0 and (r.returncode, r.stdout, r.stderr) == (0, plain.stdout, plain.stderr)
    assert not os.path.exists(out)


def _kernel_body(text, fragment):
    """the instructions of the one kernel whose mangled name holds `fragment`: from its label to its .Lfunc_end"""
    labels = re.findall(r"^(_Z\w*%s\w*):" % fragment, text, re.M)
    assert len(labels) == 1, (fragment, labels)
    start = text.index("\n" + labels[0] + ":")
    return text[start:text.index(".Lfunc_end", start)]


def test_the_built_trace_kernels_store_sixteen_bytes_a_lane():
    """the ISA the build wrote (--save-temps) for the file that holds trace_kernel: the aligned path of every form stores with
    global_store_dwordx4, the division is the correctly rounded one, the 16-bit forms round with v_rndne_f32"""
    files = [f for f in glob.glob(os.path.join(LIB, "obj", "isa", "*-hip-amdgcn-*.s")) if "trace_kernel" in open(f).read()]
    assert len(files) == 1, files
    text = open(files[0]).read()
    for name in ("trace_kernelIfE", "trace_kernelIsE", "trace_interleaved_s16_kernel"):
        body = _kernel_body(text, name)
        assert "global_store_dwordx4" in body, name
        assert "v_div_fixup_f32" in body, name                      # not a reciprocal multiply
        assert ("v_rndne_f32" in body) == (name != "trace_kernelIfE"), name
