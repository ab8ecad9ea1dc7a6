"""16-bit PCM entry points on the host (no GPU): the six *_s16 functions are declared in the C header, exported and bound,
they refuse what their fp32 twins refuse before any device is touched, and the Python and C++ surfaces take int16 only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, detector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["syldet_run_device_s16", "syldet_run_s16", "syldet_run_interleaved_device_s16", "syldet_run_interleaved_s16",
       "syldet_append_s16", "syldet_append_interleaved_s16"]


def test_the_s16_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert "const int16_t *" in header
    assert lib.syldet_abi_version() == 1                     # nothing existing changed


def test_null_handle_is_refused_by_every_s16_entry_point():
    lib = _abi.lib
    x = np.zeros(64, np.int16)
    p = x.ctypes.data_as(_abi.c_int16_p)
    out, fl = np.zeros(64, np.float32), np.zeros(64, np.uint8)
    po, pf = out.ctypes.data_as(_abi.c_float_p), fl.ctypes.data_as(_abi.c_uint8_p)
    bad = _abi.ERR_INVALID_ARGUMENT
    assert lib.syldet_run_device_s16(None, x.ctypes.data, 64, 64, out.ctypes.data, fl.ctypes.data, None) == bad
    assert lib.syldet_run_s16(None, p, 64, 64, po, pf) == bad
    assert lib.syldet_run_interleaved_device_s16(None, x.ctypes.data, 64, 1, out.ctypes.data, fl.ctypes.data, None) == bad
    assert lib.syldet_run_interleaved_s16(None, p, 64, 1, po, pf) == bad
    assert lib.syldet_append_s16(None, 0, p, 64) == bad
    assert lib.syldet_append_interleaved_s16(None, p, 64, 1) == bad
    # (and the fp32 twins say the same)
    assert lib.syldet_run(None, out.ctypes.data_as(_abi.c_float_p), 64, 64, po, pf) == bad
    assert lib.syldet_append(None, 0, out.ctypes.data_as(_abi.c_float_p), 64) == bad


def test_python_pcm16_input_must_be_int16():
    detector._pcm16(np.zeros((2, 8), np.int16))
    for a in (np.zeros(8, np.float32), np.zeros(8, np.int32), np.zeros(8, np.uint16), [1, 2, 3]):
        with pytest.raises(ValueError):
            detector._pcm16(a)
    for m in ("runPCM16", "runPCM16Host", "runInterleavedPCM16", "runInterleavedPCM16Host", "appendAudioDataPCM16",
              "appendInterleavedDataPCM16"):
        assert callable(getattr(sd.SyllableDetector, m)), m
    assert "runPCM16Host" in sd.SyllableDetector.runHost.__doc__


def test_header_declarations_compile_as_c99_and_the_cpp_mirror_has_the_methods(tmp_path):
    c = tmp_path / "s16.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    int16_t x[4] = {0, 1, -1, 32767}; float o[4]; uint8_t f[4];\n"
                 "    int st = syldet_run_s16(NULL, x, 4, 4, o, f) + syldet_run_device_s16(NULL, x, 4, 4, o, f, NULL) +\n"
                 "             syldet_run_interleaved_s16(NULL, x, 4, 1, o, f) + syldet_run_interleaved_device_s16(NULL, x, 4, 1, o, f, NULL) +\n"
                 "             syldet_append_s16(NULL, 0, x, 4) + syldet_append_interleaved_s16(NULL, x, 4, 1);\n"
                 "    return st == 6 * SYLDET_ERR_INVALID_ARGUMENT ? 0 : 1;\n"
                 "}\n")
    lib = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
    exe = tmp_path / "s16"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + lib, "-lsyldet", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
    cpp = tmp_path / "s16.cpp"
    cpp.write_text('#include "syldet.hpp"\n'
                   "void f(syldetxx::SyllableDetectorBank &b, syldetxx::SyllableDetector &d, const int16_t *x) {\n"
                   "    std::vector<float> o; std::vector<uint8_t> fl;\n"
                   "    b.runPCM16(x, 4, o, fl); b.runDevicePCM16(x, 4, 4, nullptr, nullptr, nullptr);\n"
                   "    b.runInterleavedPCM16(x, 4, o, fl); b.runInterleavedDevicePCM16(x, 4, nullptr, nullptr, nullptr);\n"
                   "    b.appendInterleavedDataPCM16(x, 4); d.appendAudioDataPCM16(x, 4);\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(cpp)], check=True)


def test_wav_read_s16_gives_the_stored_samples(tmp_path):
    """The tool's int16 reader (what it hands to syldet_run_interleaved_device_s16) against its fp32 reader: the same frames,
    read()'s value of every sample exactly read_s16's times 2^-15; anything but 16-bit PCM is refused."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wavutil
    rng = np.random.default_rng(1)
    frames = rng.integers(-32768, 32768, (999, 3)).astype(np.int16)
    frames[0] = [-32768, 32767, 0]
    p16, pf = tmp_path / "a.wav", tmp_path / "f.wav"
    wavutil.write_wav(str(p16), frames, 44100, "pcm16")
    wavutil.write_wav(str(pf), frames.astype(np.float32) / 32768.0, 44100, "float32")
    src = tmp_path / "rd.cpp"
    src.write_text('#include "wav.hpp"\n#include <cstring>\n'
                   "int main(int argc, char **argv) {\n"
                   "    wav::Info i1, i2; std::vector<float> f; std::vector<int16_t> x; std::string e;\n"
                   "    if (!wav::read(argv[1], i1, f, e) || !wav::read_s16(argv[1], i2, x, e)) return 2;\n"
                   "    if (x.size() != f.size() || i1.frames != i2.frames || i2.channels != 3) return 3;\n"
                   "    for (size_t k = 0; k < x.size(); k++) { float v = (float)x[k] * (1.0f / 32768.0f);\n"
                   "        if (std::memcmp(&v, &f[k], 4) != 0) return 4; }\n"
                   "    if (x[0] != -32768 || x[1] != 32767) return 5;\n"
                   "    if (wav::read_s16(argv[2], i2, x, e)) return 6;\n"
                   "    return 0;\n"
                   "}\n")
    exe = tmp_path / "rd"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "cli"),
                    str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe), str(p16), str(pf)]).returncode == 0
