"""The streaming band-limited resampler on the host (no GPU): the syldet_sinc_resampler* functions are declared, exported and
bound; syldet_sinc_ready is the numpy restatement of tests/sinc_stream_ref.py; the index arithmetic both the kernels and the host
use (csrc/sinc_stream.hpp) walks clean on the CPU, plain and under ASan + UBSan; a NULL handle is refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sinc_ref
import sinc_stream_ref
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "syllable_detector_swift_amd", "csrc")
LIB = _abi.lib
NEW = ["syldet_sinc_ready", "syldet_sinc_resampler_create", "syldet_sinc_resampler_destroy", "syldet_sinc_resampler_reset",
       "syldet_sinc_resampler_position", "syldet_sinc_resampler_count", "syldet_sinc_resampler_flush_count", "syldet_sinc_resample_device",
       "syldet_sinc_resample_device_s16", "syldet_sinc_resampler_flush_device", "syldet_sinc_resample", "syldet_sinc_resampler_flush"]
RATIOS = [(48000.0, 44100.0), (44100.0, 48000.0), (96000.0, 44100.0), (22050.0, 44100.0), (24414.0625, 44100.0), (16.0, 1.0), (1.0, 16.0)]
QUALITIES = [(4, 0.9), (8, 0.8), (32, 0.9), (64, 0.9)]             # (zero crossings, rolloff)


def test_the_streaming_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "syldet.h")).read()
    declared = set(re.findall(r"\b(syldet_[a-z_0-9]+)\s*\(", header))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES, name
    assert "typedef struct syldet_sinc_resampler syldet_sinc_resampler_t;" in header
    assert lib.syldet_abi_version() == 1                     # nothing existing changed


@pytest.mark.parametrize("rates", RATIOS)
def test_ready_is_the_numpy_restatement(rates):
    ri, ro = rates
    for Z, rho in QUALITIES:
        ns = list(range(3000)) + [2 ** 24 + k for k in range(-3, 40)] + [2 ** 40 + k for k in range(-3, 40)]
        prev, prev_n = 0, -1
        for n in ns:
            got = LIB.syldet_sinc_ready(n, ri, ro, Z, rho)
            assert got == sinc_stream_ref.ready(n, ri, ro, Z, rho), (n, ri, ro, Z)
            assert got >= prev, "monotone"
            assert got <= LIB.syldet_convert_rate_count(n, ri, ro) == sinc_ref.count(n, ri, ro)
            prev, prev_n = got, n
        H = sinc_ref.design(ri, ro, rho, Z)[1]
        assert LIB.syldet_sinc_ready(int(H), ri, ro, Z, rho) == 0 and LIB.syldet_sinc_ready(int(H) + 1, ri, ro, Z, rho) >= 1
    assert LIB.syldet_sinc_ready(-5, ri, ro, 32, 0.9) == 0


def test_ready_is_minus_one_for_refused_parameters():
    for args in [(1000, 0.0, 44100.0, 32, 0.9), (1000, 48000.0, -1.0, 32, 0.9), (1000, float("nan"), 44100.0, 32, 0.9),
                 (1000, 48000.0, float("inf"), 32, 0.9), (1000, 48000.0, 44100.0, 3, 0.9), (1000, 48000.0, 44100.0, 65, 0.9),
                 (1000, 48000.0, 44100.0, 32, 0.0), (1000, 48000.0, 44100.0, 32, 1.01), (1000, 16.001, 1.0, 32, 0.9),
                 (1000, 1.0, 16.001, 32, 0.9), (1000, 48000.0, 44100.0, 64, 1e-4)]:
        assert LIB.syldet_sinc_ready(*args) == -1, args


def _build_walk(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "sinc_stream_walk_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_index_arithmetic_walks_clean_on_the_cpu(tmp_path):
    """tests/cpp/sinc_stream_walk_test.cpp: random partitions of seven ratios and four qualities, from N = 0 and from the middle
    of a stream near 2^24 and 2^40 -- every read inside the buffer it names, the carried history the last samples of a plain
    concatenation.  The library's kernels and host code include the same header."""
    _build_walk(tmp_path / "walk", ["-O2"])
    for f in ("kernels_sinc.hip", "syldet_resampler.cpp"):
        assert '#include "sinc_stream.hpp"' in open(os.path.join(CSRC, f)).read(), f


def test_the_index_arithmetic_walks_clean_under_asan_and_ubsan(tmp_path):
    _build_walk(tmp_path / "walk_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_null_handles_and_bad_arguments_are_refused_before_any_device():
    bad = _abi.ERR_INVALID_ARGUMENT
    h = _abi.Handle()
    n = C.c_int64(-1)
    assert LIB.syldet_sinc_resampler_create(48000.0, 44100.0, 1, 0, 32, 12.0, 0.9, None) == bad
    for args in [(0.0, 44100.0, 1, 0, 32, 12.0, 0.9), (48000.0, 44100.0, 0, 0, 32, 12.0, 0.9), (48000.0, 44100.0, 65536, 0, 32, 12.0, 0.9),
                 (48000.0, 44100.0, 1, 0, 3, 12.0, 0.9), (48000.0, 44100.0, 1, 0, 32, 20.1, 0.9), (48000.0, 44100.0, 1, 0, 32, 12.0, 0.0)]:
        assert LIB.syldet_sinc_resampler_create(*args, C.byref(h)) == bad and not h.value, args
    assert LIB.syldet_sinc_resampler_create(16.001, 1.0, 1, 0, 32, 12.0, 0.9, C.byref(h)) == _abi.ERR_UNSUPPORTED and not h.value
    assert LIB.syldet_sinc_resample_device(None, None, 10, 10, None, 10, C.byref(n), None) == bad
    assert LIB.syldet_sinc_resample_device_s16(None, None, 10, 10, None, 10, C.byref(n), None) == bad
    assert LIB.syldet_sinc_resampler_flush_device(None, None, 10, C.byref(n), None) == bad
    assert LIB.syldet_sinc_resample(None, None, 10, 10, None, 10, C.byref(n)) == bad
    assert LIB.syldet_sinc_resampler_flush(None, None, 10, C.byref(n)) == bad
    assert LIB.syldet_sinc_resampler_reset(None) == bad
    assert LIB.syldet_sinc_resampler_position(None, None, None, None) == bad
    assert LIB.syldet_sinc_resampler_count(None, 1000) == 0 and LIB.syldet_sinc_resampler_flush_count(None) == 0
    assert LIB.syldet_sinc_resampler_destroy(None) == 0
    assert n.value == -1                                     # (a NULL handle is refused before anything is written)


def test_the_mirrors_have_the_class():
    hpp = open(os.path.join(ROOT, "include", "syldet.hpp")).read()
    swift = open(os.path.join(ROOT, "swift", "Resampler.swift")).read()
    assert "class ResamplerSinc {" in hpp and "ResamplerSinc(const ResamplerSinc &) = delete;" in hpp
    for m in ("resampleArray", "resampleVector", "countOutput", "flush", "reset"):
        assert re.search(r"\b%s\(" % m, hpp.split("class ResamplerSinc {")[1]), m
    assert "class ResamplerSinc: Resampler {" in swift
    for m in ("resampleVector", "resampleArray", "flush", "reset"):
        assert re.search(r"func %s\(" % m, swift.split("class ResamplerSinc: Resampler {")[1]), m
    cpp = '#include "syldet.hpp"\nint64_t f(syldetxx::ResamplerSinc &r, std::vector<float> &x) { x = r.resampleArray(x); x = r.flush(); r.reset(); return r.countOutput(32) + r.samplesIn(); }\n'
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=cpp, text=True, check=True)


def test_resampler_sinc_needs_a_device():
    import torch
    import syllable_detector_swift_amd as sd
    assert sd.sincReady(3000, 48000.0, 44100.0) == sinc_stream_ref.ready(3000, 48000.0, 44100.0)
    assert sd.sincReady(3000, 48000.0, 44100.0, zeroCrossings=2) == -1
    if torch.cuda.is_available():                           # (the device runs are tests/test_sinc_stream_gpu.py)
        with sd.ResamplerSinc(48000.0, 44100.0) as r:
            assert r.position == (0, 0, False)
        return
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.ResamplerSinc(48000.0, 44100.0)
    assert ei.value.status == _abi.ERR_NO_DEVICE
