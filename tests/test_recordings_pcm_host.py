"""The files' own sample formats, the host side (no GPU): csrc/pcm_values.hpp alone under ASan and UBSan (a program of its own,
tests/cpp/pcm_values_test.cpp), the entry points under ABI 1, syldet_pcm_decode against the numpy model of tests/pcm_ref.py, every
refusal of a byte source with its status and its recording named (syldet_pcm_check_sources makes the loads' own checks without a
handle, which cannot be made without a device; the same refusals through the device calls, with the rows left alone, are in
tests/test_recordings_pcm_gpu.py), the Python layer's argument errors, and the tool's source: its batch path calls the two loads and
converts no sample on the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pcm_ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_pcm_sample_bytes", "syldet_pcm_decode", "syldet_pcm_check_sources", "syldet_recordings_load_pcm_device",
       "syldet_recordings_load_sinc_pcm_device")


def test_the_decode_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "pcm_values_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pcm_values_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int(32_t)? %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    # the delivery the calls stand in for, and the kernel's name
    section = header[header.index("the files' own sample formats"):header.index("every recording's output track and trigger track")]
    assert "audioSettings" in section and "SyllableDetector.swift:19-23" in section and '"recordings_load_pcm_kernel"' in section
    for name, value in (("U8", 1), ("S16", 2), ("S24", 3), ("S32", 4), ("F32", 5), ("F64", 6)):
        assert "#define SYLDET_PCM_%s" % name in header and getattr(sd, "PCM_" + name) == value == getattr(pcm_ref, name)
    assert [sd.pcmSampleBytes(f) for f in pcm_ref.FORMATS] == [pcm_ref.BYTES[f] for f in pcm_ref.FORMATS]
    assert sd.pcmSampleBytes(0) == 0 and sd.pcmSampleBytes(7) == 0 and sd.pcmSampleBytes(-1) == 0
    assert callable(sd.Recordings.loadPCM) and callable(sd.Recordings.loadSincPCM) and callable(sd.pcmDecode) and callable(sd.PCM24)


@pytest.mark.parametrize("fmt", pcm_ref.FORMATS, ids=[pcm_ref.NAMES[f] for f in pcm_ref.FORMATS])
def test_decode_equals_the_model(fmt):
    rng = np.random.default_rng(100 + fmt)
    size = pcm_ref.BYTES[fmt]
    # random bytes: every bit pattern of the format, NaNs of every payload among the floats; then the format's edge cases
    for raw in (rng.integers(0, 256, size=4099 * size + 3, dtype=np.uint8), np.concatenate([pcm_ref.samples(fmt, 41, rng), np.zeros(3, np.uint8)])):
        for offset in range(4):
            for tracks in (1, 2, 3):
                step = tracks * size
                n = (raw.size - offset - size) // step + 1
                want = pcm_ref.decode(raw, fmt, n, step, offset)
                got = sd.pcmDecode(raw[offset:], fmt, n, step)
                assert got.dtype == np.float32 and pcm_ref.same(got, want), (pcm_ref.NAMES[fmt], offset, step)
    if fmt == pcm_ref.F32:
        # the bits, copied: NaN payloads too
        raw = pcm_ref.samples(fmt, 16, rng)
        assert np.array_equal(sd.pcmDecode(raw, fmt).view(np.uint32), raw.view("<u4"))
    assert sd.pcmDecode(b"", fmt).size == 0 and sd.pcmDecode(np.zeros(size - 1, np.uint8), fmt).size == 0


def test_decode_refusals():
    buf = np.zeros(64, np.uint8)
    out = np.zeros(8, np.float32)
    o = out.ctypes.data_as(_abi.c_float_p)
    bad = _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_pcm_decode(0, buf.ctypes.data, 4, 4, o) == bad and "format" in _abi.last_error()
    assert LIB.syldet_pcm_decode(7, buf.ctypes.data, 4, 8, o) == bad
    assert LIB.syldet_pcm_decode(sd.PCM_S24, buf.ctypes.data, -1, 3, o) == bad
    assert LIB.syldet_pcm_decode(sd.PCM_S24, None, 4, 3, o) == bad and LIB.syldet_pcm_decode(sd.PCM_S24, buf.ctypes.data, 4, 3, None) == bad
    assert LIB.syldet_pcm_decode(sd.PCM_S24, buf.ctypes.data, 4, 2, o) == bad and "step" in _abi.last_error()
    assert LIB.syldet_pcm_decode(sd.PCM_F64, buf.ctypes.data, 4, 7, o) == bad
    assert LIB.syldet_pcm_decode(sd.PCM_S24, None, 0, 3, None) == _abi.OK
    with pytest.raises(ValueError):
        sd.pcmDecode(buf, sd.PCM_S32, 17)                          # beyond the data
    with pytest.raises(ValueError):
        sd.pcmDecode(np.zeros(4, np.float32), sd.PCM_F32)


def check_sources(base, src_bytes, offsets, steps, formats, n):
    offsets, n, formats = np.asarray(offsets, np.int64), np.asarray(n, np.int64), np.asarray(formats, np.int32)
    steps = None if steps is None else np.asarray(steps, np.int32)
    return LIB.syldet_pcm_check_sources(base, src_bytes, offsets.ctypes.data_as(_abi.c_int64_p), None if steps is None else steps.ctypes.data_as(_abi.c_int32_p),
                                        formats.ctypes.data_as(_abi.c_int32_p), n.ctypes.data_as(_abi.c_int64_p), offsets.size)


def test_every_refusal_names_its_recording_without_a_device():
    bad, ok = _abi.ERR_INVALID_ARGUMENT, _abi.OK
    base = 1 << 20                                                  # the address the source will have: never read
    fmts = [sd.PCM_U8, sd.PCM_S16, sd.PCM_S24, sd.PCM_S32, sd.PCM_F32, sd.PCM_F64]
    n = [100] * 6
    steps = [1, 2, 3, 4, 4, 8]
    offsets = [0, 100, 300, 600, 1000, 1400]                        # ends: 100, 300, 600, 1000, 1400, 2200
    assert check_sources(base, 2200, offsets, steps, fmts, n) == ok
    assert check_sources(base, 2200, offsets, None, fmts, n) == ok   # no steps: contiguous recordings
    # the plain load's checks come first
    assert check_sources(None, 2200, offsets, steps, fmts, n) == bad and "NULL" in _abi.last_error()
    assert check_sources(base, 2200, [0, 100, -1, 600, 1000, 1400], steps, [0] * 6, n) == bad and "recording 2" in _abi.last_error()
    assert check_sources(base, 2200, offsets, [1, 2, 3, 0, 4, 8], [0] * 6, n) == bad and "recording 3" in _abi.last_error()
    # an unknown format
    for f in (0, 7, -1, 255):
        assert check_sources(base, 2200, offsets, steps, fmts[:4] + [f] + fmts[5:], n) == bad
        assert "recording 4" in _abi.last_error() and "format" in _abi.last_error()
    # a step below the sample's bytes
    for k, s in ((1, 1), (2, 2), (3, 3), (4, 2), (5, 4)):
        st = list(steps)
        st[k] = s
        assert check_sources(base, 2200, offsets, st, fmts, n) == bad and "recording %d" % k in _abi.last_error() and "step" in _abi.last_error()
    # an address or a step that is no multiple of the sample's size: S16, S32, F32, F64 -- by the offset, by the base, by the step
    for k, size in ((1, 2), (3, 4), (4, 4), (5, 8)):
        for delta in range(1, size):
            off = list(offsets)
            off[k] += delta
            assert check_sources(base, 4000, off, steps, fmts, n) == bad and "recording %d" % k in _abi.last_error() and "multiple" in _abi.last_error()
            assert check_sources(base + delta, 4000, offsets, steps, fmts, n) == bad and "multiple" in _abi.last_error()
            st = list(steps)
            st[k] = size + delta
            assert check_sources(base, 4000, offsets, st, fmts, n) == bad and "recording %d" % k in _abi.last_error()
        # the base and the offset off together, their sum a multiple: taken
        assert check_sources(base + 1, 4000, [size - 1], [3 * size], [fmts[k]], [10]) == ok
        assert check_sources(base + 1, 4000, [size], [3 * size], [fmts[k]], [10]) == bad and "recording 0" in _abi.last_error()
    # U8 and S24 take any address and any step from their size on
    for delta in range(1, 4):
        assert check_sources(base + delta, 4000, [0, 100 - delta, 300, 600 - delta, 1000 - delta, 1400 - delta], [1 + delta, 2, 3 + delta, 4, 4, 8], fmts,
                             [30] * 6) == ok
    # a recording whose last sample byte lies at or beyond src_bytes: the last byte is 2199
    assert check_sources(base, 2199, offsets, steps, fmts, n) == bad and "recording 5" in _abi.last_error() and "src_bytes" in _abi.last_error()
    assert check_sources(base, 599, offsets, steps, fmts, n) == bad and "recording 2" in _abi.last_error()
    assert check_sources(base, 2200, offsets, steps, fmts, [100, 101, 100, 100, 100, 100]) == ok           # (recordings may overlap)
    assert check_sources(base, 2200, offsets, steps, fmts, [100, 100, 100, 100, 100, 101]) == bad and "recording 5" in _abi.last_error()
    assert check_sources(base, 2200, [0, 100, 2198, 600, 1000, 1400], steps, fmts, [100, 100, 1, 100, 100, 100]) == bad
    assert check_sources(base, 2200, [0, 100, 2197, 600, 1000, 1400], steps, fmts, [100, 100, 1, 100, 100, 100]) == ok
    assert check_sources(base, -1, offsets, steps, fmts, n) == bad
    # a recording without samples reads nothing, wherever it points; lengths near 2^63 do not wrap
    assert check_sources(base, 0, [0, 10 ** 12, 5, 4, 8, 16], steps, fmts, [0] * 6) == ok
    assert check_sources(base, 2200, offsets, steps, fmts, [100, 100, 2 ** 62, 100, 100, 100]) == bad and "recording 2" in _abi.last_error()
    assert check_sources(base, 2 ** 62, [0, 100, 2 ** 62 - 3, 600, 1000, 1400], steps, fmts, [100, 100, 1, 100, 100, 100]) == ok
    assert check_sources(base, 2 ** 62, [0, 100, 2 ** 62 - 2, 600, 1000, 1400], steps, fmts, [100, 100, 1, 100, 100, 100]) == bad


@pytest.mark.parametrize("name", ["syldet_recordings_load_pcm_device", "syldet_recordings_load_sinc_pcm_device"])
def test_a_null_handle_is_refused_before_anything_else(name):
    fn = getattr(LIB, name)
    one = np.zeros(1, np.int64)
    step, fmt = np.full(1, 3, np.int32), np.full(1, sd.PCM_S24, np.int32)
    rate = np.array([48000.0])
    src = (16, 64, one.ctypes.data_as(_abi.c_int64_p), step.ctypes.data_as(_abi.c_int32_p), fmt.ctypes.data_as(_abi.c_int32_p))
    conv = (one.ctypes.data_as(_abi.c_int64_p), rate.ctypes.data_as(_abi.c_double_p), 32, 12.0, 0.9) if "sinc" in name else ()
    assert fn(None, *src, *conv, 16, 8, None) == _abi.ERR_INVALID_ARGUMENT and "NULL" in _abi.last_error()


def test_python_argument_errors_need_no_device():
    det = sd.SyllableDetector.__new__(sd.SyllableDetector)    # (no device: these are refused before one is needed)
    det._h = None
    with pytest.raises(ValueError, match="uint8, int16, int32, float32 or float64"):
        det.runRecordings([np.zeros(100, np.float32), np.zeros(100, np.int64)])
    with pytest.raises(ValueError, match="uint8, int16, int32, float32 or float64"):
        det.runRecordings([np.zeros(100, np.complex64)])
    with pytest.raises(ValueError, match="one rate per array"):
        det.runRecordings([np.zeros(100, np.float32), sd.PCM24(np.zeros((100, 1, 3), np.uint8))], rates=[48000.0], resample="sinc")
    for shape, dtype in (((100, 2), np.uint8), ((100, 3), np.int8), ((100, 2, 3, 1), np.uint8), ((100, 2, 4), np.uint8)):
        with pytest.raises(ValueError, match="PCM24"):
            sd.PCM24(np.zeros(shape, dtype))
    p = sd.PCM24(np.zeros((100, 2, 3), np.uint8))
    assert (p.frames, p.tracks) == (100, 2) and sd.PCM24(np.zeros((7, 3), np.uint8)).tracks == 1


def test_the_tools_batch_path_loads_the_files_own_bytes():
    def text(name):
        with open(os.path.join(ROOT, "syllable_detector_swift_amd", "cli", name)) as f:
            return f.read()

    main, wav, batch_hpp, one_hpp, shared = text("main.cpp"), text("wav.hpp"), text("batch.hpp"), text("one_file.hpp"), text("align.hpp")
    assert "inline bool read_raw(" in wav
    assert "process_batched(run)" in main and "#include \"batch.hpp\"" in main and "#include \"one_file.hpp\"" in batch_hpp and "#include \"align.hpp\"" in one_hpp
    # the batch path: the plan, the stages and run_batch, with what they share with the one-file path; the gatherer: process_batched
    batch = batch_hpp[batch_hpp.index("struct BatchPlan"):batch_hpp.index("int process_batched(")] + shared
    batched = batch_hpp[batch_hpp.index("int process_batched("):]
    assert "int run_batch(" in batch and "int load_and_run(" in batch and "BatchPlan plan_batch(" in batch
    assert "syldet_recordings_load_pcm_device(" in batch and "syldet_recordings_load_sinc_pcm_device(" in batch
    # an all-16-bit batch still runs int16 rows
    assert "syldet_recordings_load_device_s16(" in batch and "syldet_run_device_s16(" in batch and "syldet_recordings_load_sinc_device_s16(" in batch
    # no sample of a batched file is converted on the host: the batch reads raw bytes, and the widening loop is gone
    assert "wav::read_raw(" in batched and "wav::read(" not in batched and "wav::read_s16(" not in batched
    assert "1.0f / 32768.0f" not in batch and "wav::read" not in batch and "syldet_pcm_decode" not in batch
    # the one-file path is the reader's, as before
    one = one_hpp[one_hpp.index("struct OneFile"):] + shared
    assert "int process_file(" in one and "int read_and_probe(" in one
    assert "wav::read(" in one and "read_raw" not in one
