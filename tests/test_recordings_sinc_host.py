"""Packed recordings at other rates, the host side (no GPU): the two entry points exist under ABI 1, what they refuse without a
handle, recordingLengths against the model's count, the Python layer's argument errors, and the tool's help text.  A
syldet_recordings_t cannot be made without a device, so the statuses that need one (a length that differs from the plan's, a rate
the converter does not take, ...) are in tests/test_recordings_sinc_gpu.py -- they too come back before the device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sinc_ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
LIB = _abi.lib


def test_symbols_exist_and_the_abi_is_still_1():
    for name in ("syldet_recordings_load_sinc_device", "syldet_recordings_load_sinc_device_s16"):
        assert name in _abi.SIGNATURES and getattr(LIB, name) is not None
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    assert "int syldet_recordings_load_sinc_device(" in header and "int syldet_recordings_load_sinc_device_s16(" in header
    assert "#define SYLDET_ABI_VERSION 1" in header
    assert callable(sd.Recordings.loadSinc) and callable(sd.recordingLengths)


@pytest.mark.parametrize("name", ["syldet_recordings_load_sinc_device", "syldet_recordings_load_sinc_device_s16"])
def test_a_null_handle_is_refused_before_anything_else(name):
    fn = getattr(LIB, name)
    one = np.zeros(1, np.int64)
    rate = np.array([48000.0])
    step = np.ones(1, np.int32)
    args = (one.ctypes.data_as(_abi.c_int64_p), step.ctypes.data_as(_abi.c_int32_p), one.ctypes.data_as(_abi.c_int64_p),
            rate.ctypes.data_as(_abi.c_double_p))
    # whatever else is wrong or right with the call: no handle, no device, SYLDET_ERR_INVALID_ARGUMENT
    assert fn(None, None, None, None, None, None, 32, 12.0, 0.9, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    assert fn(None, 16, *args, 32, 12.0, 0.9, 16, 8, None) == _abi.ERR_INVALID_ARGUMENT
    assert fn(None, 16, *args, 3, 12.0, 0.9, 16, 8, None) == _abi.ERR_INVALID_ARGUMENT
    assert "NULL" in _abi.last_error()


RATES = [48000.0, 96000.0, 22050.0, 24414.0625, 44100.0, 44100.0 * 16, 44100.0 / 16, 8000.0, 192000.0]


def test_recording_lengths_equal_the_model():
    rng = np.random.default_rng(3)
    for rate in (44100.0, 48000.0, 24414.0625):
        n = [0, 1, 2, 37, 1024, 1025, 5000, 9001, 2 ** 31 + 5] + [int(v) for v in rng.integers(1, 10 ** 7, 40)]
        r = [RATES[i % len(RATES)] for i in range(len(n))]
        got = sd.recordingLengths(n, r, rate)
        assert got == [sinc_ref.count(a, b, rate) for a, b in zip(n, r)]
        assert got == [int(LIB.syldet_convert_rate_count(a, b, rate)) for a, b in zip(n, r)]
        assert all(isinstance(v, int) for v in got)
    # a recording at the network's rate keeps its length
    assert sd.recordingLengths([0, 1, 5000, 10 ** 9], [44100.0] * 4, 44100.0) == [0, 1, 5000, 10 ** 9]
    assert sd.recordingLengths([], [], 44100.0) == []
    with pytest.raises(ValueError):
        sd.recordingLengths([1, 2], [48000.0], 44100.0)


def test_run_recordings_argument_errors_need_no_device():
    det = sd.SyllableDetector.__new__(sd.SyllableDetector)    # (no device: these are refused before one is needed)
    det._h = None
    x = [np.zeros(100, np.float32)]
    with pytest.raises(ValueError, match="resample='sinc'"):
        det.runRecordings(x, rates=[48000.0])
    with pytest.raises(ValueError, match="resample='sinc'"):
        det.runRecordings(x, rates=[48000.0], resample="linear")
    with pytest.raises(ValueError, match="belong to rates"):
        det.runRecordings(x, resample="sinc")
    with pytest.raises(ValueError, match="belong to rates"):
        det.runRecordings(x, zeroCrossings=8)
    with pytest.raises(ValueError, match="one rate per array"):
        det.runRecordings(x, rates=[48000.0, 44100.0], resample="sinc")


def test_the_help_text_says_what_batch_does_with_other_rates():
    out = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert b"--resample sinc" in out and b"joins the bank" in out and b"converted as the rows load" in out
    assert b"counts with the bytes it has at its own rate" in out
