"""Packed recordings' level meters without a GPU: the new entry points are bound and refuse NULL before any device is touched;
Recordings.levelsLayout's arithmetic against syldet_levels_count recording by recording; the numpy model
(recordings_levels_ref.py) against the application's literal loop (levels_ref.replay) on every recording of a packed plan; the
header still compiles as C; the command line tool's usage errors for --levels-dir."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import levels_ref
import recordings_levels_ref as lref
import recordings_ref as ref
import util
from syllable_detector_swift_amd import _abi
from syllable_detector_swift_amd.detector import Recordings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "syllable_detector_swift_amd", "lib")
CLI = os.path.join(LIB, "syllable-detector-cli")


def test_the_entry_points_are_bound_and_refuse_null():
    for name in ("syldet_recordings_levels_layout", "syldet_recordings_levels_device", "syldet_recordings_levels_device_s16",
                 "syldet_recordings_output_levels_device"):
        assert name in _abi.SIGNATURES and getattr(_abi.lib, name).argtypes == _abi.SIGNATURES[name][1]
        assert getattr(_abi.lib, name).restype == ctypes.c_int
    args = _abi.SIGNATURES["syldet_recordings_levels_device"][1]
    assert args == _abi.SIGNATURES["syldet_recordings_levels_device_s16"][1]
    assert [args[i] for i in (2, 3, 4, 6)] == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]     # stride, L, P, capacity
    out_args = _abi.SIGNATURES["syldet_recordings_output_levels_device"][1]
    assert [out_args[i] for i in (2, 3, 4, 6)] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]  # output, L, P, capacity
    lay = _abi.SIGNATURES["syldet_recordings_levels_layout"][1]
    assert lay[1:] == [ctypes.c_int32, ctypes.c_int64, _abi.c_int64_p, _abi.c_int64_p]
    # the refusals of the layout call that need no handle, and a NULL handle everywhere: before any device is touched
    n = ctypes.c_int64(-7)
    first = np.full(3, -7, np.int64)
    assert _abi.lib.syldet_recordings_levels_layout(None, 32, 3, first.ctypes.data_as(_abi.c_int64_p), ctypes.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert n.value == -7 and (first == -7).all()
    assert _abi.lib.syldet_recordings_levels_device(None, None, 0, 32, 3, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_recordings_levels_device_s16(None, None, 0, 32, 3, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_recordings_output_levels_device(None, None, 0, 32, 3, None, 0, None) == _abi.ERR_INVALID_ARGUMENT
    for method in ("levelsLayout", "levels", "outputLevels", "levelsView"):
        assert callable(getattr(Recordings, method))


def _plan(lengths, C=3):
    cfg = util.sample_net()
    hop, need, T, D = ref.clock(cfg)
    slots, row_samples, row_evals, _ = ref.plan(lengths, hop, need, T, C)
    return cfg, slots, row_samples, row_evals


def _recordings(slots):
    """a Recordings without a device: the layout's arithmetic needs the slots alone"""
    rec = Recordings.__new__(Recordings)
    rec._h = None
    rec.count, rec.slots = len(slots), slots
    return rec


@pytest.mark.parametrize("L", [8, 32, 4096])
def test_the_layout_is_levels_count_of_every_recording(L):
    lengths = [0, 1, L - 1, L, L + 1, 0, 7, 3 * L, 3 * L + 1, 10 * L + 5, 100000]
    _, slots, _, _ = _plan(lengths)
    rec = _recordings(slots)
    for P in (1, 3, 16, 10 ** 9):                                            # the last: greater than every recording's buffer count
        first = rec.levelsLayout(L, P)
        assert first.dtype == np.int64 and first.shape == (len(lengths) + 1,) and first[0] == 0
        counts = [int(_abi.lib.syldet_levels_count(n, L, P)) for n in lengths]
        assert list(np.diff(first)) == counts and np.array_equal(first, lref.layout(slots, L, P))
        assert counts[0] == counts[5] == 0 and counts[1] == counts[2] == counts[3] == 1          # none without samples; one buffer: one reading
        assert counts[4] == (2 if P == 1 else 1)
        if P == 10 ** 9:
            assert counts == [int(n > 0) for n in lengths]
        table = np.arange(int(first[-1]))
        for k in range(len(lengths)):
            view = rec.levelsView(table, k, L, P)
            assert view.size == counts[k] and (view.size == 0 or view[0] == first[k])
    for bad in ((12, 3), (4, 3), (8192, 3), (32, 0), (32, -1)):
        with pytest.raises(ValueError):
            rec.levelsLayout(*bad)


def test_the_model_is_the_applications_loop_on_every_recording():
    lengths = [0, 1, 31, 32, 33, 7, 131, 1444, 5280, 7777, 12001]
    cfg, slots, row_samples, row_evals = _plan(lengths)
    clock = (cfg.windowLength, cfg.windowOverlap, cfg.timeRange)
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((3, row_samples)).astype(np.float32)          # the pads and the tails hold junk: the model never reads them
    outputs = (rng.random((3, row_evals, 1)) * 1.6 - 0.3).astype(np.float32)
    for L, P in ((8, 1), (32, 3), (32, 137), (4096, 2), (32, 10 ** 9)):
        first = lref.layout(slots, L, P)
        got_in = lref.input_each(slots, rows, L, P)
        got_out = lref.output_each(slots, outputs, 0, L, P, clock)
        assert got_in.size == got_out.size == first[-1]
        for k, (row, offset, first_eval, n_evals, n) in enumerate(slots):
            assert n_evals == levels_ref.count_evals(n, *clock)
            own = outputs[row, first_eval:first_eval + n_evals]
            read_in, read_out = levels_ref.replay(rows[row, offset:offset + n], L, min(P, max(1, -(-n // L))), clock, own)
            assert len(read_in) == first[k + 1] - first[k]
            assert np.array_equal(got_in[first[k]:first[k + 1]], np.asarray(read_in, np.float64))
            want = np.asarray([0.0 if v is None else v for v in read_out], np.float32)
            assert np.array_equal(got_out[first[k]:first[k + 1]], want), (L, P, k)
    # 16-bit rows mean x / 32768
    q = (rng.standard_normal((3, row_samples)) * 9000).clip(-32768, 32767).astype(np.int16)
    assert np.array_equal(lref.input_each(slots, q, 32, 3), lref.input_each(slots, q.astype(np.float32) / np.float32(32768), 32, 3))


def test_the_header_still_compiles_as_c(tmp_path):
    c = tmp_path / "recordings_levels.c"
    c.write_text('#include "syldet.h"\n'
                 "int main(void) {\n"
                 "    float x[8] = {0}, lv[2]; int16_t q[8] = {0}; double ms[2]; int64_t first[2], n = -1;\n"
                 "    int st = syldet_recordings_levels_layout(NULL, 32, 3, first, &n) + syldet_recordings_levels_device(NULL, x, 8, 32, 3, ms, 2, NULL) +\n"
                 "             syldet_recordings_levels_device_s16(NULL, q, 8, 32, 3, ms, 2, NULL) +\n"
                 "             syldet_recordings_output_levels_device(NULL, x, 0, 32, 3, lv, 2, NULL);\n"
                 "    return st == 4 * SYLDET_ERR_INVALID_ARGUMENT && n == -1 ? 0 : 1;\n"
                 "}\n")
    exe = tmp_path / "recordings_levels"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(c),
                    "-o", str(exe), "-L" + LIB, "-lsyldet", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("args,needle", [
    (["-a", "x/a.wav", "-a", "y/a.wav", "--levels-dir", "d"], b"a.wav"),                       # two files, one name
    (["-a", "x/a.wav", "-a", "y/a.wav", "--batch", "--levels-dir", "d"], b"a.wav"),
    (["-a", "a.wav", "--levels", "l.tsv", "--levels-dir", "d"], b"--levels-dir"),
    (["-a", "a.wav", "--levels-dir"], b"Missing value"),
    (["-a", "a.wav", "--levels-dir", "d", "--levels-buffer", "12"], b"power of two"),
    (["-a", "a.wav", "--levels-dir", "d", "--levels-period", "0"], b"--levels-period"),
    (["-a", "a.wav", "--batch", "--levels", "l.tsv"], b"--levels"),                            # the one-file option stays refused under --batch
])
def test_the_tools_usage_errors(args, needle, tmp_path):
    """refused as usage errors, 64, before any file is read (none of these files exists) or any directory made"""
    r = subprocess.run([CLI, "-n", "net.txt", *args], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 64 and needle in r.stderr and r.stdout.startswith(b"Usage:"), (args, r.stderr)
    assert os.listdir(str(tmp_path)) == []


def test_the_help_names_the_option():
    text = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert b"--levels-dir <dir>" in text
