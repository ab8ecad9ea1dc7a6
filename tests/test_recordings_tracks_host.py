"""Packed recordings' per-sample tracks without a GPU: the new entry points are bound; Recordings.trackLayout's arithmetic; the
numpy model (recordings_tracks_ref.py) against the reference's own loops -- the Simulator's buffer loop and the rig's callback
loop -- on every recording of a packed plan; the command line tool's usage errors for the three -dir options."""
import os
import subprocess

import numpy as np
import pytest

import recordings_ref as ref
import recordings_tracks_ref as tref
import trace_ref
import trigger_ref
import util
from syllable_detector_swift_amd import _abi
from syllable_detector_swift_amd.detector import Recordings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")


def test_the_entry_points_are_bound():
    for name in ("syldet_recordings_trace_device", "syldet_recordings_trace_device_s16", "syldet_recordings_trigger_device",
                 "syldet_recordings_trigger_device_s16", "syldet_recordings_trigger_onsets_device"):
        assert name in _abi.SIGNATURES and getattr(_abi.lib, name).argtypes == _abi.SIGNATURES[name][1]
    # NULL handles are refused before any device is touched
    z = np.zeros(1, np.int64).ctypes.data_as(_abi.c_int64_p)
    assert _abi.lib.syldet_recordings_trace_device_s16(None, None, 0, None, 0, z, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_recordings_trigger_device(None, None, 32, 44, 0, None, 0, z, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_recordings_trigger_onsets_device(None, None, 32, 44, 0, None, 0, None, None) == _abi.ERR_INVALID_ARGUMENT
    for method in ("trackLayout", "trace", "triggerTrack", "triggerOnsets", "trackView"):
        assert callable(getattr(Recordings, method))


def _plan(lengths, C=3):
    cfg = util.sample_net()
    hop, need, T, D = ref.clock(cfg)
    slots, row_samples, row_evals, _ = ref.plan(lengths, hop, need, T, C)
    return cfg, slots, row_evals, hop, D


def _recordings(slots):
    """a Recordings without a device: the layout's arithmetic needs the slots alone"""
    rec = Recordings.__new__(Recordings)
    rec._h = None
    rec.count, rec.slots = len(slots), slots
    return rec


def test_track_layout_arithmetic():
    lengths = [0, 5, 8, 9, 1444, 0, 16, 3]
    _, slots, _, _, _ = _plan(lengths)
    rec = _recordings(slots)
    off, total = rec.trackLayout()
    assert list(off) == [0, 0, 8, 16, 32, 1480, 1480, 1496] and total == 1499          # each from a multiple of 8; none takes nothing
    off1, total1 = rec.trackLayout(align=1)
    assert list(off1) == list(np.cumsum([0] + lengths)[:-1]) and total1 == sum(lengths)
    steps = [2, 2, 3, 1, 2, 2, 1, 4]
    off2, total2 = rec.trackLayout(steps, align=4)
    want, end = tref.layout(slots, steps, 4)
    assert np.array_equal(off2, want) and total2 == end
    assert off2[2] == 12 and off2[3] == 12 + (8 - 1) * 3 + 1 + 2                       # 5 samples at step 2: 9 elements from 0 -> 12; ... 34 -> 36
    for k, (n, s) in enumerate(zip(lengths, steps)):
        view = rec.trackView(np.arange(total2), k, off2, steps)
        assert view.size == n and (n == 0 or (view[0] == off2[k] and view[-1] == off2[k] + (n - 1) * s))
    with pytest.raises(ValueError):
        rec.trackLayout(align=0)
    with pytest.raises(ValueError):
        rec.trackLayout([1] * 7)
    with pytest.raises(ValueError):
        rec.trackLayout([1] * 7 + [0])


LENGTHS = [0, 1439, 1443, 1444, 5280, 7777, 1575, 12001, 333]


def test_the_model_is_the_simulators_loop_on_every_recording():
    cfg, slots, row_evals, hop, D = _plan(LENGTHS)
    W, ov, T = cfg.windowLength, cfg.windowOverlap, cfg.timeRange
    rng = np.random.default_rng(3)
    outputs = (rng.random((3, row_evals, 1)) * 1.6 - 0.3).astype(np.float32)            # junk evaluations between the recordings included
    thr = [[0.71], [0.5], [0.9]]                                                          # a threshold a row
    steps = [1 + k % 3 for k in range(len(slots))]
    offsets, total = tref.layout(slots, steps, 8)
    for s16 in (False, True):
        dst, owned = tref.scatter(np.full(total, -7, np.int16 if s16 else np.float32), tref.trace_each(slots, outputs, thr, D, hop, 0, s16), offsets, steps)
        assert owned.sum() == sum(LENGTHS) and (dst[~owned] == -7).all()
        for k, s in enumerate(slots):
            row, _, first, n_evals, n = s
            assert n_evals == trace_ref.count_evals(n, W, ov, T)
            v = trace_ref.values(outputs[row, first:first + n_evals], thr[row])
            loop = trace_ref.simulator_loop(v, W, ov, T, n, rng)
            loop[np.isnan(loop)] = 0                                                      # (behind the last hold: the closed form's zeros)
            got = dst[offsets[k]:offsets[k] + (n - 1) * steps[k] + 1:steps[k]] if n else dst[:0]
            assert np.array_equal(got, trace_ref.to_s16(loop) if s16 else loop), "recording %d" % k


def test_the_model_is_the_rigs_loop_on_every_recording():
    cfg, slots, row_evals, hop, D = _plan(LENGTHS)
    W, ov, T = cfg.windowLength, cfg.windowOverlap, cfg.timeRange
    rng = np.random.default_rng(4)
    flags = (rng.random((3, row_evals)) < 0.2).astype(np.uint8)
    for row, _, first, n_evals, _ in slots:                                              # a flag in every recording's last evaluation
        if n_evals:
            flags[row, first + n_evals - 1] = 1
    offsets, total = tref.layout(slots)
    for L, N, lat in [(8, 1, 0), (32, 44, 0), (32, 32, 221), (4096, 44, 0), (8, 20000, 2000)]:
        dst, owned = tref.scatter(np.full(total, -7, np.int16), tref.trigger_each(slots, flags, D, hop, L, N, lat, True), offsets)
        assert (dst[~owned] == -7).all()
        edges = tref.onsets_each(slots, flags, D, hop, L, N, lat)
        for k, (row, _, first, n_evals, n) in enumerate(slots):
            loop = trigger_ref.rig_loop(flags[row, first:first + n_evals], W, ov, T, L, N, lat, n)
            got = dst[offsets[k]:offsets[k] + n]
            assert np.array_equal(got, trigger_ref.as_s16(loop)), "recording %d, L %d N %d latency %d" % (k, L, N, lat)
            assert np.array_equal(edges[k], trigger_ref.rising_edges(loop))


@pytest.mark.parametrize("args,needle", [
    (["-a", "x/a.wav", "-a", "y/a.wav", "--simulate-dir", "d"], b"a.wav"),
    (["-a", "x/a.wav", "-a", "y/a.wav", "--batch", "--ttl-onsets-dir", "d"], b"a.wav"),
    (["-a", "a.wav", "--simulate", "s.wav", "--simulate-dir", "d"], b"--simulate-dir"),
    (["-a", "a.wav", "--ttl", "s.wav", "--ttl-dir", "d"], b"--ttl-dir"),
    (["-a", "a.wav", "--ttl-onsets", "s.tsv", "--ttl-onsets-dir", "d"], b"--ttl-onsets-dir"),
    (["-a", "a.wav", "-a", "b.wav", "--batch", "--ttl-dir", "d", "--ttl-mux"], b"--ttl-mux"),
    (["-a", "a.wav", "--batch", "--levels", "l.tsv"], b"--levels"),
    (["-a", "a.wav", "--batch", "--simulate", "s.wav"], b"--simulate-dir"),
    (["-a", "a.wav", "--simulate-dir"], b"Missing value"),
])
def test_the_tools_usage_errors(args, needle, tmp_path):
    """refused as usage errors, 64, before any file is read (none of these files exists) or any directory made"""
    r = subprocess.run([CLI, "-n", "net.txt", *args], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 64 and needle in r.stderr and r.stdout.startswith(b"Usage:"), (args, r.stderr)
    assert os.listdir(str(tmp_path)) == []


def test_the_help_names_the_options():
    text = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    for word in (b"--simulate-dir <dir>", b"--ttl-dir <dir>", b"--ttl-onsets-dir <dir>", b"2 bytes per sample"):
        assert word in text
