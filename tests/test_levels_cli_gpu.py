"""The command line tool's --levels on the GPU: the table it writes holds, for every reading and track, the time of the reading's
end, the input RMS and the output level of tests/levels_ref.py on the file's samples -- exact after the printer's round trip --
and its standard output is what it is without the option."""
import os
import subprocess

import numpy as np
import pytest

import levels_ref
import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def parse(path):
    rows = []
    for line in open(path).read().splitlines():
        track, t, rms, out = line.split("\t")
        rows.append((int(track), float(t), float(rms), None if out == "" else np.float32(out)))
    return rows


def expected(cfg, f, L, P):
    """f [C, S] float32 as the detector is fed -> the table's rows"""
    import torch
    C, S = f.shape
    with sd.SyllableDetector(cfg, channels=C) as det:
        out, _ = det.run(torch.from_numpy(np.ascontiguousarray(f)).cuda())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    clock = (cfg.windowLength, cfg.windowOverlap, cfg.timeRange)
    rms = [np.sqrt(levels_ref.input_readings(f[c], L, P)) for c in range(C)]
    lv = [levels_ref.output_readings(out[c], 0, S, L, P, clock) for c in range(C)]
    rows = []
    for m in range(levels_ref.levels_count(S, L, P)):
        for c in range(C):
            rows.append((c, min((m + 1) * P * L, S) / cfg.samplingRate, float(rms[c][m]), None if lv[c][1][m] else lv[c][0][m]))
    return rows


def same(got, want):
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g[:3] == w[:3], (g, w)                                   # the shortest digits that round-trip: exact
        assert (g[3] is None) == (w[3] is None), (g, w)
        if g[3] is not None:
            assert np.float32(g[3]).view(np.uint32) == np.float32(w[3]).view(np.uint32), (g, w)


def test_levels_of_a_two_track_pcm16_file(tmp_path):
    cfg = util.sample_net()
    net = tmp_path / "net.txt"
    net.write_text(cfg.toText())
    n = FS
    q = np.stack([np.clip(np.round(synth.syllable_channel(n, util.template(), seed=21 + c) * (32768.0 if c == 0 else 9000.0)), -32768, 32767).astype(np.int16)
                  for c in range(2)], axis=1)
    a, out = str(tmp_path / "stereo.wav"), str(tmp_path / "levels.tsv")
    wavutil.write_wav(a, q, FS, "pcm16")
    plain = run("-n", str(net), "-a", a)
    with_levels = run("-n", str(net), "-a", a, "--levels", out, "--levels-buffer", "32", "--format", "shortest")
    assert with_levels == plain and len(plain.splitlines()) >= 1       # the detection lines, byte for byte
    f = wavutil.to_float(q, "pcm16").T
    P = max(1, int(0.1 * FS / 32))
    got = parse(out)
    same(got, expected(cfg, f, 32, P))
    assert len(got) == 2 * levels_ref.levels_count(n, 32, P) and got[-1][1] == n / FS
    assert all(r[3] is not None for r in got)                           # (every 0.1 s of this file holds evaluations)
    # another buffer and period
    out2 = str(tmp_path / "levels2.tsv")
    assert run("-n", str(net), "-a", a, "--levels", out2, "--levels-buffer", "256", "--levels-period", "0.25") == plain
    same(parse(out2), expected(cfg, f, 256, int(0.25 * FS / 256)))


def test_levels_of_a_file_shorter_than_one_evaluation(tmp_path):
    cfg = util.sample_net()
    net = tmp_path / "net.txt"
    net.write_text(cfg.toText())
    q = (np.arange(700 * 1).reshape(700, 1) * 37 % 2000 - 1000).astype(np.int16)
    a, out = str(tmp_path / "short.wav"), str(tmp_path / "levels.tsv")
    wavutil.write_wav(a, q, FS, "pcm16")
    assert run("-n", str(net), "-a", a, "--levels", out, "--levels-period", "0.005") == b""
    got = parse(out)
    P = int(0.005 * FS / 32)
    f = wavutil.to_float(q, "pcm16").T
    want = np.sqrt(levels_ref.input_readings(f[0], 32, P))
    assert [r[2] for r in got] == [float(v) for v in want] and all(r[3] is None for r in got) and len(got) == levels_ref.levels_count(700, 32, P)
