"""The command line tool's --simulate on the GPU: the 16-bit WAV it writes holds the Simulator's output track of every track of
the file (ViewControllerSimulator.swift:251-344) -- the frames simulate() gives on the audio the detector was fed, as many of them
-- and its standard output is what it is without the option."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def read_wav(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2
        n, ch = w.getnframes(), w.getnchannels()
        return np.frombuffer(w.readframes(n), "<i2").reshape(n, ch), w.getframerate()


def write_net(tmp_path, cfg, name="net.txt"):
    p = tmp_path / name
    p.write_text(cfg.toText())
    return str(p)


def simulate_frames(cfg, x, output=0):
    """x [C, S] float32 as the detector is fed -> simulate()'s track as frames [S, C] int16"""
    import torch
    with sd.SyllableDetector(cfg, channels=x.shape[0]) as det:
        tr, _, _ = det.simulate(torch.from_numpy(np.ascontiguousarray(x)).cuda(), output=output)
        torch.cuda.synchronize()
        return tr.cpu().numpy().T


def test_simulate_on_a_two_track_pcm16_file(tmp_path):
    cfg = util.sample_net()
    net = write_net(tmp_path, cfg)
    n = 3 * FS + 17
    q = np.stack([np.clip(np.round(synth.syllable_channel(n, util.template(), seed=21 + c) * 32768.0), -32768, 32767).astype(np.int16)
                  for c in range(2)], axis=1)
    a, out = str(tmp_path / "stereo.wav"), str(tmp_path / "sim.wav")
    wavutil.write_wav(a, q, FS, "pcm16")
    plain = run("-n", net, "-a", a)
    with_track = run("-n", net, "-a", a, "--simulate", out)
    assert with_track == plain and len(plain.splitlines()) >= 2       # the detection lines, byte for byte
    frames, rate = read_wav(out)
    assert rate == FS and frames.shape == (n, 2)
    want = simulate_frames(cfg, wavutil.to_float(q, "pcm16").T)
    assert np.array_equal(frames, want)
    assert frames.max() == 32767 and not frames[:cfg.geometry().first_index].any()


def test_simulate_on_a_float_file_at_another_rate(tmp_path):
    import torch
    cfg = util.sample_net()
    net = write_net(tmp_path, cfg)
    x48 = np.stack([synth.syllable_channel(2 * 48000 + 5, util.template(), seed=41 + c, every=24000).astype(np.float32) for c in range(2)], axis=1)
    a, out = str(tmp_path / "r48.wav"), str(tmp_path / "sim.wav")
    wavutil.write_wav(a, x48, 48000, "float32")
    plain = run("-n", net, "-a", a)
    assert run("-n", net, "-a", a, "--simulate", out) == plain
    # the audio the detector was fed: the library's own rate conversion of the decoded tracks
    n = x48.shape[0]
    m = int(_abi.lib.syldet_convert_rate_count(n, 48000.0, cfg.samplingRate))
    d_in = torch.from_numpy(np.ascontiguousarray(x48.T)).cuda()
    d_out = torch.empty((2, m), dtype=torch.float32, device="cuda")
    got = C.c_int64(0)
    st = _abi.lib.syldet_convert_rate_device(d_in.data_ptr(), n, n, 2, 48000.0, cfg.samplingRate, d_out.data_ptr(), m, C.byref(got),
                                             int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0 and got.value == m
    frames, rate = read_wav(out)
    assert rate == int(cfg.samplingRate) and frames.shape == (m, 2)    # as many frames as the detector was fed
    assert np.array_equal(frames, simulate_frames(cfg, d_out.cpu().numpy()))
    assert frames.max() > 0


def test_simulate_output_picks_the_output(tmp_path):
    base = util.sample_net()
    cfg = nets.variant(base, thresholds=[0.3, 0.2])
    cfg.net = nets.random_net(np.random.default_rng(8), base.geometry().bins * base.timeRange, (4,), 2)
    net = write_net(tmp_path, cfg)
    cfg = sd.SyllableDetectorConfig.fromTextFile(net)                 # (the values the tool reads)
    n = FS
    q = np.clip(np.round(synth.syllable_channel(n, util.template(), seed=5) * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    a = str(tmp_path / "mono.wav")
    wavutil.write_wav(a, q, FS, "pcm16")
    tracks = []
    for k in (0, 1):
        out = str(tmp_path / ("sim%d.wav" % k))
        run("-n", net, "-a", a, "--simulate", out, "--simulate-output", str(k))
        frames, _ = read_wav(out)
        assert np.array_equal(frames, simulate_frames(cfg, wavutil.to_float(q, "pcm16").T, output=k)), k
        tracks.append(frames)
    assert not np.array_equal(tracks[0], tracks[1])
    r = subprocess.run([CLI, "-n", net, "-a", a, "--simulate", str(tmp_path / "no.wav"), "--simulate-output", "2"], capture_output=True)
    assert r.returncode == 64 and not os.path.exists(str(tmp_path / "no.wav"))


def test_a_track_that_cannot_be_written_does_not_cost_the_detection_lines(tmp_path):
    cfg = util.sample_net()
    net = write_net(tmp_path, cfg)
    n = 2 * FS
    q = np.clip(np.round(synth.syllable_channel(n, util.template(), seed=21) * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    a = str(tmp_path / "mono.wav")
    wavutil.write_wav(a, q, FS, "pcm16")
    plain = run("-n", net, "-a", a)
    r = subprocess.run([CLI, "-n", net, "-a", a, "--simulate", str(tmp_path / "no_such_directory" / "sim.wav")], capture_output=True, timeout=600)
    assert r.returncode == 1 and b"Unable to write" in r.stderr
    assert r.stdout == plain and len(plain.splitlines()) >= 1
