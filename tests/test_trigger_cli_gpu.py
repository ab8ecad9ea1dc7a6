"""The command line tool's --ttl, --ttl-mux and --ttl-onsets on the GPU: the 16-bit WAV holds the trigger tracks the Python path
gives for the audio the detector was fed (with --ttl-mux beside the audio itself), the table holds their rising edges, and the
tool's standard output is what it is without the options."""
import os
import subprocess
import wave

import numpy as np
import pytest

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


def read_wav(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2                                   # 16 bit
        n, ch = w.getnframes(), w.getnchannels()
        return np.frombuffer(w.readframes(n), "<i2").reshape(n, ch), w.getframerate()


def read_tsv(path):
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert all(len(r) == 3 for r in rows)
    return [(int(c), int(s), t) for c, s, t in rows]


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """a two-track 16-bit file with planted syllables, the network, and the tool's plain output"""
    d = tmp_path_factory.mktemp("ttl")
    cfg = util.sample_net()
    net = d / "net.txt"
    net.write_text(cfg.toText())
    n = 2 * FS + 17
    q = np.stack([np.clip(np.round(synth.syllable_channel(n, util.template(), seed=21 + c) * 32768.0), -32768, 32767).astype(np.int16)
                  for c in range(2)], axis=1)
    a = str(d / "stereo.wav")
    wavutil.write_wav(a, q, FS, "pcm16")
    return cfg, str(net), a, q, run("-n", str(net), "-a", a)


def python_path(cfg, q, L, N, lat):
    """-> (frames [S, C], mux [S, 2 C], onsets per channel) from the library's Python methods on the int16 rows"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(q.T)).cuda()
    with sd.SyllableDetector(cfg, channels=q.shape[1]) as det:
        _, fl = det.runPCM16(x)
        frames = det.triggerTrackInterleavedPCM16(fl, q.shape[0], L, N, lat)
        mux = det.triggerMuxPCM16(fl, x, L, N, lat)
        idx, cnt = det.triggerOnsets(fl, q.shape[0], L, N, lat)
        torch.cuda.synchronize()
        assert int(fl.sum()) > 0
        return frames.cpu().numpy(), mux.cpu().numpy(), [idx[c, :int(cnt[c])].cpu().numpy() for c in range(q.shape[1])]


def test_ttl_and_onsets_with_the_defaults(tmp_path, recording):
    cfg, net, a, q, plain = recording
    out, tsv = str(tmp_path / "ttl.wav"), str(tmp_path / "on.tsv")
    assert run("-n", net, "-a", a, "--ttl", out, "--ttl-onsets", tsv) == plain and len(plain.splitlines()) >= 2
    frames, rate = read_wav(out)
    want, _, onsets = python_path(cfg, q, 32, 44, 0)                   # 1 ms at 44100 Hz, buffers of 32, no latency
    assert rate == FS and frames.shape == (len(q), 2)
    assert np.array_equal(frames, want) and frames.max() == 32767 and set(np.unique(frames)) == {0, 32767}
    rows = read_tsv(tsv)
    assert [(c, s) for c, s, _ in rows] == [(c, int(s)) for c in range(2) for s in onsets[c]] and len(rows) >= 2
    for _, s, t in rows:
        assert float(t) == s / FS                                      # the seconds are sample / rate


def test_ttl_mux_with_every_option(tmp_path, recording):
    cfg, net, a, q, plain = recording
    out, tsv = str(tmp_path / "mux.wav"), str(tmp_path / "on.tsv")
    got = run("-n", net, "-a", a, "--ttl", out, "--ttl-mux", "--ttl-steps", "20", "--ttl-buffer", "64", "--ttl-latency", "0.005", "--ttl-onsets", tsv)
    assert got == plain
    frames, rate = read_wav(out)
    _, want, onsets = python_path(cfg, q, 64, 20 * 64, int(0.005 * FS))
    assert rate == FS and frames.shape == (len(q), 4)                  # audio and trigger alternating
    assert np.array_equal(frames[:, 0::2], q) and np.array_equal(frames, want)
    assert [(c, s) for c, s, _ in read_tsv(tsv)] == [(c, int(s)) for c in range(2) for s in onsets[c]]
    # --ttl-width in seconds
    out2 = str(tmp_path / "w.wav")
    run("-n", net, "-a", a, "--ttl", out2, "--ttl-width", "0.01")
    assert np.array_equal(read_wav(out2)[0], python_path(cfg, q, 32, 441, 0)[0])


def test_ttl_mux_refuses_a_float_file_and_a_short_file_gives_zeros(tmp_path, recording):
    cfg, net, _, q, _ = recording
    a = str(tmp_path / "f.wav")
    wavutil.write_wav(a, wavutil.to_float(q[:5000], "pcm16").astype(np.float32), FS, "float32")
    out = str(tmp_path / "no.wav")
    r = subprocess.run([CLI, "-n", net, "-a", a, "--ttl", out, "--ttl-mux"], capture_output=True, timeout=600)
    assert r.returncode == 1 and b"--ttl-mux takes 16-bit PCM" in r.stderr and not os.path.exists(out)
    short = str(tmp_path / "short.wav")
    wavutil.write_wav(short, q[:1000], FS, "pcm16")                    # shorter than one evaluation
    tsv = str(tmp_path / "none.tsv")
    run("-n", net, "-a", short, "--ttl", out, "--ttl-mux", "--ttl-onsets", tsv)
    frames, _ = read_wav(out)
    assert frames.shape == (1000, 4) and np.array_equal(frames[:, 0::2], q[:1000]) and not frames[:, 1::2].any()
    assert open(tsv).read() == ""
