"""The command line tool's --resample sinc end to end on the GPU: a 4 s file at 48 kHz with planted syllables, once as float32
and once as 16-bit PCM, against the events the oracle finds in the rows convertRate(..., method="sinc") returns for the same
samples.  Sample numbers and timestamps exact, outputs to the 1e-5 bar (the checks of tests/test_cli_gpu.py).  Without the
option, and with --resample linear, the lines are the linear converter's, as before."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pyoracle as po
import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
EX_USAGE = 64


def cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)


def run(*args):
    r = cli(*args)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    cfg = util.sample_net()
    p = tmp_path_factory.mktemp("net") / "net.txt"
    p.write_text(cfg.toText())
    return cfg, str(p)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{kind: (path, the decoded samples [2, n] as the tool reads them: float32, or int16)}: two tracks at 48 kHz."""
    d = tmp_path_factory.mktemp("wav48")
    from scipy.signal import resample_poly
    # the syllables as a 48 kHz recorder would have taken them: made at the network's 44.1 kHz, brought to 48 kHz (160 / 147)
    x = np.stack([resample_poly(synth.syllable_channel(4 * 44100, util.template(), seed=41 + c).astype(np.float64), 160, 147).astype(np.float32)
                  for c in range(2)], axis=1)
    q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    out = {}
    for kind, stored in (("float32", x), ("pcm16", q)):
        p = str(d / (kind + ".wav"))
        wavutil.write_wav(p, stored, 48000, kind)
        out[kind] = (p, np.ascontiguousarray(stored.T))
    return out


def expected_events(cfg, x):
    """[(sample, seconds-string, outputs)] of one channel at the network's rate (tests/test_cli_gpu.py)."""
    o = util.oracle_for(cfg)
    _, _, o64 = o.run(x, po.F64, po.RULE_ANY)
    flags = (o64 >= np.asarray(cfg.thresholds)[None, :]).any(axis=1).astype(np.uint8)
    idx = o.detections(flags, 0.0)
    hop = cfg.windowLength - cfg.windowOverlap
    base = cfg.windowLength + hop * (cfg.timeRange - 1) + max(0, -cfg.windowOverlap)
    return [(int(i), repr(int(i) / cfg.samplingRate), o64[(int(i) - base) // hop]) for i in idx]


def check_lines(lines, want):
    assert len(lines) == len(want), (lines[:5], want[:5])
    for line, (ch, sample, secs, outs) in zip(lines, want):
        parts = line.split(",")
        assert int(parts[0]) == ch and int(parts[1]) == sample
        assert parts[2] == secs
        got = np.array([float(v) for v in parts[3:]])
        assert got.shape == outs.shape
        assert np.abs(got - outs).max() <= util.TOL * max(1.0, np.abs(outs).max())


def wanted(cfg, rows):
    """The lines of a file whose tracks the detector is fed as `rows` [C, S]; --chunk 0: channel by channel."""
    per = [expected_events(cfg, rows[c]) for c in range(rows.shape[0])]
    assert sum(len(e) for e in per) >= 4, "fixture should fire a few times"
    return [(c, s, t, o) for c in range(rows.shape[0]) for (s, t, o) in per[c]]


@pytest.mark.parametrize("kind", ["float32", "pcm16"])
@pytest.mark.parametrize("quality", [None, "8,6,0.8"])
def test_sinc_lines_are_the_converted_rows_events(net, files, kind, quality):
    """Each file against its own conversion: the float32 file through the fp32 converter, the 16-bit file through the int16
    one (whose rows are the bits of the fp32 converter on x / 32768)."""
    cfg, net_path = net
    path, samples = files[kind]
    q = dict(zip(("zeroCrossings", "beta", "rolloff"), (float(v) for v in quality.split(",")))) if quality else {}
    rows = sd.convertRate(torch.from_numpy(samples).cuda(), 48000.0, cfg.samplingRate, method="sinc", **q).cpu().numpy()
    args = ["-n", net_path, "-a", path, "--chunk", "0", "--resample", "sinc"] + (["--resample-quality", quality] if quality else [])
    check_lines(run(*args), wanted(cfg, rows))


def test_default_and_linear_are_todays_lines(net, files):
    cfg, net_path = net
    path, samples = files["float32"]
    rows = sd.convertRate(torch.from_numpy(samples).cuda(), 48000.0, cfg.samplingRate).cpu().numpy()
    want = wanted(cfg, rows)
    plain = run("-n", net_path, "-a", path, "--chunk", "0")
    check_lines(plain, want)
    assert run("-n", net_path, "-a", path, "--chunk", "0", "--resample", "linear") == plain
    sinc = run("-n", net_path, "-a", path, "--chunk", "0", "--resample", "sinc")
    assert sinc != plain, "the two converters should not print the same outputs"


def test_simulate_sees_the_converted_rows(net, files, tmp_path):
    """--simulate behind --resample sinc: a track of as many frames as the converter delivered, at the network's rate."""
    cfg, net_path = net
    path, samples = files["pcm16"]
    track = str(tmp_path / "track.wav")
    run("-n", net_path, "-a", path, "--resample", "sinc", "--simulate", track)
    r = cli("--probe", "-a", track)
    n_out = int((samples.shape[1] - 1) * cfg.samplingRate / 48000.0) + 1
    assert r.returncode == 0 and "2 channel(s)" in r.stdout and "%d frames" % n_out in r.stdout, r.stdout


def test_levels_and_ttl_see_the_converted_rows(net, files, tmp_path):
    """--levels and --ttl behind --resample sinc: the readings are those of the rows the converter delivered (their count,
    and the input RMS of every full reading from the rows themselves), the trigger track has their length, and the detection
    lines do not change."""
    cfg, net_path = net
    path, samples = files["float32"]
    rows = sd.convertRate(torch.from_numpy(samples).cuda(), 48000.0, cfg.samplingRate, method="sinc").cpu().numpy().astype(np.float64)
    S, L = rows.shape[1], 32
    P = int(0.1 * cfg.samplingRate / L)
    M = int(sd._abi.lib.syldet_levels_count(S, L, P))
    table, track = str(tmp_path / "levels.tsv"), str(tmp_path / "ttl.wav")
    plain = run("-n", net_path, "-a", path, "--resample", "sinc")
    assert run("-n", net_path, "-a", path, "--resample", "sinc", "--levels", table, "--ttl", track) == plain
    lines = [l.split("\t") for l in open(table).read().splitlines()]
    assert len(lines) == 2 * M and M == -(-S // (P * L))
    for m in range(S // (P * L)):                                # the full readings: the loudest buffer's RMS
        for c in range(2):
            t, secs, rms, _ = lines[2 * m + c]
            assert int(t) == c and float(secs) == pytest.approx((m + 1) * P * L / cfg.samplingRate, abs=1e-9)
            want = np.sqrt((rows[c, m * P * L:(m + 1) * P * L].reshape(P, L) ** 2).mean(axis=1).max())
            assert float(rms) == pytest.approx(want, rel=1e-5)
    r = cli("--probe", "-a", track)
    assert r.returncode == 0 and "2 channel(s)" in r.stdout and "%d frames" % S in r.stdout, r.stdout


@pytest.mark.parametrize("args", [["--resample", "cubic"], ["--resample"], ["--resample", "sinc", "--resample-quality", "32,12"],
                                  ["--resample", "sinc", "--resample-quality", "32,12,0.9,1"], ["--resample", "sinc", "--resample-quality", "x,12,0.9"],
                                  ["--resample", "sinc", "--resample-quality", "32,,0.9"], ["--resample", "sinc", "--resample-quality", "3,12,0.9"],
                                  ["--resample", "sinc", "--resample-quality", "32,21,0.9"], ["--resample", "sinc", "--resample-quality", "32,12,0"],
                                  ["--resample", "sinc", "--resample-quality", "32,12,1.5"], ["--resample", "sinc", "--resample-quality", "32,12,nan"],
                                  ["--resample-quality", "32,12,0.9"], ["--resample", "linear", "--resample-quality", "32,12,0.9"]])
def test_usage_errors(net, files, args):
    cfg, net_path = net
    r = cli("-n", net_path, "-a", files["float32"][0], *args)
    assert r.returncode == EX_USAGE and "Usage:" in r.stdout and "--resample" in r.stdout
