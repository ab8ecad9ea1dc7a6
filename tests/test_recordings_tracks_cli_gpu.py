"""The command line tool's --simulate-dir, --ttl-dir and --ttl-onsets-dir on the GPU: under --batch (the tracks made by the packed
bank's calls, one download a product), under --batch with two rows, and without --batch, every file written equals, byte for
byte, the file --simulate, --ttl and --ttl-onsets write for that input alone; standard output and the exit status are those of
the same command without the three options."""
import os
import subprocess

import numpy as np
import pytest

import util
import wavutil
from syllable_detector_swift_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, timeout=600)


def _pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    """five small WAVs and, for each, what the single-file options write for it alone"""
    d = tmp_path_factory.mktemp("archive")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    tmpl = util.template()

    def sound(n, seed, fs=FS):
        return synth.syllable_channel(n, tmpl, seed=seed, every=int(0.25 * fs))

    files = {
        "mono16.wav": (_pcm(sound(30011, 1))[:, None], FS, "pcm16"),
        "stereo16.wav": (_pcm(np.stack([sound(22222, 2), sound(22222, 3)], axis=1)), FS, "pcm16"),
        "monofloat.wav": (sound(14001, 4)[:, None].astype(np.float32), FS, "float32"),
        "mono48k.wav": (_pcm(sound(40000, 5, 48000))[:, None], 48000, "pcm16"),
        "short.wav": (_pcm(sound(1000, 6))[:, None], FS, "pcm16"),
    }
    paths = []
    for name, (frames, rate, kind) in files.items():
        wavutil.write_wav(str(d / name), frames, rate, kind)
        paths.append(str(d / name))
    alone = d / "alone"
    alone.mkdir()
    want = {}
    for p in paths:
        base = os.path.basename(p)
        out = [str(alone / (base + ".sim")), str(alone / (base + ".ttl")), str(alone / (base + ".tsv"))]
        r = _run("-n", str(net), "-a", p, "--resample", "sinc", "--simulate", out[0], "--ttl", out[1], "--ttl-onsets", out[2])
        assert r.returncode == 0, r.stderr.decode()
        want[base] = [open(o, "rb").read() for o in out]
    assert sum(len(w[2]) > 0 for w in want.values()) >= 3                 # onsets in most files: the tracks are not all zeros
    return str(net), paths, want, d


@pytest.mark.parametrize("mode", [["--batch"], ["--batch", "--batch-rows", "2"], []])
def test_every_file_is_what_the_single_file_options_write(archive, mode, tmp_path):
    net, paths, want, _ = archive
    audio = [a for p in paths for a in ("-a", p)]
    A, B, T = str(tmp_path / "sim"), str(tmp_path / "made" / "ttl"), str(tmp_path / "onsets")   # (none exists; one is two levels deep)
    plain = _run("-n", net, *audio, "--resample", "sinc", *mode)
    got = _run("-n", net, *audio, "--resample", "sinc", *mode, "--simulate-dir", A, "--ttl-dir", B, "--ttl-onsets-dir", T)
    assert plain.returncode == 0, plain.stderr.decode()
    assert got.returncode == plain.returncode and got.stdout == plain.stdout, got.stderr.decode()
    assert len(plain.stdout.splitlines()) > len(paths)                    # the names and some detection lines
    for base, (sim, ttl, onsets) in want.items():
        assert open(os.path.join(A, base), "rb").read() == sim, base
        assert open(os.path.join(B, base), "rb").read() == ttl, base
        assert open(os.path.join(T, base + ".tsv"), "rb").read() == onsets, base
    assert sorted(os.listdir(A)) == sorted(want) and sorted(os.listdir(B)) == sorted(want)


def test_a_track_that_cannot_be_written_costs_one_and_no_line(archive, tmp_path):
    net, paths, _, _ = archive
    audio = [a for p in paths[:2] for a in ("-a", p)]
    blocked = tmp_path / "blocked"
    blocked.write_text("a file where the directory should be")
    plain = _run("-n", net, *audio, "--batch")
    got = _run("-n", net, *audio, "--batch", "--simulate-dir", str(blocked))
    assert plain.returncode == 0 and got.returncode == 1 and got.stdout == plain.stdout
    assert b"Unable to write" in got.stderr
