"""The command line tool's --batch on the GPU: standard output and the exit status are byte for byte those of the same command
without it -- the file-name lines, the order of the files, the tracks' events interleaved by --chunk -- for files of one and two
tracks, 16-bit and float32, one shorter than a window, one at another rate (processed alone in its place) and one that cannot
be read."""
import os
import subprocess

import numpy as np
import pytest

import util
import wavutil
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """six small WAVs with planted syllables (0.1 to 1.5 s, and one shorter than a window), and two networks"""
    d = tmp_path_factory.mktemp("batch")
    cfg = util.sample_net()
    net0, net1 = d / "net0.txt", d / "net1.txt"
    net0.write_text(cfg.toText())
    net1.write_text(nets.perturbed(cfg, 1).toText())
    tmpl = util.template()

    def track(n, seed, fs_scale=1.0):
        return synth.syllable_channel(n, tmpl, seed=seed, every=6000)

    paths = {}
    def put(name, frames, rate, kind):
        paths[name] = str(d / (name + ".wav"))
        wavutil.write_wav(paths[name], frames, rate, kind)

    put("mono16", _pcm(track(int(1.5 * FS), 1))[:, None], FS, "pcm16")
    put("stereo16", np.stack([_pcm(track(int(0.8 * FS) + 1, 2)), _pcm(track(int(0.8 * FS) + 1, 3))], axis=1), FS, "pcm16")
    put("monof", track(int(0.1 * FS), 4)[:, None], FS, "float32")
    put("short16", _pcm(track(200, 5))[:, None], FS, "pcm16")                 # shorter than a window
    put("mono48k", _pcm(track(int(0.6 * 48000), 6))[:, None], 48000, "pcm16")  # another rate: converted, alone, in its place
    put("stereof", np.stack([track(int(0.5 * FS), 7), track(int(0.5 * FS), 8)], axis=1), FS, "float32")
    order = ["mono16", "stereo16", "monof", "short16", "mono48k", "stereof"]
    return str(net0), str(net1), paths, [paths[k] for k in order]


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


@pytest.mark.parametrize("extra", [[], ["-d", "0"], ["-d", "0.05"], ["--format", "swift4"], ["--chunk", "1000"], ["--chunk", "0", "-d", "0.05"]])
def test_batch_prints_what_the_loop_over_the_files_prints(files, extra):
    net0, _, paths, order = files
    rc, plain, _ = run("-n", net0, *_audio(order), *extra)
    events = [l for l in plain.splitlines() if l.count(b",") >= 3]
    assert rc == 0 and len(events) >= 6 and plain.count(b".wav\n") == 6
    assert any(l.startswith(b"1,") for l in events)                            # a second track fired too
    assert run("-n", net0, *_audio(order), *extra, "--batch")[:2] == (rc, plain)


def test_batch_rows_and_batch_bytes(files):
    net0, _, paths, order = files
    rc, plain, _ = run("-n", net0, *_audio(order), "-d", "0.05")
    assert run("-n", net0, *_audio(order), "-d", "0.05", "--batch", "--batch-rows", "2")[:2] == (rc, plain)
    assert run("-n", net0, *_audio(order), "-d", "0.05", "--batch", "--batch-rows", "1")[:2] == (rc, plain)
    # 150 000 bytes: mono16 (132 300) and stereo16 pass it together, monof and short16 end at the 48 kHz file, stereof is the third
    assert os.path.getsize(paths["mono16"]) < 150000 < os.path.getsize(paths["mono16"]) + os.path.getsize(paths["stereo16"])
    assert os.path.getsize(paths["monof"]) + os.path.getsize(paths["short16"]) < 150000
    assert run("-n", net0, *_audio(order), "-d", "0.05", "--batch", "--batch-bytes", "150000")[:2] == (rc, plain)
    assert run("-n", net0, *_audio(order), "--batch", "--batch-bytes", "1")[:2] == run("-n", net0, *_audio(order))[:2]   # a batch a file
    # one file: no file-name line either way
    rc1, one, _ = run("-n", net0, "-a", paths["stereo16"])
    assert b".wav" not in one and run("-n", net0, "-a", paths["stereo16"], "--batch")[:2] == (rc1, one)


def test_batch_with_two_networks_and_files_it_cannot_take(files, tmp_path):
    net0, net1, paths, _ = files
    missing = str(tmp_path / "missing.wav")
    # network t runs on track t: the stereo files share a bank; the mono file (one track for two networks) and the missing one
    # are reported as without --batch, and the others proceed
    order = [paths["stereo16"], paths["mono16"], paths["stereof"], missing, paths["stereo16"]]
    rc, plain, err = run("-n", net0, "-n", net1, *_audio(order), "-d", "0.05")
    assert rc == 0 and sum(l.count(b",") >= 3 for l in plain.splitlines()) >= 4 and b"missing.wav" in err and b"2 networks" in err
    rcb, got, errb = run("-n", net0, "-n", net1, *_audio(order), "-d", "0.05", "--batch")
    assert (rcb, got) == (rc, plain) and b"missing.wav" in errb and b"2 networks" in errb
    # the second network's thresholds and weights are its own: the two tracks' lines differ from a one-network run's
    assert run("-n", net0, "-a", paths["stereo16"], "-d", "0.05")[1] != run("-n", net0, "-n", net1, "-a", paths["stereo16"], "-d", "0.05", "--batch")[1]
