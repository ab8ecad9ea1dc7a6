"""The command line tool's --match on the GPU: on 4 files of 2 s with planted syllables (one of two tracks), matches.tsv is byte for
byte the same under --batch and file by file (also when --batch-bytes cuts the files into several batches); its lines are what
Matcher.find gives from Python on every track alone, in command-line order, then track, then sample; standard output and the exit
status are those of the commands without the options; the file, fed back as --score matches.tsv, is read without error; and the
usage errors follow the tool's table (exit 64, the message first on stderr)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import match_cases as mc
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
    return r.returncode, r.stdout, r.stderr


def _pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    d = tmp_path_factory.mktemp("match")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    tmpl = util.template()
    syl = lambda seed: _pcm(synth.syllable_channel(2 * FS, tmpl, seed=seed, every=9000))
    files = [("a", [syl(1)]), ("b", [syl(2), syl(3)]), ("c", [syl(4)]), ("d", [syl(5)])]
    paths, tracks = [], {}
    for name, chans in files:
        p = str(d / (name + ".wav"))
        wavutil.write_wav(p, np.stack(chans, axis=1), FS, "pcm16")
        paths.append(p)
        tracks[p] = chans
    template = str(d / "template.npy")
    np.save(template, mc.exemplar())
    return d, str(net), paths, tracks, template


def test_matches_tsv_is_the_same_bytes_with_and_without_batch(archive):
    d, net, paths, tracks, template = archive
    audio = [a for p in paths for a in ("-a", p)]
    opts = ["--match", template, "--match-threshold", "0.77", "--match-separation", str(12.5 * 132 / FS)]       # 12 whole frames
    plain = run("-n", net, *audio, "-d", "0.05")
    plain_batch = run("-n", net, *audio, "-d", "0.05", "--batch")
    assert plain[0] == 0 and plain_batch[0] == 0 and plain[1] == plain_batch[1]
    outs = {}
    for name, extra in (("files", []), ("batch", ["--batch"]), ("batches", ["--batch", "--batch-bytes", "200000"])):
        out = str(d / (name + ".tsv"))
        rc, stdout, stderr = run("-n", net, *audio, "-d", "0.05", *extra, *opts, "--match-out", out)
        assert rc == 0 and stdout == plain[1], (name, stderr)
        outs[name] = open(out, "rb").read()
    assert outs["files"] == outs["batch"] == outs["batches"] and len(outs["files"]) > 0
    # the lines: Matcher.find on every track alone, in command-line order, then track, then sample
    want = []
    with sd.SyllableDetector(util.sample_net(), channels=1) as one, one.matcher(np.load(template)) as m:
        for p in paths:
            for t, x in enumerate(tracks[p]):
                cols = one.spectrogram(torch.from_numpy(x[None, :]).cuda().float() * (1.0 / 32768.0))
                events, _ = m.find(cols, 0.77, 12)
                want += ["%s\t%d\t%d\n" % (p, t, s) for s in events[0]]
    assert outs["files"].decode() == "".join(want) and len(want) >= 8
    # ... and back in as labels: read without error, and the matches are where the detector fires (the table has hits)
    table = str(d / "table.tsv")
    rc, stdout, stderr = run("-n", net, *audio, "-d", "0.05", "--batch", "--score", str(d / "files.tsv"), "--score-out", table)
    assert rc == 0 and stdout == plain[1], stderr
    assert open(table).read().strip().splitlines()[-1].startswith("# best")
    # another anchor moves every sample by whole hops
    out0 = str(d / "anchor0.tsv")
    assert run("-n", net, *audio, *opts, "--match-anchor", "0", "--match-out", out0)[0] == 0
    a0 = [int(l.split("\t")[2]) for l in open(out0).read().splitlines()]
    a11 = [int(l.split("\t")[2]) for l in outs["files"].decode().splitlines()]
    assert [s + 11 * 132 for s in a0] == a11


def test_usage_errors(archive):
    d, net, paths, tracks, template = archive
    out = str(d / "never.tsv")
    bad7 = str(d / "bins7.npy")
    np.save(bad7, np.ones((3, 7), np.float32))
    zero = str(d / "zero.npy")
    np.save(zero, np.zeros((12, 29)))
    ints = str(d / "ints.npy")
    np.save(ints, np.ones((12, 29), np.int32))
    flat = str(d / "flat.npy")
    np.save(flat, np.ones(29, np.float32))
    for args, first in ((["--match", template], b"--match <template.npy> needs --match-out <matches.tsv>."),
                        (["--match-out", out], b"--match-out, --match-threshold, --match-separation and --match-anchor need --match <template.npy>."),
                        (["--match-threshold", "0.5"], b"--match-out, --match-threshold, --match-separation and --match-anchor need --match <template.npy>."),
                        (["--match", template, "--match-out", out, "--match-threshold", "nan"], b"--match-threshold takes a number."),
                        (["--match", template, "--match-out", out, "--match-separation", "-1"], b"--match-separation takes a number of seconds, 0 or more."),
                        (["--match", template, "--match-out", out, "--match-separation", "100"], b"--match-separation may be 4096 frames at most."),
                        (["--match", template, "--match-out", out, "--match-anchor", "12"], b"--match-anchor takes a frame of the template, 0 to 11."),
                        (["--match", str(d / "missing.npy"), "--match-out", out], b"--match: unable to open"),
                        (["--match", bad7, "--match-out", out], b"--match: the template has 7 bins, the network's columns 29."),
                        (["--match", zero, "--match-out", out], b"--match: the template is all zero."),
                        (["--match", ints, "--match-out", out], b"--match: " + ints.encode() + b": not little-endian float32 or float64."),
                        (["--match", flat, "--match-out", out], b"--match: " + flat.encode() + b": not an array [frames][bins]")):
        rc, stdout, stderr = run("-n", net, "-a", paths[0], *args)
        assert rc == 64 and stderr.startswith(first) and stdout.startswith(b"Usage:"), (args, stderr[:200])
        assert not os.path.exists(out)
    # a float64 template is the float32 one
    t64 = str(d / "t64.npy")
    np.save(t64, np.load(template).astype(np.float64))
    a, b = str(d / "t32.tsv"), str(d / "t64.tsv")
    assert run("-n", net, "-a", paths[0], "--match", template, "--match-out", a)[0] == 0
    assert run("-n", net, "-a", paths[0], "--match", t64, "--match-out", b)[0] == 0
    assert open(a, "rb").read() == open(b, "rb").read() != b""
