"""The command line tool's --match given several times, on the GPU: two --match / --match-out pairs, one a file [2][frames][bins] of
two exemplars of one syllable.  The 2-D class's file is byte for byte what the single --match command writes for that template
(itself held to Matcher.find by tests/test_match_cli_gpu.py); the 3-D class's file is the lines made from MatcherBank.find on every
track alone; the bytes are the same with and without --batch; standard output and the exit status are those of the command without
the options; and the new usage errors (exit 64, the message first on stderr)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import match_bank_cases as bc
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
    d = tmp_path_factory.mktemp("match_bank")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    tmpl = util.template()
    syl = lambda seed: _pcm(synth.syllable_channel(2 * FS, tmpl, seed=seed, every=9000))
    files = [("a", [syl(1)]), ("b", [syl(2), syl(3)]), ("c", [syl(4)])]
    paths, tracks = [], {}
    for name, chans in files:
        p = str(d / (name + ".wav"))
        wavutil.write_wav(p, np.stack(chans, axis=1), FS, "pcm16")
        paths.append(p)
        tracks[p] = chans
    one, two = str(d / "one.npy"), str(d / "two.npy")
    np.save(one, mc.exemplar())                                           # [12][29]
    np.save(two, bc.exemplars())                                          # [2][12][29]: one class of two exemplars
    return d, str(net), paths, tracks, one, two


def test_two_classes_each_into_its_own_file(archive):
    d, net, paths, tracks, one, two = archive
    audio = [a for p in paths for a in ("-a", p)]
    sep = ["--match-separation", str(12.5 * 132 / FS)]                    # 12 whole frames
    plain = run("-n", net, *audio, "-d", "0.05")
    assert plain[0] == 0
    # the single command for the 2-D template, at the threshold class 0 gets below
    single = str(d / "single.tsv")
    rc, stdout, stderr = run("-n", net, *audio, "-d", "0.05", "--match", one, "--match-out", single, "--match-threshold", "0.7", *sep)
    assert rc == 0 and stdout == plain[1], stderr
    outs = {}
    for name, extra in (("files", []), ("batch", ["--batch"])):
        o0, o1 = str(d / (name + "0.tsv")), str(d / (name + "1.tsv"))
        rc, stdout, stderr = run("-n", net, *audio, "-d", "0.05", *extra, "--match", one, "--match-out", o0, "--match", two, "--match-out", o1,
                                 "--match-threshold", "0.7", "--match-threshold", str(bc.THRESHOLD), *sep)
        assert rc == 0 and stdout == plain[1], (name, stderr)
        outs[name] = (open(o0, "rb").read(), open(o1, "rb").read())
    assert outs["files"] == outs["batch"]
    assert outs["files"][0] == open(single, "rb").read() and len(outs["files"][0]) > 0
    # class 1: MatcherBank.find on every track alone, in command-line order, then track, then sample
    want = []
    with sd.SyllableDetector(util.sample_net(), channels=1) as det, det.matcherBank(np.load(two), [0, 0]) as bank:
        for p in paths:
            for t, x in enumerate(tracks[p]):
                cols = det.spectrogram(torch.from_numpy(x[None, :]).cuda().float() * (1.0 / 32768.0))
                events, _, _ = bank.find(cols, bc.THRESHOLD, 12)
                want += ["%s\t%d\t%d\n" % (p, t, s) for s in events[0][0]]
    assert outs["files"][1].decode() == "".join(want) and len(want) >= 8
    # one threshold is every class's; the 3-D file alone is a run of one class
    o0, o1, alone = str(d / "same0.tsv"), str(d / "same1.tsv"), str(d / "alone.tsv")
    assert run("-n", net, *audio, "--match", one, "--match-out", o0, "--match", two, "--match-out", o1, "--match-threshold", str(bc.THRESHOLD), *sep)[0] == 0
    assert run("-n", net, *audio, "--match", two, "--match-out", alone, "--match-threshold", str(bc.THRESHOLD), *sep)[0] == 0
    assert open(o1, "rb").read() == outs["files"][1] == open(alone, "rb").read()


def test_the_new_usage_errors(archive):
    d, net, paths, tracks, one, two = archive
    out, out2 = str(d / "never.tsv"), str(d / "never2.tsv")
    short = str(d / "short.npy")
    np.save(short, np.ones((11, 29), np.float32))
    many = str(d / "many.npy")
    np.save(many, np.ones((33, 12, 29), np.float32))
    sixty_five = str(d / "sixty_five.npy")
    np.save(sixty_five, np.ones((65, 12, 29), np.float32))
    four = str(d / "four.npy")
    np.save(four, np.ones((1, 2, 12, 29), np.float32))
    pair = ["--match", one, "--match-out", out]
    cases = ((["--match", one, "--match", two, "--match-out", out],
              b"--match and --match-out are given equally often"),
             ([*pair, "--match-out", out2], b"--match and --match-out are given equally often"),
             ([*pair, "--match", short, "--match-out", out2], b"--match: " + one.encode() + b" is [12][29] and " + short.encode() + b" [11][29]"),
             ([*pair, "--match", two, "--match-out", out2, "--match-threshold", "0.5", "--match-threshold", "0.6", "--match-threshold", "0.7"],
              b"--match-threshold is given once for all classes, or as many times as --match."),
             (["--match", many, "--match-out", out, "--match", many, "--match-out", out2], b"--match takes 64 exemplars at most"),
             (["--match", sixty_five, "--match-out", out], b"--match: " + sixty_five.encode() + b": not 1 to 64 exemplars"),
             (["--match", four, "--match-out", out], b"--match: " + four.encode() + b": not an array [frames][bins]"),
             ([a for k in range(17) for a in ("--match", one, "--match-out", out + str(k))], b"--match may be given 16 times at most."))
    for args, first in cases:
        rc, stdout, stderr = run("-n", net, "-a", paths[0], *args)
        assert rc == 64 and stderr.startswith(first) and stdout.startswith(b"Usage:"), (args, stderr[:200])
        assert not os.path.exists(out) and not os.path.exists(out2)
