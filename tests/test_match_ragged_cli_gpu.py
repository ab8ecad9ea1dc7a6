"""The command line tool's --match with files of different frame counts, on the GPU: with --match-ragged two --match / --match-out
pairs, one [12][29] and one [2][10][29], make a ragged bank (without it the run is the usage error it was).  Every class's file is the lines made from the Python ragged bank's events
(MatcherBank.find on every track alone, held to the single matchers by tests/test_match_ragged_gpu.py); the bytes are the same with
and without --batch; --match-anchor and --match-separation given once a class are honoured; standard output and the exit status are
those of the command without the options; and the new usage errors (exit 64, the message first on stderr)."""
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
    d = tmp_path_factory.mktemp("match_ragged")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    tmpl = util.template()
    syl = lambda seed: _pcm(synth.syllable_channel(2 * FS, tmpl, seed=seed, every=9000))
    files = [("a", [syl(1)]), ("b", [syl(2), syl(3)])]
    paths, tracks = [], {}
    for name, chans in files:
        p = str(d / (name + ".wav"))
        wavutil.write_wav(p, np.stack(chans, axis=1), FS, "pcm16")
        paths.append(p)
        tracks[p] = chans
    long_, short = str(d / "long.npy"), str(d / "short.npy")
    np.save(long_, mc.exemplar())                                         # [12][29]
    np.save(short, bc.exemplars()[:, 2:])                                 # [2][10][29]: two exemplars, the syllable's last 10 frames
    return d, str(net), paths, tracks, long_, short


def _lines(paths, tracks, templates, classes, anchor, thresholds, separation):
    """a list with, a class, the file the tool must write: MatcherBank.find on every track alone"""
    want = [[] for _ in range(max(classes) + 1)]
    with sd.SyllableDetector(util.sample_net(), channels=1) as det, det.matcherBank(templates, classes, anchor, ragged=True) as bank:
        assert bank.ragged
        for p in paths:
            for t, x in enumerate(tracks[p]):
                cols = det.spectrogram(torch.from_numpy(x[None, :]).cuda().float() * (1.0 / 32768.0))
                events, _, _ = bank.find(cols, thresholds, separation)
                for c in range(len(want)):
                    want[c] += ["%s\t%d\t%d\n" % (p, t, s) for s in events[c][0]]
    return ["".join(w).encode() for w in want]


def test_files_of_different_frame_counts_make_a_ragged_bank(archive):
    d, net, paths, tracks, long_, short = archive
    audio = [a for p in paths for a in ("-a", p)]
    plain = run("-n", net, *audio, "-d", "0.05")
    assert plain[0] == 0
    templates = [np.load(long_)] + list(np.load(short))
    classes = [0, 1, 1]
    thr = ["--match-threshold", "0.7", "--match-threshold", "0.75"]
    # the defaults: every class's last frame, every class's own length as separation (12 and 10 frames)
    outs = {}
    for name, extra in (("files", []), ("batch", ["--batch"])):
        o0, o1 = str(d / (name + "0.tsv")), str(d / (name + "1.tsv"))
        rc, stdout, stderr = run("-n", net, *audio, "-d", "0.05", *extra, "--match-ragged", "--match", long_, "--match-out", o0, "--match", short, "--match-out", o1,
                                 *thr)
        assert rc == 0 and stdout == plain[1], (name, stderr)
        outs[name] = (open(o0, "rb").read(), open(o1, "rb").read())
    assert outs["files"] == outs["batch"]
    want = _lines(paths, tracks, templates, classes, None, [0.7, 0.75], [12, 10])
    assert list(outs["files"]) == want and all(len(w.splitlines()) >= 4 for w in want)
    # an anchor and a separation a class
    sep = ["--match-separation", str(20.5 * 132 / FS), "--match-separation", str(6.5 * 132 / FS)]     # 20 and 6 whole frames
    for name, extra in (("files", []), ("batch", ["--batch"])):
        o0, o1 = str(d / (name + "2.tsv")), str(d / (name + "3.tsv"))
        rc, stdout, stderr = run("-n", net, *audio, *extra, "--match", long_, "--match-out", o0, "--match", short, "--match-out", o1, *thr,
                                 "--match-anchor", "2", "--match-anchor", "0", *sep, "--match-ragged")
        assert rc == 0, (name, stderr)
        outs[name] = (open(o0, "rb").read(), open(o1, "rb").read())
    assert outs["files"] == outs["batch"]
    want2 = _lines(paths, tracks, templates, classes, [2, 0, 0], [0.7, 0.75], [20, 6])
    assert list(outs["files"]) == want2 and want2 != want and all(len(w) > 0 for w in want2)
    # one anchor is every class's: a frame of the shortest template
    o0, o1 = str(d / "same0.tsv"), str(d / "same1.tsv")
    assert run("-n", net, *audio, "--match-ragged", "--match", long_, "--match-out", o0, "--match", short, "--match-out", o1, *thr, "--match-anchor", "9")[0] == 0
    assert [open(o0, "rb").read(), open(o1, "rb").read()] == _lines(paths, tracks, templates, classes, 9, [0.7, 0.75], [12, 10])


def test_the_ragged_usage_errors(archive):
    d, net, paths, tracks, long_, short = archive
    out, out2 = str(d / "never.tsv"), str(d / "never2.tsv")
    bare = ["--match", long_, "--match-out", out, "--match", short, "--match-out", out2]
    pair = [*bare, "--match-ragged"]
    narrow = str(d / "narrow.npy")
    np.save(narrow, np.ones((12, 28), np.float32))
    cases = ((bare, b"--match: " + long_.encode() + b" is [12][29] and " + short.encode() + b" [10][29]: the templates of one run share their frames and bins"),
             (["--match", long_, "--match-out", out, "--match", narrow, "--match-out", out2, "--match-ragged"],
              b"--match: " + long_.encode() + b" is [12][29] and " + narrow.encode() + b" [12][28]"),
             (["--match-ragged"], b"--match-ragged needs --match <template.npy>."),
             ([*pair, "--match-anchor", "10"], b"--match-anchor takes a frame of the template, 0 to 9."),
             ([*pair, "--match-anchor", "11", "--match-anchor", "10"], b"--match-anchor takes a frame of the template: " + short.encode() + b" has the frames 0 to 9."),
             ([*pair, "--match-anchor", "1", "--match-anchor", "1", "--match-anchor", "1"],
              b"--match-anchor is given once for all classes, or as many times as --match."),
             ([*pair, "--match-separation", "0.01", "--match-separation", "0.01", "--match-separation", "0.01"],
              b"--match-separation is given once for all classes, or as many times as --match."),
             ([*pair, "--match-separation", "0.01", "--match-separation", "100"], b"--match-separation may be 4096 frames at most."))
    for args, first in cases:
        rc, stdout, stderr = run("-n", net, "-a", paths[0], *args)
        assert rc == 64 and stderr.startswith(first) and stdout.startswith(b"Usage:"), (args, stderr[:200])
        assert not os.path.exists(out) and not os.path.exists(out2)
