"""The command line tool's --score on the GPU: TABLE is, as text, the table the numpy model (tests/score_ref.py) gives on each
track's own outputs; standard output and the exit status are those of the run without --score; --batch-bytes that cuts the files
into two batches gives the same TABLE; without --batch the option is a usage error."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import recordings_ref
import score_ref as ref
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
    """three small 16-bit WAVs with planted syllables, one of two tracks; each track's outputs of a run alone (the packed run's
    bits on the fold kernel: include/syldet.h, "packed recordings"); labels made from the detections at 50 ms of debounce --
    some moved off their detection, some left out (false positives), some where nothing fires (misses) -- in no order"""
    d = tmp_path_factory.mktemp("score")
    cfg = util.sample_net()
    net = d / "net.txt"
    net.write_text(cfg.toText())
    tmpl = util.template()
    frames = {"a": [_pcm(synth.syllable_channel(FS, tmpl, seed=1, every=6000))],
              "b": [_pcm(synth.syllable_channel(int(0.8 * FS) + 1, tmpl, seed=2, every=6000)), _pcm(synth.syllable_channel(int(0.8 * FS) + 1, tmpl, seed=3, every=6000))],
              "c": [_pcm(synth.syllable_channel(FS // 2, tmpl, seed=4, every=6000))]}
    paths, tracks, lines = [], [], []
    hop, _, _, first = recordings_ref.clock(cfg)
    with sd.SyllableDetector(cfg, channels=1) as one:
        for name, chans in frames.items():
            p = str(d / (name + ".wav"))
            wavutil.write_wav(p, np.stack(chans, axis=1), FS, "pcm16")
            paths.append(p)
            for t, x in enumerate(chans):
                out, fl = one.runPCM16(torch.from_numpy(x[None, :]).cuda())
                torch.cuda.synchronize()
                idx, _ = recordings_ref.events(fl[0].cpu().numpy(), first, hop, int(0.05 * FS))
                # (detections are more than 2205 samples apart, the labels move by 400 at most: windows of 2 x 882 stay disjoint)
                labels = [int(i) - 300 + 100 * (n % 5) for n, i in enumerate(idx) if n % 4 != 3] + [-5000, x.size + 5000]
                assert len(idx) >= 1
                tracks.append((p, t, out[0, :, 0].cpu().numpy().copy(), sorted(labels)))
                lines += ["%s\t%d\t%d" % (p, t, s) for s in reversed(labels)]
    lab = d / "labels.tsv"
    lab.write_text("# file\ttrack\tsample\n" + "\n".join(lines) + "\n")
    return str(net), paths, tracks, str(lab), (hop, first)


def _table_text(tracks, clock, thr, tolerance, debounce_frames, cost):
    hop, first = clock
    tables = [ref.score(y, thr, labels, tolerance, first, hop, debounce_frames) for _, _, y, labels in tracks]
    n_labels = sum(len(labels) for _, _, _, labels in tracks)
    k, totals, costs = ref.choose(np.stack(tables), [len(labels) for _, _, _, labels in tracks], cost)
    lines = []
    for i, th in enumerate(thr):
        det, hits, fp, rep, s1, s2 = (int(v) for v in totals[i])
        if hits:
            mean = s1 / hits
            stats = "%.17g\t%.17g" % (mean, math.sqrt(max(s2 / hits - mean * mean, 0.0)))
        else:
            stats = "nan\tnan"
        lines.append("%.17g\t%d\t%d\t%d\t%d\t%d\t%s\t%.17g" % (th, det, hits, n_labels - hits, fp, rep, stats, costs[i]))
    lines.append("# best %.17g" % thr[k])
    return "\n".join(lines) + "\n", totals


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


def test_table_is_the_models_and_standard_output_is_untouched(archive, tmp_path):
    net, paths, tracks, lab, clock = archive
    out = str(tmp_path / "table.tsv")
    rc, plain, _ = run("-n", net, *_audio(paths), "-d", "0.01", "--batch")
    assert rc == 0 and sum(l.count(b",") >= 3 for l in plain.splitlines()) >= 9
    got = run("-n", net, *_audio(paths), "-d", "0.01", "--batch", "--score", lab, "--score-out", out)
    assert got[:2] == (rc, plain), got[2]
    thr = [0.0 + (1.0 - 0.0) * i / (101 - 1) for i in range(101)]
    want, totals = _table_text(tracks, clock, thr, int(0.02 * FS), int(0.01 * FS), 1.0)
    assert open(out).read() == want
    assert (totals[:, 1] > 0).any() and (totals[:, 2] > 0).any() and (totals[:, 3] > 0).any()      # hits, false positives, repeats
    assert want.count("\n") == 102
    # the other options, and two batches: a and b pass 200 000 bytes together, c is the second batch
    assert os.path.getsize(paths[0]) < 200000 < os.path.getsize(paths[0]) + os.path.getsize(paths[1])
    opts = ["--score-thresholds", "0.1:0.9:17", "--score-tolerance", "0.01", "--score-cost", "2.5", "--score-output", "0"]
    thr = [0.1 + (0.9 - 0.1) * i / (17 - 1) for i in range(17)]
    want, _ = _table_text(tracks, clock, thr, int(0.01 * FS), int(0.05 * FS), 2.5)
    rc, plain, _ = run("-n", net, *_audio(paths), "-d", "0.05", "--batch")
    for extra in ([], ["--batch-bytes", "200000"], ["--batch-rows", "2"]):
        if os.path.exists(out):
            os.remove(out)
        got = run("-n", net, *_audio(paths), "-d", "0.05", "--batch", "--score", lab, "--score-out", out, *opts, *extra)
        assert got[:2] == (rc, plain), (extra, got[2])
        assert open(out).read() == want, extra


def test_usage_errors(archive, tmp_path):
    net, paths, _, lab, _ = archive
    out = str(tmp_path / "table.tsv")
    base = ["-n", net, *_audio(paths), "--batch", "--score", lab, "--score-out", out]
    broken = tmp_path / "broken.tsv"
    broken.write_text("%s\t0\n" % paths[0])
    cases = [["-n", net, *_audio(paths), "--score", lab, "--score-out", out],             # without --batch
             ["-n", net, *_audio(paths), "--batch", "--score", lab],                      # no TABLE
             ["-n", net, *_audio(paths), "--batch", "--score-out", out],                  # options for a table nobody asked for
             ["-n", net, *_audio(paths), "--batch", "--score-cost", "2"],
             base + ["--score-thresholds", "0:1"], base + ["--score-thresholds", "0:1:0"], base + ["--score-thresholds", "0:1:4097"],
             base + ["--score-thresholds", "a:1:5"], base + ["--score-thresholds", "nan:1:5"], base + ["--score-thresholds"],
             base + ["--score-tolerance", "-1"], base + ["--score-tolerance", "30"], base + ["--score-tolerance", "soon"],
             base + ["--score-cost", "-1"], base + ["--score-cost", "nan"], base + ["--score-output", "1"], base + ["--score-output", "-1"],
             ["-n", net, *_audio(paths), "--batch", "--score", str(tmp_path / "none.tsv"), "--score-out", out],
             ["-n", net, *_audio(paths), "--batch", "--score", str(broken), "--score-out", out]]
    for args in cases:
        rc, stdout, stderr = run(*args)
        assert rc == 64 and b"Path to trained network file." in stdout, (args, rc, stderr)
        assert not os.path.exists(out), args
    assert b"--score needs --batch" in run(*cases[0])[2]
    u = run("-h")[1]
    for opt in (b"--score <labels.tsv>", b"--score-out <table.tsv>", b"--score-thresholds <lo:hi:n>", b"--score-tolerance <seconds>",
                b"--score-cost <c>", b"--score-output <k>"):
        assert opt in u, opt
