"""The command line tool's --train on the GPU, end to end: a network made by the tool from nothing but a labelled 16-bit recording
detects held-out syllables through the tool's own --score.

planted_channel(1) (tests/train_cases.py) as a 16-bit WAV, labels at its positions + first_index; --train-seed 0, --train-fit-map,
200 steps.  The log is a first line "# positives <n> negatives <n>" and then 200 lines, one a step.  The bars are tests/test_train_fit_gpu.py's: the last logged loss at or below 0.05 of the first, and on the held-out
channels 2 and 3, at thresholds 0.7, tolerance 2 hops and 50 ms of debounce, every label a hit and no false positive.  Standard
output is that of the same command without the --train options, and the command run twice writes the same bytes."""
import os
import subprocess

import numpy as np
import pytest

import recordings_ref
import train_cases as cases
import util
import wavutil

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _wav(path, x):
    wavutil.write_wav(str(path), np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)[:, None], FS, "pcm16")
    return str(path)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("train")
    cfg = util.sample_net()
    base = d / "base.txt"
    base.write_text(cfg.toText())
    hop, _, _, first = recordings_ref.clock(cfg)
    x, pos = cases.planted_channel(1)
    audio = _wav(d / "train.wav", x)
    labels = d / "labels.tsv"
    labels.write_text("".join("%s\t0\t%d\n" % (audio, p + first) for p in pos))
    net, log = str(d / "net.txt"), str(d / "log.tsv")
    common = ["-n", str(base), "-a", audio, "--batch"]
    options = ["--train", str(labels), "--train-out", net, "--train-seed", "0", "--train-fit-map", "--train-steps", "200", "--train-log", log]
    plain = run(*common)
    got = run(*common, *options)
    return dict(dir=d, hop=hop, first=first, net=net, log=log, common=common, options=options, plain=plain, got=got)


def test_the_tool_trains_a_network_that_detects_held_out_syllables(trained):
    d, hop, first = trained["dir"], trained["hop"], trained["first"]
    rc, out, err = trained["got"]
    assert rc == 0, err
    lines = open(trained["log"]).read().splitlines()
    assert lines[0].startswith("# positives ") and " negatives " in lines[0]
    n_pos, n_neg = int(lines[0].split()[2]), int(lines[0].split()[4])
    steps = [l.split("\t") for l in lines if not l.startswith("#")]
    assert len(steps) == 200 and [int(s[0]) for s in steps] == list(range(1, 201))
    loss = [float(s[1]) for s in steps]
    print("%d positives, %d negatives; mean loss %.4g at the start, %.4g in front of step 200 (%.4g of the start)" % (n_pos, n_neg, loss[0], loss[-1], loss[-1] / loss[0]))
    assert n_pos >= 22 and n_neg > n_pos
    assert loss[-1] <= 0.05 * loss[0]
    # the held-out channels through the tool's own --score
    text = open(trained["net"]).read()
    held_net = d / "held.txt"
    held_net.write_text("".join("thresholds = 0.7\n" if l.startswith("thresholds") else l + "\n" for l in text.splitlines()))
    held, lab = [], []
    for seed in (2, 3):
        x, pos = cases.planted_channel(seed)
        p = _wav(d / ("held%d.wav" % seed), x)
        held.append(p)
        lab += ["%s\t0\t%d" % (p, q + first) for q in pos]
    (d / "held.tsv").write_text("\n".join(lab) + "\n")
    table = str(d / "table.tsv")
    rc, out, err = run("-n", str(held_net), "-a", held[0], "-a", held[1], "-d", "0.05", "--batch", "--score", str(d / "held.tsv"), "--score-out", table,
                       "--score-thresholds", "0.7:0.7:1", "--score-tolerance", repr((2 * hop + 0.5) / FS))
    assert rc == 0, err
    row = open(table).read().splitlines()[0].split("\t")
    detections, hits, misses, false_positives = (int(v) for v in row[1:5])
    print("held out: %d labels, %d detections, %d hits, %d misses, %d false positives" % (len(lab), detections, hits, misses, false_positives))
    assert hits == len(lab) and misses == 0 and false_positives == 0


def test_standard_output_is_the_run_without_the_options_and_the_bytes_repeat(trained):
    assert trained["got"][0] == trained["plain"][0] == 0 and trained["got"][1] == trained["plain"][1]
    first = open(trained["net"], "rb").read()
    log = open(trained["log"], "rb").read()
    os.remove(trained["net"])
    rc, out, err = run(*trained["common"], *trained["options"])
    assert rc == 0 and out == trained["plain"][1], err
    assert open(trained["net"], "rb").read() == first and open(trained["log"], "rb").read() == log
    assert b"processInputs1.function = mapminmax" in first and b"layer0.weights" in first


def test_files_that_pass_the_batch_are_refused(trained, tmp_path):
    out = str(tmp_path / "net.txt")
    audio = trained["common"][3]
    rc, _, err = run("-n", trained["common"][1], "-a", audio, "-a", audio, "--batch", "--batch-bytes", "1000", "--train", trained["options"][1], "--train-out", out,
                     "--train-steps", "1")
    assert rc == 1 and b"--batch-bytes" in err and not os.path.exists(out)
