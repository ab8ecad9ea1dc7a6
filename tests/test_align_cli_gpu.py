"""The command line tool's --align-dir on the GPU: every file it writes is byte for byte the same with and without --batch (also
when --batch-bytes cuts the files into several batches); <name>.npy equals Aligner.windows from Python on the same file and the
numpy model (tests/align_ref.py); <name>.tsv names every window's track, sample and time; count.npy, sum.npy and sumsq.npy are the
model's tree over the files in command-line order; standard output and the exit status are those of the command without the
options.  Five short WAV files with planted syllables: one at 48 kHz (under --resample sinc), one of two tracks."""
import os
import subprocess

import numpy as np
import pytest
import torch

import align_ref as ref
import recordings_ref
import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100
DEBOUNCE = 0.05
SOURCES = {"columns": ref.COLUMNS, "outputs": ref.OUTPUTS, "samples": ref.SAMPLES}


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    """-> (net, paths, tracks, labels file): tracks[path] = per track (rows, columns, outputs, detections, labels), the arrays made
    through a one-channel handle on the track alone (the 48 kHz file converted as the tool converts it)"""
    d = tmp_path_factory.mktemp("align")
    cfg = util.sample_net()
    net = d / "net.txt"
    net.write_text(cfg.toText())
    tmpl = util.template()
    syl = lambda n, seed: _pcm(synth.syllable_channel(n, tmpl, seed=seed, every=6000))
    files = [("a", FS, [syl(FS, 1)]), ("b", FS, [syl(30001, 2), syl(30001, 3)]), ("c", FS, [syl(FS // 2, 4)]),
             ("d48", 48000, [syl(40000, 5)]), ("e", FS, [syl(1400, 6)])]                      # e: nine frames, no evaluation
    hop, _, _, first = recordings_ref.clock(cfg)
    paths, tracks, lines = [], {}, []
    with sd.SyllableDetector(cfg, channels=1) as one:
        for name, rate, chans in files:
            p = str(d / (name + ".wav"))
            wavutil.write_wav(p, np.stack(chans, axis=1), rate, "pcm16")
            paths.append(p)
            tracks[p] = []
            for t, x in enumerate(chans):
                q = torch.from_numpy(x[None, :]).cuda()
                rows = sd.convertRate(q, float(rate), float(FS), method="sinc") if rate != FS else q.float() * (1.0 / 32768.0)
                S = rows.shape[1]
                if one.countEvaluations(S) > 0:
                    out, fl = one.run(rows)
                    det, _ = recordings_ref.events(fl[0].cpu().numpy(), first, hop, int(DEBOUNCE * FS))
                else:
                    out, det = torch.zeros((1, 0, 1), device="cuda"), np.zeros(0, np.int64)
                cols = one.spectrogram(rows) if one.countFrames(S) > 0 else torch.zeros((1, 0, one.geometry.bins), device="cuda")
                torch.cuda.synchronize()
                labels = sorted([-100, 500, 3000 + 7 * t, S - 1, S + 50])
                tracks[p].append((rows.clone(), cols, out, det, np.asarray(labels, np.int64)))
                lines += ["%s\t%d\t%d" % (p, t, s) for s in reversed(labels)]
    assert sum(len(tr[3]) for trs in tracks.values() for tr in trs) >= 5                      # detections exist
    lab = d / "labels.tsv"
    lab.write_text("\n".join(lines) + "\n")
    return cfg, str(net), paths, tracks, str(lab)


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


def _read(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}


def _check(archive, tmp_path, name, at, before, after):
    cfg, net, paths, tracks, lab = archive
    source = SOURCES[name]
    T = cfg.timeRange
    b, a = (T - 1 if before is None else before), (T - 1 if after is None else after)
    base = ["-n", net, *_audio(paths), "-d", str(DEBOUNCE), "--resample", "sinc"]
    opts = (["--align", name] if name != "columns" else []) + (["--align-at", "labels", "--score", lab] if at == "labels" else [])
    opts += (["--align-before", str(before)] if before is not None else []) + (["--align-after", str(after)] if after is not None else [])
    plain = run(*base)
    assert plain[0] == 0 and plain[1].count(b",") >= 5, plain
    dirs = {k: str(tmp_path / k) for k in ("files", "batch", "batches")}
    one = run(*base, "--align-dir", dirs["files"], *opts)
    score = ["--score-out", str(tmp_path / "table.tsv"), "--score-tolerance", "0.0001"] if at == "labels" else []   # (labels 51 samples apart)
    many = run(*base, "--batch", "--align-dir", dirs["batch"], *opts, *score)
    cut = run(*base, "--batch", "--batch-rows", "2", "--batch-bytes", "150000", "--align-dir", dirs["batches"], *opts, *score)
    for got in (one, many, cut):
        assert got[0] == plain[0] and got[1] == plain[1], (got[0], got[2][-400:])           # standard output and the exit status
    want = _read(dirs["files"])
    assert sorted(want) == sorted([os.path.basename(p) + ext for p in paths for ext in (".npy", ".tsv")] + ["count.npy", "sum.npy", "sumsq.npy"])
    assert _read(dirs["batch"]) == want and _read(dirs["batches"]) == want                    # byte for byte
    # every file's windows: Aligner.windows from Python on the same file, and the model
    origin, step = ref.anchor(cfg, source)
    stack_w, stack_m = [], []
    with sd.SyllableDetector(cfg, channels=1) as det, det.aligner(name, b, a) as al:
        for p in paths:
            arr = np.load(os.path.join(dirs["files"], os.path.basename(p) + ".npy"))
            assert arr.dtype == np.dtype("<f4") and arr.shape[1:] == (b + a + 1, al.shape[2])
            text = open(os.path.join(dirs["files"], os.path.basename(p) + ".tsv")).read().splitlines()
            parts, rows_of = [], []
            for t, (rows, cols, out, detections, labels) in enumerate(tracks[p]):
                events = labels if at == "labels" else detections
                array = {ref.COLUMNS: cols, ref.OUTPUTS: out, ref.SAMPLES: rows}[source]
                got = al.windows(array, [events]).cpu().numpy()
                model, present = ref.windows(array[0].cpu().numpy(), [int(s) for s in events], origin, step, b, a, np.float32(np.nan))
                ref.same(got, model, "%s, track %d: Aligner.windows against the model" % (p, t))
                parts.append(got)
                stack_w.append(got)
                stack_m.append(present)
                rows_of += ["%d\t%d" % (t, s) for s in events]
            ref.same(arr, np.concatenate(parts), "%s: the tool's windows against Aligner.windows" % p)
            assert len(text) == arr.shape[0] and all(line.startswith(r + "\t") for line, r in zip(text, rows_of))
            assert all(abs(float(line.split("\t")[2]) - int(line.split("\t")[1]) / FS) < 1e-9 for line in text)
    # the three stack files: the model's tree over the files in order
    windows, present = np.concatenate(stack_w), np.concatenate(stack_m)
    assert windows.shape[0] >= 5 and present.any() and (at == "detections" or not present.all())   # (labels lie before 0 and behind the end)
    count, total, squares = ref.stats_one(windows, present)
    for fname, model in (("count.npy", count), ("sum.npy", total), ("sumsq.npy", squares)):
        got = np.load(os.path.join(dirs["files"], fname))
        assert got.shape == (1,) + model.shape
        ref.same(got[0], model, fname)


def test_columns_at_the_detections_with_the_defaults(archive, tmp_path):
    _check(archive, tmp_path, "columns", "detections", None, None)


@pytest.mark.parametrize("name,at,before,after", [("outputs", "labels", 3, 4), ("samples", "detections", 700, 2), ("columns", "labels", 9, 0)])
def test_the_other_sources_and_the_labels(archive, tmp_path, name, at, before, after):
    _check(archive, tmp_path, name, at, before, after)


def test_the_refusals(archive, tmp_path):
    cfg, net, paths, tracks, lab = archive
    d = str(tmp_path / "out")
    for args, word in ((["--align", "columns"], b"--align-dir"), (["--align-dir", d, "--align", "bins"], b"columns, outputs or samples"),
                       (["--align-dir", d, "--align-at", "labels"], b"--score"), (["--align-dir", d, "--align-before", "-1"], b"0 or more"),
                       (["--align-dir", d, "--align", "samples", "--align-before", "600000", "--align-after", "600000"], b"at most"),
                       (["--align-dir", d, "-a", paths[0]], b"two of those are called")):
        rc, out, err = run("-n", net, *_audio(paths[:2]), *args)
        assert rc == 64 and word in err, (args, err[-300:])
    assert not os.path.exists(d)
