"""The command line tool's --batch with files at other sampling rates (GPU): under --resample sinc such files join the bank and
are converted as its rows load, and standard output and the exit status stay those of the same command without --batch -- also on
fewer rows than tracks and with the files cut into several batches.  Under the default linear conversion nothing changes.  --score
now counts these files' labels."""
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
FS = 44100.0
LEFT_OUT = b"does not go through the bank; its labels are left out"


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def _at(x, rate):
    """a 44.1 kHz signal at another rate, by linear interpolation (test material: it only has to hold its syllables)"""
    if rate == FS:
        return x.astype(np.float32)
    n = int((x.size - 1) * rate / FS) + 1
    return np.interp(np.arange(n) * (FS / rate), np.arange(x.size), x).astype(np.float32)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    """five short WAVs with planted syllables: 44.1 kHz 16-bit mono, 48 kHz 16-bit stereo, 22.05 kHz float mono, 48 kHz 16-bit
    mono, 44.1 kHz float mono; labels for every track (their sample numbers are at the network's rate)"""
    d = tmp_path_factory.mktemp("mixed_rates")
    cfg = util.sample_net()
    net = d / "net.txt"
    net.write_text(cfg.toText())
    tmpl = util.template()

    def syl(n, seed):
        return synth.syllable_channel(n, tmpl, seed=seed, every=6000)

    files = [("a", 44100, "pcm16", [syl(39691, 1)]), ("b", 48000, "pcm16", [syl(30871, 2), syl(30871, 3)]),
             ("c", 22050, "float32", [syl(35281, 4)]), ("d", 48000, "pcm16", [syl(22051, 5)]), ("e", 44100, "float32", [syl(26461, 6)])]
    paths, labels = [], []
    for name, rate, kind, chans in files:
        p = str(d / (name + ".wav"))
        frames = np.stack([_at(x, float(rate)) for x in chans], axis=1)
        wavutil.write_wav(p, _pcm(frames) if kind == "pcm16" else frames, rate, kind)
        paths.append(p)
        for t in range(len(chans)):
            labels += ["%s\t%d\t%d" % (p, t, s) for s in (3000 + 500 * t, 9000, 15000)]
    lab = d / "labels.tsv"
    lab.write_text("\n".join(labels) + "\n")
    return str(net), paths, str(lab), len(labels)


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


def test_batch_with_sinc_prints_what_the_files_print_one_by_one(archive):
    net, paths, _, _ = archive
    rc, plain, err = run("-n", net, *_audio(paths), "-d", "0.01", "--resample", "sinc")
    assert rc == 0, err
    # every file fires, the converted ones too
    names = [p.encode() for p in paths]
    per_file, cur = {}, None
    for l in plain.splitlines():
        if l in names:
            cur = l
        elif l.count(b",") >= 3:
            per_file[cur] = per_file.get(cur, 0) + 1
    assert all(per_file.get(n, 0) >= 1 for n in names), per_file
    for extra in ([], ["--batch-rows", "2"], ["--batch-bytes", "150000"]):
        got = run("-n", net, *_audio(paths), "-d", "0.01", "--resample", "sinc", "--batch", *extra)
        assert got[:2] == (rc, plain), (extra, got[2])
    # 150 000 bytes cut the set: a and b pass them together (all 16-bit: the int16 converting load, a copied), then c, d and e
    # (float and 16-bit files: widened on the host)
    assert os.path.getsize(paths[0]) < 150000 < os.path.getsize(paths[0]) + os.path.getsize(paths[1])
    # another quality goes the same way
    q = ["--resample", "sinc", "--resample-quality", "8,12,0.9"]
    rc8, plain8, err = run("-n", net, *_audio(paths), "-d", "0.01", *q)
    assert rc8 == 0 and plain8 != plain, err
    assert run("-n", net, *_audio(paths), "-d", "0.01", *q, "--batch")[:2] == (rc8, plain8)


def test_batch_with_the_default_linear_conversion_is_unchanged(archive):
    net, paths, _, _ = archive
    rc, plain, err = run("-n", net, *_audio(paths), "-d", "0.01")
    assert rc == 0, err
    for extra in ([], ["--resample", "linear"], ["--batch-rows", "2"]):
        got = run("-n", net, *_audio(paths), "-d", "0.01", "--batch", *extra)
        assert got[:2] == (rc, plain), (extra, got[2])
    # ... which is not what the band-limited conversion prints
    assert run("-n", net, *_audio(paths), "-d", "0.01", "--resample", "sinc")[1] != plain


def test_score_counts_the_labels_of_converted_files(archive, tmp_path):
    net, paths, lab, n_labels = archive
    out = str(tmp_path / "table.tsv")
    # one threshold above every output: no detection, every label a miss
    opts = ["--batch", "--score", lab, "--score-out", out, "--score-thresholds", "10:10:1"]
    rc, plain, _ = run("-n", net, *_audio(paths), "--resample", "sinc")
    got = run("-n", net, *_audio(paths), "--resample", "sinc", *opts)
    assert got[:2] == (rc, plain) and rc == 0, got[2]
    assert LEFT_OUT not in got[2]
    line = open(out).read().splitlines()[0].split("\t")
    assert float(line[0]) == 10.0 and int(line[1]) == 0 and int(line[3]) == n_labels == 18
    # under the linear conversion the files at other rates still run alone: their labels are left out, and the message says so
    os.remove(out)
    got = run("-n", net, *_audio(paths), *opts)
    assert got[0] == 0 and got[2].count(LEFT_OUT) == 3
    for p in (paths[1], paths[2], paths[3]):
        assert p.encode() in got[2]
    assert int(open(out).read().splitlines()[0].split("\t")[3]) == 6
