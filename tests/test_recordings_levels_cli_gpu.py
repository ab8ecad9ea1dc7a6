"""The command line tool's --levels-dir (GPU): for any number of audio files, with or without --batch, every file's
<dir>/<name>.tsv is byte for byte what --levels writes for that file alone -- under --batch from the batch's packed rows (int16
rows for 16-bit files, fp32 rows for float files, the converted rows under --resample sinc) -- and standard output and the exit
status are those of the same command without the option."""
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
    """four small WAVs with planted syllables -- 16-bit mono, 16-bit stereo, float mono, 16-bit mono at 48 kHz -- and a fifth, 16-bit,
    shorter than one evaluation; with each file's own --levels table under the options of each case"""
    d = tmp_path_factory.mktemp("levels_dir")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    tmpl = util.template()

    def syl(n, seed):
        return synth.syllable_channel(n, tmpl, seed=seed, every=6000)

    files = [("a", 44100, "pcm16", [syl(20011, 1)]), ("b", 44100, "pcm16", [syl(14003, 2), syl(14003, 3)]), ("c", 44100, "float32", [syl(17777, 4)]),
             ("d", 48000, "pcm16", [syl(15001, 5)]), ("s", 44100, "pcm16", [syl(700, 6)])]
    paths = []
    for name, rate, kind, chans in files:
        p = str(d / (name + ".wav"))
        frames = np.stack([_at(x, float(rate)) for x in chans], axis=1)
        wavutil.write_wav(p, _pcm(frames) if kind == "pcm16" else frames, rate, kind)
        paths.append(p)
    return str(net), paths, d


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


def _alone(net, path, out, *opts):
    """the file's own --levels table"""
    rc, _, err = run("-n", net, "-a", path, "--levels", out, *opts)
    assert rc == 0, err
    return open(out, "rb").read()


def _check_dir(net, paths, d, tag, opts, batch):
    """opts: the options of the tables (--levels-buffer, --levels-period) and of the conversion, which both forms take"""
    general = [o for i, o in enumerate(opts) if not (o.startswith("--levels-") or (i > 0 and opts[i - 1].startswith("--levels-")))]
    plain = run("-n", net, *_audio(paths), "-d", "0.01", *general, *batch)
    assert plain[0] == 0, plain[2]
    out = str(d / ("tables_" + tag))
    got = run("-n", net, *_audio(paths), "-d", "0.01", *opts, *batch, "--levels-dir", out)
    assert got[:2] == plain[:2], got[2]                                     # standard output and the status: unchanged
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) + ".tsv" for p in paths)
    sizes = []
    for p in paths:
        want = _alone(net, p, str(d / ("alone_" + tag + ".tsv")), *opts)
        table = open(os.path.join(out, os.path.basename(p) + ".tsv"), "rb").read()
        assert table == want, (tag, p)
        sizes.append(len(want))
    return sizes


def test_batch_levels_dir_writes_every_files_own_table(archive):
    net, paths, d = archive
    # all five through one bank under --resample sinc: a mixed batch, fp32 rows, the 48 kHz file converted as the rows load
    sizes = _check_dir(net, paths, d, "sinc", ["--resample", "sinc"], ["--batch"])
    assert all(s > 0 for s in sizes)
    stereo = open(str(d / "tables_sinc" / "b.wav.tsv")).read().splitlines()
    assert [l.split("\t")[0] for l in stereo[:4]] == ["0", "1", "0", "1"] and all(len(l.split("\t")) == 4 for l in stereo)
    short = open(str(d / "tables_sinc" / "s.wav.tsv")).read().splitlines()
    assert short and all(l.endswith("\t") for l in short) and not any(l.endswith("\t") for l in stereo)   # readings without an evaluation, and with


@pytest.mark.parametrize("tag,which,opts,batch", [
    # the 16-bit files alone: int16 rows; another buffer and period; fewer rows than tracks
    ("s16", [0, 1, 4], ["--levels-buffer", "8", "--levels-period", "0.013"], ["--batch", "--batch-rows", "2"]),
    # without --resample sinc the 48 kHz file does not join the bank: it ends the batch of the 16-bit file (int16 rows), runs alone in
    # its place -- its table is written all the same -- and the float file makes a batch of fp32 rows
    ("linear", [0, 3, 2], ["--levels-period", "0.05"], ["--batch"]),
    # a batch whose files are all shorter than one evaluation: no event, the input levels all the same
    ("short", [4], ["--levels-buffer", "64"], ["--batch"]),
])
def test_batch_levels_dir_on_other_rows(archive, tag, which, opts, batch):
    net, paths, d = archive
    _check_dir(net, [paths[i] for i in which], d, tag, opts, batch)


def test_levels_dir_without_batch(archive):
    net, paths, d = archive
    _check_dir(net, [paths[1], paths[2], paths[4]], d, "each", [], [])
    _check_dir(net, [paths[3]], d, "one", ["--resample", "sinc", "--levels-buffer", "4096"], [])
