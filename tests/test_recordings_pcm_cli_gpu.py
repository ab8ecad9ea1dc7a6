"""The command line tool's --batch on files in their own sample formats (GPU): 16-bit, 24-bit, float and 8-bit files in one batch
are uploaded as their data chunks store them and decoded as the rows load (syldet_recordings_load_pcm_device; under --resample sinc
syldet_recordings_load_sinc_pcm_device), and standard output, the exit status and every --simulate-dir, --ttl-dir, --levels-dir file
are byte for byte those of the same command without --batch (which reads each file through the WAV reader's own conversion).
--score needs --batch, so its table is held to the table of the same recordings stored as 32-bit float files of the decoded
values.  These are guards of behaviour that must not change; that the batch took the new path is tests/test_recordings_pcm_host.py's
check of the tool's source."""
import os
import subprocess

import numpy as np
import pytest

import pcm_ref
import util
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
FS = 44100.0


def run(*args):
    r = subprocess.run([CLI, *args], capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def _bytes(x, fmt):
    """a float signal in [-1, 1) as the format's bytes (frame-major)"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if fmt == pcm_ref.U8:
        return (np.clip(np.round(x * 128.0), -128, 127) + 128).astype(np.uint8)
    if fmt == pcm_ref.S16:
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2").view(np.uint8)
    if fmt == pcm_ref.S24:
        return np.clip(np.round(x * 8388608.0), -8388608, 8388607).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()
    return x.astype("<f4").view(np.uint8)


def _at(x, rate):
    if rate == FS:
        return x
    n = int((x.size - 1) * rate / FS) + 1
    return np.interp(np.arange(n) * (FS / rate), np.arange(x.size), x).astype(np.float32)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    """short files with planted syllables, 1 to 1.5 s: 16-bit mono, 24-bit mono, 24-bit stereo, float32, 8-bit, and a 24-bit file at
    48 kHz; beside each a 32-bit float file of the values its bytes mean; two networks; labels for --score"""
    d = tmp_path_factory.mktemp("pcm_batch")
    cfg = util.sample_net()
    net0, net1 = d / "net0.txt", d / "net1.txt"
    net0.write_text(cfg.toText())
    net1.write_text(nets.perturbed(cfg, 1).toText())
    tmpl = util.template()

    def syl(n, seed):
        return synth.syllable_channel(n, tmpl, seed=seed, every=6000) * np.float32(0.9)

    spec = [("mono16", pcm_ref.S16, FS, [syl(44101, 1)]), ("mono24", pcm_ref.S24, FS, [syl(66150, 2)]), ("stereo24", pcm_ref.S24, FS, [syl(44103, 3), syl(44103, 7)]),
            ("float32", pcm_ref.F32, FS, [syl(52921, 4)]), ("mono8", pcm_ref.U8, FS, [syl(44105, 5)]), ("mono24at48k", pcm_ref.S24, 48000.0, [syl(44106, 6)])]
    paths, floats, labels = {}, {}, []
    for name, fmt, rate, chans in spec:
        frames = np.stack([_at(x, rate) for x in chans], axis=1)
        raw = _bytes(frames, fmt)
        paths[name] = str(d / (name + ".wav"))
        pcm_ref.write_wav(paths[name], raw, fmt, len(chans), rate, extensible=(name == "stereo24"))
        floats[name] = str(d / (name + "_as_float.wav"))
        pcm_ref.write_wav(floats[name], pcm_ref.decode(raw, fmt).view(np.uint8), pcm_ref.F32, len(chans), rate)
        for t in range(len(chans)):
            labels += [(name, t, s) for s in range(6000, frames.shape[0], 6000)]
    return str(net0), str(net1), paths, floats, labels, d


def _audio(paths):
    return [a for p in paths for a in ("-a", p)]


def _same_dirs(a, b, names):
    for sub in names:
        files = sorted(os.listdir(os.path.join(a, sub)))
        assert files and files == sorted(os.listdir(os.path.join(b, sub))), sub
        for f in files:
            assert open(os.path.join(a, sub, f), "rb").read() == open(os.path.join(b, sub, f), "rb").read(), (sub, f)


def _dirs(root):
    return ["--simulate-dir", os.path.join(root, "sim"), "--ttl-dir", os.path.join(root, "ttl"), "--levels-dir", os.path.join(root, "levels")]


def test_a_batch_of_mixed_formats_is_the_loop_over_the_files(archive):
    net0, _, paths, floats, labels, d = archive
    order = [paths[k] for k in ("mono16", "mono24", "stereo24", "float32", "mono8")]
    one, many = str(d / "one"), str(d / "many")
    rc, plain, err = run("-n", net0, *_audio(order), "-d", "0.05", *_dirs(one))
    assert rc == 0, err
    events = [l for l in plain.splitlines() if l.count(b",") >= 3]
    assert len(events) >= 6 and plain.count(b".wav\n") == 5 and any(l.startswith(b"1,") for l in events)
    got = run("-n", net0, *_audio(order), "-d", "0.05", "--batch", *_dirs(many))
    assert got[:2] == (rc, plain), got[2]
    _same_dirs(one, many, ("sim", "ttl", "levels"))
    # fewer rows than tracks, and a batch a file (every file alone in a bank: a 24-bit file, an 8-bit file, ... each through the new load)
    assert run("-n", net0, *_audio(order), "-d", "0.05", "--batch", "--batch-rows", "2")[:2] == (rc, plain)
    assert run("-n", net0, *_audio(order), "-d", "0.05", "--batch", "--batch-bytes", "1")[:2] == (rc, plain)
    # --score: the table of the same recordings stored as float files of the decoded values
    tables = []
    for tag, names in (("own", paths), ("float", floats)):
        lab = str(d / ("labels_%s.tsv" % tag))
        with open(lab, "w") as f:
            f.writelines("%s\t%d\t%d\n" % (names[n], t, s) for n, t, s in labels if n != "mono24at48k")
        out = str(d / ("table_%s.tsv" % tag))
        r = run("-n", net0, *_audio([names[k] for k in ("mono16", "mono24", "stereo24", "float32", "mono8")]), "-d", "0.05", "--batch", "--score", lab,
                "--score-out", out)
        assert r[0] == 0, r[2]
        if tag == "own":
            assert r[1] == plain
        tables.append(open(out, "rb").read())
    assert tables[0] == tables[1] and len(tables[0].splitlines()) > 3


def test_a_two_network_call_on_24_bit_stereo(archive):
    net0, net1, paths, floats, _, d = archive
    order = [paths["stereo24"], floats["stereo24"], paths["stereo24"]]
    rc, plain, err = run("-n", net0, "-n", net1, *_audio(order), "-d", "0.05")
    assert rc == 0 and sum(l.count(b",") >= 3 for l in plain.splitlines()) >= 4, err
    assert run("-n", net0, "-n", net1, *_audio(order), "-d", "0.05", "--batch")[:2] == (rc, plain)
    # the second network is its own: other lines than a one-network run's
    assert run("-n", net0, "-a", paths["stereo24"], "-d", "0.05", "--batch")[1] != run("-n", net0, "-n", net1, "-a", paths["stereo24"], "-d", "0.05", "--batch")[1]


def test_a_batch_of_mixed_formats_and_rates_under_resample_sinc(archive):
    net0, _, paths, _, _, d = archive
    order = [paths[k] for k in ("mono24at48k", "mono16", "stereo24", "mono8", "float32", "mono24")]
    one, many = str(d / "one_sinc"), str(d / "many_sinc")
    rc, plain, err = run("-n", net0, *_audio(order), "-d", "0.05", "--resample", "sinc", *_dirs(one))
    assert rc == 0 and sum(l.count(b",") >= 3 for l in plain.splitlines()) >= 6, err
    got = run("-n", net0, *_audio(order), "-d", "0.05", "--resample", "sinc", "--batch", *_dirs(many))
    assert got[:2] == (rc, plain), got[2]
    _same_dirs(one, many, ("sim", "ttl", "levels"))
