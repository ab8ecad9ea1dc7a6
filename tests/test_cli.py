"""The command line tool without a GPU: options, usage text and exit code (SyllableDetectorCLI/main.swift:19-41),
the WAV reader's header handling, error messages.  Nothing here computes."""
import os
import subprocess

import numpy as np
import pytest

import util
import wavutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        pytest.fail("syllable-detector-cli has not been built: python -c 'import __graft_entry__ as g; g.build()'")


@pytest.mark.parametrize("args", [["-h"], ["--help"], ["--bogus"], [], ["-a", "x.wav"]])
def test_usage_text_and_exit_code(args):
    r = run(*args)
    assert r.returncode == 64                                   # EX_USAGE, main.swift:40
    assert "Path to trained network file." in r.stdout
    assert "\t0,1593298,36.1292063492063,0.918557" in r.stdout  # the example line of main.swift:33
    assert "4. The first neural network output." in r.stdout


def test_missing_option_value():
    r = run("-n")
    assert r.returncode == 64 and "Missing value for --net" in r.stderr


def test_unreadable_network_file(tmp_path):
    r = run("-n", str(tmp_path / "nope.txt"), "-a", "x.wav")
    assert r.returncode == 1
    assert r.stderr.startswith("Unable to load the network configuration:")


@pytest.mark.parametrize("kind,bits,label", [("pcm16", 16, "pcm"), ("pcm8", 8, "pcm"), ("pcm24", 24, "pcm"), ("pcm32", 32, "pcm"),
                                             ("float32", 32, "float"), ("float64", 64, "float")])
@pytest.mark.parametrize("extensible", [False, True])
def test_probe_reads_headers(tmp_path, kind, bits, label, extensible):
    rng = np.random.default_rng(bits)
    a = rng.integers(-100, 100, size=(1237, 3)) if label == "pcm" else rng.standard_normal((1237, 3))
    if kind == "pcm8":
        a = a + 128
    p = str(tmp_path / ("t_%s.wav" % kind))
    wavutil.write_wav(p, a, 22050, kind, extensible)
    r = run("--probe", "-a", p)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "%s: 3 channel(s), 22050.0 Hz, %s %d-bit, 1237 frames" % (p, label, bits)


def test_probe_reports_bad_files(tmp_path):
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFFxxxxWAVEjunk")
    notwav = tmp_path / "x.txt"
    notwav.write_text("hello world, not audio")
    r = run("--probe", "-a", str(bad), "-a", str(notwav), "-a", str(tmp_path / "missing.wav"))
    assert r.returncode == 1
    lines = r.stderr.strip().splitlines()
    assert lines[0] == "Unable to read %s: no fmt chunk" % bad
    assert lines[1] == "Unable to read %s: not a RIFF/WAVE file" % notwav
    assert lines[2] == "Unable to read %s: cannot open file" % (tmp_path / "missing.wav")


def test_the_one_output_line_the_reference_holds():
    """SyllableDetectorCLI/main.swift:33 shows an event line, `0,1593298,36.1292063492063,0.918557`: channel 0, sample
    1 593 298 at 44.1 kHz, output 0.918557 -- 15 and 6 significant digits, which is what `\\(Double)` / `\\(Float)` print under
    the Swift 4.0 toolchain the project declares (project.pbxproj:593).  `--format swift4` must reproduce it byte for byte
    from (sample, rate, fp32 output); the default prints the shortest digits that round-trip (Swift >= 4.2)."""
    r = run("--format", "swift4", "--format-line", "0", "1593298", "44100", "0.918557")
    assert r.returncode == 0 and r.stdout == "0,1593298,36.1292063492063,0.918557\n"
    r = run("--format-line", "0", "1593298", "44100", "0.918557")
    assert r.returncode == 0 and r.stdout == "0,1593298,%r,%s\n" % (1593298 / 44100, "0.918557")
    # whole numbers get ".0" in both forms; small and large values keep C's exponent form under swift4
    assert run("--format", "swift4", "--format-line", "3", "88200", "44100", "1", "0.5").stdout == "3,88200,2.0,1.0,0.5\n"
    assert run("--format", "swift4", "--format-line", "1", "1", "3", "0.33333334", "1e-7").stdout == "1,1,0.333333333333333,0.333333,1e-07\n"
    assert run("--format", "shortest", "--format-line", "1", "1", "3", "0.33333334").stdout == "1,1,0.3333333333333333,0.33333334\n"
    assert run("--format", "swift5").returncode == 64


@pytest.fixture(scope="module")
def net_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("clinet") / "net.txt")
    with open(p, "w") as f:
        f.write(util.sample_net().toText())
    return p


@pytest.fixture(scope="module")
def usage_text():
    return run("-h").stdout


# Every message that precedes a usage exit: the shortest argv that reaches it and the first line of standard error.  "NET" is the
# example network (one output, 44100 Hz), "LABELS" a readable labels file, "BROKEN" one whose first line is not a label, "MISSING"
# a path that is not there.  The audio files need not exist: every one of these is refused before a file is read.
OPTION_ERRORS = [
    # ... while the options are read
    (["-n", "NET", "-a"], "Missing value for --audio."),
    (["--batch-rows", "70000"], "--batch-rows takes a number of rows from 1 to 65535."),
    (["--batch-bytes", "1x"], "--batch-bytes takes a number of bytes, 1 or more."),
    (["--score-thresholds", "0:1"], "--score-thresholds takes lo:hi:n, two numbers and a count from 1 to 4096."),
    (["--score-thresholds", "0:1:4097"], "--score-thresholds takes lo:hi:n, two numbers and a count from 1 to 4096."),
    (["--score-tolerance", "-1"], "--score-tolerance takes a number, 0 or more."),
    (["--score-cost", "inf"], "--score-cost takes a number, 0 or more."),
    (["--score-output", "65536"], "--score-output takes the number of a network output, 0 or more."),
    (["--align", "rows"], "--align takes columns, outputs or samples."),
    (["--align-at", "onsets"], "--align-at takes detections or labels."),
    (["--align-before", "-1"], "--align-before and --align-after take a number of units, 0 or more."),
    (["--align-after", "2x"], "--align-before and --align-after take a number of units, 0 or more."),
    (["--resample", "cubic"], "--resample takes linear or sinc."),
    (["--resample-quality", "32,12"],
     "--resample-quality takes Z,beta,rolloff: 4 to 64 zero crossings, beta from 0 to 20, a rolloff above 0 and at most 1."),
    (["--resample-quality", "3,12,0.9"],
     "--resample-quality takes Z,beta,rolloff: 4 to 64 zero crossings, beta from 0 to 20, a rolloff above 0 and at most 1."),
    (["--simulate-output", "2147483648"], "--simulate-output takes an output number (0, 1, ...)."),
    (["--levels-buffer", "24"], "--levels-buffer takes a power of two from 8 to 4096."),
    (["--levels-period", "2e15"], "--levels-period takes a positive number of seconds."),
    (["--ttl-width", "0x"], "--ttl-width takes a positive number of seconds."),
    (["--ttl-latency", "-0.5"], "--ttl-latency takes a number of seconds, 0 or more."),
    (["--ttl-steps", "16777217"], "--ttl-steps takes a number of buffers, 1 or more."),
    (["--ttl-buffer", "48"], "--ttl-buffer takes a power of two from 8 to 4096."),
    # ... the options against each other
    (["-n", "NET", "--resample-quality", "32,12,0.9"], "--resample-quality needs --resample sinc."),
    (["-n", "NET", "-a", "a.wav", "--simulate", ""], "--simulate writes the track of exactly one audio file (-a)."),
    (["-n", "NET", "--ttl-dir", ""], "--simulate-dir, --ttl-dir and --ttl-onsets-dir take the name of a directory."),
    (["-n", "NET", "--ttl-onsets", "o.tsv", "--ttl-onsets-dir", "d"],
     "--simulate-dir, --ttl-dir and --ttl-onsets-dir write what --simulate, --ttl and --ttl-onsets write, for every audio file: give the one or the other."),
    (["-n", "NET", "--levels-dir", ""], "--levels-dir takes the name of a directory."),
    (["-n", "NET", "--levels", "l.tsv", "--levels-dir", "d"], "--levels-dir writes what --levels writes, for every audio file: give the one or the other."),
    (["-n", "NET", "--align-dir", ""], "--align-dir takes the name of a directory."),
    (["-n", "NET", "--align", "outputs"], "--align, --align-at, --align-before and --align-after need --align-dir <dir>."),
    (["-n", "NET", "--align-dir", "d", "--align-at", "labels"], "--align-at labels needs --score <labels.tsv>."),
    (["-n", "NET", "-a", "x/count", "--align-dir", "d"],
     "--align-dir names its files after the audio files (and count, sum, sumsq): two of those are called count."),
    (["-n", "NET", "-a", "x/a.wav", "-a", "a.wav", "--ttl-dir", "d"],
     "--simulate-dir, --ttl-dir, --ttl-onsets-dir and --levels-dir name their files after the audio files: two of those are called a.wav."),
    (["-n", "NET", "--ttl-mux", "--batch"], "--ttl-mux is not available under --batch."),
    (["-n", "NET", "--simulate-output", "0"], "--simulate-output needs --simulate <out.wav> or --simulate-dir <dir>."),
    (["-n", "NET", "-a", "a.wav", "--levels", ""], "--levels writes the readings of exactly one audio file (-a)."),
    (["-n", "NET", "--levels-period", "0.5"], "--levels-buffer and --levels-period need --levels <out.tsv> or --levels-dir <dir>."),
    (["-n", "NET", "--ttl-onsets", "o.tsv"], "--ttl and --ttl-onsets write the triggers of exactly one audio file (-a)."),
    (["-n", "NET", "--ttl-mux"], "--ttl-mux needs --ttl <out.wav> or --ttl-dir <dir>."),
    (["-n", "NET", "--ttl-latency", "0.1"],
     "--ttl-width, --ttl-steps, --ttl-buffer and --ttl-latency need --ttl <out.wav>, --ttl-onsets <out.tsv>, --ttl-dir <dir> or --ttl-onsets-dir <dir>."),
    (["-n", "NET", "--ttl-dir", "d", "--ttl-width", "0.001", "--ttl-steps", "20"], "--ttl-width and --ttl-steps both set the pulse's width: give one."),
    (["-n", "NET", "--batch-bytes", "4096"], "--batch-rows and --batch-bytes need --batch."),
    (["-n", "NET", "-a", "a.wav", "--levels", "l.tsv", "--batch"], "--levels is not available under --batch: it takes exactly one file and a bank of its own."),
    (["-n", "NET", "-a", "a.wav", "--ttl-onsets", "o.tsv", "--batch"],
     "--batch runs many files through one bank; --simulate, --ttl and --ttl-onsets take exactly one file: give --simulate-dir, --ttl-dir and --ttl-onsets-dir instead."),
    (["-n", "NET", "--score", "l.tsv"], "--score needs --batch."),
    (["-n", "NET", "--score-cost", "2"], "--score-out, --score-thresholds, --score-tolerance, --score-cost and --score-output need --score <labels.tsv>."),
    (["-n", "NET", "--batch", "--score", "l.tsv"], "--score <labels.tsv> needs --score-out <table.tsv>."),
    (["-n", "NET", "--batch", "--score", "MISSING", "--score-out", "t.tsv"], "--score: unable to open MISSING."),
    (["-n", "NET", "--batch", "--score", "BROKEN", "--score-out", "t.tsv"], "--score: BROKEN, line 2: not file<TAB>track<TAB>sample."),
    # ... and against the networks, once they are loaded
    (["-n", "NET", "--simulate-dir", "d", "--simulate-output", "3"], "--simulate-output 3: the network has 1 output(s)."),
    (["-n", "NET", "--ttl-dir", "d", "--ttl-width", "1e-6"], "--ttl-width: shorter than one sample at 44100.0 Hz."),
    (["-n", "NET", "--ttl-onsets-dir", "d", "--ttl-latency", "400"], "The pulse's width and --ttl-latency may be 16777216 samples at most."),
    (["-n", "NET", "--batch", "--score", "LABELS", "--score-out", "t.tsv", "--score-tolerance", "24"], "--score-tolerance may be 1048576 samples at most."),
    (["-n", "NET", "--batch", "--score", "LABELS", "--score-out", "t.tsv", "--score-output", "1"], "--score-output 1: the network has 1 output(s)."),
    (["-n", "NET", "--align-dir", "d", "--align-before", "1048576"], "--align-before and --align-after: a window may hold 1048576 values at most."),
    # two faults at once: the one that is reported
    (["-n", "NET", "-a", "a.wav", "-a", "b.wav", "--resample-quality", "32,12,0.9", "--simulate", "s.wav"], "--resample-quality needs --resample sinc."),
    (["-n", "NET", "--ttl-width", "0.001", "--ttl-steps", "20"],
     "--ttl-width, --ttl-steps, --ttl-buffer and --ttl-latency need --ttl <out.wav>, --ttl-onsets <out.tsv>, --ttl-dir <dir> or --ttl-onsets-dir <dir>."),
    (["-n", "NET", "--batch", "--ttl-mux", "--simulate-output", "0"], "--ttl-mux is not available under --batch."),
    (["-n", "NET", "--score", "MISSING", "--score-out", "t.tsv"], "--score needs --batch."),
    (["--batch-rows", "4", "--resample", "cubic", "--ttl-buffer", "48"], "--resample takes linear or sinc."),
    (["-n", "NET", "--simulate-dir", "d", "--simulate-output", "3", "--ttl-dir", "e", "--ttl-width", "1e-6"], "--simulate-output 3: the network has 1 output(s)."),
    (["-n", "NET", "--batch", "--score", "LABELS", "--score-out", "t.tsv", "--score-tolerance", "24", "--score-output", "1"],
     "--score-tolerance may be 1048576 samples at most."),
    (["-n", "NET", "--ttl-dir", "d", "--ttl-width", "400", "--align-dir", "e", "--align-before", "1048576"],
     "The pulse's width and --ttl-latency may be 16777216 samples at most."),
]


@pytest.mark.parametrize("args,message", OPTION_ERRORS, ids=[" ".join(a) or "-" for a, _ in OPTION_ERRORS])
def test_option_errors(args, message, net_file, usage_text, tmp_path):
    """the first line of standard error, 64, and the usage text on standard output; nothing is written"""
    labels, bad = tmp_path / "labels.tsv", tmp_path / "bad.tsv"
    labels.write_text("a.wav\t0\t1000\n")
    bad.write_text("# labels\na.wav 0 1000\n")
    names = {"NET": net_file, "LABELS": str(labels), "BROKEN": str(bad), "MISSING": str(tmp_path / "missing.tsv")}

    def put(s):
        for k, v in names.items():
            s = s.replace(k, v)
        return s

    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([CLI, *[put(a) for a in args]], capture_output=True, text=True, timeout=120, cwd=str(work))
    assert r.stderr.splitlines()[:1] == [put(message)], (args, r.stderr)
    assert r.returncode == 64
    assert r.stdout == usage_text and usage_text.startswith("Usage: syllable-detector-cli -n <net>")
    assert os.listdir(str(work)) == []
