"""The one detector table of the scorer, the aligner, the trainer and the matchers (csrc/detector_spans.hpp), the host side (no
GPU): the header alone under ASan and UBSan, a program of its own (tests/cpp/detector_spans_test.cpp) that holds the unit rules,
the bounds rule, the by_row table and the lookup the kernels run -- the header's own text -- against brute force over 300 seeded
plans; and that the copies the table replaced are gone from csrc."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "syllable_detector_swift_amd", "csrc")


def test_the_table_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "detector_spans_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "detector_spans_test.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1] == "ok" and not r.stderr, (r.stdout, r.stderr)


def test_one_copy_of_each_rule_in_csrc():
    """A search of the source text, so it knows spellings, not meanings.  If it fires on a rewording of the one copy (the sort's
    comparator, up16's parameter list, the search's `.first <= q`, a message), change the pattern with the code; if it fires on a
    count of 2, a second copy of a rule has come back: call detector_spans.hpp / carve.hpp / DetectorTable instead."""
    text = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".cpp", ".hpp", ".hip"))}
    count = lambda pattern: sum(len(re.findall(pattern, t)) for t in text.values())
    assert count(r"stable_sort\([^;]*DetSpan") == 1 and "stable_sort" in text["detector_spans.hpp"]
    assert count(r"\bup16\([a-zA-Z_:<> ]+ n\)") == 1 and "up16(T n)" in text["carve.hpp"]
    assert count(r"\.first <= q\b") == 1                                      # the binary search over a by_row table
    for kernel, calls in (("kernels_train.hip", 1), ("kernels_match.hip", 1)):
        assert text[kernel].count("span_at_or_before(") == calls
    assert count(r"\b(AlignDetDev|TrainDetDev|MatchDetDev)\b") == 0
    assert count(r'reaches beyond its row"') == 1 and count(r"must be the packed rows'") == 1
