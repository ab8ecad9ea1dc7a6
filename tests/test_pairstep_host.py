"""The fold kernel's progress words (kernels_fused_s.hip at hop 132: each wave publishes its tile in one LDS word, its SIMD partner
reads it), their places walked on the host (no GPU): tests/cpp/pair_progress_test.cpp goes over csrc/pair_progress.hpp -- the
header the kernel and its launcher are compiled from -- for timeRange 1 .. 12: eight distinct, aligned words, each inside its
wave's share of the LDS and outside ring, mirror, rows, zero quads and lane-group table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_progress_words_layout(tmp_path):
    exe = str(tmp_path / "pair_progress_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pair_progress_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
