"""The fold kernel's compile-time ring schedule at hop 132, walked on the host (no GPU): tests/cpp/hopk_schedule_test.cpp models a
wave over the constexpr tables of csrc/hopk_schedule.hpp -- the header the kernel itself is compiled from -- for segments of 1 to
40 tiles: every read lies in a chunk that is there, nothing a tile still needs is overwritten, the mirror is slot 0's chunk."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_model(tmp_path):
    exe = str(tmp_path / "hopk_schedule_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "hopk_schedule_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
