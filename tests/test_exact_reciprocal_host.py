"""The output gain's exact reciprocal (csrc/exact_reciprocal.hpp: where the fold kernel's lean form may multiply instead of divide)
on the host (no GPU): tests/cpp/exact_reciprocal_test.cpp holds x * (1 / g) against x / g bit for bit for every power of two the
function accepts, and that no other gain gets a reciprocal.  The plan is that header's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "syllable_detector_swift_amd", "csrc")


def test_exact_reciprocal_against_the_division(tmp_path):
    exe = str(tmp_path / "exact_reciprocal_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "exact_reciprocal_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    assert "exact_reciprocal_f32(" in open(os.path.join(CSRC, "fused_plan.cpp")).read()
