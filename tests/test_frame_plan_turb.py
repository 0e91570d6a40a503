"""CPU test of defer_turb (ocean-simulation_amd/csrc/frame_plan.h, deferred TURB).

The stand-alone program tests/frame_plan_turb_test.cpp plans the benchmark shapes and one frame per reason not to
defer (the knob, the pointer handed out, an H0 upload, OCEAN_Q=0, OCEAN_A4=0, a column band, a parity,
displacement only, N = 256 / 2048 / 4096) and checks the flag every step carries.  Run the program with any
argument to print the cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ocean-simulation_amd", "csrc")
TEST_SRC = os.path.join(ROOT, "tests", "frame_plan_turb_test.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_defer_turb_per_frame(tmp_path):
    exe = tmp_path / "frame_plan_turb_test.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, TEST_SRC, "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
