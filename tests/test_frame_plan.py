"""CPU test of the frame schedule ("Frame schedule").

What a fused frame launches -- three-plane or four-plane passes, unit chunks, column bands, pass BQ's DISP store
policy, pruned or dense kernels -- is decided by ocean-simulation_amd/csrc/frame_plan.h, host code without HIP.
The stand-alone program tests/frame_plan_test.cpp collects the steps of plan_frame for the benchmark shapes and
for every such choice and compares them with plans derived by hand (the derivation is at each case).  Run the
program with any argument to print the plans."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ocean-simulation_amd", "csrc")
TEST_SRC = os.path.join(ROOT, "tests", "frame_plan_test.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_plans_against_hand_derived(tmp_path):
    exe = tmp_path / "frame_plan_test.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, TEST_SRC, "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
