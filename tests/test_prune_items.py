"""CPU test of the item table of the pruned pass AQ (band-limited cascades).

ocean_init_spectrum reduces every unit's spectrum to its live extent m_u and builds, on the host, the list
of live mirror-pair items the row pass runs (ocean-simulation_amd/csrc/prune_items.h, no HIP).  The
stand-alone program tests/prune_items_test.cpp checks that builder against brute force for random extents
(-1 .. N/2, up to 8 units, N = 512): the count, the (u, y1) of every item in order, every chunk's sub-range
and the empty chunk."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ocean-simulation_amd", "csrc")
TEST_SRC = os.path.join(ROOT, "tests", "prune_items_test.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_item_table_against_brute_force(tmp_path):
    exe = tmp_path / "prune_items_test.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, TEST_SRC, "-o", str(exe)],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
