"""CPU tests of the C-ABI boundary (no compute calls: no GPU here).

- liboceanhip.so loads and exports every symbol declared in include/ocean/ocean.h
- argument validation that happens before any device call
- the Python host mirror's surface matches the reference's (WaterBody / IFFT / WaterCascade)
"""
import os
import re
import subprocess

import pytest

import ocean_hip as oh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ocean", "ocean.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ocean_[a-z0-9_]+)\s*\(", src)))


def test_library_built_for_gfx950():
    lib = oh.LIB_PATH
    assert os.path.exists(lib), "run __graft_entry__.build() first"
    data = open(lib, "rb").read()
    assert b"gfx950" in data
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data


def test_exports_every_header_symbol():
    L = oh.load_library()
    syms = header_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(L, s), f"{s} declared in ocean.h but not exported"
    assert set(syms) == set(oh.EXPORTED_SYMBOLS)
    # and nothing else with C linkage under the ocean_ prefix
    out = subprocess.check_output(["nm", "-D", "--defined-only", oh.LIB_PATH]).decode()
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if re.search(r" T ocean_", ln)})
    assert exported == syms


def test_abi_version():
    assert oh.load_library().ocean_abi_version() == 4


@pytest.mark.parametrize("n,c,t,code", [(100, 1, 1, oh.E_UNSUPPORTED), (8, 1, 1, oh.E_UNSUPPORTED),
                                         (8192, 1, 1, oh.E_UNSUPPORTED), (64, 0, 1, oh.E_UNSUPPORTED),
                                         (64, 6, 1, oh.E_UNSUPPORTED), (64, 1, 0, oh.E_INVALID_ARG)])
def test_create_validates_before_touching_device(n, c, t, code):
    with pytest.raises(oh.OceanError) as ei:
        oh.OceanContext(n, c, t)
    assert ei.value.code == code
    assert oh.load_library().ocean_last_error()


def test_create_rejects_bad_flags():
    with pytest.raises(oh.OceanError) as ei:
        oh.OceanContext(64, 1, 1, flags=0x80)
    assert ei.value.code == oh.E_INVALID_ARG
    with pytest.raises(oh.OceanError) as ei:
        oh.OceanContext(64, 1, 1, flags=oh.F_DISPLACEMENT_ONLY | oh.F_NORMALS)
    assert ei.value.code == oh.E_INVALID_ARG


def test_null_context_is_an_error_not_a_crash():
    import ctypes
    L = oh.load_library()
    assert L.ocean_step(None, ctypes.c_float(0.0)) == oh.E_INVALID_ARG
    assert L.ocean_synchronize(None) == oh.E_INVALID_ARG
    L.ocean_destroy(None)  # no-op
    # ABI 4's entries: validated before any device call
    out = ctypes.c_void_p()
    assert L.ocean_set_readback_timing(None, 1) == oh.E_INVALID_ARG
    assert L.ocean_read_height_async(None, 0, 0, None, 64, ctypes.byref(out)) == oh.E_INVALID_ARG
    assert L.ocean_read_height_async(None, 0, 0, None, 64, None) == oh.E_INVALID_ARG
    assert L.ocean_readback_status(None) == oh.E_INVALID_ARG
    ms = ctypes.c_float()
    assert L.ocean_readback_copy_ms(None, ctypes.byref(ms)) == oh.E_INVALID_ARG
    L.ocean_readback_release(None)  # no-op


def test_host_mirror_surface_matches_reference():
    """WaterBody.cs public fields/methods and defaults (WaterBody.cs:10-33, 180, 195)."""
    wb = oh.WaterBody()
    assert (wb.windSpeed, wb.windDirection, wb.gravity, wb.fetch, wb.depth, wb.texturesSize) == \
        (1.0, (1.0, 1.0), 9.81, 1.0, 4.0, 256)
    for name in ("Awake", "CalculateWavesTexturesAtTime", "Update", "GetWaterHeight", "OnDisable", "OnValidate"):
        assert callable(getattr(wb, name))
    assert wb.GetWaterHeight((0.0, 0.0, 0.0)) == 0.0  # no readback yet -> 0 (WaterBody.cs:197)
    c = oh.WaterCascade()
    assert (c.wavelength, c.cutoffHigh, c.cutoffLow, c.swell, c.fade) == (10.0, 5.0, 0.0001, 0.4, 0.1)
    scene = oh.scene_water_body()
    assert scene.texturesSize == 512 and len(scene.cascades) == 3 and scene.windDirection == (1.0, -1.0)
    assert callable(oh.IFFT.InverseFastFourierTransform)


def test_cpp_host_builds_and_checks_arguments():
    """The compiled C++ host of the WaterBody lifecycle (ocean-simulation_amd/host) links against
    liboceanhip.so; with bad arguments it exits before any GPU call (tests/test_gpu_host.py runs it)."""
    import subprocess
    host = os.path.join(ROOT, "ocean-simulation_amd", "host", "abi_host")
    assert os.path.exists(host), "build it: make -C ocean-simulation_amd"
    r = subprocess.run([host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_sequence_host_builds_and_checks_arguments(tmp_path):
    """The compiled host that plays a sequence of calls (host/abi_sequence; tests/test_gpu_host_sequences.py runs
    it): with no arguments, with an op it does not know, with an op of the wrong length or with flags that
    water_body.h cannot make, it exits 2 with a usage line before any device call (which, without a GPU, would
    fail with exit 1)."""
    import subprocess
    host = os.path.join(ROOT, "ocean-simulation_amd", "host", "abi_sequence")
    assert os.path.exists(host), "build it: make -C ocean-simulation_amd"
    r = subprocess.run([host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr and r.stdout == ""
    for ops, flags, why in (("step 0\nsplash 1 2\n", "8", "unknown op splash"), ("step 0\ngrid 1 4 0\n", "8", "grid takes 9"),
                            ("step 0\n", "12", "flags"), ("ctx 1 64 2 7 2\n", "8", "flags")):
        with open(tmp_path / "ops.txt", "w") as f:
            f.write(ops)
        r = subprocess.run([host, str(tmp_path), "64", "2", flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr and why in r.stderr and r.stdout == "", (ops, r.stderr)


def test_env_knobs_match_integration_table():
    """Every environment variable the library reads (getenv in csrc/) is one of INTEGRATION.md's
    knob table, and every row of that table is read: no hidden schedule switches, and no knob that
    skips work."""
    csrc = os.path.join(ROOT, "ocean-simulation_amd", "csrc")
    read = set()
    for name in os.listdir(csrc):
        src = open(os.path.join(csrc, name)).read()
        read |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', src))
        assert not re.search(r"getenv\([^\"]", src), f"{name}: getenv of a computed name"
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    table = set(re.findall(r"^\| `([A-Z0-9_]+)`", sec, flags=re.M))
    assert read == table, f"read but undocumented: {read - table}; documented but not read: {table - read}"
    strings = open(oh.LIB_PATH, "rb").read()
    for word in (b"NOSTORE", b"A3_VARIANT", b"A4_WHOLE", b"OCEAN_GRAPH"):
        assert word not in strings, word
