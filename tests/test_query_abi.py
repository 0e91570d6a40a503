"""CPU tests of the surface-query entries (ocean_query_surface, _device, _async; include/ocean/ocean.h):
what can be checked without a GPU -- the symbols, the validation that precedes every device call,
and the hosts' surface (OceanContext.query_surface, WaterBody readback "probes").  The kernels and
the semantics are tested on the GPU in tests/test_gpu_query.py."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh

QUERY_SYMBOLS = ("ocean_query_surface", "ocean_query_surface_device", "ocean_query_surface_async")


def test_query_symbols_exported():
    L = oh.load_library()
    for s in QUERY_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.QUERY_REFERENCE, oh.QUERY_SURFACE, oh.QUERY_MAX_POINTS) == (0, 1, 65536)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)


def test_query_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    pts = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 8), np.float32)
    req = ctypes.c_void_p(0x1234)
    assert L.ocean_query_surface(None, 0, oh.QUERY_SURFACE, 4, pts.ctypes.data, 4, out.ctypes.data) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert L.ocean_query_surface_device(None, 0, oh.QUERY_SURFACE, 4, pts.ctypes.data, 4,
                                        out.ctypes.data) == oh.E_INVALID_ARG
    assert L.ocean_query_surface_async(None, 0, oh.QUERY_SURFACE, 4, pts.ctypes.data, 4, out.ctypes.data,
                                       ctypes.byref(req)) == oh.E_INVALID_ARG
    assert req.value is None  # no request handed back
    assert L.ocean_query_surface_async(None, 0, oh.QUERY_SURFACE, 4, pts.ctypes.data, 4, out.ctypes.data,
                                       None) == oh.E_INVALID_ARG
    assert not out.any()


def test_host_surface_of_the_queries():
    assert callable(oh.OceanContext.query_surface) and callable(oh.OceanContext.query_surface_async)
    wb = oh.WaterBody(readback="probes")
    assert (wb.probeMode, wb.probeIterations) == (oh.QUERY_SURFACE, 4)
    assert wb.ProbeHeights is None
    wb.SetProbes([[1.0, 99.0, 2.0], [3.0, -5.0, 4.0]])  # [M][3]: x and z are used
    np.testing.assert_array_equal(wb._probes, np.array([[1.0, 2.0], [3.0, 4.0]], np.float32))
    assert wb.GetWaterHeight((0.0, 0.0, 0.0)) == 0.0 and wb.buoyancyData is None
    with pytest.raises(ValueError):
        oh.OceanContext._query_points(np.zeros((3, 3), np.float32))


def test_other_readback_strings_are_still_refused(monkeypatch):
    """Awake refuses an unknown readback string (after the context exists, as before): the context is
    stubbed, there is no GPU here."""
    class Stub:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, name):
            return lambda *a, **k: None

    monkeypatch.setattr(oh, "OceanContext", Stub)
    monkeypatch.setattr(oh, "PinnedBuffer", Stub)
    for bad in ("probe", "heights", "", "PROBES"):
        with pytest.raises(ValueError, match="readback must be"):
            oh.WaterBody(readback=bad).Awake()
    wb = oh.WaterBody(readback="probes", probeCapacity=7).Awake()  # the new mode passes the same check
    assert len(wb._ring) == wb._in_flight() + 1 and wb._probe_cap == 7
    with pytest.raises(ValueError):
        wb.SetProbes(np.zeros((8, 3)))  # more than the ring was sized for
