"""CPU tests of the whitecap emitters (ocean_whitecaps, _device, _async; include/ocean/ocean.h): what can be checked
without a GPU -- the symbols, the constant, the ctypes signatures, and the validation that precedes every device
call.  The argument checks that need no context come before the context's own, so with a null context every bad
argument is still reported as itself (the message names it) and no device is touched: here there is none."""
import ctypes
import math

import numpy as np
import pytest

import ocean_hip as oh

f32 = np.float32
SYMBOLS = ("ocean_whitecaps", "ocean_whitecaps_device", "ocean_whitecaps_async")
GOOD = dict(tile=0, lod=0.0, threshold=0.5, x0=0.0, z0=0.0, dx=1.0, dz=1.0, nx=4, ny=4, capacity=7)

# every OCEAN_E_INVALID_ARG case of ocean.h that needs no context, with a word of the message that names it
BAD = [
    (dict(out=None), b"output"),
    (dict(lod=math.nan), b"lod"), (dict(lod=math.inf), b"lod"), (dict(lod=-0.5), b"lod"),
    (dict(threshold=math.nan), b"threshold"), (dict(threshold=math.inf), b"threshold"),
    (dict(threshold=-math.inf), b"threshold"),
    (dict(x0=math.nan), b"origin and spacing"), (dict(x0=math.inf), b"origin and spacing"),
    (dict(z0=math.nan), b"origin and spacing"), (dict(z0=-math.inf), b"origin and spacing"),
    (dict(dx=math.nan), b"origin and spacing"), (dict(dx=math.inf), b"origin and spacing"),
    (dict(dz=math.nan), b"origin and spacing"), (dict(dz=-math.inf), b"origin and spacing"),
    (dict(nx=0), b"at least 1"), (dict(ny=0), b"at least 1"), (dict(nx=-4), b"at least 1"), (dict(ny=-1), b"at least 1"),
    (dict(nx=2049, ny=2048), b"OCEAN_GRID_MAX_NODES"), (dict(nx=1 << 16, ny=1 << 16), b"OCEAN_GRID_MAX_NODES"),
    (dict(nx=1 << 30, ny=4), b"OCEAN_GRID_MAX_NODES"),
    (dict(capacity=0), b"capacity"), (dict(capacity=-1), b"capacity"), (dict(capacity=65536), b"capacity"),
    (dict(bytes=8 * 32 - 4), b"byte count"), (dict(bytes=7 * 32), b"byte count"), (dict(bytes=9 * 32), b"byte count"),
    (dict(bytes=0), b"byte count"),
]


def call(L, form, ctx=None, **kw):
    """-> (status, request handle or None) of one C entry, every argument overridable."""
    a = dict(GOOD, **{k: v for k, v in kw.items() if k not in ("bytes", "out")})
    out = kw.get("out", call.buf.ctypes.data)
    nbytes = kw.get("bytes", (a["capacity"] + 1) * 32)
    args = (ctx, a["tile"], a["lod"], a["threshold"], a["x0"], a["z0"], a["dx"], a["dz"], a["nx"], a["ny"], a["capacity"],
            ctypes.c_void_p(out), ctypes.c_size_t(nbytes))
    if form == "host":
        return L.ocean_whitecaps(*args), None
    if form == "device":
        return L.ocean_whitecaps_device(*args), None
    req = ctypes.c_void_p(0x1234)
    return L.ocean_whitecaps_async(*args, ctypes.byref(req)), req.value


call.buf = np.zeros((8, 8), f32)  # 16-byte aligned or not, the host forms take it


def test_whitecap_symbols_constant_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert oh.WHITECAP_MAX_RECORDS == 65535
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    base = [P, i, f, f, f, f, f, f, i, i, i, P, sz]
    want = {"ocean_whitecaps": base, "ocean_whitecaps_device": base, "ocean_whitecaps_async": base + [ctypes.POINTER(P)]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("whitecaps", "whitecaps_async", "whitecaps_device", "parse_whitecaps"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Whitecaps) and callable(oh.Readback.whitecaps)
    # the list fits the smallest readback slot (ocean.h: at most 2 MiB)
    assert (oh.WHITECAP_MAX_RECORDS + 1) * 32 == 2 << 20 <= oh.QUERY_MAX_POINTS * 40


@pytest.mark.parametrize("form", ["host", "device", "async"])
def test_whitecap_invalid_arguments_without_a_context(form):
    L = oh.load_library()
    for kw, word in BAD:
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert call(L, form, **kw) == (oh.E_INVALID_ARG, None), kw
        assert word in L.ocean_last_error(), (kw, L.ocean_last_error())
    # good arguments: the null context itself
    L.ocean_host_alloc(0, None)
    assert call(L, form) == (oh.E_INVALID_ARG, None)
    assert b"context" in L.ocean_last_error()
    assert not call.buf.any()  # nothing was written


def test_whitecap_device_alignment_and_null_request():
    L = oh.load_library()
    base = call.buf.ctypes.data
    base += -base % 16
    for off in (4, 8, 12):
        assert call(L, "device", out=base + off) == (oh.E_INVALID_ARG, None), off
        assert b"aligned" in L.ocean_last_error()
        for form in ("host", "async"):  # host destinations need no alignment: the null context is what is wrong
            assert call(L, form, out=base + off) == (oh.E_INVALID_ARG, None)
            assert b"context" in L.ocean_last_error()
    a = GOOD
    assert L.ocean_whitecaps_async(None, a["tile"], a["lod"], a["threshold"], a["x0"], a["z0"], a["dx"], a["dz"], a["nx"],
                                   a["ny"], a["capacity"], ctypes.c_void_p(base), ctypes.c_size_t(8 * 32),
                                   None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


def test_parse_whitecaps():
    """The header's eight uint32 sit in the first record's floats; W records follow."""
    buf = np.full((6, 8), 7.0, f32)
    buf[0].view(np.uint32)[:] = (9, 3, 16, 5, 0, 0, 0, 0)
    buf[1:4, 7] = (2, 5, 11)
    total, rec = oh.OceanContext.parse_whitecaps(buf)
    assert total == 9 and rec.shape == (3, 8) and rec.dtype == f32
    np.testing.assert_array_equal(rec[:, 7], f32([2, 5, 11]))
    rec[:] = 0  # a copy
    assert buf[1, 0] == 7.0
