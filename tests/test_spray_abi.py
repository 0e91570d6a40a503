"""CPU tests of the spray particles (ocean_spray_step, _device, _async; include/ocean/ocean.h): what can be checked
without a GPU -- the symbols, the constants, the ctypes signatures, and the validation that precedes every device
call.  The argument checks that need no context come before the context's own, so with a null context every bad
argument is still reported as itself (the message names it) and no device is touched: here there is none."""
import ctypes
import math

import numpy as np
import pytest

import ocean_hip as oh

f32 = np.float32
SYMBOLS = ("ocean_spray_step", "ocean_spray_step_device", "ocean_spray_step_async")
CAP, ECAP = 7, 5
GOOD = dict(tile=0, iterations=2, substeps=4, capacity=CAP, emit_capacity=ECAP)
SPRAY = oh.OceanContext.spray_params(1.0 / 240.0, 9.81, 0.5, (3.0, 0.0, 1.0), 2.0, 1.0, 8.0)


def spray_with(k, value):
    sp = SPRAY.copy()
    sp[k] = value
    return sp


# every OCEAN_E_INVALID_ARG case of ocean.h that needs no context, with a word of the message that names it
BAD = [
    (dict(spray=None), b"null spray"), (dict(pool=None), b"pool"), (dict(out=None), b"output"),
    (dict(iterations=-1), b"iterations"), (dict(iterations=17), b"iterations"),
    (dict(substeps=0), b"substeps"), (dict(substeps=-3), b"substeps"), (dict(substeps=65), b"substeps"),
    (dict(capacity=0), b"capacity"), (dict(capacity=-1), b"capacity"),
    (dict(emit_capacity=0), b"emit_capacity"), (dict(emit_capacity=-2), b"emit_capacity"),
    (dict(emit_capacity=65536), b"emit_capacity"),
    (dict(emitters=None), b"without emitters"),  # NULL emitters with emit_capacity = 5
    (dict(bytes=(CAP + 1) * 32 - 4), b"byte count"), (dict(bytes=CAP * 32), b"byte count"),
    (dict(bytes=(CAP + 2) * 32), b"byte count"), (dict(bytes=0), b"byte count"),
]
BAD += [(dict(spray=spray_with(k, v)), b"not finite") for k in range(oh.SPRAY_FLOATS)
        for v in (math.nan, math.inf, -math.inf)]
BAD += [(dict(spray=spray_with(k, v)), b"reserved") for k in range(9, oh.SPRAY_FLOATS) for v in (1.0, -1e-30)]


def call(L, form, ctx=None, **kw):
    """-> (status, request handle or None) of one C entry, every argument overridable."""
    a = dict(GOOD, **{k: v for k, v in kw.items() if k in GOOD})
    spray = kw.get("spray", SPRAY)
    pool = kw.get("pool", call.pool.ctypes.data)
    emitters = kw.get("emitters", call.emitters.ctypes.data)
    out = kw.get("out", call.buf.ctypes.data)
    nbytes = kw.get("bytes", (a["capacity"] + 1) * 32)
    args = (ctx, a["tile"], a["iterations"], a["substeps"], None if spray is None else spray.ctypes.data,
            ctypes.c_void_p(pool), a["capacity"], ctypes.c_void_p(emitters), a["emit_capacity"], ctypes.c_void_p(out),
            ctypes.c_size_t(nbytes))
    if form == "host":
        return L.ocean_spray_step(*args), None
    if form == "device":
        return L.ocean_spray_step_device(*args), None
    req = ctypes.c_void_p(0x1234)
    return L.ocean_spray_step_async(*args, ctypes.byref(req)), req.value


def _aligned(records):
    """A zeroed float32[records][8] whose first byte is 16-byte aligned."""
    raw = np.zeros(records * 8 + 4, f32)
    off = (-raw.ctypes.data % 16) // 4
    return raw[off:off + records * 8].reshape(records, 8)


call.pool, call.emitters, call.buf = _aligned(CAP + 1), _aligned(ECAP + 1), _aligned(CAP + 1)


def test_spray_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.SPRAY_FLOATS, oh.SPRAY_MAX_PARTICLES, oh.SPRAY_MAX_STAGED, oh.SPRAY_MAX_SUBSTEPS) == \
        (16, (1 << 20) - 1, 65535, 64)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    base = [P, i, i, i, P, P, i, P, i, P, sz]
    want = {"ocean_spray_step": base, "ocean_spray_step_device": base, "ocean_spray_step_async": base + [ctypes.POINTER(P)]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("spray_step", "spray_step_async", "spray_step_device", "parse_spray", "spray_params", "spray_pool"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Spray) and callable(oh.Readback.spray)
    # a staged pool's result fits the smallest readback slot (ocean.h: at most 2 MiB)
    assert (oh.SPRAY_MAX_STAGED + 1) * 32 == 2 << 20 <= oh.QUERY_MAX_POINTS * 40
    sp = oh.OceanContext.spray_params(0.25, 9.0, 0.5, (1.0, 2.0, 3.0), 4.0, 5.0, 6.0)
    np.testing.assert_array_equal(sp, f32([0.25, 9, 0.5, 1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 0, 0, 0]))


@pytest.mark.parametrize("form", ["host", "device", "async"])
def test_spray_invalid_arguments_without_a_context(form):
    L = oh.load_library()
    for kw, word in BAD:
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert call(L, form, **kw) == (oh.E_INVALID_ARG, None), kw
        assert word in L.ocean_last_error(), (kw, L.ocean_last_error())
    # the limit of the form: the staged forms take 65,535 particles, the device form 1,048,575
    staged, device = oh.SPRAY_MAX_STAGED, oh.SPRAY_MAX_PARTICLES
    for cap, refused in ((staged + 1, form != "device"), (device + 1, True)):
        L.ocean_host_alloc(0, None)
        # (one substep, so that the product below stays inside its own limit)
        assert call(L, form, capacity=cap, substeps=1, bytes=(cap + 1) * 32) == (oh.E_INVALID_ARG, None)
        assert (b"capacity" if refused else b"context") in L.ocean_last_error(), (form, cap, L.ocean_last_error())
    # (capacity + emit_capacity) * substeps above 1 << 24, in 64 bits
    for cap, ecap, sub in ((staged, staged, 64), (staged, staged, 2), (1 << 18, ECAP, 64)):
        if form != "device" and cap > staged:
            continue
        L.ocean_host_alloc(0, None)
        assert call(L, form, capacity=cap, emit_capacity=ecap, substeps=sub, bytes=(cap + 1) * 32) == \
            (oh.E_INVALID_ARG, None)
        refused = (cap + ecap) * sub > 1 << 24
        assert (b"substeps = " if refused else b"context") in L.ocean_last_error(), (cap, ecap, sub, L.ocean_last_error())
    # NULL emitters with emit_capacity 0 are good arguments, and so are the defaults: the null context itself
    for kw in (dict(), dict(emitters=None, emit_capacity=0)):
        L.ocean_host_alloc(0, None)
        assert call(L, form, **kw) == (oh.E_INVALID_ARG, None)
        assert b"context" in L.ocean_last_error()
    assert not call.buf.any()  # nothing was written


def test_spray_device_alignment_and_null_request():
    L = oh.load_library()
    ptrs = dict(pool=call.pool.ctypes.data, emitters=call.emitters.ctypes.data, out=call.buf.ctypes.data)
    assert all(p % 16 == 0 for p in ptrs.values())
    for name, base in ptrs.items():
        for off in (4, 8, 12):
            assert call(L, "device", **{name: base + off}) == (oh.E_INVALID_ARG, None), (name, off)
            assert b"aligned" in L.ocean_last_error()
            for form in ("host", "async"):  # host buffers need no alignment: the null context is what is wrong
                assert call(L, form, **{name: base + off}) == (oh.E_INVALID_ARG, None)
                assert b"context" in L.ocean_last_error()
    assert L.ocean_spray_step_async(None, 0, 2, 4, SPRAY.ctypes.data, ctypes.c_void_p(ptrs["pool"]), CAP,
                                    ctypes.c_void_p(ptrs["emitters"]), ECAP, ctypes.c_void_p(ptrs["out"]),
                                    ctypes.c_size_t((CAP + 1) * 32), None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


def test_parse_spray_and_spray_pool():
    """The header's eight uint32 sit in the first record's floats; W records follow."""
    buf = np.full((6, 8), 7.0, f32)
    buf[0].view(np.uint32)[:] = (9, 3, 16, 5, 0, 0, 0, 0)
    buf[1:4, 7] = (2, 5, 11)
    total, cand, rec = oh.OceanContext.parse_spray(buf)
    assert (total, cand) == (9, 16) and rec.shape == (3, 8) and rec.dtype == f32
    np.testing.assert_array_equal(rec[:, 7], f32([2, 5, 11]))
    rec[:] = 0  # a copy
    assert buf[1, 0] == 7.0
    pool = oh.OceanContext.spray_pool(np.arange(16, dtype=f32).reshape(2, 8), 4)
    assert pool.shape == (5, 8) and pool.dtype == f32
    np.testing.assert_array_equal(pool[0].view(np.uint32), np.uint32([2, 2, 2, 4, 0, 0, 0, 0]))
    np.testing.assert_array_equal(pool[1:3].ravel(), np.arange(16, dtype=f32))
    assert not pool[3:].any()
    assert oh.OceanContext.parse_spray(np.zeros((5, 8), f32))[:2] == (0, 0)  # an all-zero header: an empty pool
    with pytest.raises(ValueError):
        oh.OceanContext.spray_pool(np.zeros((5, 8), f32), 4)
