"""CPU tests of the mesh-hull entries (ocean_body_hydrostatics, _device, _async; include/ocean/ocean.h): what can be
checked without a GPU -- the symbols, the constants, the ctypes signatures, and the validation that precedes every device
call.  The argument checks that need no context come before the context's own, so with a null context every bad argument
is still reported as itself (the message names it) and no device is touched: here there is none."""
import ctypes
import os
import re

import numpy as np
import pytest

import ocean_hip as oh

f32 = np.float32
SYMBOLS = ("ocean_body_hydrostatics", "ocean_body_hydrostatics_device", "ocean_body_hydrostatics_async")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ocean", "ocean.h")
V, T, M = 8, 12, 2
GOOD = dict(tile=0, iterations=4, nverts=V, ntris=T, count=M)


def _aligned(shape, dtype):
    """A zeroed array whose first byte is 16-byte aligned."""
    n = int(np.prod(shape))
    raw = np.zeros(n + 4, dtype)
    off = (-raw.ctypes.data % 16) // 4
    return raw[off:off + n].reshape(shape)


BUF = dict(vertices=_aligned((oh.HULL_MAX_VERTICES, 3), f32), triangles=_aligned((oh.HULL_MAX_TRIANGLES, 3), np.int32),
           bodies=_aligned((M, 10), f32), out=_aligned((M, 16), f32))
BUF["triangles"][:T] = oh.OceanContext.box_mesh(1, 1, 1)[1]


def call(L, form, ctx=None, **kw):
    """-> (status, request handle or None) of one C entry, every argument overridable; a buffer by its address."""
    a = dict(GOOD, **{k: v for k, v in kw.items() if k in GOOD})
    p = {k: kw.get(k, BUF[k].ctypes.data) for k in BUF}
    args = (ctx, a["tile"], a["iterations"], ctypes.c_void_p(p["vertices"]), a["nverts"], ctypes.c_void_p(p["triangles"]),
            a["ntris"], ctypes.c_void_p(p["bodies"]), a["count"], ctypes.c_void_p(p["out"]))
    if form == "host":
        return L.ocean_body_hydrostatics(*args), None
    if form == "device":
        return L.ocean_body_hydrostatics_device(*args), None
    req = ctypes.c_void_p(0x1234)
    return L.ocean_body_hydrostatics_async(*args, ctypes.byref(req)), req.value


def refused(L, form, word, **kw):
    L.ocean_host_alloc(0, None)  # (leaves another message behind)
    assert call(L, form, **kw) == (oh.E_INVALID_ARG, None), (form, kw)  # *req is NULL after the failure
    assert word in L.ocean_last_error(), (form, kw, L.ocean_last_error())


def test_hull_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.HULL_MAX_VERTICES, oh.HULL_MAX_TRIANGLES, oh.HULL_RECORD_FLOATS) == (2048, 4096, 16)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i = ctypes.c_void_p, ctypes.c_int
    base = [P, i, i, P, i, P, i, P, i, P]
    for name, args in ((SYMBOLS[0], base), (SYMBOLS[1], base), (SYMBOLS[2], base + [ctypes.POINTER(P)])):
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("body_hydrostatics", "body_hydrostatics_async", "body_hydrostatics_device", "box_mesh"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Hydrostatics)
    # the staged forms' arrays and records fit the point queries' place in the smallest readback slot
    staged = oh.BODY_MAX_BODIES * 40 + oh.HULL_MAX_VERTICES * 12 + oh.HULL_MAX_TRIANGLES * 12
    assert staged <= oh.QUERY_MAX_POINTS * 8 and oh.BODY_MAX_BODIES * 64 <= oh.QUERY_MAX_POINTS * 32


def test_hull_header_python_and_constants_agree():
    h = open(HEADER).read()
    for name, value in (("OCEAN_HULL_MAX_VERTICES", oh.HULL_MAX_VERTICES), ("OCEAN_HULL_MAX_TRIANGLES", oh.HULL_MAX_TRIANGLES),
                        ("OCEAN_HULL_RECORD_FLOATS", oh.HULL_RECORD_FLOATS)):
        assert int(re.search(r"#define " + name + r" (\d+)", h).group(1)) == value
    history = h[:h.index("#define OCEAN_ABI_VERSION")]
    for s in SYMBOLS + ("OCEAN_HULL_MAX_VERTICES", "OCEAN_HULL_MAX_TRIANGLES", "OCEAN_HULL_RECORD_FLOATS"):
        assert re.search(r"\b" + s + r"\b", history), s  # the version history names the new entries
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for s in SYMBOLS:
        proto = re.search(r"int " + s + r"\(([^)]*)\);", code).group(1)
        names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
        want = ["ctx", "tile", "iterations", "vertices", "nverts", "triangles", "ntris", "bodies", "count", "out"]
        assert names == want + (["req"] if s.endswith("_async") else []), s


@pytest.mark.parametrize("form", ["host", "device", "async"])
def test_hull_invalid_arguments_without_a_context(form):
    L = oh.load_library()
    for name in ("vertices", "triangles", "bodies", "out"):
        refused(L, form, b"null vertices", **{name: None})
    for k in (-1, 17):
        refused(L, form, b"iterations", iterations=k)
    for n in (0, -1, oh.HULL_MAX_VERTICES + 1):
        refused(L, form, b"nverts", nverts=n)
    for n in (0, -1, oh.HULL_MAX_TRIANGLES + 1):
        refused(L, form, b"ntris", ntris=n)
    refused(L, form, b"negative body count", count=-1)
    # the staged forms stage at most OCEAN_BODY_MAX_BODIES; the device form is bounded by the samples alone
    refused(L, form, b"OCEAN_BODY_MAX_BODIES" if form != "device" else b"context", count=oh.BODY_MAX_BODIES + 1)
    # count * nverts in 64 bits: 2^13 * 2^11 = 2^24 > 2^22, and 2^31 - 1 bodies of 2048 vertices wrap 32 bits
    refused(L, form, b"OCEAN_BODY_MAX_SAMPLES", count=oh.BODY_MAX_BODIES, nverts=oh.HULL_MAX_VERTICES)
    refused(L, form, b"OCEAN_BODY_MAX_SAMPLES" if form == "device" else b"OCEAN_BODY_MAX_BODIES", count=2 ** 31 - 1,
            nverts=oh.HULL_MAX_VERTICES)
    if form == "device":
        refused(L, form, b"OCEAN_BODY_MAX_SAMPLES", count=(1 << 22) // V + 1)
        refused(L, form, b"context", count=(1 << 22) // V)
    # the limits themselves pass, and so do the defaults: what is wrong then is the null context
    refused(L, form, b"context")
    refused(L, form, b"context", iterations=0)
    refused(L, form, b"context", iterations=16)
    refused(L, form, b"context", nverts=oh.HULL_MAX_VERTICES, ntris=oh.HULL_MAX_TRIANGLES)
    refused(L, form, b"context", count=0)
    assert not BUF["out"].any()  # nothing was written


@pytest.mark.parametrize("form", ["host", "async"])
def test_hull_bad_indices_refused_in_the_staged_forms(form):
    L = oh.load_library()
    tris = BUF["triangles"][:T].copy()
    for where, value in (((0, 0), -1), ((T - 1, 2), V), ((5, 1), 1 << 30), ((3, 0), -(1 << 31))):
        bad = tris.copy()
        bad[where] = value
        refused(L, form, b"triangles[%d][%d]" % where, triangles=bad.ctypes.data)
    # an index is checked against nverts, not against the array it came with
    refused(L, form, b"outside [0, nverts)", nverts=V - 1)
    # the device form cannot see them (its pointer is the device's): the same call goes on to the context
    bad = tris.copy()
    bad[0, 0] = -1
    refused(L, "device", b"context", triangles=bad.ctypes.data)


def test_hull_device_alignment_and_null_request():
    L = oh.load_library()
    assert all(b.ctypes.data % 16 == 0 for b in BUF.values())
    for name, steps in (("vertices", (1, 2, 3)), ("triangles", (1, 2, 3)), ("bodies", (1, 2, 3)), ("out", (4, 8, 12))):
        for off in steps:
            refused(L, "device", b"aligned", **{name: BUF[name].ctypes.data + off})
    for name in ("vertices", "bodies"):  # inputs need 4 bytes only
        refused(L, "device", b"context", **{name: BUF[name].ctypes.data + 4})
    for form in ("host", "async"):  # host buffers need no alignment: the null context is what is wrong
        refused(L, form, b"context", out=BUF["out"].ctypes.data + 4)
    args = (None, 0, 4, BUF["vertices"].ctypes.data, V, BUF["triangles"].ctypes.data, T, BUF["bodies"].ctypes.data, M,
            BUF["out"].ctypes.data)
    L.ocean_host_alloc(0, None)
    assert L.ocean_body_hydrostatics_async(*args, None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


def test_hull_python_argument_shapes():
    mesh = oh.OceanContext.box_mesh(1, 1, 1)
    ok = np.zeros((1, 10), f32)
    for v, t, b in ((np.zeros((8, 2), f32), mesh[1], ok), (mesh[0], np.zeros((12, 4), np.int32), ok),
                    (mesh[0], mesh[1], np.zeros((1, 9), f32))):
        with pytest.raises(ValueError):
            oh.OceanContext._mesh_args(v, t, b)
    v, t, b = oh.OceanContext._mesh_args(mesh[0].astype(np.float64), mesh[1].astype(np.int64), ok)
    assert (v.dtype, t.dtype, b.dtype) == (f32, np.int32, f32)
