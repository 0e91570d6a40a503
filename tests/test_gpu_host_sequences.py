"""Sequences of C-ABI calls from ONE compiled process (ocean-simulation_amd/host/abi_sequence) against the same
sequences through the Python binding, bit for bit.

The other compiled-host tests (tests/test_gpu_*_host.py) make one consumer call per process, and every GPU test in
Python runs on the HIP runtime torch bundles, which ocean_hip loads first on purpose.  A shipping host is a compiled
program on the system's runtime that calls the library every frame for as long as it lives.  Here the host plays a
list of ops (defined in this file, written to ops.txt; abi_sequence.cpp only interprets them): the same blocking call
again, the three consumers without staged inputs back to back and across a frame, interleaved with the consumers that
stage inputs, output blocks that grow and shrink, calls while a request is in flight, and two contexts side by side.
Before every call the host fills the output buffer with a NaN bit pattern, and its summary line says how many words
still hold it, so a failure reads as "untouched", "all zero" or "wrong numbers".  The summary also carries the path of
the libamdhip64 the host mapped, which must not be torch's copy.

No tolerances: the Python forms are held to numpy restatements by their own suites (tests/test_gpu_grid.py and its
siblings); this file shows that a compiled process gets the same bits.  Every expected array of a consumer is
asserted finite and not all zero, so that equality with an untouched or cleared buffer can never pass.

Two sequences are also replayed by a child Python process that blocks torch before it imports the binding, which then
binds to the system's runtime: that separates "system runtime" from "compiled host" as the condition of a failure.
With the per-call hipMallocAsync block that run_staged_impl had before this file existed, seven of the ten tests
failed on ROCm 7.2.0's runtime, the camera child among them (docs/MEASUREMENTS.md section 24)."""
import sys

if __name__ == "__main__":  # the torch-less child (see the end of the file): before ocean_hip is imported
    sys.modules["torch"] = None

import functools
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (under pytest, conftest.py has done this)
    for _p in (ROOT, os.path.join(ROOT, "ocean-simulation_amd"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, _p)

import ocean_hip as oh
import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

HOST = os.path.join(ROOT, "ocean-simulation_amd", "host", "abi_sequence")
f32 = np.float32
MIPS, VEL = oh.F_MIPS, oh.F_MIPS | oh.F_VELOCITY
NO_DATA = ("step", "wait", "ctx")

# the inputs of the staged consumers: abi_host.cpp's points, rays, boxes and motions
POINTS = f32([[0.0, 0.0], [37.5, -12.25], [-410.0, 250.75], [1e4, -3333.0], [-0.5, 64.0]])
POINTS3 = f32([[-300.0 + 97.5 * i, 40.0 - 13.25 * i, 0.5 * i] for i in range(8)])
RAYS = f32([[0.0, 40.0, 0.0, 0.0, -1.0, 0.0, 0.0, 80.0], [37.5, 25.0, -12.25, 0.6, -0.8, 0.0, 0.0, 100.0],
            [-410.0, 30.0, 250.75, -2.0, -1.0, 3.0, 0.0, 60.0], [1e4, 35.0, -3333.0, 1.0, 0.0, 0.0, 0.0, 500.0],
            [-0.5, 20.0, 64.0, 0.0, 1.0, 0.5, 0.0, 50.0], [12.0, -50.0, 7.0, 0.0, 1.0, 0.0, 0.0, 10.0]])
HULL = oh.OceanContext.box_hull(4, 3)
BODIES = f32([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0, 1.0, 2.0], [37.5, 0.25, -12.25, 0.5, 0.5, 0.5, 0.5, 3.0, 2.0, 3.0],
              [-410.0, -0.5, 250.75, 0.0, 0.0, 0.6, 0.8, 6.0, 1.5, 2.5], [1e4, 0.125, -3333.0, 0.28, 0.0, 0.0, 0.96, 2.0, 0.75, 8.0],
              [-0.5, -0.25, 64.0, 0.0, -0.6, 0.0, 0.8, 5.0, 3.0, 1.0]])
MOTION = f32([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [1.0, 2.0, -3.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0, 0.0],
              [-2.5, 0.125, 4.0, 0.25, -0.5, 0.75], [0.5, -1.0, 0.25, -1.5, 0.125, 0.0]])
# two cameras of 45 x 37 pixels: one 30 m up whose image the horizon crosses, one that looks straight down from 25 m,
# so that every pixel meets the water and its range image is finite; and a single pixel of the second
HORIZON = oh.look_at_camera((3.0, 30.0, -4.0), (40.0, 22.0, 80.0), (0.0, 1.0, 0.0), 1.0, 45, 37, 0.0, 600.0)
DOWN = oh.look_at_camera((5.0, 25.0, -7.0), (5.0, 0.0, -7.0), (0.0, 0.0, 1.0), 1.0, 45, 37, 0.0, 60.0)
PIXEL = oh.look_at_camera((5.0, 25.0, -7.0), (5.0, 0.0, -7.0), (0.0, 0.0, 1.0), 1.0, 1, 1, 0.0, 60.0)
MATERIAL = oh.material(lod_slope=0.004)
K, S, B = 2, 32, 6  # a camera's fixed-point steps, march steps and bisections


def grid(mode, x0, z0, dx, dz, nx, ny, lod=0.0, name="grid"):
    return (name, mode, 0 if mode == oh.GRID_VERTICES else 4, lod, x0, z0, dx, dz, nx, ny)


def camera(mode, cam, w, h):
    return ("camera", mode, K, S, B, w, h, cam, MATERIAL if mode == oh.CAMERA_COLOR else None)


def whitecaps(threshold, x0, z0, dx, dz, nx, ny, capacity, lod=0.0):
    return ("whitecaps", lod, threshold, x0, z0, dx, dz, nx, ny, capacity)


REGION = (-40.0, -25.0, 3.5, 2.25, 5, 4)      # 20 nodes
REGION_B = (100.0, -300.0, 7.0, 11.0, 9, 7)   # another place, 63 nodes
REGION_C = (12.5, 8.0, -1.5, 0.75, 3, 2)      # 6 nodes, a negative spacing
FOAM_REGION = (-500.0, -500.0, 40.0, 40.0, 26, 26)


def make_ctx(n, C, flags, seed):
    ctx = oh.OceanContext(n, C, 1, flags)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(seed)
    ctx.init_spectrum()
    return ctx


@functools.lru_cache(maxsize=None)
def foam_median(n, C, flags, *times):
    """A whitecap threshold that means something on this context after steps at `times`: the smallest, over the
    frames, of the median foam of FOAM_REGION's nodes, so that every frame selects at least half of them (the foam is
    the sum over the cascades of 1 - saturate(TURB.x): its scale is the scene's)."""
    ctx = make_ctx(n, C, flags, 42)
    medians = []
    for t in times:
        ctx.step(t)
        medians.append(float(np.median(ctx.surface_grid(*FOAM_REGION, mode=oh.GRID_VERTICES)[..., 3])))
    ctx.close()
    return min(medians)


def whitecap_list(ctx, op):
    """The whole list as the host writes it: the header, the W records, zeros (ocean.h leaves the rest unspecified)."""
    _, lod, threshold, x0, z0, dx, dz, nx, ny, capacity = op
    total, rec = ctx.whitecaps(threshold, x0, z0, dx, dz, nx, ny, capacity, lod)
    buf = np.zeros((capacity + 1, 8), f32)
    buf[0].view(np.uint32)[:4] = (total, len(rec), nx * ny, capacity)
    buf[1:1 + len(rec)] = rec
    return buf


def replay(ops, n, C, flags):
    """The ops through the Python binding: the expected array of every op (None where an op yields none; a request's
    array stands at the request's own index, read when the sequence waits)."""
    ctxs = {0: make_ctx(n, C, flags, 42)}
    ctx, want, pending = ctxs[0], [None] * len(ops), []
    for k, op in enumerate(ops):
        name, a = op[0], op[1:]
        if name == "ctx":
            if len(a) == 5:
                ctxs[a[0]] = make_ctx(a[1], a[2], a[4], a[3])
            ctx = ctxs[a[0]]
        elif name == "step":
            ctx.step(a[0])
        elif name == "grid":
            want[k] = ctx.surface_grid(*a[3:], mode=a[0], iterations=a[1], lod=a[2])
        elif name == "camera":
            want[k] = ctx.camera(a[6], a[4], a[5], a[0], a[7], 0, a[1], a[2], a[3])
        elif name == "whitecaps":
            want[k] = whitecap_list(ctx, op)
        elif name == "query_surface":
            want[k] = ctx.query_surface(a[2], 0, a[0], a[1])
        elif name == "query_velocity":
            want[k] = ctx.query_velocity(a[1], 0, a[0])
        elif name == "raycast":
            want[k] = ctx.raycast(a[3], 0, a[0], a[1], a[2])
        elif name == "body_buoyancy":
            want[k] = ctx.body_buoyancy(a[2], a[3], a[1], a[0])
        elif name == "body_dynamics":
            want[k] = ctx.body_dynamics(a[3], a[4], a[5], a[1], a[0], a[2])
        elif name == "sample_world":
            want[k] = ctx.sample_world(a[0])
        elif name == "surface_bounds":
            want[k] = ctx.surface_bounds()
        elif name == "read":
            want[k] = ctx.read(a[0], 0, a[1])
        elif name == "read_height_async":
            pending.append((k, ctx.read_height_async(0, a[0])))
        elif name == "grid_async":
            pending.append((k, ctx.surface_grid_async(*a[3:], mode=a[0], iterations=a[1], lod=a[2])))
        elif name == "wait":
            for j, rb in pending:
                want[j] = rb.data
                rb.release()
            pending = []
        else:
            raise ValueError(name)
    assert not pending, "a sequence ends with its wait"
    for c in ctxs.values():
        c.close()
    return want


def write_ops(path, ops):
    """ops.txt and the input files of a sequence: an array becomes in_<k>_<j>.bin, None "-", a float its repr (which
    strtod reads back to the same double; both sides then narrow it to float)."""
    lines = []
    for k, op in enumerate(ops):
        words = [op[0]]
        for j, a in enumerate(op[1:]):
            if a is None:
                words.append("-")
            elif isinstance(a, np.ndarray):
                name = f"in_{k}_{j}.bin"
                np.ascontiguousarray(a, f32).tofile(os.path.join(path, name))
                words.append(name)
            elif isinstance(a, float):
                words.append(repr(a))
            else:
                words.append(str(int(a)))
        lines.append(" ".join(words))
    with open(os.path.join(path, "ops.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def mapped_runtime():
    """The libamdhip64 mapped into this process (after the library is loaded), resolved."""
    oh.load_library()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, f"one HIP runtime per process, found {sorted(paths)}"
    return os.path.realpath(paths.pop())


def torch_dir():
    import torch
    return os.path.realpath(os.path.dirname(torch.__file__)) + os.sep


def assert_system_runtime(path, who, record_property):
    """`who` runs on a runtime outside torch's package; where that is also this process's runtime (a machine with one
    runtime only) the test says so and still runs."""
    real = os.path.realpath(path)
    assert path and not real.startswith(torch_dir()), f"{who} mapped torch's HIP runtime: {path}"
    mine = mapped_runtime()
    record_property(f"{who}_hip_runtime", real)
    record_property("python_hip_runtime", mine)
    print(f"{who}: HIP runtime {real}; this process: {mine}" + ("  (one runtime on this machine)" if real == mine else ""))


def describe(got, want, entry, others):
    """What a wrong buffer looks like: never written, cleared, another op's result, or wrong numbers."""
    if entry["words"] and entry["sentinel"] == entry["words"]:
        return "untouched: every word still holds the host's sentinel"
    if not got.view(np.uint32).any():
        return "all zero"
    for j, o in others:
        if o.size == got.size and np.array_equal(o.view(np.uint32), got.view(np.uint32)):
            return f"holds the result of op {j}"
    differ = got.view(np.uint32) != want.view(np.uint32)
    return (f"wrong numbers: {int(differ.sum())} of {got.size} words differ, the first at {int(differ.argmax())}, "
            f"{int((got.view(np.uint32) == 0).sum())} are zero, {entry['sentinel']} still hold the sentinel")


def assert_meaningful(op, want, k):
    """No expected array is one that an untouched or cleared buffer could equal."""
    assert np.isfinite(want).all() and want.any(), f"op {k} {op[0]}: the expected array must be finite and not all zero"
    if op[0] == "whitecaps":  # (the header alone is never zero)
        head = want[0].view(np.uint32)
        assert head[1] > 0 and want[1:1 + head[1]].any(), f"op {k} whitecaps: the expected list must hold records"


def run_once(argv):
    """One child process, 120 s, no retry.  A child that a signal killed or that had to be killed ends the session:
    nothing more is started on a device that may have faulted."""
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=120, env=dict(os.environ))
    except subprocess.TimeoutExpired:
        pytest.exit(f"{argv[0]} did not finish in 120 s", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"{argv[0]} died with {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr
    return r


def run_host(tmp_path, ops, n, C, flags, record_property):
    """One process plays the ops; returns (summary, the array of every op that yields one, flat)."""
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    write_ops(str(tmp_path), ops)
    r = run_once([HOST, str(tmp_path), str(n), str(C), str(flags)])
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert [e["op"] for e in summary["ops"]] == [op[0] for op in ops]
    assert_system_runtime(summary["hip_runtime"], "host", record_property)
    got = []
    for k, (op, e) in enumerate(zip(ops, summary["ops"])):
        assert e["rc"] == oh.OK, f"op {k} {op[0]} returned {e['rc']}"
        path = os.path.join(tmp_path, f"out_{k}.bin")
        got.append(None if op[0] in NO_DATA else np.fromfile(path, f32))
    return summary, got


def check_sequence(tmp_path, ops, n, C, flags, record_property, want=None):
    """The host's result of every op equals the binding's, bit for bit; returns the expected arrays."""
    want = replay(ops, n, C, flags) if want is None else want
    for k, (op, w) in enumerate(zip(ops, want)):
        assert (w is None) == (op[0] in NO_DATA), f"op {k} {op[0]}"
        if w is not None:
            assert_meaningful(op, w, k)
    summary, got = run_host(tmp_path, ops, n, C, flags, record_property)
    bad = []
    for k, (op, w, g, e) in enumerate(zip(ops, want, got, summary["ops"])):
        if w is None:
            continue
        w = np.ascontiguousarray(w, f32).reshape(-1)
        assert e["words"] == w.size == g.size, f"op {k} {op[0]}: {e['words']} words, expected {w.size}"
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            others = [(j, np.ascontiguousarray(o, f32).reshape(-1)) for j, o in enumerate(want) if o is not None and j != k]
            bad.append(f"op {k} {op[0]}: {describe(g, w, e, others)}")
        else:  # (a whitecap list's unspecified tail may keep what the block held before)
            assert e["sentinel"] == 0 or op[0] == "whitecaps", f"op {k} {op[0]}: equal, yet {e['sentinel']} sentinels"
    print("\n".join(bad) if bad else f"{sum(w is not None for w in want)} results equal bit for bit")
    assert not bad, "; ".join(bad)
    for k, (w, g) in enumerate(zip(want, got)):  # and through numpy's own comparison, shapes restored
        if w is not None:
            np.testing.assert_array_equal(g.reshape(np.shape(w)), w, err_msg=f"op {k}")
    return want


def same_call_again(family):
    """step, X, X, X of another shape with more output, X of a third shape with less; (ops, n, C, flags)."""
    if family == "grid":
        return [("step", 0.5), grid(oh.GRID_SURFACE, *REGION), grid(oh.GRID_SURFACE, *REGION),
                grid(oh.GRID_VERTICES, *REGION_B, lod=1.5), grid(oh.GRID_HEIGHTFIELD, *REGION_C)], 64, 2, MIPS
    if family == "camera":
        return [("step", 0.5), camera(oh.CAMERA_HITS, HORIZON, 45, 37), camera(oh.CAMERA_HITS, HORIZON, 45, 37),
                camera(oh.CAMERA_RANGE, DOWN, 45, 37), camera(oh.CAMERA_COLOR, HORIZON, 45, 37)], 64, 2, MIPS
    th = foam_median(64, 2, VEL, 0.5)
    return [("step", 0.5), whitecaps(th, *FOAM_REGION, 1024), whitecaps(th, *FOAM_REGION, 1024),
            whitecaps(th, -700.0, 300.0, 25.0, 35.0, 40, 31, 2048, lod=1.25), whitecaps(th, *FOAM_REGION, 5)], 64, 2, VEL


@functools.lru_cache(maxsize=None)
def again(family):
    """A same-call-again sequence and its expected arrays, computed once: the host's test and the torch-less child's
    share them."""
    ops, n, C, flags = same_call_again(family)
    return ops, n, C, flags, replay(ops, n, C, flags)


def test_same_grid_again(tmp_path, record_property):
    """ocean_surface_grid four times after one step: the same grid twice (the documented failure is the second), a
    larger one elsewhere in another mode, a smaller height field."""
    ops, n, C, flags, want = again("grid")
    check_sequence(tmp_path, ops, n, C, flags, record_property, want)
    assert np.array_equal(want[1], want[2]) and want[3].size > want[1].size > want[4].size


@pytest.mark.parametrize("family", ["camera", "whitecaps"])
def test_same_call_again(tmp_path, family, record_property):
    """The same for ocean_camera (HITS, HITS, RANGE, COLOR) and ocean_whitecaps (a list twice, a longer one at another
    lod elsewhere, one cut off at its capacity)."""
    ops, n, C, flags, want = again(family)
    check_sequence(tmp_path, ops, n, C, flags, record_property, want)
    assert np.array_equal(want[1], want[2])
    if family == "whitecaps":
        head = want[4][0].view(np.uint32)
        assert head[0] > head[1] == 5  # the last list overflows its capacity


def test_no_input_families_across_a_frame(tmp_path, record_property):
    """grid, camera, whitecaps back to back after step t0 and again after step t1: the second frame's results are
    Python's for t1 and not the first frame's again."""
    th = foam_median(64, 2, VEL, 0.25, 1.75)
    frame = [grid(oh.GRID_VERTICES, *REGION_B), camera(oh.CAMERA_COLOR, HORIZON, 45, 37), whitecaps(th, *FOAM_REGION, 1024)]
    ops = [("step", 0.25)] + frame + [("step", 1.75)] + frame
    want = check_sequence(tmp_path, ops, 64, 2, VEL, record_property)
    for k in (1, 2, 3):
        assert not np.array_equal(want[k], want[k + 4]), f"op {k}: the water moved between the frames"


def test_interleaved_with_staged_inputs(tmp_path, record_property):
    """The consumers without inputs between the ones that upload theirs first, and the plain reads."""
    th = foam_median(128, 3, VEL, 0.75)
    g = grid(oh.GRID_SURFACE, *REGION)
    ops = [("step", 0.75), ("raycast", 4, 32, 8, RAYS), g, ("query_surface", oh.QUERY_SURFACE, 4, POINTS),
           camera(oh.CAMERA_HITS, HORIZON, 45, 37), ("body_buoyancy", oh.QUERY_SURFACE, 4, HULL, BODIES),
           whitecaps(th, *FOAM_REGION, 1024), ("sample_world", POINTS3), g, ("surface_bounds",),
           ("read", oh.TEX_DISP, 1), ("query_velocity", 4, POINTS),
           ("body_dynamics", oh.QUERY_SURFACE, 4, oh.DRAG_QUADRATIC, HULL, BODIES, MOTION), g]
    want = check_sequence(tmp_path, ops, 128, 3, VEL, record_property)
    assert np.array_equal(want[2], want[8]) and np.array_equal(want[2], want[13])


def test_output_sizes_grow_and_shrink(tmp_path, record_property):
    """Grids of 32 B (one node), 192 B (3 x 2), 2 MiB (256 x 256) and 32 B again; cameras of 1 x 1, then 45 x 37."""
    ops = [("step", 0.5), grid(oh.GRID_SURFACE, 3.25, -8.5, 1.0, 1.0, 1, 1), grid(oh.GRID_SURFACE, *REGION_C),
           grid(oh.GRID_VERTICES, -320.0, -320.0, 2.5, 2.5, 256, 256), grid(oh.GRID_SURFACE, 3.25, -8.5, 1.0, 1.0, 1, 1),
           camera(oh.CAMERA_RANGE, PIXEL, 1, 1), camera(oh.CAMERA_HITS, DOWN, 45, 37)]
    want = check_sequence(tmp_path, ops, 64, 2, MIPS, record_property)
    assert [w.nbytes for w in want[1:5]] == [32, 192, 2 << 20, 32] and want[5].nbytes == 4
    assert np.array_equal(want[1], want[4])


def test_blocking_calls_beside_a_request_in_flight(tmp_path, record_property):
    """step; read_height_async; grid; grid; wait; grid_async; grid; wait: every result is right, the requests'
    included, and the request's grid equals the blocking one."""
    g, ga = grid(oh.GRID_SURFACE, *REGION), grid(oh.GRID_SURFACE, *REGION, name="grid_async")
    ops = [("step", 0.5), ("read_height_async", 0), g, g, ("wait",), ga, g, ("wait",)]
    want = check_sequence(tmp_path, ops, 64, 2, MIPS, record_property)
    assert want[1].shape == (64, 64) and np.array_equal(want[5], want[6])


def test_two_contexts_in_one_process(tmp_path, record_property):
    """Context A (64, 2 cascades, seed 42) and context B (128, 3 cascades, seed 7, a velocity context) take turns with
    grids and cameras; each result is its own Python context's."""
    g, cam = grid(oh.GRID_SURFACE, *REGION), camera(oh.CAMERA_HITS, DOWN, 45, 37)
    ops = [("step", 0.5), ("ctx", 1, 128, 3, 7, VEL), ("step", 0.5), ("ctx", 0), g, ("ctx", 1), g, ("ctx", 0), cam,
           ("ctx", 1), cam, ("ctx", 0), g, ("ctx", 1), g]
    want = check_sequence(tmp_path, ops, 64, 2, MIPS, record_property)
    assert not np.array_equal(want[4], want[6]) and not np.array_equal(want[8], want[10])
    assert np.array_equal(want[4], want[12]) and np.array_equal(want[6], want[14])


@pytest.mark.parametrize("family", ["grid", "camera"])
def test_binding_on_the_system_runtime(tmp_path, family, record_property):
    """The first sequence once more (and the cameras', whose results are the larger), replayed by a fresh Python
    process in which torch cannot be imported, so that ocean_hip binds to the system's runtime as a compiled host
    does: its results equal this process's."""
    ops, n, C, flags, want = again(family)
    r = run_once([sys.executable, os.path.abspath(__file__), str(tmp_path), family])
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["torch"] is False
    assert_system_runtime(summary["hip_runtime"], "child", record_property)
    bad = []
    for k, w in enumerate(want):
        if w is None:
            continue
        assert_meaningful(ops[k], w, k)
        g = np.load(os.path.join(tmp_path, f"child_{k}.npy"))
        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            bad.append(f"op {k} {ops[k][0]}: " + ("all zero" if not g.any() else "wrong numbers"))
    print("\n".join(bad) if bad else "the child's results equal bit for bit")
    assert not bad, "; ".join(bad)


if __name__ == "__main__":
    # The child of test_binding_on_the_system_runtime: torch is blocked (the head of the file), the binding has
    # loaded the library against the system's runtime; replay the sequence argv[2] and leave the arrays in argv[1].
    _ops, _n, _C, _flags = same_call_again(sys.argv[2])
    for _k, _w in enumerate(replay(_ops, _n, _C, _flags)):
        if _w is not None:
            np.save(os.path.join(sys.argv[1], f"child_{_k}.npy"), _w)
    print(json.dumps({"hip_runtime": mapped_runtime(), "torch": "torch" in sys.modules and sys.modules["torch"] is not None}))
