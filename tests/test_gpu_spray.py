"""GPU tests of the spray particles (ocean_spray_step / _device / _async, csrc/spray.hip).  The yardstick is a numpy
fp32 restatement of ocean.h's definition, one rounding per operation in the order written; its eta comes from
ctx.query_surface, the point entry (tests/test_gpu_query.py checks that one against the textures), with the call's
own K.  The kernels run the same fp32 operations in the same order, so every comparison is bit for bit, header and
records, on the uint32 view (a tag is carried whatever its bits are, a NaN's included).

Scenes are N = 64 with the scene's 34 m cascade alone (C = 1; it folds at 64^2, so it has foam and a whitecap list)
and with its last three cascades (C = 3)."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_parity import _ctx_with_env
from test_gpu_query import make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32, u32 = np.float32, np.uint32
SENTINEL = f32(-12345.0)
N = 64
SCENES = {1: O.SCENE_CASCADES[3:4], 3: O.SCENE_CASCADES[1:4]}
REGION = (-37.0, 21.0, 1.3, 0.7, 40, 30)  # 1200 nodes for the emitters
PHYSICS = oh.OceanContext.spray_params(1.0 / 60.0, 9.81, 0.7, (4.0, 0.5, -2.0), 1.5, 1.2, 5.0)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def candidates(sp, pool, emitters):
    """The candidates of ocean.h, float32[M][8], from a pool and an emitter list (or None), headers clamped."""
    n = min(int(bits(pool[0])[1]), len(pool) - 1)
    cand = pool[1:1 + n].copy()
    if emitters is not None:
        e = min(int(bits(emitters[0])[1]), len(emitters) - 1)
        r = emitters[1:1 + e]
        jet, lift = sp[7], sp[8]
        born = np.zeros((e, 8), f32)
        born[:, 0:3] = r[:, 0:3]
        born[:, 4] = jet * r[:, 4]
        born[:, 5] = jet * r[:, 5] + lift * r[:, 3]
        born[:, 6] = jet * r[:, 6]
        born[:, 7] = r[:, 7]
        cand = np.concatenate([cand, born])
    return cand


def restate(ctx, sp, pool, emitters, substeps, iterations, tile=0):
    """(header uint32[8], records float32[W][8], died_in: substep of each candidate's death or 0) of the definition."""
    sp = np.asarray(sp, f32)
    h, g, kd, wx, wy, wz, life = (f32(x) for x in sp[:7])
    capacity = len(pool) - 1
    c = candidates(sp, pool, emitters)
    alive = np.ones(len(c), bool)
    died_in = np.zeros(len(c), np.int64)
    with np.errstate(all="ignore"):
        for s in range(substeps):
            i = np.flatnonzero(alive)
            if not len(i):
                break
            p, a, v = c[i, 0:3], c[i, 3], c[i, 4:7]
            ax, ay, az = kd * (wx - v[:, 0]), kd * (wy - v[:, 1]) - g, kd * (wz - v[:, 2])
            vx, vy, vz = v[:, 0] + h * ax, v[:, 1] + h * ay, v[:, 2] + h * az
            px, py, pz = p[:, 0] + h * vx, p[:, 1] + h * vy, p[:, 2] + h * vz
            a2 = a + h
            for x in (vx, vy, vz, px, py, pz, a2):
                assert x.dtype == f32
            eta = ctx.query_surface(np.stack([px, pz], axis=1), tile, iterations=iterations)[:, 0]
            for col, x in enumerate((px, py, pz, a2, vx, vy, vz)):  # (the tag's column is not touched)
                c[i, col] = x
            ok = (py > eta) & (a2 < life)
            alive[i] = ok
            died_in[i[~ok]] = s + 1
    surv = np.flatnonzero(alive)
    w = min(len(surv), capacity)
    return np.array([len(surv), w, len(c), capacity, 0, 0, 0, 0], u32), c[surv[:w]], died_in


def restate_tagged(ctx, sp, pool, emitters, substeps, iterations, tile=0):
    """restate with the survivors' tags taken from the candidates by their bits."""
    head, rec, died = restate(ctx, sp, pool, emitters, substeps, iterations, tile)
    tags = bits(candidates(np.asarray(sp, f32), pool, emitters)[:, 7])
    keep = np.flatnonzero(died == 0)[:len(rec)]
    rec = rec.copy()
    rec.view(u32)[:, 7] = tags[keep]
    return head, rec, died


def assert_pool(out, head, rec, msg):
    np.testing.assert_array_equal(bits(out[0]), head, err_msg=f"header, {msg}")
    np.testing.assert_array_equal(bits(out[1:1 + len(rec)]), bits(rec), err_msg=msg)


def air_height(ctx, tile=0):
    """H as DESIGN.md states it: fl(sum_c max_c) + 2^-19 fl(sum_c max(|min_c|, |max_c|)) over DISP.y's bounds."""
    b = ctx.surface_bounds(tile)
    top, mag = f32(0), f32(0)
    for c in range(len(b)):
        top = top + b[c, 5]
        mag = mag + max(abs(b[c, 1]), abs(b[c, 5]))
    return f32(top + mag * f32(2.0 ** -19))


def step_ulps(x, k):
    x = np.array(x, f32)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


PLACED = oh.OceanContext.spray_params(1.0 / 64.0, 0.0, 0.0, (2.0, 1.0, -3.0), 2.0, 1.0, 0.0)


def placed_pool(ctx, iterations, tile=0, m=40):
    """A pool at g = kd = 0, v = 0 (a particle stays where it is and only ages) holding every class by construction.
    -> (pool float32[capacity + 1][8], {class: indices})."""
    h, life = PLACED[0], PLACED[6]
    rng = np.random.default_rng(3 + iterations)
    q = rng.uniform(-60.0, 60.0, (m, 2)).astype(f32)
    eta = ctx.query_surface(q, tile, iterations=iterations)[:, 0]
    H = air_height(ctx, tile)
    assert (eta < H).all()
    rows, cls = [], {}

    def add(name, x, y, z, a):
        cls.setdefault(name, []).extend(range(len(rows), len(rows) + len(x)))
        for k in range(len(x)):
            rows.append((x[k], y[k], z[k], a[k], 0.0, 0.0, 0.0, 0.0))

    zero = np.zeros(m, f32)
    for k in (1, 2, 5):
        add("just above eta", q[:, 0], step_ulps(eta, k), q[:, 1], zero)
        add("at or below eta", q[:, 0], step_ulps(eta, 1 - k), q[:, 1], zero)
    for k in (1, 2, 3):
        add("above H", q[:, 0], np.full(m, step_ulps(H, k)), q[:, 1], zero)
        add("at or below H", q[:, 0], np.full(m, step_ulps(H, 1 - k)), q[:, 1], zero)
    edge = f32(life - h)
    for k in range(-3, 4):
        a = step_ulps(edge, k)
        name = "young" if f32(a + h) < life else "old"
        add(name, q[:, 0], eta + f32(1.0), q[:, 1], np.full(m, a))
    a = f32(life - f32(2.5) * h)
    assert f32(a + h) < life and f32(f32(a + h) + h) < life and not f32(f32(f32(a + h) + h) + h) < life
    add("dies in substep 3", q[:, 0], eta + f32(1.0), q[:, 1], np.full(m, a))
    nan = np.full(m, np.nan, f32)
    add("NaN height", q[:, 0], nan, q[:, 1], zero)
    add("NaN x", nan, eta + f32(1.0), q[:, 1], zero)
    rec = np.array(rows, f32)
    rec[:, 7] = np.arange(len(rec), dtype=f32)
    rec.view(u32)[::7, 7] = 0x7FC12345 + np.arange(len(rec[::7]), dtype=u32)  # tags that are NaNs with a payload
    order = rng.permutation(len(rec))  # the classes interleaved over the waves
    inv = np.argsort(order)
    return oh.OceanContext.spray_pool(rec[order], len(rec) + 5), {k: inv[np.array(v)] for k, v in cls.items()}


@pytest.mark.parametrize("C", [1, 3])
def test_spray_placed_classes(C):
    """Every class of the definition, there by construction: heights a few ulp either side of eta and of H, ages
    either side of life - h, a particle that dies in its third substep, NaN positions.  K in {0, 2}, S in {1, 4}."""
    ctx = make_ctx(N, SCENES[C])
    for K in (0, 2):
        pool, cls = placed_pool(ctx, K)
        for name in ("just above eta", "at or below eta", "above H", "at or below H", "young", "old",
                     "dies in substep 3", "NaN height", "NaN x"):
            assert len(cls[name]) > 0, name
        for S in (1, 4):
            head, rec, died = restate_tagged(ctx, PLACED, pool, None, S, K)
            msg = f"C {C}, K {K}, S {S}"
            # the classes behave as they were placed
            assert (died[cls["just above eta"]] == 0).all() and (died[cls["at or below eta"]] == 1).all(), msg
            assert (died[cls["above H"]] == 0).all() and (died[cls["at or below H"]] == 0).all(), msg
            assert (died[cls["old"]] == 1).all() and (died[cls["NaN height"]] == 1).all(), msg
            assert (died[cls["NaN x"]] == 1).all(), msg
            assert (died[cls["dies in substep 3"]] == (3 if S == 4 else 0)).all(), msg
            if S == 1:
                assert (died[cls["young"]] == 0).all(), msg
            out = ctx.spray_step(PLACED, pool, None, S, K)
            assert_pool(out, head, rec, msg)
            assert 0 < head[0] < head[2] == len(pool) - 6
            total, cand, got = oh.OceanContext.parse_spray(out)
            assert (total, cand) == (head[0], head[2]) and got.shape == (head[1], 8)
    ctx.close()


def aged_candidates(ctx, m, e, iterations, tile=0):
    """M = n + e candidates of the PLACED regime, 1.0 above the queried surface, that only age: the pool's n carry ages
    on a fixed pattern either side of life - h (every seventh is old, and at M = 769 the whole of wave 4), the e spawned
    ones are born at age 0.  -> (records float32[n][8], emitters float32[e + 1][8] or None, survives bool[M]), survives
    being decided here, by the ages alone."""
    h, life = PLACED[0], PLACED[6]
    n = m - e
    rng = np.random.default_rng(100 + m)
    q = rng.uniform(-60.0, 60.0, (m, 2)).astype(f32)
    y = ctx.query_surface(q, tile, iterations=iterations)[:, 0] + f32(1.0)
    j = np.arange(n)
    old = (j % 7 == 1) | ((m == 769) & (j >= 256) & (j < 320))
    ages = np.array([step_ulps(f32(life - h), (1 + k % 3) if o else -(1 + k % 3)) for k, o in zip(j, old)], f32).reshape(n)
    rec = np.zeros((n, 8), f32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = q[:n, 0], y[:n], q[:n, 1], ages
    rec[:, 7] = j
    survives = np.concatenate([(ages + h).astype(f32) < life, np.ones(e, bool)])
    assert (survives[:n] == ~old).all()
    emitters = None
    if e:
        emitters = np.zeros((e + 1, 8), f32)
        bits(emitters[0])[:4] = e
        emitters[1:, 0], emitters[1:, 1], emitters[1:, 2], emitters[1:, 3] = q[n:, 0], y[n:], q[n:, 1], 0.5
        emitters[1:, 7] = 1000 + np.arange(e)
    return rec, emitters, survives


# (M, e): e = 37 from M = 64 on, so that the seam between the pool and the spawned falls inside a wave; the last case is
# 769 again with more spawned particles than the pattern retires, which the split of 37 cannot give (below)
EDGE_CASES = [(1, 0), (63, 0), (64, 37), (65, 37), (255, 37), (256, 37), (257, 37), (769, 37), (769, 300)]
# the cases whose survivors - 1 still admit the whole pool: the entry clamps a pool to its capacity, so a capacity
# below n cannot be given all M candidates.  With e = 0 (M = 63) survivors - 1 < n always; at (769, 37) the empty wave
# alone retires 64 > 37 particles.
OVERFLOW_CASES = {(64, 37), (65, 37), (255, 37), (256, 37), (257, 37), (769, 300)}


@pytest.mark.parametrize("M,e", EDGE_CASES)
def test_spray_candidate_counts_at_the_wave_and_chunk_edges(M, e):
    """M = n + e at the edges of a wave (64) and of a chunk (256), 769 being three chunks and one lane, with survivors
    that are known in advance, neither none nor all, and in the 769 cases a whole wave without one.

    With all M candidates: the capacity that holds all survivors T; the smallest capacity the pool admits, n; and, in
    OVERFLOW_CASES, T - 1.  The last two overflow there (T > capacity, asserted), over two chunks at M = 257, where the
    second chunk's offset has reached the capacity n, and over three at (769, 300), where T - 1 cuts inside the last
    chunk.  At M = 63 and (769, 37) no capacity both admits the pool and overflows, so neither T - 1 nor 1 exists
    with M candidates; at M = 1 all three capacities are 1.

    A capacity below n (T - 1 outside OVERFLOW_CASES, and 1) is run with the pool it admits, the first `capacity` of
    the n particles before the same spawned ones: capacity + e candidates, not M, compared like the others."""
    ctx = make_ctx(N, SCENES[1])
    K = 2
    rec, emitters, survives = aged_candidates(ctx, M, e, K)
    n, T = len(rec), int(survives.sum())
    assert n + e == M
    if M >= 2:
        assert 0 < T < M
    if M == 769:
        assert any(not survives[w:w + 64].any() for w in range(0, M, 64))
    overflows = (M, e) in OVERFLOW_CASES
    assert (T - 1 >= n) == overflows
    if (M, e) == (257, 37):
        assert int(survives[:256].sum()) >= n  # capacity n: the workgroup is done at the second chunk
    if (M, e) == (769, 300):
        assert int(survives[:512].sum()) < T - 1  # capacity T - 1: the cut is inside the third chunk
    whole = {max(n, T): False, n: overflows}
    if overflows:
        whole[T - 1] = True
    for capacity, over in sorted(whole.items(), reverse=True):
        assert (T > capacity) == over
        pool = oh.OceanContext.spray_pool(rec, capacity)
        head, got, died = restate_tagged(ctx, PLACED, pool, emitters, 1, K)
        msg = f"M {M}, e {e}, capacity {capacity}"
        assert ((died == 0) == survives).all(), msg
        assert (head[0], head[1], head[2]) == (T, min(T, capacity), M), msg
        assert_pool(ctx.spray_step(PLACED, pool, emitters, 1, K), head, got, msg)
    for capacity in sorted({max(T - 1, 1), 1} - set(range(n, M + 1)), reverse=True):  # below n: the admitted pool
        pool = oh.OceanContext.spray_pool(rec[:capacity], capacity)
        want_t = int(survives[:capacity].sum()) + e
        head, got, died = restate_tagged(ctx, PLACED, pool, emitters, 1, K)
        msg = f"M {M}, e {e}, capacity {capacity} < n"
        assert ((died == 0) == np.concatenate([survives[:capacity], survives[n:]])).all(), msg
        assert (head[0], head[1], head[2]) == (want_t, min(want_t, capacity), capacity + e), msg
        assert_pool(ctx.spray_step(PLACED, pool, emitters, 1, K), head, got, msg)
    ctx.close()


def random_pool(rng, n, capacity, life):
    rec = np.zeros((n, 8), f32)
    rec[:, 0] = rng.uniform(-50, 50, n)
    rec[:, 1] = rng.uniform(-1.0, 4.0, n)
    rec[:, 2] = rng.uniform(-50, 50, n)
    rec[:, 3] = rng.uniform(0, life, n)
    rec[:, 4:7] = rng.uniform(-3, 3, (n, 3))
    rec[:, 7] = rng.integers(0, 1 << 20, n)
    return oh.OceanContext.spray_pool(rec, capacity)


def emitter_list(ctx, e, tile=0, slack=0):
    """A real whitecap list of exactly e records (every node of REGION is selected below any foam), as the library
    writes it, in a buffer of e + slack + 1 records; e = 0: a list with W = 0."""
    cap = max(e, 1)
    buf = np.zeros((cap + slack + 1, 8), f32)
    th = -1.0 if e else 1e30
    rc = ctx.lib.ocean_whitecaps(ctx._h, tile, 0.0, th, *REGION, cap, buf.ctypes.data, (cap + 1) * 32)
    assert rc == oh.OK, ctx.lib.ocean_last_error()
    assert int(bits(buf[0])[1]) == e
    return buf


# (n, e): M = 0, 1, 63, 64, 65, 255, 256, 257, 700: the edges of a wave (64) and of a chunk (256), three chunks
SHAPES = [(0, 0), (0, 1), (40, 23), (64, None), (1, 64), (200, 55), (128, 128), (257, None), (400, 300)]


@pytest.mark.parametrize("C,flags", [(1, oh.F_VELOCITY), (3, oh.F_VELOCITY)])
def test_spray_physics_from_a_real_whitecap_list(C, flags):
    """A random pool and a real ocean_whitecaps list of the same context under gravity, drag, wind, jet and lift."""
    ctx = make_ctx(N, SCENES[C], flags)
    rng = np.random.default_rng(11)
    seen = set()
    for n, e in SHAPES:
        emitters = None if e is None else emitter_list(ctx, e)
        if emitters is not None and e >= 55:
            assert emitters[1:, 4:7].any() and (emitters[1:, 3] > 0).any()  # a velocity and foam to spawn from
        pool = random_pool(rng, n, n + (e or 0) + 3, float(PHYSICS[6]))
        for S in (1, 3):
            head, rec, died = restate_tagged(ctx, PHYSICS, pool, emitters, S, 2)
            assert head[2] == n + (e or 0)
            out = ctx.spray_step(PHYSICS, pool, emitters, S, 2)
            assert_pool(out, head, rec, f"C {C}, n {n}, e {e}, S {S}")
            seen.add(int(head[2]))
            if n + (e or 0) == 700:
                assert 0 < head[0] < 700  # survivors and retirees both
                assert (died[n:] == 0).any() and (died[:n] == 0).any()  # among the spawned and among the old
    assert seen == {0, 1, 63, 64, 65, 255, 256, 257, 700}
    ctx.close()


def test_spray_air_skip_changes_no_bit():
    """OCEAN_RAY_BOUNDS=0 (no skip, no bounds launches) and the default agree on the placed pool, whose heights
    straddle H by a few ulp."""
    cas = SCENES[3]
    a, _ = _ctx_with_env({"OCEAN_RAY_BOUNDS": "0"}, N, cas)
    b, _ = _ctx_with_env({}, N, cas)
    for c in (a, b):
        for t in (0.5, 1.0):
            c.step(t)
    for K in (0, 2):
        pool, cls = placed_pool(b, K)
        for S in (1, 4):
            oa, ob = a.spray_step(PLACED, pool, None, S, K), b.spray_step(PLACED, pool, None, S, K)
            np.testing.assert_array_equal(bits(oa), bits(ob))
            head, rec, _ = restate_tagged(b, PLACED, pool, None, S, K)
            assert_pool(oa, head, rec, f"no skip, K {K}, S {S}")
    # physics above and below H as well
    rng = np.random.default_rng(5)
    pool = random_pool(rng, 500, 600, 1.5)
    pool[1:501, 1] += f32(3.0) * (np.arange(500) % 2).astype(f32)  # every other one well above the water
    np.testing.assert_array_equal(bits(a.spray_step(PHYSICS, pool, None, 3, 2)), bits(b.spray_step(PHYSICS, pool, None, 3, 2)))
    a.close()
    b.close()


def dev(ctx, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, f32)).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    return t


def device_step(ctx, sp, pool, emitters, S, K, capacity=None, emit_capacity=None, extra=2, tile=0):
    """The device form into a sentinel-filled buffer with `extra` guard records behind it -> float32[..][8]."""
    import torch
    capacity = len(pool) - 1 if capacity is None else capacity
    dp = dev(ctx, pool)
    de = None if emitters is None else dev(ctx, emitters)
    ecap = 0 if emitters is None else (len(emitters) - 1 if emit_capacity is None else emit_capacity)
    o = torch.full(((capacity + 1 + extra) * 8,), float(SENTINEL), dtype=torch.float32, device=dp.device)
    torch.cuda.synchronize()
    ctx.spray_step_device(o.data_ptr(), sp, dp.data_ptr(), capacity, de.data_ptr() if de is not None else 0, ecap, S, K, tile)
    ctx.synchronize()
    return o.cpu().numpy().reshape(-1, 8)


HIGH = oh.OceanContext.spray_params(1.0 / 60.0, 9.81, 0.0, (0.0, 0.0, 0.0), 100.0, 1.0, 50.0)  # lift 50: the spawned fly


def test_spray_overflow_and_ownership():
    """A capacity below T: W = capacity, T counts every survivor, the first `capacity` survivors in candidate order are
    kept (the old before the spawned), and nothing beyond the buffer is written; without overflow the records past
    W are left alone too."""
    ctx = make_ctx(N, SCENES[3], oh.F_VELOCITY)
    rng = np.random.default_rng(2)
    cap = 100
    pool = random_pool(rng, cap, cap, 1.0)
    pool[1:, 1] = rng.uniform(20.0, 30.0, cap)  # high and young: all survive
    pool[2:40:3, 1] = -50.0  # ... but these
    emitters = emitter_list(ctx, 300)
    emitters[1:, 3] = np.maximum(emitters[1:, 3], f32(0.5))  # (foam for the lift)
    head, rec, died = restate_tagged(ctx, HIGH, pool, emitters, 2, 2)
    assert head[0] > cap == head[1] and head[2] == cap + 300 and len(rec) == cap
    buf = device_step(ctx, HIGH, pool, emitters, 2, 2)
    assert_pool(buf, head, rec, "overflow")
    np.testing.assert_array_equal(buf[cap + 1:], np.full((2, 8), SENTINEL))
    old = int((died[:cap] == 0).sum())
    assert 0 < old < cap
    np.testing.assert_array_equal(rec[:old, 7], pool[1:][died[:cap] == 0, 7])  # the old come first, in order
    np.testing.assert_array_equal(rec[old:, 7], emitters[1:][died[cap:] == 0][:cap - old, 7])
    # no overflow: records W + 1 .. capacity and the guards keep the sentinel
    big = oh.OceanContext.spray_pool(pool[1:], 600)
    head, rec, _ = restate_tagged(ctx, HIGH, big, emitters, 2, 2)
    assert head[0] == head[1] < 600
    buf = device_step(ctx, HIGH, big, emitters, 2, 2)
    assert_pool(buf, head, rec, "no overflow")
    np.testing.assert_array_equal(buf[1 + head[1]:], np.full((602 - head[1], 8), SENTINEL))
    ctx.close()


def test_spray_header_clamp():
    """A header that claims more than the capacity is clamped on the device.  The buffers really hold capacity + 8
    records (all of them live particles), so a kernel that trusted the header would stay inside the allocation and
    fail by value."""
    ctx = make_ctx(N, SCENES[3], oh.F_VELOCITY)
    rng = np.random.default_rng(9)
    cap, ecap = 70, 130
    pool = random_pool(rng, cap + 7, cap + 7, 1.0)
    pool[1:, 1] = rng.uniform(20.0, 30.0, cap + 7)
    emitters = emitter_list(ctx, ecap + 7)
    emitters[1:, 3] = np.maximum(emitters[1:, 3], f32(0.5))
    honest_pool, honest_emitters = pool.copy(), emitters.copy()
    bits(honest_pool[0])[1] = cap
    bits(honest_emitters[0])[1] = ecap
    bits(pool[0])[:3] = cap + 3
    bits(emitters[0])[:2] = ecap + 3
    want = device_step(ctx, HIGH, honest_pool, honest_emitters, 2, 2, capacity=cap, emit_capacity=ecap)
    head, rec, _ = restate_tagged(ctx, HIGH, honest_pool[:cap + 1], honest_emitters[:ecap + 1], 2, 2)
    assert head[2] == cap + ecap and head[0] == cap + ecap  # all survive, so an extra candidate would show in T
    assert_pool(want, head, rec, "honest headers")
    for p, e in ((pool, honest_emitters), (honest_pool, emitters), (pool, emitters)):
        got = device_step(ctx, HIGH, p, e, 2, 2, capacity=cap, emit_capacity=ecap)
        np.testing.assert_array_equal(bits(got), bits(want))
    ctx.close()


def test_spray_does_not_depend_on_the_launch_grid():
    """The launch is three chunks (capacity + emit_capacity = 768).  OCEAN_MAX_GROUPS=1: one workgroup walks them in
    order; 2: one workgroup walks chunks 0 and 2 and the other chunk 1, so the turn of the count's LDS buffers is taken
    with unequal shares.  Bit-equal to the default grid's."""
    cas = SCENES[3]
    b, _ = _ctx_with_env({}, N, cas, flags=oh.F_VELOCITY)
    for t in (0.5, 1.0):
        b.step(t)
    rng = np.random.default_rng(4)
    pool = random_pool(rng, 400, 468, 1.5)
    emitters = emitter_list(b, 300)
    assert (len(pool) - 1 + len(emitters) - 1 + 255) // 256 == 3
    for groups in ("1", "2"):
        a, _ = _ctx_with_env({"OCEAN_MAX_GROUPS": groups}, N, cas, flags=oh.F_VELOCITY)
        for t in (0.5, 1.0):
            a.step(t)
        for S in (1, 3):
            oa, ob = device_step(a, PHYSICS, pool, emitters, S, 2), device_step(b, PHYSICS, pool, emitters, S, 2)
            np.testing.assert_array_equal(bits(oa), bits(ob))
            head, rec, _ = restate_tagged(b, PHYSICS, pool, emitters, S, 2)
            assert_pool(oa, head, rec, f"{groups} workgroups, S {S}")
            assert 0 < head[0] < 700
        # ... and with a capacity that overflows (the emit kernel's early exit)
        small = oh.OceanContext.spray_pool(pool[1:61], 60)
        np.testing.assert_array_equal(bits(device_step(a, HIGH, small, emitters, 2, 2)),
                                      bits(device_step(b, HIGH, small, emitters, 2, 2)))
        assert a.kernel_name(2) == b.kernel_name(2) and "k_spray_emit" in a.kernel_name(2)
        a.close()
    b.close()


def test_spray_chaining():
    """One call of S = 4 equals four calls of S = 1 with the emitters in the first call only: T, W and the records
    (the header's M is each call's own)."""
    ctx = make_ctx(N, SCENES[3], oh.F_VELOCITY)
    rng = np.random.default_rng(6)
    pool = random_pool(rng, 300, 520, 1.5)
    emitters = emitter_list(ctx, 200)
    once = ctx.spray_step(PHYSICS, pool, emitters, 4, 2)
    chain = pool
    for s in range(4):
        chain = ctx.spray_step(PHYSICS, chain, emitters if s == 0 else None, 1, 2)
    ho, hc = bits(once[0]), bits(chain[0])
    assert 0 < ho[0] < 500
    np.testing.assert_array_equal(ho[[0, 1, 3]], hc[[0, 1, 3]])
    assert ho[2] == 500 and hc[2] < 500  # (the last link saw only the survivors of the third)
    np.testing.assert_array_equal(bits(once[1:1 + ho[1]]), bits(chain[1:1 + ho[1]]))
    ctx.close()


def test_spray_pipeline_forms_and_async_snapshot():
    """whitecaps_device -> spray_step_device with no host copy equals the host form fed the read-back list; the three
    forms agree; the async request made after step t1, with two more steps queued right behind it, holds t1's
    answer (a second context gives it)."""
    import torch
    cas = SCENES[3]
    ctx, ref = make_ctx(N, cas, oh.F_VELOCITY, times=(0.0, 0.25)), make_ctx(N, cas, oh.F_VELOCITY, times=(0.0, 0.25))
    ecap, cap = 512, 900
    rng = np.random.default_rng(8)
    pool = random_pool(rng, 300, cap, 1.5)
    # the pipeline on the device
    d_list = torch.zeros((ecap + 1) * 8, dtype=torch.float32, device=torch.device("cuda", 0))
    d_pool = dev(ctx, pool)
    d_out = torch.full(((cap + 1) * 8,), float(SENTINEL), dtype=torch.float32, device=d_pool.device)
    torch.cuda.synchronize()
    foam = ctx.surface_grid(*REGION, mode=oh.GRID_VERTICES)[..., 3]
    th = float(np.sort(foam.ravel())[-ecap // 2])  # about 256 of the 1200 nodes
    ctx.whitecaps_device(d_list.data_ptr(), th, *REGION, ecap)
    ctx.spray_step_device(d_out.data_ptr(), PHYSICS, d_pool.data_ptr(), cap, d_list.data_ptr(), ecap, 3, 2)
    ctx.synchronize()
    piped = d_out.cpu().numpy().reshape(-1, 8)
    lst = d_list.cpu().numpy().reshape(-1, 8)
    e = int(bits(lst[0])[1])
    assert 100 < e < ecap
    lst[1 + e:] = 0  # (unspecified in the library's output)
    host = ctx.spray_step(PHYSICS, pool, lst, 3, 2)
    w = int(bits(host[0])[1])
    assert 0 < w < 300 + e and bits(host[0])[2] == 300 + e
    np.testing.assert_array_equal(bits(piped[:1 + w]), bits(host[:1 + w]))
    head, rec, _ = restate_tagged(ctx, PHYSICS, pool, lst, 3, 2)
    assert_pool(host, head, rec, "pipeline")
    # the async form, snapshotting t1 behind later steps
    slot = oh.PinnedBuffer((cap + 1) * 32)
    rb = ctx.spray_step_async(PHYSICS, pool, lst, 3, 2, buf=slot)
    assert "k_spray_emit" in ctx.kernel_name(2)  # the last of the three launches
    pool_copy, lst_copy = pool.copy(), lst.copy()
    pool[:] = 0  # consumed before the call returned
    lst[:] = 0
    ctx.step(0.5)
    ctx.step(0.75)
    rb.wait()
    assert rb.done()
    total, cand, got = rb.spray()
    np.testing.assert_array_equal(bits(rb.view()[:1 + w]), bits(host[:1 + w]))
    assert (total, cand, len(got)) == (head[0], head[2], w)
    rb.release()
    slot.release()
    want = ref.spray_step(PHYSICS, pool_copy, lst_copy, 3, 2)
    np.testing.assert_array_equal(bits(want[:1 + w]), bits(host[:1 + w]))
    # frame t3: another answer
    later = ctx.spray_step(PHYSICS, pool_copy, lst_copy, 3, 2)
    assert not np.array_equal(bits(later), bits(host))
    ctx.close()
    ref.close()


def c_call(ctx, form, bufs, capacity=7, tile=0, nbytes=None, substeps=2):
    pool, out = bufs
    args = (ctx._h, tile, 2, substeps, PHYSICS.ctypes.data, ctypes.c_void_p(pool), capacity, None, 0, ctypes.c_void_p(out),
            ctypes.c_size_t((capacity + 1) * 32 if nbytes is None else nbytes))
    if form == "host":
        return ctx.lib.ocean_spray_step(*args), None
    if form == "device":
        return ctx.lib.ocean_spray_step_device(*args), None
    req = ctypes.c_void_p(0x1234)
    return ctx.lib.ocean_spray_step_async(*args, ctypes.byref(req)), req.value


def test_spray_tiles_contexts_and_errors():
    import torch
    # tile 1 of a two-tile context, against its own textures
    ctx = make_ctx(N, SCENES[3], tiles=2)
    rng = np.random.default_rng(12)
    pool = random_pool(rng, 300, 300, 1.5)
    outs = []
    for tile in (0, 1):
        head, rec, _ = restate_tagged(ctx, PHYSICS, pool, None, 3, 2, tile)
        out = ctx.spray_step(PHYSICS, pool, None, 3, 2, tile)
        assert_pool(out, head, rec, f"tile {tile}")
        assert 0 < head[0] < 300
        outs.append(out)
    assert not np.array_equal(bits(outs[0]), bits(outs[1]))
    # a context without OCEAN_F_VELOCITY spawns from +0 velocities, as its whitecap list says
    lst = emitter_list(ctx, 100, tile=1)
    assert not bits(lst[1:, 4:7]).any()
    head, rec, _ = restate_tagged(ctx, PHYSICS, pool, lst, 2, 2, 1)
    assert_pool(ctx.spray_step(PHYSICS, pool, lst, 2, 2, 1), head, rec, "no velocity")
    host = np.zeros((8, 8), f32)
    pinned = oh.PinnedBuffer(8 * 32)
    devbuf = torch.zeros(2 * 64 + 8, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    d0 = devbuf.data_ptr()
    bufs = {"host": (host.ctypes.data, host.ctypes.data), "async": (host.ctypes.data, pinned.ptr.value),
            "device": (d0, d0 + 8 * 32)}
    for form, b in bufs.items():
        for tile in (2, -1):
            assert c_call(ctx, form, b, tile=tile) == (oh.E_INVALID_ARG, None), (form, tile)
        assert c_call(ctx, form, b, nbytes=7 * 32) == (oh.E_INVALID_ARG, None), form
        rc, req = c_call(ctx, form, b)
        assert rc == oh.OK and (req is not None) == (form == "async"), form
        if req is not None:
            assert ctx.lib.ocean_readback_wait(ctypes.c_void_p(req)) == oh.OK
            ctx.lib.ocean_readback_release(ctypes.c_void_p(req))
    for off in (4, 8, 12):
        assert c_call(ctx, "device", (d0 + off, d0 + 8 * 32)) == (oh.E_INVALID_ARG, None)
        assert c_call(ctx, "device", (d0, d0 + 8 * 32 + off)) == (oh.E_INVALID_ARG, None)
    ctx.synchronize()
    ctx.close()
    # OCEAN_E_STATE before ocean_init_spectrum, after the argument checks
    raw = oh.OceanContext(N, 2, 1)
    for form, b in bufs.items():
        assert c_call(raw, form, b) == (oh.E_STATE, None), form
        assert c_call(raw, form, b, substeps=0) == (oh.E_INVALID_ARG, None), form
    with pytest.raises(oh.OceanError) as e:
        raw.spray_step(PHYSICS, pool)
    assert e.value.code == oh.E_STATE
    raw.close()
    # DISPLACEMENT_ONLY contexts are valid
    d = make_ctx(N, SCENES[3], oh.F_DISPLACEMENT_ONLY)
    head, rec, _ = restate_tagged(d, PHYSICS, pool, None, 3, 2)
    assert_pool(d.spray_step(PHYSICS, pool, None, 3, 2), head, rec, "displacement only")
    assert 0 < head[0] < 300
    d.close()
    # a column-parity shard holds half the columns: unsupported, as the queries
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    for form, b in bufs.items():
        assert c_call(par, form, b) == (oh.E_UNSUPPORTED, None), form
    par.close()
    pinned.release()


def test_spray_leaves_the_frames_unchanged():
    """Three frames with spray calls in between (all three forms) and three frames without: every texture is
    bit-equal, and the context that never asked launched none of the kernels."""
    cas = SCENES[3]
    flags = oh.F_VELOCITY
    a, b = make_ctx(N, cas, flags, times=()), make_ctx(N, cas, flags, times=())
    rng = np.random.default_rng(1)
    pool = random_pool(rng, 300, 400, 1.5)
    for t in (0.25, 0.5, 0.75):
        a.step(t)
        b.step(t)
        lst = emitter_list(a, 64)
        emitter_list(b, 64)
        a.spray_step(PHYSICS, pool, lst, 2, 2)
        rb = a.spray_step_async(PHYSICS, pool, lst, 2, 2)
        device_step(a, PHYSICS, pool, lst, 2, 2)
        rb.wait()
        rb.release()
    for tex in (oh.TEX_DISP, oh.TEX_DERIV, oh.TEX_TURB, oh.TEX_VELOCITY):
        np.testing.assert_array_equal(a.read_all(tex), b.read_all(tex))
    assert "spray" in a.kernel_name(2) and "spray" not in b.kernel_name(2)
    a.close()
    b.close()


# The child of test_spray_scratch_is_allocated_by_the_first_call: argv = the directories to import from.  It prints
# one JSON line, a list of rounds, each (bytes taken by a stretch without a spray call, by the stretch with the
# context's first one, by the stretch with its second one).
ALLOC_CHILD = r"""
import json, sys
sys.path[:0] = sys.argv[1:]
import numpy as np
import torch
import ocean_hip as oh
import oracle as O

cap = (1 << 18) - 1
sp = oh.OceanContext.spray_params(1.0 / 60.0)
pool = torch.zeros((cap + 1) * 8, dtype=torch.float32, device=torch.device("cuda", 0))
out = torch.empty((cap + 1) * 8, dtype=torch.float32, device=torch.device("cuda", 0))
torch.cuda.synchronize()

def make():
    ctx = oh.OceanContext(64, 2, 1, oh.F_VELOCITY)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[2:4])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    return ctx

def stretch(ctx, spray):
    ctx.step(0.5)
    ctx.surface_bounds()
    if spray:
        ctx.spray_step_device(out.data_ptr(), sp, pool.data_ptr(), cap)
    ctx.step(1.0)
    ctx.synchronize()

def free():
    return torch.cuda.mem_get_info(0)[0]

first = make()
stretch(first, True)  # every code object is loaded from here on
rounds = []
for _ in range(3):
    ctx = make()
    stretch(ctx, False)
    f0 = free()
    stretch(ctx, False)
    f1 = free()
    stretch(ctx, True)
    f2 = free()
    stretch(ctx, True)
    f3 = free()
    ctx.close()
    rounds.append((f0 - f1, f1 - f2, f2 - f3))
first.close()
print(json.dumps(rounds))
"""


def test_spray_scratch_is_allocated_by_the_first_call(tmp_path):
    """A context that never steps spray allocates no scratch, and nothing is allocated per call after the first
    (tests/test_gpu_whitecaps.py has the method: free device memory in a fresh process with the fragment allocator
    off, three rounds, one undisturbed round asked for).  The scratch of a pool of 2^18 - 1 with no emitters is 1024
    chunks x (256 x 32 B of records + 32 B of masks + 4 B of counts) + 16 B."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_DISABLE_FRAGMENT_ALLOCATOR="1")
    r = subprocess.run([sys.executable, "-c", ALLOC_CHILD, os.path.join(root, "ocean-simulation_amd"),
                        os.path.join(root, "oracle")], capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                       env=env)
    assert r.returncode == 0, r.stderr
    rounds = json.loads(r.stdout.strip().splitlines()[-1])
    scratch = 1024 * (256 * 32 + 32 + 4) + 16
    print("free-memory deltas per round (idle, first call, second call):", rounds, "scratch:", scratch)
    clean = [idle == 0 and scratch <= first <= scratch + (2 << 20) and second == 0 for idle, first, second in rounds]
    assert any(clean), rounds
