"""CPU tests of the mesh hulls' arithmetic (ocean_body_hydrostatics; include/ocean/ocean.h): restate_hull, the numpy
statement of the entry that tests/test_gpu_hull.py compares the kernel with bit for bit, written from the header, and
pinned here in float64 over flat water by closed forms that share nothing with it: Archimedes on boxes clipped by an
independent polygon clipper (faces as quads, Sutherland-Hodgman, volume and centroid by the divergence theorem), a
regular tetrahedron dipped apex first, and the invariances and edge cases of the clip."""
import numpy as np
import pytest

import ocean_hip as oh

f32 = np.float32
f64 = np.float64
LANES = 256


def cross(u, a):
    """(u x a) as ocean.h writes it: each component p * q - r * s, in that order."""
    return (u[1] * a[2] - u[2] * a[1], u[2] * a[0] - u[0] * a[2], u[0] * a[1] - u[1] * a[0])


def tree_sum(pieces, dtype=f32, combine=np.add):
    """The reduction of ocean.h over the last axis: 256 lanes from +0; lane l takes its items k = l, l + 256, ... in
    ascending order and within an item the arrays of `pieces` in turn (a triangle's piece 1, then piece 2); then the
    upper half of the lanes is folded onto the lower half until one is left.  tree_sum of tests/test_body_abi.py with the
    width fixed at 256 and more than one term per item; `combine` is np.add or np.fmax."""
    pieces = [np.asarray(p, dtype) for p in pieces]
    n = pieces[0].shape[-1]
    t = np.zeros(pieces[0].shape[:-1] + (LANES,), dtype)
    for j0 in range(0, n, LANES):
        for p in pieces:
            c = p[..., j0:j0 + LANES]
            t[..., :c.shape[-1]] = combine(t[..., :c.shape[-1]], c)
    w = LANES
    while w > 1:
        w //= 2
        t = combine(t[..., :w], t[..., w:2 * w])
    return t[..., 0]


def place(vertices, bodies, dtype):
    """d (the vertices' offsets from the body origin, scaled and rotated) and w = c + d as tuples of [M][V] arrays, in
    ocean_body_buoyancy's operation order."""
    v = np.asarray(vertices, dtype)[None, :, :]
    b = np.asarray(bodies, dtype)[:, None, :]
    two = dtype(2.0)
    u, qw = (b[..., 3], b[..., 4], b[..., 5]), b[..., 6]
    a = (b[..., 7] * v[..., 0], b[..., 8] * v[..., 1], b[..., 9] * v[..., 2])
    t = tuple(two * c for c in cross(u, a))
    ut = cross(u, t)
    d = tuple((a[i] + qw * t[i]) + ut[i] for i in range(3))
    w = tuple(b[..., i] + d[i] for i in range(3))
    return d, w


def _piece(Q0, Q1, Q2, y0, y1, y2, dtype):
    """The eleven summed terms of one piece, in the record's order: F xyz, ar, Tq xyz, G xyz, Av.y."""
    half, three, twelve = dtype(0.5), dtype(3.0), dtype(12.0)
    e1 = tuple(Q1[i] - Q0[i] for i in range(3))
    e2 = tuple(Q2[i] - Q0[i] for i in range(3))
    av = tuple(half * c for c in cross(e1, e2))
    s = (y0 + y1) + y2
    p = s / three
    w0, w1, w2 = y0 + s, y1 + s, y2 + s
    mo = tuple(((Q0[i] * w0 + Q1[i] * w1) + Q2[i] * w2) / twelve for i in range(3))
    mc = cross(mo, av)
    ar = np.sqrt((av[0] * av[0] + av[1] * av[1]) + av[2] * av[2])
    g = tuple(ar * (((Q0[i] + Q1[i]) + Q2[i]) / three) for i in range(3))
    return [-(p * av[0]), -(p * av[1]), -(p * av[2]), ar, -mc[0], -mc[1], -mc[2], g[0], g[1], g[2], av[1]]


def restate_hull(vertices, triangles, bodies, lookup, dtype=f32):
    """ocean_body_hydrostatics in numpy, in ocean.h's operation order.  `lookup` maps q [M * V][2] to the [M * V][8]
    records of ocean_query_surface (height, -, -, r, ...).  Returns (out dtype[M][16], m int[M][T]: the number of wet
    vertices of every triangle).  A division by zero or an invalid operation raises: the header says none occurs."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    b = np.asarray(bodies, dtype)
    nb, nv = len(b), len(np.asarray(vertices))
    d, w = place(vertices, b, dtype)
    q = np.stack([w[0].ravel(), w[2].ravel()], axis=1)
    rec = np.asarray(lookup(q), dtype).reshape(nb, nv, 8)
    zero = dtype(0.0)
    with np.errstate(divide="raise", invalid="raise"):
        z, r = rec[..., 0] - w[1], rec[..., 3]
        idx = np.clip(tri, 0, nv - 1)  # what the device form's kernel does with an index it cannot trust
        P = [tuple(d[a][:, idx[:, k]] for a in range(3)) for k in range(3)]
        Z = [z[:, idx[:, k]] for k in range(3)]
        wet = [zz > zero for zz in Z]
        m = wet[0].astype(np.int64) + wet[1] + wet[2]
        first = np.where(m == 1, np.where(wet[0], 0, np.where(wet[1], 1, 2)),
                         np.where(m == 2, np.where(~wet[2], 0, np.where(~wet[0], 1, 2)), 0))

        def pick(j):
            sel = (first + j) % 3
            pos = tuple(np.where(sel == 0, P[0][a], np.where(sel == 1, P[1][a], P[2][a])) for a in range(3))
            return pos, np.where(sel == 0, Z[0], np.where(sel == 1, Z[1], Z[2]))

        (A, zA), (B, zB), (C, zC) = pick(0), pick(1), pick(2)

        def waterline(X, zx, Y, zy, mask):
            den = np.where(mask, zx - zy, dtype(1.0))
            assert (den > zero).all()  # zX > 0 >= zY whenever the quotient is formed
            t = np.where(mask, zx, zero) / den
            return tuple(X[i] + t * (Y[i] - X[i]) for i in range(3))

        AB, AC = waterline(A, zA, B, zB, m == 1), waterline(A, zA, C, zC, m == 1)
        BC, CA = waterline(B, zB, C, zC, m == 2), waterline(A, zA, C, zC, m == 2)
        o = np.zeros_like(zA)
        full = _piece(A, B, C, zA, zB, zC, dtype)
        tip = _piece(A, AB, AC, zA, o, o, dtype)
        quad1 = _piece(A, B, BC, zA, zB, o, dtype)
        quad2 = _piece(A, BC, CA, zA, o, o, dtype)
        out = np.zeros((nb, 16), dtype)
        for k, col in enumerate((0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 14)):
            one = np.where(m == 3, full[k], np.where(m == 1, tip[k], np.where(m == 2, quad1[k], zero)))
            two = np.where(m == 2, quad2[k], zero)
            out[:, col] = tree_sum([one, two], dtype)
        out[:, 7] = tree_sum([r], dtype, np.fmax)
        out[:, 11] = tree_sum([(m > 0).astype(dtype)], dtype)
        out[:, 12] = tree_sum([z], dtype, np.fmax)
        out[:, 13] = tree_sum([(z > zero).astype(dtype)], dtype)
    assert out.dtype == dtype
    return out, m


def flat(q):
    """The surface query's records over flat water at 0."""
    return np.zeros((len(q), 8), f64)


# ---- the independent closed forms ----

def rotation_matrix(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


BOX_FACES = ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))  # outward, corner = ix + 2 iy + 4 iz


def clip_below(poly):
    """Sutherland-Hodgman: the part of a polygon (a list of points) with y <= 0."""
    out = []
    for i, p in enumerate(poly):
        n = poly[(i + 1) % len(poly)]
        if p[1] <= 0:
            out.append(p)
        if (p[1] <= 0) != (n[1] <= 0):
            t = p[1] / (p[1] - n[1])
            out.append(p + t * (n - p))
    return out


def polygon_area_vector(poly):
    return sum((0.5 * np.cross(poly[i] - poly[0], poly[i + 1] - poly[0]) for i in range(1, len(poly) - 1)), np.zeros(3))


def clipped_box(size, body):
    """What Archimedes says of the box of `size`, posed by `body` (c, q, s), under flat water at y = 0, about the
    body origin c: (submerged volume, centre of buoyancy - c, wetted area, waterplane area)."""
    c, s = np.asarray(body[:3], f64), np.asarray(body[7:10], f64)
    R = rotation_matrix(body[3:7])
    corners = [R @ (s * np.asarray(size, f64) * (np.array([ix, iy, iz]) - 0.5)) + c
               for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]
    faces, cap = [], []
    for f in BOX_FACES:
        poly = clip_below([corners[i] for i in f])
        if len(poly) >= 3:
            faces.append(poly)
            cap += [p for p in poly if abs(p[1]) < 1e-13]
    wetted = sum(np.linalg.norm(polygon_area_vector(p)) for p in faces)
    closed, waterplane = list(faces), 0.0
    if len(cap) >= 3:
        mid = np.mean(cap, axis=0)
        cap.sort(key=lambda p: np.arctan2(p[2] - mid[2], p[0] - mid[0]))
        cap = [p for i, p in enumerate(cap) if np.linalg.norm(p - cap[i - 1]) > 1e-12]  # each point came from two faces
        if polygon_area_vector(cap)[1] < 0:
            cap.reverse()  # the lid looks up
        waterplane = polygon_area_vector(cap)[1]
        closed.append(cap)
    vol, moment = 0.0, np.zeros(3)
    for poly in closed:  # tetrahedra from the body origin over a fan of every face
        for i in range(1, len(poly) - 1):
            a, b2, c2 = poly[0] - c, poly[i] - c, poly[i + 1] - c
            v = np.dot(a, np.cross(b2, c2)) / 6.0
            vol += v
            moment += v * (a + b2 + c2) / 4.0
    return vol, (moment / vol if vol > 0 else np.zeros(3)), wetted, waterplane


def body(c=(0, 0, 0), q=(0, 0, 0, 1), s=(1, 1, 1)):
    q = np.asarray(q, f64)
    return np.concatenate([np.asarray(c, f64), q / np.linalg.norm(q), np.asarray(s, f64)])[None, :]


def close(got, want, scale=None, tol=1e-12):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    scale = np.linalg.norm(want) if scale is None else scale
    return np.abs(got - want).max() <= tol * scale


TILTED = [((2.0, 1.0, 3.0), (0.3, 0.1, -0.2), (0.31, -0.12, 0.2, 0.9), (1, 1, 1)),
          ((2.0, 1.0, 3.0), (5.0, -0.4, 7.0), (-0.5, 0.3, 0.1, 0.7), (1.5, 0.75, 0.5)),
          ((1.0, 1.0, 1.0), (0.0, 0.2, 0.0), (0.1, 0.9, -0.3, 0.2), (2.0, 3.0, 0.5)),
          ((3.0, 1.0, 2.0), (-1.0, 0.05, 2.0), (0.0, 0.0, 0.05, 1.0), (1, 1, 1))]


@pytest.mark.parametrize("case", range(len(TILTED)))
def test_tilted_boxes_against_archimedes(case):
    size, c, q, s = TILTED[case]
    verts, tris = oh.OceanContext.box_mesh(*size)
    assert verts.shape == (8, 3) and tris.shape == (12, 3)
    b = body(c, q, s)
    out, m = restate_hull(verts.astype(f64), tris, b, flat, f64)
    vol, cb, wetted, waterplane = clipped_box(size, b[0])
    assert 0 < vol < np.prod(size) * np.prod(s)  # partly submerged
    assert {1, 2} & set(m.ravel())  # and the clip was taken
    force = np.array([0.0, vol, 0.0])
    assert close(out[0, 0:3], force)
    assert close(out[0, 4:7], np.cross(cb, force), scale=np.linalg.norm(cb) * vol)
    assert close(out[0, 3], wetted)
    assert close(-out[0, 14], waterplane)
    assert out[0, 7] == 0 and out[0, 15] == 0
    assert out[0, 11] == (m > 0).sum() and out[0, 13] == (place(verts.astype(f64), b, f64)[1][1] < 0).sum()
    assert out[0, 12] == -place(verts.astype(f64), b, f64)[1][1].min()  # the draught: the deepest corner


def test_submerged_and_dry_boxes():
    size, q, s = (2.0, 1.0, 3.0), (0.31, -0.12, 0.2, 0.9), (1.0, 2.0, 0.5)
    verts, tris = oh.OceanContext.box_mesh(*size, 2, 1, 3)
    deep, _ = restate_hull(verts.astype(f64), tris, body((1, -10, 2), q, s), flat, f64)
    vol = 6.0
    assert close(deep[0, 0:3], [0, vol, 0])
    assert np.abs(deep[0, 4:7]).max() <= 1e-12 * 10 * vol  # the centre of buoyancy is the body origin
    assert close(deep[0, 3], 2 * (2 * 2 + 2 * 1.5 + 2 * 1.5))  # the scaled box is 2 x 2 x 1.5
    assert abs(deep[0, 14]) <= 1e-12 and deep[0, 11] == len(tris) and deep[0, 13] == len(verts)
    dry, m = restate_hull(verts.astype(f64), tris, body((1, 10, 2), q, s), flat, f64)
    assert not dry.any() and not m.any()
    assert not np.signbit(dry).any()  # +0 throughout


def test_regular_tetrahedron_apex_down():
    """Edge a, the apex down at depth dip, the base horizontal above the water: the submerged part is the tetrahedron
    scaled by k = dip / H (H = a sqrt(2/3)): volume k^3 V, waterplane k^2 A, wetted area 3 k^2 A, and its centroid is
    dip / 4 below the water, on the axis."""
    a, dip = 1.5, 0.4
    H, rad = a * np.sqrt(2.0 / 3.0), a / np.sqrt(3.0)
    ang = np.deg2rad([90.0, 210.0, 330.0])
    verts = np.array([[0.0, 0.0, 0.0]] + [[rad * np.cos(t), H, rad * np.sin(t)] for t in ang])
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])
    c = np.array([0.7, -dip, -0.3])  # the body origin is the apex
    # outward winding: the closed mesh's area vectors sum to zero and its signed volume is positive
    full, _ = restate_hull(verts, tris, body(c - [0, 50, 0]), flat, f64)
    vol_t, area_t = a ** 3 / (6 * np.sqrt(2.0)), np.sqrt(3.0) / 4 * a * a
    assert close(full[0, 0:3], [0, vol_t, 0]) and close(full[0, 3], 4 * area_t)
    out, m = restate_hull(verts, tris, body(c), flat, f64)
    k = dip / H
    assert sorted(m.ravel()) == [0, 1, 1, 1]
    assert close(out[0, 0:3], [0, k ** 3 * vol_t, 0])
    assert close(out[0, 3], 3 * k * k * area_t) and close(-out[0, 14], k * k * area_t)
    cb = np.array([0.0, 0.75 * dip, 0.0])  # from the apex
    assert close(out[0, 4:7], np.cross(cb, [0, k ** 3 * vol_t, 0]), scale=dip * vol_t)
    assert out[0, 12] == dip and out[0, 13] == 1 and out[0, 11] == 3


def test_subdivision_and_relabelling_do_not_change_the_record():
    """Flat water: the integral does not depend on how a face is cut, nor on which vertex a triangle names first.
    The box (3, 1, 2) puts every lattice point of (3, 2, 4) on a dyadic coordinate, exact in float32."""
    b = body((0.2, -0.1, 0.4), (0.2, 0.3, -0.1, 0.9), (1.25, 0.5, 2.0))
    v1, t1 = oh.OceanContext.box_mesh(3, 1, 2, 1, 1, 1)
    v2, t2 = oh.OceanContext.box_mesh(3, 1, 2, 3, 2, 4)
    assert v2.shape == (2 * (6 + 8 + 12) + 2, 3) and t2.shape == (4 * (6 + 8 + 12), 3)
    a, _ = restate_hull(v1.astype(f64), t1, b, flat, f64)
    c, m = restate_hull(v2.astype(f64), t2, b, flat, f64)
    assert {0, 1, 2, 3} <= set(m.ravel())
    sums = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 14]
    assert close(c[0, sums], a[0, sums])
    assert c[0, 12] == a[0, 12]
    for roll in (1, 2):
        r, _ = restate_hull(v2.astype(f64), np.roll(t2, roll, axis=1), b, flat, f64)
        assert close(r[0, sums], c[0, sums])
        np.testing.assert_array_equal(r[0, [7, 11, 12, 13, 15]], c[0, [7, 11, 12, 13, 15]])


def test_box_mesh_is_closed_and_outward():
    for dims in ((1, 1, 1), (3, 2, 4), (6, 6, 6), (8, 8, 4)):
        v, t = oh.OceanContext.box_mesh(2.0, 1.0, 3.0, *dims)
        s = dims[0] * dims[1] + dims[1] * dims[2] + dims[2] * dims[0]
        assert v.dtype == f32 and t.dtype == np.int32 and v.shape == (2 * s + 2, 3) and t.shape == (4 * s, 3)
        assert t.min() == 0 and t.max() == len(v) - 1 and len(np.unique(v, axis=0)) == len(v)
        p = v.astype(f64)[t]
        av = 0.5 * np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert np.abs(av.sum(axis=0)).max() < 1e-6  # closed
        assert (np.einsum("ij,ij->i", av, p.mean(axis=1)) > 0).all()  # every normal points away from the centre
        assert abs(np.einsum("ij,ij->i", av, p[:, 0]).sum() / 3 - 6.0) < 1e-5  # the volume, by the divergence theorem
    assert oh.OceanContext.box_mesh(1, 1, 1, 16, 16, 16)[0].shape == (1538, 3)
    with pytest.raises(ValueError):
        oh.OceanContext.box_mesh(1, 1, 1, 0, 1, 1)


@pytest.mark.parametrize("dtype", [f32, f64])
def test_a_vertex_on_the_surface_is_dry(dtype):
    """z = +0 and z = -0 are dry: the triangle with one vertex on the waterline is class m = 2, its pieces are cut at
    that very vertex (t = zB / (zB - 0) = 1), and nothing divides by zero."""
    verts = np.array([[0, -1, 0], [1, -1, 0], [0, 0, 1]], dtype)
    tris = np.array([[0, 1, 2]])
    b = body().astype(dtype)
    whole = dtype(0.5) * np.sqrt(dtype(2.0))
    for eta in (0.0, -0.0):
        out, m = restate_hull(verts, tris, b, lambda q: np.full((len(q), 8), eta), dtype)
        assert m.tolist() == [[2]] and out[0, 13] == 2 and out[0, 11] == 1
        assert abs(out[0, 3] - whole) <= 4 * np.finfo(dtype).eps  # the wetted area is the triangle's
        assert np.isfinite(out).all()
    # all three on the surface: dry
    out, m = restate_hull(verts * dtype(0), tris, b, flat, dtype)
    assert not m.any() and not out.any()


@pytest.mark.parametrize("dtype", [f32, f64])
def test_a_degenerate_triangle_adds_exactly_zero(dtype):
    verts, tris = oh.OceanContext.box_mesh(1, 1, 1)
    b = body((0.1, -0.2, 0.3), (0.2, -0.4, 0.1, 0.8)).astype(dtype)
    a, _ = restate_hull(verts.astype(dtype), tris, b, flat, dtype)
    more = np.concatenate([tris, [[0, 0, 0], [6, 1, 1], [2, 5, 2]]])  # a point, and two edges walked there and back
    c, m = restate_hull(verts.astype(dtype), more, b, flat, dtype)
    sums = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 14]
    np.testing.assert_array_equal(c[0, sums], a[0, sums])
    assert c[0, 11] == a[0, 11] + (m[0, 12:] > 0).sum()  # they are still counted as wet triangles


def test_tree_sum_order_written_out():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(600) * 10.0 ** rng.uniform(-3, 3, 600)).astype(f32)
    y = (rng.standard_normal(600) * 10.0 ** rng.uniform(-3, 3, 600)).astype(f32)
    lanes = [f32(0)] * LANES
    for k in range(600):
        lanes[k % LANES] = (lanes[k % LANES] + x[k]) + y[k]  # piece 1, then piece 2
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ s] for l in range(LANES)]  # the butterfly itself, every lane
    assert tree_sum([x, y]) == lanes[0] and len({float(v) for v in lanes}) == 1
    assert tree_sum([x], combine=np.fmax) == max(x.max(), f32(0))
    assert tree_sum([-np.abs(x)], combine=np.fmax) == 0  # the maxima start from 0
