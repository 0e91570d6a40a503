"""The scenes of tests/test_gpu_camera_edges.py, and CPU tests that each scene holds the case it is named for.

k_camera_bodies and k_camera_scene (csrc/view.hip) reach the bits that include/ocean/ocean.h defines by culls, a
compaction and a stopped march; the edge cases of the definition (a ray parallel to a face, the eye inside a box, the
search window, ties, a quaternion off unit) and of the culls (wide cones, bodies behind the eye, tiles with one water
pixel, bodies at the reach) need inputs that random boxes under one pose never give.  Every builder here takes the
surface bounds and returns a scene (camera, image size, box, bodies); every check_* takes the textures, evaluates the
restatements (tests/test_camera_bodies_abi.py, tests/test_camera_scene_abi.py) over them, asserts the conditions that
make the scene a test of its case, and returns the images the device must give bit for bit with the counts it
measured.  The CPU tests run the checks over the oracle's textures (n = 64, one cascade, t = 1); the GPU tests run
the same checks over the device's own textures before they compare.  All constants were chosen here, on the oracle's
textures; the docstrings state them.

Where a condition needs tn, tf, db or a per-body `met`, slab_terms restates the slab test for one body with rot."""
import functools

import numpy as np

import ocean_hip as oh
import oracle as O
from test_camera_abi import camera_rays
from test_camera_bodies_abi import QUIET, body_pixels, restate_camera_bodies, rot
from test_camera_scene_abi import (BOX, OPTICS, SUN, link_shares, meet_rays, oracle_bounds, restate_camera_scene,
                                   scene_boxes)
from test_ray_abi import _oracle_textures

f32 = np.float32
K, STEPS, REFINE = 2, 32, 6
W, H = 45, 37  # the image of the neighbouring modules, which check_colour needs
UP = (0.0, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def oracle_scene(ncasc=1, n=64):
    """The oracle's textures of the GPU tests' context (n = 64, `ncasc` cascades, t = 1) and their bounds."""
    cas = O.SCENE_CASCADES[:ncasc]
    tex = _oracle_textures(n, cas, O.generate_noise(n, 20251121))
    return tex, oracle_bounds(tex)


def top_of(bounds):
    return float(bounds[:, 5].astype(np.float64).sum())


def pose(bounds, w, h, fov=0.9, t0=0.0, t1=400.0, up=4.0, pitch=8.0):
    """test_gpu_camera.pose_above with the image, the field of view, the window, the height over the highest crest
    the bounds allow and the pitch below the level left open."""
    eye = np.float64([3.0, top_of(bounds) + up, -4.0])
    ahead = np.float64([0.6, 0.0, 0.8])
    target = eye + 100.0 * ahead + np.float64([0.0, -100.0 * np.tan(np.radians(pitch)), 0.0])
    return oh.look_at_camera(eye, target, UP, fov, w, h, t0, t1)


# ---------------------------------------------------------------------------- restated parts of the kernels' inputs
def slab_terms(o, d, t0, t1, box, rec):
    """ocean.h's slab test of the rays (o, d [M][3]) against the one body `rec`, statement by statement as body_pixels
    makes them: db, ob, beside (db_i == 0), between, tn, tf, overlap (no axis beside and outside, tn <= tf), met."""
    o, d, rec = np.asarray(o, f32), np.ascontiguousarray(d, f32), np.asarray(rec, f32)
    lo, hi = np.asarray(box, f32)[:3], np.asarray(box, f32)[3:]
    c, u, qw, s = rec[0:3], rec[3:6], rec[6], rec[7:10]
    ob = rot(-u, qw, o - c)
    db = rot(-u, qw, d)
    l, h = s * lo, s * hi
    with np.errstate(**QUIET):
        a, e = (l - ob)[None, :] / db, (h - ob)[None, :] / db
    beside = db == 0
    between = (np.minimum(l, h) <= ob) & (ob <= np.maximum(l, h))
    n = np.where(beside, f32(-np.inf), np.minimum(a, e))
    f = np.where(beside, f32(np.inf), np.maximum(a, e))
    tn = np.maximum(np.maximum(n[:, 0], n[:, 1]), n[:, 2])
    tf = np.minimum(np.minimum(f[:, 0], f[:, 1]), f[:, 2])
    overlap = (~beside | between[None, :]).all(axis=1) & (tn <= tf)
    met = overlap & (tf >= f32(t0)) & (tn <= f32(t1)) & (not f32(t1) < f32(t0))
    return dict(db=db, ob=ob, beside=beside, between=between, tn=tn, tf=tf, overlap=overlap, met=met)


def body_spheres(box, bodies):
    """view.hip's body_sphere over every record, in its fp32 statements: r = ctr - c [B][3], rad, and qq, the |q|^2
    that decides `unit` (|qq - 1| <= 2^-10)."""
    b = np.asarray(bodies, f32)[:, :10]
    lo, hi = np.asarray(box, f32)[:3], np.asarray(box, f32)[3:]
    l, h = b[:, 7:10] * lo[None, :], b[:, 7:10] * hi[None, :]
    bc, e = f32(0.5) * (l + h), f32(0.5) * (h - l)
    hd = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    bc1 = (np.abs(bc[:, 0]) + np.abs(bc[:, 1])) + np.abs(bc[:, 2])
    u, w = b[:, 3:6], b[:, 6]
    qq = ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) + w * w
    r = np.stack([rot(u[k], w[k], bc[k]) for k in range(len(b))])
    rad = hd * f32(1.0 + 2.0 ** -8) + bc1 * f32(2.0 ** -7)
    assert r.dtype == f32 and rad.dtype == f32 and qq.dtype == f32
    return r, rad, qq


def _direction(cam, fi, fj):
    c = np.asarray(cam, f32)
    raw = (c[3:6] + f32(fi) * c[6:9]) + f32(fj) * c[9:12]
    return raw / np.sqrt((raw[0] * raw[0] + raw[1] * raw[1]) + raw[2] * raw[2])


def tile_cones(cam, w, h):
    """The cone of every 16 x 16 tile as view.hip's primary_body forms it, in fp32: {(ti, tj): (axis, ct, st)}."""
    out = {}
    for tj in range((h + 15) // 16):
        for ti in range((w + 15) // 16):
            i0, j0 = 16 * ti, 16 * tj
            ax = _direction(cam, f32(i0) + f32(7.5), f32(j0) + f32(7.5))
            ct, st = f32(1), f32(0)
            for c in range(4):
                e = _direction(cam, i0 + 15 * (c & 1), j0 + 15 * (c >> 1))
                x = np.stack([e[1] * ax[2] - e[2] * ax[1], e[2] * ax[0] - e[0] * ax[2], e[0] * ax[1] - e[1] * ax[0]])
                ct = min(ct, (e[0] * ax[0] + e[1] * ax[1]) + e[2] * ax[2])
                st = max(st, np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]))
            out[ti, tj] = (ax, f32(ct), f32(st))
    return out


def restate_images(tex, sc, bodies=None, cam=None):
    """The HITS and RANGE images of the scene by restate_camera_bodies, and its info."""
    cam = sc["cam"] if cam is None else cam
    bodies = sc["bodies"] if bodies is None else bodies
    w, h = sc["w"], sc["h"]
    hits, info = restate_camera_bodies(tex, cam, None, w, h, oh.CAMERA_HITS, K, STEPS, REFINE, sc["box"], None, bodies)
    rng, _ = restate_camera_bodies(tex, cam, None, w, h, oh.CAMERA_RANGE, K, STEPS, REFINE, sc["box"], None, bodies)
    return dict(cam=cam, w=w, h=h, box=sc["box"], bodies=bodies, hits=hits, rng=rng, info=info)


def _unit_quats(rng, count):
    q = rng.normal(size=(count, 4))
    return q / np.linalg.norm(q, axis=1)[:, None]


def _turn(q, a):
    """a [..][3] rotated by the unit quaternion q = (u, w), in float64."""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, a)
    return a + w * t + np.cross(u, t)


# ---------------------------------------------------------------------------- 1. exact parallels
QUATS = ((0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0))  # the identity and half turns about y and x: exact, db = +-d
KINDS = ("holds", "face_low", "face_high", "beyond_low", "beyond_high")


def parallels(bounds):
    """A camera of dyadic numbers: eye (3, Y, -4), Y the next multiple of 1/8 at or over 4 m above the highest crest,
    d00 = (-22/32, 18/32, 1), du = (1/32, 0, 0), dv = (0, -1/32, 0), 45 x 37: column 22 has d.x == 0 and row 18 has
    d.y == 0 exactly.  BOX, 27 bodies with the quaternions QUATS in turn, so db is +-d per component, -0 included.
    Twelve stand along column 22, one every three rows, each five columns wide; by KINDS in turn the world box's x
    interval holds the eye's x = 3 inside, has a face exactly at 3 (ob.x == l or == h: the <=), or begins 1/64 m
    beyond it, on either side.  Fifteen stand along row 18, one every three columns, the same in y about Y.  Below the
    level the boxes stand in front of the water.  Row 18 is level and over every crest, so it holds no water HIT pixel:
    its pixels that are no body pixels are MISS."""
    ey = float(np.ceil((top_of(bounds) + 4.0) * 8.0) / 8.0)
    cam = f32([3.0, ey, -4.0, -22 / 32, 18 / 32, 1.0, 1 / 32, 0, 0, 0, -1 / 32, 0, 0.0, 400.0])
    recs = []

    def place(lo_w, centre, kind, half_low, half_high):
        """The origin's coordinate: the world interval is [c - half_low, c + half_high]; `centre` where it would be
        centred; the eye's coordinate is `lo_w` (an exact number)."""
        if kind == "holds":
            return centre - 0.5 * (half_high - half_low)
        if kind == "face_low":
            return lo_w + half_low
        if kind == "face_high":
            return lo_w - half_high
        if kind == "beyond_low":
            return lo_w + half_low + 1 / 64
        return lo_w - half_high - 1 / 64

    for k, row in enumerate(range(1, 36, 3)):  # along column 22
        slope = (18 - row) / 32
        dist = 20.0 if slope >= 0 else min(20.0, 2.0 / -slope)
        q = QUATS[k % 3]
        sx, sy, sz = max(round(dist * 5 / 32 * 8) / 8, 0.125), dist * 3 / 32, 0.5
        cx = place(3.0, 3.0 + (0.25 if k % 2 else -0.25) * sx / 2, KINDS[k % 5], sx / 2, sx / 2)
        cy = ey + dist * slope + (0.25 if q[0] else -0.25) * sy
        recs.append([cx, cy, -4.0 + dist + 0.25, *q, sx, sy, sz])
    for k, col in enumerate(range(1, 45, 3)):  # along row 18
        dist = 10.0 + 2.0 * k
        q = QUATS[(k + 1) % 3]
        sx, sy, sz = dist * 3 / 32, round(dist * 4 / 32 * 8) / 8, 0.5
        down, upw = (0.75 * sy, 0.25 * sy) if q[0] else (0.25 * sy, 0.75 * sy)  # the half turn about x flips y
        cy = place(ey, ey + (0.2 if k % 2 else -0.2) * sy, KINDS[k % 5], down, upw)
        recs.append([3.0 + dist * (col - 22) / 32, cy, -4.0 + dist + 0.25, *q, sx, sy, sz])
    return dict(cam=cam, w=45, h=37, box=BOX, bodies=np.asarray(recs, np.float64).astype(f32))


def check_parallels(tex, sc):
    """At least 20 (pixel, body) pairs with some db_i == 0, `between` true on every such axis and the body met; at
    least 20 with db_i == 0 and `between` false on that axis where the neighbouring pixel across the zero line on the
    body's side meets the body (the plane of the parallel rays separates a box beside it from the other neighbour, so
    both neighbours never meet it); both kinds on both axes; a face exactly at the eye's coordinate among the first;
    column 22 holds body, water HIT and MISS pixels, row 18 body pixels and MISS pixels."""
    out = restate_images(tex, sc)
    w, h, info = sc["w"], sc["h"], out["info"]
    rays = camera_rays(sc["cam"], w, h)
    d = rays[:, 3:6].reshape(h, w, 3)
    assert (d[:, 22, 0] == 0).all() and (d[18, :, 1] == 0).all() and (d[:, 21, 0] != 0).all() and (d[17, :, 1] != 0).all()
    inside, outside, faces = np.zeros(3, int), np.zeros(3, int), 0
    for rec in sc["bodies"]:
        t = slab_terms(rays[0, 0:3], rays[:, 3:6], 0.0, 400.0, sc["box"], rec)
        beside, met = t["beside"].reshape(h, w, 3), t["met"].reshape(h, w)
        for axis in range(3):
            z = beside[..., axis]
            if not z.any():
                continue
            if t["between"][axis]:
                n = int((z & met & (~beside | t["between"][None, None, :]).all(axis=2)).sum())
                inside[axis] += n
                l, hh = rec[7 + axis] * sc["box"][axis], rec[7 + axis] * sc["box"][3 + axis]
                faces += n if t["ob"][axis] in (l, hh) else 0
            else:
                near = np.zeros((h, w), bool)
                if axis == 0:
                    near[:, 1:-1] = met[:, :-2] | met[:, 2:]
                    assert not (met[:, :-2] & met[:, 2:])[:, 21].any()
                else:
                    near[1:-1, :] = met[:-2, :] | met[2:, :]
                assert not (z & met).any()
                outside[axis] += int((z & near).sum())
    body, status = info["body"].reshape(h, w), info["rec"][:, 3].reshape(h, w)
    counts = dict(parallel_met=inside.tolist(), parallel_beside=outside.tolist(), on_a_face=faces,
                  column=(int(body[:, 22].sum()), int((~body & (status == oh.RAY_HIT))[:, 22].sum()),
                          int((~body & (status == oh.RAY_MISS))[:, 22].sum())),
                  row=(int(body[18].sum()), int((~body & (status == oh.RAY_MISS))[18].sum())))
    print("parallels:", counts)
    assert inside[2] == 0 and min(inside[:2]) >= 10 and inside.sum() >= 20 and min(outside[:2]) >= 10 and outside.sum() >= 20
    assert faces >= 10 and min(counts["column"]) >= 3 and min(counts["row"]) >= 5, counts
    return out, counts


# ---------------------------------------------------------------------------- 2. inside, windows and ties
def _scatter(cam, count, seed, w=W, h=H, radii=None, sides=(0.03, 0.09)):
    """test_gpu_camera_bodies.scatter_boxes' recipe with the distances given (default: 12 to 350 m, log-uniform)."""
    rng = np.random.default_rng(seed)
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (w - 1) / 2 + c[9:12] * (h - 1) / 2
    heading = np.arctan2(ahead[0], ahead[2])
    half = np.arctan(np.linalg.norm(c[6:9]) * w / 2)
    ang = heading + half * rng.uniform(-0.95, 0.95, count)
    r = 12.0 * (350.0 / 12.0) ** rng.uniform(0, 1, count) if radii is None else np.asarray(radii, np.float64)
    rec = np.empty((count, 10))
    rec[:, 0], rec[:, 2] = c[0] + r * np.sin(ang), c[2] + r * np.cos(ang)
    rec[:, 1] = rng.uniform(-2.0, 2.5, count)
    rec[:, 3:7] = _unit_quats(rng, count)
    rec[:, 7:10] = r[:, None] * rng.uniform(*sides, (count, 3))
    return rec.astype(f32)


def inside_boxes(bounds):
    """t0 = 0.25, the pose of pose_above: 40 scattered boxes, and at indices 3 and 7 two overlapping boxes of sides 4
    to 7 m, turned any way, that hold the eye; indices 0 to 2 are scattered boxes further off."""
    cam = pose(bounds, W, H, t0=0.25)
    bodies = _scatter(cam, 40, 21)
    q = _unit_quats(np.random.default_rng(22), 2)
    e = cam[0:3].astype(np.float64)
    bodies[3] = np.r_[e + [0.3, -0.2, 0.5], q[0], 6.0, 5.0, 7.0]
    bodies[7] = np.r_[e - [0.4, 0.1, 0.2], q[1], 4.0, 6.0, 5.0]
    return dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies)


def check_inside(tex, sc):
    """Every pixel is a body pixel of body 3 with te == t0 and nw == -d; body 7 is met from inside at every pixel too
    (tn < t0 <= tf), so the lower index wins a tie at every pixel."""
    out = restate_images(tex, sc)
    info, rays = out["info"], camera_rays(sc["cam"], sc["w"], sc["h"])
    for b in (3, 7):
        t = slab_terms(rays[0, 0:3], rays[:, 3:6], rays[0, 6], rays[0, 7], sc["box"], sc["bodies"][b])
        assert (t["met"] & (t["tn"] < f32(0.25)) & (t["tf"] >= f32(0.25))).all()
    assert info["body"].all() and (info["b"] == 3).all() and (info["te"] == f32(0.25)).all()
    np.testing.assert_array_equal(info["nw"], -rays[:, 3:6])
    np.testing.assert_array_equal(out["hits"][:, 4:7], -rays[:, 3:6])
    counts = dict(pixels_inside_both=len(rays))
    print("inside:", counts)
    return out, counts


def window_boxes(bounds):
    """t0 = 40, t1 = 120, the pose of pose_above: 300 boxes scattered from 12 to 350 m as scatter_boxes does, then 30
    at 40 m and 30 at 120 m from the eye, which straddle the two ends of the window."""
    cam = pose(bounds, W, H, t0=40.0, t1=120.0)
    bodies = np.concatenate([_scatter(cam, 300, 31), _scatter(cam, 30, 32, radii=np.full(30, 40.0), sides=(0.05, 0.1)),
                             _scatter(cam, 30, 33, radii=np.full(30, 120.0))])
    return dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies)


def check_window(tex, sc):
    """At least 10 bodies each: crossed by some pixel's ray but wholly nearer than t0 on every ray that crosses them;
    met with tn < t0 <= tf; met with tn <= t1 < tf; crossed but wholly beyond t1.  At least 20 body pixels have
    te == t0 with nw == -d, and bodies of each met class own pixels."""
    out = restate_images(tex, sc)
    info, rays = out["info"], camera_rays(sc["cam"], sc["w"], sc["h"])
    t0, t1 = rays[0, 6], rays[0, 7]
    near, cut0, cut1, far = [], [], [], []
    for b, rec in enumerate(sc["bodies"]):
        t = slab_terms(rays[0, 0:3], rays[:, 3:6], t0, t1, sc["box"], rec)
        g = t["overlap"] & (t["tf"] >= 0)
        if g.any() and (t["tf"][g] < t0).all():
            near.append(b)
        if g.any() and (t["tn"][g] > t1).all():
            far.append(b)
        if (t["met"] & (t["tn"] < t0)).any():
            cut0.append(b)
        if (t["met"] & (t1 < t["tf"])).any():
            cut1.append(b)
    owners = set(info["b"][info["body"]])
    started = info["body"] & (info["te"] == t0)
    np.testing.assert_array_equal(info["nw"][started], -rays[started, 3:6])
    counts = dict(wholly_near=len(near), cut_by_t0=len(cut0), cut_by_t1=len(cut1), wholly_far=len(far),
                  pixels_at_t0=int(started.sum()), owners_cut_by_t0=len(owners & set(cut0)),
                  owners_cut_by_t1=len(owners & set(cut1)), body_share=float(info["body"].mean()))
    print("window:", counts)
    assert min(len(near), len(cut0), len(cut1), len(far)) >= 10 and started.sum() >= 20, counts
    assert counts["owners_cut_by_t0"] >= 5 and counts["owners_cut_by_t1"] >= 5 and not owners & (set(near) | set(far))
    return out, counts


TIES = ((10, 200), (5, 261, 517))  # two waves of one chunk of 256; three chunks


def tie_boxes(bounds):
    """520 boxes scattered from 30 to 350 m, and two records repeated: a box 16 m ahead on the left at indices 10 and
    200 (lanes of waves 0 and 3 of the first chunk) and one 20 m ahead on the right at 5, 261 and 517 (three chunks)."""
    cam = pose(bounds, W, H)
    rng = np.random.default_rng(41)
    bodies = _scatter(cam, 520, 42, radii=30.0 * (350.0 / 30.0) ** rng.uniform(0, 1, 520))
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (W - 1) / 2 + c[9:12] * (H - 1) / 2
    flat = np.float64([ahead[0], 0.0, ahead[2]]) / np.hypot(ahead[0], ahead[2])
    side = np.float64([flat[2], 0.0, -flat[0]])
    q = _unit_quats(rng, 2)
    for where, (dist, off, size) in zip(TIES, ((16.0, -4.0, (3.0, 3.0, 3.0)), (20.0, 5.0, (4.0, 3.0, 2.0)))):
        at = c[0:3] + dist * flat + off * side
        for b in where:
            bodies[b] = np.r_[at[0], 1.0, at[2], q[TIES.index(where)], size]
    return dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies)


def check_ties(tex, sc):
    """Each repeated record is the nearest body of at least 20 pixels, the lowest of its indices owns every one of
    them, and at those pixels each repeat is met with the very te."""
    out = restate_images(tex, sc)
    info, rays = out["info"], camera_rays(sc["cam"], sc["w"], sc["h"])
    counts = {}
    for where in TIES:
        own = info["b"] == where[0]
        for b in where[1:]:
            np.testing.assert_array_equal(sc["bodies"][b], sc["bodies"][where[0]])
            assert not (info["b"] == b).any()
            t = slab_terms(rays[0, 0:3], rays[:, 3:6], rays[0, 6], rays[0, 7], sc["box"], sc["bodies"][b])
            assert t["met"][own].all() and (np.maximum(t["tn"], rays[0, 6])[own] == info["te"][own]).all()
        counts[where] = (int(own.sum()), int((own & info["body"]).sum()))
        assert counts[where][1] >= 20, counts
    print("ties:", counts)
    return out, counts


def backwards_window(bounds):
    """t1 = 10 < t0 = 50 over scatter_boxes' 300 boxes: no body is met."""
    sc = dict(cam=pose(bounds, W, H, t0=50.0, t1=10.0), w=W, h=H, box=BOX)
    sc["bodies"] = _scatter(sc["cam"], 300, 7)
    return sc


def check_backwards(tex, sc):
    """With the window [0, 400] the same bodies are met at a tenth of the pixels or more; with t1 < t0 at none."""
    out = restate_images(tex, sc)
    rays = camera_rays(sc["cam"], sc["w"], sc["h"])
    rays[:, 6], rays[:, 7] = 0.0, 400.0
    seen = float((body_pixels(rays, sc["box"], sc["bodies"])[0] >= 0).mean())
    print("backwards window: share of pixels that meet a body within [0, 400]:", seen)
    assert seen >= 0.1 and (out["info"]["b"] == -1).all() and not (out["hits"][:, 3] == oh.RAY_BODY).any()
    return out, dict(met_in_open_window=seen)


# ---------------------------------------------------------------------------- 3. cones
CONE_IMAGES = dict(A=(48, 48, 2.55), B=(16, 16, 2.6), C=(5, 3, 0.3), D=(32, 16, 1.0))


def shell(bounds):
    """The eye 6 m over the highest crest in the middle of 300 boxes in every direction, 8 to 60 m off (log-uniform),
    turned any way, each side 10 to 25 % of the distance; and 16 planks 40 x 0.6 x 0.6 m whose middle lies 3 m from
    the eye: their bounding spheres hold the eye and the boxes do not.  Four images from the one eye looking ahead and
    8.5 degrees down: A 48 x 48 at fov 2.55 rad, B 16 x 16 at 2.6 (one tile), C 5 x 3 at 0.3 (a partial tile, its cone that of the whole tile), D
    32 x 16 at 1.0 (whole tiles only)."""
    rng = np.random.default_rng(51)
    eye = np.float64([3.0, top_of(bounds) + 6.0, -4.0])
    n, planks = 300, 16
    dirs = rng.normal(size=(n + planks, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    r = np.r_[8.0 * (60.0 / 8.0) ** rng.uniform(0, 1, n), np.full(planks, 3.0)]
    q = _unit_quats(rng, n + planks)
    s = r[:, None] * rng.uniform(0.1, 0.25, (n + planks, 3))
    s[n:] = (40.0, 0.6, 0.6)
    bc = s * (0.5 * (BOX[:3] + BOX[3:]).astype(np.float64))[None, :]
    c = eye[None, :] + r[:, None] * dirs - _turn(q, bc)  # the box's centre lies at eye + r dir
    bodies = np.concatenate([c, q, s], axis=1).astype(f32)
    cams = {k: oh.look_at_camera(eye, eye + np.float64([60.0, -15.0, 80.0]), UP, fov, w, h, 0.0, 400.0)
            for k, (w, h, fov) in CONE_IMAGES.items()}
    return dict(cams=cams, box=BOX, bodies=bodies, cam=cams["A"], w=48, h=48)


def check_shell(tex, sc):
    """Image A holds tiles whose cone's half angle is between 40 and 60 degrees (ct in [0.5, cos 40]); image B's one
    tile has ct < 0.5; in every tile of every image at least 30 bodies lie behind the apex (dot(ctr - o, axis) < 0,
    in fp32 as the cull forms them); at least 10 bodies have the eye in their bounding sphere and not in their box;
    body pixels are a tenth of each image or more, and bodies that lie behind the axis of another tile own pixels."""
    r, rad, _ = body_spheres(sc["box"], sc["bodies"])
    bodies = sc["bodies"]
    outs, counts = {}, {}
    for k, (w, h, _) in CONE_IMAGES.items():
        cam = sc["cams"][k]
        one = dict(sc, cam=cam, w=w, h=h)
        outs[k] = restate_images(tex, one)
        info = outs[k]["info"]
        o = cam[0:3]
        v = (bodies[:, 0:3] - o[None, :]) + r
        cones = tile_cones(cam, w, h)
        behind = {t: (v[:, 0] * ax[0] + v[:, 1] * ax[1]) + v[:, 2] * ax[2] < 0 for t, (ax, _, _) in cones.items()}
        owners = np.unique(info["b"][info["body"]])
        counts[k] = dict(ct=[round(float(ct), 3) for _, ct, _ in cones.values()], behind=min(int(b.sum()) for b in behind.values()),
                         body_share=float(info["body"].mean()),
                         owners_behind_some_tile=int(np.any([b[owners] for b in behind.values()], axis=0).sum()))
        assert counts[k]["behind"] >= 30 and counts[k]["body_share"] >= 0.1, counts[k]
    dist = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    rays = camera_rays(sc["cams"]["A"], 1, 1)
    holds = [slab_terms(rays[0, 0:3], rays[:, 3:6], 0, 0, sc["box"], rec)["between"].all() for rec in bodies]
    counts["eye_in_sphere_not_in_box"] = int(((dist < rad) & ~np.asarray(holds)).sum())
    band = [ct for ct in counts["A"]["ct"] if 0.5 <= ct <= np.cos(np.radians(40.0))]
    counts["tiles_40_to_60_degrees"] = len(band)
    print("shell:", counts)
    assert len(band) >= 1 and counts["B"]["ct"][0] < 0.5 and len(counts["B"]["ct"]) == 1
    assert counts["eye_in_sphere_not_in_box"] >= 10 and counts["A"]["owners_behind_some_tile"] >= 10
    assert len(counts["C"]["ct"]) == 1 and len(counts["D"]["ct"]) == 2
    return outs, counts


# ---------------------------------------------------------------------------- 4. grazing
def _on_rays(cam, w, h, bounds, rng, count, far=150.0, snap=0):
    """`count` points in view, float64: each on the ray through a uniformly drawn image position, in the air over the
    highest crest the bounds allow; returns (points, distances).  The first `snap` positions are moved to within 0.6
    of a pixel of a border between two tiles, alternately a vertical and a horizontal one."""
    c = cam.astype(np.float64)
    fi, fj = rng.uniform(-0.5, w - 0.5, count), rng.uniform(-0.5, h - 0.5, count)
    for k in range(snap):
        f, size = (fi, w) if k % 2 else (fj, h)
        f[k] = 16.0 * rng.integers(1, (size + 15) // 16) - 0.5 + rng.uniform(-0.6, 0.6)
    d = c[3:6][None, :] + fi[:, None] * c[6:9][None, :] + fj[:, None] * c[9:12][None, :]
    d /= np.linalg.norm(d, axis=1)[:, None]
    room = np.where(d[:, 1] < 0, 0.8 * (c[1] - top_of(bounds)) / np.maximum(-d[:, 1], 1e-9), far)
    dist = np.maximum(rng.uniform(0.3, 1.0, count) * np.minimum(room, far), 3.0)
    return c[0:3][None, :] + dist[:, None] * d, dist


def grazing(bounds):
    """600 boxes over pose_above, each 1 to 2.4 pixels a side (one to three pixels across, the turn included), their
    centres on the rays of uniformly drawn image positions, a third of them moved to a border between tiles, in the
    air.  The first 60 are flat plates (one scale 0, so
    tn == tf on that axis), the next 60 mirrored (one scale negative, l > h)."""
    cam = pose(bounds, W, H)
    rng = np.random.default_rng(61)
    n = 600
    at, dist = _on_rays(cam, W, H, bounds, rng, n, snap=n // 3)
    pix = float(np.linalg.norm(cam[6:9].astype(np.float64)))
    q = _unit_quats(rng, n)
    s = dist[:, None] * pix * rng.uniform(1.0, 2.4, (n, 3))
    axis = rng.integers(0, 3, n)
    s[np.arange(60), axis[:60]] = 0.0
    s[np.arange(60, 120), axis[60:120]] *= -1.0
    bc = s * (0.5 * (BOX[:3] + BOX[3:]).astype(np.float64))[None, :]
    bodies = np.concatenate([at - _turn(q, bc), q, s], axis=1).astype(f32)
    return dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies)


def _tiles_of(info, w, h):
    """Per owning body: {tile: pixels it owns there}."""
    own = {}
    b, body = info["b"].reshape(h, w), info["body"].reshape(h, w)
    for j, i in zip(*np.nonzero(body)):
        t = own.setdefault(int(b[j, i]), {})
        t[i // 16, j // 16] = t.get((i // 16, j // 16), 0) + 1
    return own


def check_grazing(tex, sc):
    """At least 50 bodies own pixels in two or more tiles, at least 50 own exactly one pixel of some tile, and at least
    10 plates and 10 mirrored boxes own pixels."""
    out = restate_images(tex, sc)
    own = _tiles_of(out["info"], sc["w"], sc["h"])
    s = sc["bodies"][:, 7:10]
    assert ((s == 0).sum(axis=1) == 1)[:60].all() and ((s < 0).sum(axis=1) == 1)[60:120].all() and (s[120:] > 0).all()
    counts = dict(owners=len(own), in_two_tiles=sum(len(t) >= 2 for t in own.values()),
                  one_pixel_of_a_tile=sum(1 in t.values() for t in own.values()),
                  plates=sum(b < 60 for b in own), mirrored=sum(60 <= b < 120 for b in own),
                  body_share=float(out["info"]["body"].mean()))
    print("grazing:", counts)
    assert counts["in_two_tiles"] >= 50 and counts["one_pixel_of_a_tile"] >= 50 and counts["plates"] >= 10 and \
        counts["mirrored"] >= 10, counts
    return out, counts


# ---------------------------------------------------------------------------- 5. quaternions off unit
LONG_BOX = f32([2.0, -0.5, -0.5, 10.0, 0.5, 0.5])  # off centre by six lengths of its scale: bc is large
OFF_UNIT = (0.9 * 2.0 ** -10, -0.9 * 2.0 ** -10, 2.0 ** -9, -2.0 ** -9)  # |q|^2 - 1, by index modulo 4


def off_unit(bounds):
    """240 long thin boxes over pose_above, LONG_BOX scaled so that each is 4 to 10 pixels long and 1.5 to 3 pixels
    thick, its middle on the ray of a uniformly drawn image position, in the air; unit quaternions scaled by
    sqrt(1 + e), e = OFF_UNIT[b % 4]: inside kUnitQuat for b % 4 < 2, outside for the rest."""
    cam = pose(bounds, W, H)
    rng = np.random.default_rng(71)
    n = 240
    at, dist = _on_rays(cam, W, H, bounds, rng, n, far=120.0)
    pix = float(np.linalg.norm(cam[6:9].astype(np.float64)))
    q = _unit_quats(rng, n)
    s = dist[:, None] * pix * np.c_[rng.uniform(0.5, 1.25, n), rng.uniform(1.5, 3.0, (n, 2))]
    bc = s * (0.5 * (LONG_BOX[:3] + LONG_BOX[3:]).astype(np.float64))[None, :]
    q_off = q * np.sqrt(1.0 + np.float64(OFF_UNIT)[np.arange(n) % 4])[:, None]
    bodies = np.concatenate([at - _turn(q, bc), q_off, s], axis=1).astype(f32)
    return dict(cam=cam, w=W, h=H, box=LONG_BOX, bodies=bodies)


def check_off_unit(tex, sc):
    """By the fp32 qq of body_sphere: at least 100 bodies with |qq - 1| <= 2^-10 and at least 100 outside, none within
    2^-14 of the threshold, both signs in both classes; at least 20 of each class own pixels; a tenth of all bodies or
    more own a pixel in the first or last row or column of a tile."""
    out = restate_images(tex, sc)
    info, w, h = out["info"], sc["w"], sc["h"]
    _, _, qq = body_spheres(sc["box"], sc["bodies"])
    e = qq.astype(np.float64) - 1.0
    unit = np.abs(qq - f32(1)) <= f32(2.0 ** -10)
    assert (np.abs(np.abs(e) - 2.0 ** -10) > 2.0 ** -14).all()
    assert min((unit & (e > 0)).sum(), (unit & (e < 0)).sum(), (~unit & (e > 0)).sum(), (~unit & (e < 0)).sum()) >= 40
    pix = np.flatnonzero(info["body"])
    i, j = pix % w, pix // w
    edge = np.isin(i % 16, (0, 15)) | np.isin(j % 16, (0, 15))
    owners, at_edge = np.unique(info["b"][pix]), np.unique(info["b"][pix[edge]])
    counts = dict(unit=int(unit.sum()), off=int((~unit).sum()), unit_owners=int(unit[owners].sum()),
                  off_owners=int((~unit)[owners].sum()), owners_at_a_tile_edge=len(at_edge),
                  body_share=float(info["body"].mean()))
    print("off unit:", counts)
    assert counts["unit"] >= 100 and counts["off"] >= 100 and counts["unit_owners"] >= 20 and counts["off_owners"] >= 20
    assert len(at_edge) * 10 >= len(sc["bodies"]), counts
    return out, counts


# ---------------------------------------------------------------------------- 6. the scene's secondary rays
def sun_material(direction=SUN, length=1.0):
    """The material of the scene tests with the light towards `direction`, its length `length`."""
    m = oh.material(roughness=0.3, light_direction=direction)
    m[20:23] = (m[20:23].astype(np.float64) * length).astype(f32)
    return m


def restate_links(tex, sc):
    """The LINKS image of the scene by restate_camera_scene, and its info."""
    return restate_camera_scene(tex, sc["cam"], sc["mat"], sc["w"], sc["h"], oh.CAMERA_LINKS, K, STEPS, REFINE, sc["box"],
                                None, sc["optics"], sc["bodies"])


def _flat_frame(cam, w, h):
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (w - 1) / 2 + c[9:12] * (h - 1) / 2
    flat = np.float64([ahead[0], 0.0, ahead[2]]) / np.hypot(ahead[0], ahead[2])
    return c[0:3], flat, np.float64([flat[2], 0.0, -flat[0]])


LOW_SUN = (-0.55, -0.2, 0.35)


def scene_variants(bounds):
    """scene_boxes under pose_above, one thing varied at a time:
    low_sun:   the light towards LOW_SUN, L.y < 0;
    no_reach:  reach = 0, and a box 12 x 6 x 12 m standing in the water 22 m ahead, from 1.5 m under the mean level;
    long_sun:  the light towards SUN with length 3, OPTICS' reach of 120 m, and three towers 16 x 200 x 16 m that stand
               180, 220 and 260 m from the water 25, 45 and 70 m ahead, towards the sun: only shadow rays longer than 120 m reach
               them."""
    cam = pose(bounds, W, H)
    bodies = scene_boxes(cam, bounds, W, H)
    eye, flat, side = _flat_frame(cam, W, H)
    base = dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies, mat=sun_material(), optics=OPTICS)
    near = eye + 22.0 * flat
    tub = f32([[near[0], -1.5 + 0.25 * 6.0, near[2], 0, 0, 0, 1, 12, 6, 12]])
    sun = np.float64([SUN[0], 0.0, SUN[2]]) / np.hypot(SUN[0], SUN[2])
    feet = [eye + ahead * flat + dist * sun for ahead, dist in ((25.0, 180.0), (45.0, 220.0), (70.0, 260.0))]
    towers = f32([[p[0], 50.0, p[2], 0, 0, 0, 1, 16, 200, 16] for p in feet])
    return dict(low_sun=dict(base, mat=sun_material(LOW_SUN)),
                no_reach=dict(base, optics=oh.optics(shadow_color=(0.02, 0.03, 0.08), shadow_intensity=0.6, fog_density=0.15,
                                                     reach=0.0), bodies=np.concatenate([bodies, tub])),
                long_sun=dict(base, mat=sun_material(SUN, 3.0), bodies=np.concatenate([bodies, towers])))


def check_low_sun(tex, sc):
    """No pixel is shadowed although, with the sun mirrored over the horizon, at least 20 would be; at least 20 mirror
    links remain."""
    want, info = restate_links(tex, sc)
    s = link_shares(info)
    up = sc["mat"][20:23] * f32([1, -1, 1])
    would = int((meet_rays(info["q"], np.tile(up, (len(info["q"]), 1)), 0.0, sc["optics"][5], sc["box"], sc["bodies"])[0] >= 0).sum())
    print("low sun:", s, "shadowed under the mirrored sun:", would)
    assert sc["mat"][21] < 0 and s["shadowed"] == 0 and s["mirrored"] >= 20 and s["through"] >= 20 and would >= 20, s
    return want, dict(s, shadowed_if_up=would)


def check_no_reach(tex, sc):
    """reach = 0: every link of a water pixel has its q inside a box by the zero-length slab test.  A box that holds q
    is crossed by the ray from the eye in front of q, so such a pixel is a body pixel unless te == t*: the count of
    water points inside a box is what rounding leaves, and it is printed, not bounded from below.  The standing box is
    in the picture, and at least 20 water pixels see it through the water."""
    want, info = restate_links(tex, sc)
    s = link_shares(info)
    wp, q = info["wp"], info["q"]
    zero = np.zeros_like(q)
    zero[:, 1] = 1
    inside = meet_rays(q, zero, 0.0, 0.0, sc["box"], sc["bodies"])[0] >= 0
    linked = (info["sf"][wp] == 0) | (info["b2"][wp] >= 0)
    tub = len(sc["bodies"]) - 1
    counts = dict(s, water_points_inside_a_box=int(inside.sum()), linked=int(linked.sum()),
                  tub_pixels=int((info["b"][info["body"]] == tub).sum()), through_tub=int((info["b1t"][wp] == tub).sum()))
    print("no reach:", counts)
    assert sc["optics"][5] == 0 and not (linked & ~inside).any() and counts["tub_pixels"] >= 20 and counts["through_tub"] >= 20
    return want, counts


def check_long_sun(tex, sc):
    """|L| = 3: at least 20 water pixels are shadowed by a body that the ray q + s L meets only for s beyond reach / 3,
    which a ray of length `reach` would not reach; the scene keeps every kind of link (check_link_shares' shares)."""
    want, info = restate_links(tex, sc)
    s = link_shares(info)
    L = np.tile(sc["mat"][20:23], (len(info["q"]), 1))
    third = meet_rays(info["q"], L, 0.0, sc["optics"][5] / f32(3), sc["box"], sc["bodies"])[0] >= 0
    shadowed = info["sf"][info["wp"]] == 0
    counts = dict(s, length=float(np.linalg.norm(sc["mat"][20:23].astype(np.float64))),
                  shadowed_beyond_a_unit_ray=int((shadowed & ~third).sum()))
    print("long sun:", counts)
    assert abs(counts["length"] - 3.0) < 1e-6 and counts["shadowed_beyond_a_unit_ray"] >= 20
    assert min(s["shadowed"], s["through"], s["mirrored"], s["free"]) >= 20 and s["top"] >= 256, s
    return want, counts


HOLES = (5, 20, 40)  # the columns of row 31 that stay open, one per tile of the middle row of tiles


def lonely_pixels(bounds):
    """parallels' camera over scene_boxes, and 2 m in front of the eye five flat plates (z scale 0) across the view:
    one hides rows 0 to 30 whole, four hide row 31 but for the columns HOLES; rows 32 to 36 stay open.  Each of the
    three tiles of rows 16 to 31 has exactly one water HIT pixel, so the box of its q is a point (pr == 0).  The
    plates' edges lie half a pixel from the pixel centres."""
    cam = parallels(bounds)["cam"]
    ey = float(cam[1])
    plates = []

    def plate(x0, x1, y0, y1):
        plates.append([0.5 * (x0 + x1), y0 + 0.25 * (y1 - y0), -2.0, 0, 0, 0, 1, x1 - x0, y1 - y0, 0.0])

    def x_of(i):
        return 3.0 + 2.0 * (i - 22) / 32

    y30, y31 = ey + 2.0 * (18 - 30.5) / 32, ey + 2.0 * (18 - 31.5) / 32
    plate(-1.0, 7.0, y30, y30 + 5.0)
    edges = [-1.0] + [x_of(i + k) for i in HOLES for k in (-0.5, 0.5)] + [7.0]
    for x0, x1 in zip(edges[0::2], edges[1::2]):
        plate(x0, x1, y31, y30 + 0.01)
    bodies = np.concatenate([scene_boxes(cam, bounds, W, H), f32(plates)])
    return dict(cam=cam, w=W, h=H, box=BOX, bodies=bodies, mat=sun_material(), optics=OPTICS)


def check_lonely_pixels(tex, sc):
    """Tiles (0, 1), (1, 1) and (2, 1) hold exactly one water HIT pixel each, (HOLES[k], 31); rows 32 to 36 are water
    HIT pixels with links among them."""
    want, info = restate_links(tex, sc)
    water = info["water"].reshape(sc["h"], sc["w"])
    per_tile = {(ti, tj): int(water[16 * tj:16 * tj + 16, 16 * ti:16 * ti + 16].sum()) for tj in range(3) for ti in range(3)}
    s = link_shares(info)
    lonely = [t for t, n in per_tile.items() if n == 1]
    counts = dict(s, water_per_tile=per_tile, tiles_with_one_water_pixel=len(lonely))
    print("lonely pixels:", counts)
    assert len(lonely) >= 3 and all(water[31, i] for i in HOLES) and water[32:].all() and not water[:31].any()
    assert s["mirrored"] + s["shadowed"] + s["through"] >= 20
    return want, counts


def at_the_reach(tex, bounds):
    """scene_boxes under pose_above's pose in a 64 x 64 image, and over the water a roof 60 x 60 m, 0.4 m thick, that
    comes down from 9 m over the mean level 20 m ahead to the water 80 m ahead (slope 0.1457), so that the mirror rays
    of most water pixels meet it some 20 to 25 m from their q: many bodies, and this one for many pixels, sit at the
    reach.  The reach is set to the median, over the water pixels
    whose mirror ray meets a body at any distance, of the distance to the nearest body it meets (taken over `tex`)."""
    cam = pose(bounds, 64, 64)
    eye, flat, side = _flat_frame(cam, 64, 64)
    half = 0.5 * np.arctan(0.1457)
    q = np.r_[side * np.sin(half), np.cos(half)]
    q = q if _turn(q, flat)[1] < 0 else np.r_[-q[:3], q[3]]
    at = eye + 50.0 * flat
    roof = f32([[at[0], 5.0, at[2], *q, 60, 0.4, 60]])
    bodies = np.concatenate([scene_boxes(cam, bounds, 64, 64), roof])
    sc = dict(cam=cam, w=64, h=64, box=BOX, bodies=bodies, mat=sun_material(), optics=OPTICS)
    _, info = restate_links(tex, dict(sc, optics=oh.optics(reach=0.0)))
    b, te, _ = meet_rays(info["q"], info["rd"], 0.0, 3.0e38, sc["box"], sc["bodies"])
    reach = f32(np.median(te[b >= 0]))
    sc["optics"] = oh.optics(shadow_color=(0.02, 0.03, 0.08), shadow_intensity=0.6, fog_density=0.15, reach=float(reach))
    sc["mirror_te"] = np.where(b >= 0, te, f32(np.inf))
    return sc


def check_at_the_reach(tex, sc):
    """At least 50 mirror links with te2 in [0.95 reach, reach] and at least 50 mirror rays whose nearest body lies in
    (reach, 1.05 reach]."""
    want, info = restate_links(tex, sc)
    reach, te = sc["optics"][5], sc["mirror_te"]
    linked = info["b2"][info["wp"]] >= 0
    np.testing.assert_array_equal(linked, te <= reach)
    counts = dict(link_shares(info), reach=float(reach), links_within_5_percent=int((linked & (te >= 0.95 * reach)).sum()),
                  near_misses_within_5_percent=int((~linked & (te <= 1.05 * reach)).sum()))
    print("at the reach:", counts)
    assert counts["links_within_5_percent"] >= 50 and counts["near_misses_within_5_percent"] >= 50, counts
    return want, counts


# ---------------------------------------------------------------------------- the scenes over the oracle's textures
def test_parallels_scene_holds_exact_zeros_inside_and_beside_the_slabs():
    tex, bounds = oracle_scene()
    check_parallels(tex, parallels(bounds))


def test_inside_window_tie_and_backwards_scenes_hold_their_cases():
    tex, bounds = oracle_scene()
    check_inside(tex, inside_boxes(bounds))
    check_window(tex, window_boxes(bounds))
    check_ties(tex, tie_boxes(bounds))
    check_backwards(tex, backwards_window(bounds))


def test_shell_scene_holds_wide_cones_and_bodies_behind_the_eye():
    tex, bounds = oracle_scene()
    check_shell(tex, shell(bounds))


def test_grazing_scene_holds_bodies_across_tiles_plates_and_mirrored_boxes():
    tex, bounds = oracle_scene()
    check_grazing(tex, grazing(bounds))


def test_off_unit_scene_holds_both_classes_of_quaternions():
    tex, bounds = oracle_scene()
    check_off_unit(tex, off_unit(bounds))


def test_scene_variants_hold_their_cases():
    tex, bounds = oracle_scene()
    v = scene_variants(bounds)
    check_low_sun(tex, v["low_sun"])
    check_no_reach(tex, v["no_reach"])
    check_long_sun(tex, v["long_sun"])


def test_lonely_pixel_and_reach_scenes_hold_their_cases():
    tex, bounds = oracle_scene()
    check_lonely_pixels(tex, lonely_pixels(bounds))
    check_at_the_reach(tex, at_the_reach(tex, bounds))
