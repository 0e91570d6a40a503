"""GPU tests of k_camera_bodies and k_camera_scene (csrc/view.hip) on the edge cases of the slab test and of the two
culls: the scenes of tests/test_camera_edges_scenes.py, whose CPU tests show on the oracle's textures that each holds
its case.  Here every check_* runs again over the context's own read-back textures, so each condition is asserted
before the comparison it guards, and then

  - the HITS and RANGE images of ocean_camera_bodies equal restate_camera_bodies', and the LINKS image of
    ocean_camera_scene equals restate_camera_scene's, bit for bit (te, nw and b of every body pixel, b1 and b2 of every
    water pixel);
  - the image of a context created with OCEAN_CAMERA_CULL=0 equals the default context's, bit for bit, in every mode
    the case runs;
  - where a case runs COLOR it is check_colour of tests/test_gpu_camera_bodies.py or tests/test_gpu_camera_scene.py.

One pair of contexts (cull on, cull off; n = 64, one cascade, two steps) serves the whole module."""
import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
import test_camera_edges_scenes as S
import test_gpu_camera_bodies as bodies_tests
import test_gpu_camera_scene as scene_tests
from test_camera_scene_abi import OPTICS, PAINT
from test_gpu_parity import _ctx_with_env
from test_gpu_query import Textures

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

K, STEPS, REFINE = S.K, S.STEPS, S.REFINE
HITS, RANGE, LINKS, COLOR = oh.CAMERA_HITS, oh.CAMERA_RANGE, oh.CAMERA_LINKS, oh.CAMERA_COLOR


@pytest.fixture(scope="module")
def pair():
    """(the default context, the one with every body a survivor of both culls, the textures, the bounds)."""
    cas = O.SCENE_CASCADES[:1]
    on, off = (_ctx_with_env(env, 64, cas)[0] for env in ({}, {"OCEAN_CAMERA_CULL": "0"}))
    for ctx in (on, off):
        ctx.step(0.5)
        ctx.step(1.0)
    yield on, off, Textures(on, cas), on.surface_bounds()
    on.close()
    off.close()


def compare_bodies(pair, out):
    """ocean_camera_bodies' HITS and RANGE images of both contexts against the restatement's (check_*'s `out`)."""
    on, off = pair[0], pair[1]
    for mode, want in ((HITS, out["hits"]), (RANGE, out["rng"])):
        got, blind = (ctx.camera_bodies(out["cam"], out["w"], out["h"], out["bodies"], out["box"], None, mode, None, 0, K,
                                        STEPS, REFINE) for ctx in (on, off))
        np.testing.assert_array_equal(got.reshape(want.shape), want)
        np.testing.assert_array_equal(blind, got)


def compare_links(pair, sc, want):
    """ocean_camera_scene's LINKS image of both contexts against restate_camera_scene's."""
    got, blind = (ctx.camera_scene(sc["cam"], sc["w"], sc["h"], sc["bodies"], sc["box"], None, sc["optics"], LINKS, sc["mat"],
                                   0, K, STEPS, REFINE) for ctx in pair[:2])
    np.testing.assert_array_equal(got.reshape(-1, 4), want)
    np.testing.assert_array_equal(blind, got)


def links_of(pair, sc):
    """The scene of an ocean_camera_bodies case under the scene tests' sun and optics: its LINKS image too."""
    sc = dict(sc, mat=S.sun_material(), optics=OPTICS)
    compare_links(pair, sc, S.restate_links(pair[2], sc)[0])


def test_rays_parallel_to_faces(pair):
    """db_i == 0 exactly, inside the slab, on its faces and beside it, on a column and a row of the image."""
    sc = S.parallels(pair[3])
    out, _ = S.check_parallels(pair[2], sc)
    compare_bodies(pair, out)
    links_of(pair, sc)


def test_eye_inside_two_boxes(pair):
    """tn < t0 at every pixel: te == t0, nw == -d, the lower index."""
    sc = S.inside_boxes(pair[3])
    out, _ = S.check_inside(pair[2], sc)
    compare_bodies(pair, out)
    links_of(pair, sc)


def test_window_cuts_bodies_at_both_ends(pair):
    """t0 = 40, t1 = 120: the cull's range clauses, and the slab test's tf >= t0 and tn <= t1; COLOR by the yardstick."""
    sc = S.window_boxes(pair[3])
    assert sc["w"] == bodies_tests.W and sc["h"] == bodies_tests.H and np.array_equal(sc["box"], bodies_tests.BOX)
    out, _ = S.check_window(pair[2], sc)
    compare_bodies(pair, out)
    links_of(pair, sc)
    mat = oh.material(roughness=0.3)
    got = bodies_tests.check_colour(pair[0], pair[2], sc["cam"], mat, sc["bodies"])
    blind = pair[1].camera_bodies(sc["cam"], sc["w"], sc["h"], sc["bodies"], sc["box"], bodies_tests.PAINT, COLOR, mat, 0, K,
                                  STEPS, REFINE)
    np.testing.assert_array_equal(blind.reshape(got.shape), got)


def test_ties_between_waves_and_between_chunks(pair):
    """Equal records in two waves of one chunk and in three chunks: the lowest index owns the pixels."""
    out, _ = S.check_ties(pair[2], S.tie_boxes(pair[3]))
    compare_bodies(pair, out)


def test_window_that_ends_before_it_starts(pair):
    """t1 < t0: no body is met; the early return lies in front of the barriers."""
    sc = S.backwards_window(pair[3])
    out, _ = S.check_backwards(pair[2], sc)
    compare_bodies(pair, out)
    links_of(pair, sc)


def test_wide_cones_and_bodies_all_around(pair):
    """Cones of 55 degrees and wider than 60 (no cull), bodies behind and beside the eye and around it; an image
    smaller than a tile and one of whole tiles only."""
    sc = S.shell(pair[3])
    outs, _ = S.check_shell(pair[2], sc)
    for k in S.CONE_IMAGES:
        compare_bodies(pair, outs[k])
    links_of(pair, dict(sc, cam=sc["cams"]["C"], w=5, h=3))
    links_of(pair, dict(sc, cam=sc["cams"]["D"], w=32, h=16))


def test_small_bodies_on_tile_borders(pair):
    """Boxes of one to three pixels, flat plates and mirrored boxes among them, on the borders between tiles."""
    out, _ = S.check_grazing(pair[2], S.grazing(pair[3]))
    compare_bodies(pair, out)


def test_quaternions_off_unit(pair):
    """|q|^2 - 1 = +-0.9 * 2^-10 (culled with the widened sphere) and +-2^-9 (survivors of every cull)."""
    sc = S.off_unit(pair[3])
    out, _ = S.check_off_unit(pair[2], sc)
    compare_bodies(pair, out)
    links_of(pair, sc)


def test_scene_sun_down_no_reach_and_a_long_light_vector(pair):
    """sun_up false; reach == 0 (rl = 0); |L| = 3 (rl = reach |L|), LINKS bit for bit and COLOR by the yardstick."""
    v = S.scene_variants(pair[3])
    for name, check in (("low_sun", S.check_low_sun), ("no_reach", S.check_no_reach), ("long_sun", S.check_long_sun)):
        want, _ = check(pair[2], v[name])
        compare_links(pair, v[name], want)
    sc = v["long_sun"]
    assert sc["w"] == scene_tests.W and sc["h"] == scene_tests.H and np.array_equal(sc["optics"], scene_tests.OPTICS)
    got, _ = scene_tests.check_colour(pair[0], pair[2], sc["cam"], sc["mat"], sc["bodies"])
    blind = pair[1].camera_scene(sc["cam"], sc["w"], sc["h"], sc["bodies"], sc["box"], PAINT, OPTICS, COLOR, sc["mat"], 0, K,
                                 STEPS, REFINE)
    np.testing.assert_array_equal(blind.reshape(got.shape), got)


def test_scene_tiles_with_one_water_pixel(pair):
    """pr == 0: the second cull's box of q is a point in three tiles."""
    sc = S.lonely_pixels(pair[3])
    want, _ = S.check_lonely_pixels(pair[2], sc)
    compare_links(pair, sc, want)


def test_scene_bodies_at_the_reach(pair):
    """The reach at the median distance of the mirror rays' nearest bodies: links and near misses within 5 % of it."""
    sc = S.at_the_reach(pair[2], pair[3])
    want, _ = S.check_at_the_reach(pair[2], sc)
    compare_links(pair, sc, want)
