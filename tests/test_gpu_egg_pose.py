"""GPU tests of SBX_APP_EGG_POSE (include/sbx.h): src/app_egg.h as shipped over the caller's pose, bit for bit
against tests/egg_pose_model.py and against the frames the reference header itself rendered with the fixture poses written into it
(tests/golden/egg_poses/): no block = SBX_APP_EGG; the four fixtures under the four kernel variants through rows, points, a rank
split and the 8-bit format; poses outside the domain of k_egg's culls (a NaN knee, a camera inside the bounding sphere, fov = 0,
non-finite values) into poisoned buffers; alternating poses; the dispatch-order table of a pose that stands still; host/sbx_render."""
import numpy as np
import pytest

from tests import egg_pose_model as M
from tests.app_checks import assert_same, bits_differ, check_rgba8, frame_cache, run_sbx_render, same_tensor
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu
APP = "egg_pose"
W, H = M.SIZE
POISON = -7.25


model_frame = frame_cache(lambda key, w, h: M.frame(M.scene_of(POSES[key]), w, h))
POSES = dict(M.POSES)
POSES["fov0"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), fov=0.)
POSES["eye_is_look_at"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), eye=(0., .25, 5.25), look_at=(0., .25, 5.25))
POSES["nan_eye"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), eye=(np.nan, .25, 5.25))
POSES["inf_fov"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), fov=np.inf)
POSES["tiny_fov"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), fov=1e-30)
POSES["far_eye"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), eye=(0., 3e19, 5.25), look_at=(0., 0., 0.))
POSES["nan_turn"] = M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), turn_deg=np.nan)
POSES["knee_on_foot"] = M.pose((0., 0., .2), (-.3, 1.1, -.2))          # the left foot at its pelvis: G = 0


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


@pytest.mark.parametrize("w,h", [(64, 36), (67, 35)])
def test_no_block_is_the_shipped_app(renderer, w, h):
    import shaderbox_amd
    for t in (0.0, 1.3, 7.77):
        egg = renderer.render("egg", w, h, t)
        same_tensor(renderer.render(APP, w, h, t), egg, ("NULL aux", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, aux=shaderbox_amd.egg_pose_default(t)), egg, ("the default block; u_time is not read", w, h, t))
    assert_same(renderer.render(APP, w, h, 1.3), M.frame(M.scene_of(M.default_pose(1.3)), w, h), ("the model", w, h))


@pytest.mark.parametrize("name", sorted(M.POSES))
def test_fixture_poses_are_the_reference(renderer, variant_restored, name):
    import torch
    from shaderbox_amd import shard
    fx, a = M.fixture(name), M.as_aux(M.POSES[name])
    for variant in (0, 1, 2, 3):
        renderer.set_variant(variant)
        whole = renderer.render(APP, W, H, 0.0, aux=a)
        assert_same(whole, fx["frame"], (name, "frame", variant))
        parts = [renderer.render(APP, W, H, 0.0, aux=a, rows=(r0, r1)) for r0, r1 in ((0, 5), (5, 24), (24, H))]
        same_tensor(torch.cat(parts), whole, (name, "rows", variant))
        assert_same(renderer.render_points(APP, W, H, 0.0, torch.from_numpy(fx["points"]), aux=a), fx["points_out"], (name, "points", variant))
    renderer.set_variant(0)
    n, br = 2, 8                                                      # one rank split, gathered and assembled
    rows_max = shard.rank_rows_max(H, br, n, 1, 1)
    gathered = torch.empty((n * rows_max, W, 4), dtype=torch.float32, device=renderer.tdev)
    for r in range(n):
        renderer.render_rank(APP, W, H, 0.0, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], aux=a, root_rounds=1, rounds=1)
    assert_same(renderer.assemble(gathered, W, H, br, n, root_rounds=1, rounds=1), fx["frame"], (name, "rank split"))
    assert_same(check_rgba8(renderer, APP, W, H, 0.0, aux=a), fx["frame"], (name, "the float frame beside the 8-bit one"))


@pytest.mark.parametrize("key", ["inside", "reach", "fov0", "eye_is_look_at", "nan_eye", "inf_fov", "tiny_fov", "far_eye", "nan_turn", "knee_on_foot"])
def test_poses_outside_the_culls_domain_into_a_poisoned_buffer(renderer, key):
    """67x35: ragged in both directions.  No poison is left and the frame is the model's, whatever it holds"""
    w, h = 67, 35
    out = renderer.render(APP, w, h, 0.0, aux=M.as_aux(POSES[key]), out=poisoned(renderer, w, h))
    got = out.cpu().numpy()
    assert not (got == F(POISON)).any(), key
    assert_same(got, model_frame(key, w, h), key)
    assert (got[..., 3] == 1).all()


def test_alternating_poses_keep_their_frames(renderer):
    a, b = M.as_aux(M.POSES["stride"]), M.as_aux(M.POSES["bones"])
    for _ in range(4):
        assert_same(renderer.render(APP, W, H, 0.0, aux=a), M.fixture("stride")["frame"], "stride")
        assert_same(renderer.render(APP, W, H, 0.0, aux=b), M.fixture("bones")["frame"], "bones")


def test_a_pose_that_stands_still_gets_a_table(renderer):
    """500x515: 32 x 129 tiles of 16 x 4, ragged.  Launch 1 runs in the kernel's own order; a table is there a few launches later and
    every frame keeps launch 1's bits (a tile the table lost would stay poison)"""
    import torch
    w, h = 500, 515
    a = M.as_aux(M.POSES["stride"])
    first, built = None, 0
    for k in range(10):
        got = renderer.render(APP, w, h, 0.0, aux=a, out=poisoned(renderer, w, h))
        torch.cuda.synchronize()
        if first is None:
            first = got.clone()
            assert not bool((first == POISON).any())
        assert bits_differ(got, first) == 0, ("launch", k + 1, "tables built", built)
        built = renderer.tile_order(APP)[0]
    assert built >= 1, "no dispatch-order table after 10 launches of one pose"
    built, _, table = renderer.tile_order(APP)
    assert table is not None and np.array_equal(np.sort((table >> 16).astype(np.int64) * 32 + (table & 0xffff)), np.arange(32 * 129))
    # another pose is another scene: its frame is its own
    b = M.as_aux(M.POSES["bones"])
    assert_same(renderer.render(APP, W, H, 0.0, aux=b), M.fixture("bones")["frame"], "bones after stride's table")


def test_sbx_render_app_egg_pose(tmp_path):
    """host/sbx_render --app egg_pose with every pose flag: the `stride` fixture; without flags: SBX_APP_EGG's frame of --time"""
    P = M.POSES["stride"]
    c = lambda v: ",".join(repr(float(x)) for x in v)  # noqa: E731
    flags = ("--pose-eye", c(P["eye"]), "--pose-look-at", c(P["look_at"]), "--pose-fov", repr(float(P["fov"])), "--turn", repr(float(P["turn_deg"])),
             "--left-foot", c(P["left_foot"]), "--right-foot", c(P["right_foot"]), "--femur", repr(float(P["femur"])), "--tibia", repr(float(P["tibia"])))
    assert_same(run_sbx_render(tmp_path, APP, W, H, 0.0, flags=flags), M.fixture("stride")["frame"], "--app egg_pose, stride")
    assert_same(run_sbx_render(tmp_path, APP, W, H, 1.3), M.frame(M.scene_of(M.default_pose(1.3)), W, H), "--app egg_pose, no flags")
