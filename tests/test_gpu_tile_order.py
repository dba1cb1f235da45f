"""The DISPATCH ORDER (csrc/sbx_tile_order.h, kern_util.hip k_order_count / _scan / _place, sbx_device.h ordered_tile) tested
on its own: a wrong table is a wrong frame — a tile it lost is never written, a tile it names twice is written by two workgroups while
another is skipped.

1. the sort itself (include/sbx_test.h sbx_debug_order_build) on cost words no frame ever produced, against a few lines of numpy;
2. frames through a table at the smallest shapes that take one, none of them a multiple of the tile, every launch into a buffer
   full of NaN;
3. the host policy at those shapes: more shapes than a context keeps, the strips of two ranks, a moving scene, the per-lane
   kernel of APP_CLOUDS that takes no table;
4. the same for the seven builds that have an order grid (sbx_apps.h kApps).

The reference of the sort is tested on a hand-written case without a GPU (test_reference_of_the_sort_on_a_hand_written_case)."""
import numpy as np
import pytest

from tests.app_checks import bits_differ, same_tensor
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)

CLASSES = 1024                             # kern_util.hip ORDER_CLASSES: cost >> 6, the last one open
CHUNKS = 64                                # ORDER_G workgroups over contiguous chunks of the tiles
MIN_TILES = 4096                           # sbx_tile_order.h tile_order_begin: smaller launches take no table
TILE = {"clouds": (32, 2), "vinyl": (32, 8), "egg": (16, 4)}     # pixels per tile: clouds_grid / vinyl_grid / egg_grid
FAMILY = {"clouds": "clouds", "clouds_sky": "clouds", "clouds_height": "clouds", "clouds_luminance": "clouds",
          "vinyl": "vinyl", "vinyl_closeup": "vinyl", "vinyl_ridges": "vinyl", "vinyl_noshadow": "vinyl",
          "egg": "egg", "egg_straight": "egg", "egg_oval": "egg"}
T0 = 0.37


# ---- the reference of the sort ----------------------------------------------------------------------------------------------------
def classes_of(cost):
    """class 0 = the longest tiles: 1023 - min(cost >> 6, 1023)"""
    return (CLASSES - 1) - np.minimum(np.asarray(cost, dtype=np.uint32).astype(np.int64) >> 6, CLASSES - 1)


def encode(tiles, gx):
    tiles = np.asarray(tiles, dtype=np.int64)
    return ((tiles % gx) | ((tiles // gx) << 16)).astype(np.uint32)


def reference_segments(cost, gx, gy):
    """-> (count[class], the tiles class by class, increasing within a class — the ORDER within a class is not the kernel's promise)"""
    cls = classes_of(cost)
    assert cls.size == gx * gy
    return np.bincount(cls, minlength=CLASSES), np.argsort(cls, kind="stable")


def table_errors(table, cost, gx, gy):
    """what is wrong with `table` as the sorted order of `cost`: a list of strings, empty for a correct table"""
    n = gx * gy
    table = np.asarray(table, dtype=np.uint32)
    if table.size != n:
        return ["%d entries for %d tiles" % (table.size, n)]
    bad = []
    x, y = (table & 0xffff).astype(np.int64), (table >> 16).astype(np.int64)
    if (x >= gx).any() or (y >= gy).any():                               # (a) every entry a tile of the grid ...
        return ["an entry outside the %d x %d grid" % (gx, gy)]
    tiles = y * gx + x
    if not np.array_equal(np.sort(tiles), np.arange(n)):                 # ... and every tile exactly once
        bad.append("not a permutation: %d tiles missing" % (n - np.unique(tiles).size))
    cls = classes_of(cost)
    if (np.diff(cls[tiles]) < 0).any():                                  # (b) longest class first
        bad.append("classes decrease along the table")
    count, want = reference_segments(cost, gx, gy)                       # (c) every class's segment holds the reference's set
    segment = np.repeat(np.arange(CLASSES), count)                       # the class that owns each place of the table
    if not np.array_equal(tiles[np.lexsort((tiles, segment))], want):
        bad.append("a class's segment does not hold that class's tiles")
    return bad


def test_reference_of_the_sort_on_a_hand_written_case():
    """2 x 3 tiles, worked out by hand: a wrong reference must not agree with a wrong kernel"""
    gx, gy = 2, 3
    #       tile 0 (0,0)  1 (1,0)  2 (0,1)  3 (1,1)     4 (0,2)    5 (1,2)
    cost = [0,            64,      63,      0xffffffff, 1023 * 64, 128]
    assert classes_of(cost).tolist() == [1023, 1022, 1023, 0, 0, 1021]
    assert classes_of([1022 * 64 + 63, 1023 * 64 + 1, 65535, 65536]).tolist() == [1, 0, 0, 0]
    assert encode([0, 1, 2, 3, 4, 5], gx).tolist() == [0x00000, 0x00001, 0x10000, 0x10001, 0x20000, 0x20001]
    count, order = reference_segments(cost, gx, gy)
    assert order.tolist() == [3, 4, 5, 1, 0, 2]
    assert count.sum() == 6 and (count[0], count[1021], count[1022], count[1023]) == (2, 1, 1, 2)
    # the two tables the kernel may give for it, and tables it must not
    for good in ([3, 4, 5, 1, 0, 2], [4, 3, 5, 1, 2, 0]):
        assert table_errors(encode(good, gx), cost, gx, gy) == []
    assert table_errors(np.array([0x10001, 0x20000, 0x20001, 0x00001, 0x00000, 0x10000], dtype=np.uint32), cost, gx, gy) == []
    for wrong in ([3, 4, 5, 1, 0, 0],              # tile 2 lost, tile 0 twice
                  [3, 4, 5, 1, 0],                 # short
                  [3, 4, 1, 5, 0, 2],              # classes 1022 and 1021 the wrong way round
                  [0, 4, 5, 1, 3, 2],              # a permutation with a long tile at the end
                  [5, 1, 0, 2, 3, 4]):             # shortest first
        assert table_errors(encode(wrong, gx), cost, gx, gy) != [], wrong
    assert table_errors(np.array([0x00002, 0x20000, 0x20001, 0x00001, 0x00000, 0x10000], dtype=np.uint32), cost, gx, gy) != []   # x = gx
    assert table_errors(np.array([0x30000, 0x20000, 0x20001, 0x00001, 0x00000, 0x10000], dtype=np.uint32), cost, gx, gy) != []   # y = gy


# ---- 1. the sort on given cost words ----------------------------------------------------------------------------------------------
def cost_words(n):
    """name -> n cost words: what the sort's comment promises to survive, and the edges of its classes"""
    i = np.arange(n, dtype=np.int64)
    chunk = (n + CHUNKS - 1) // CHUNKS
    top = CLASSES * 64 + 63                                              # a little into the open last class
    ramp = (i * top // max(n - 1, 1)).astype(np.uint32)
    edges = np.array([63, 64, 1022 * 64 + 63, 1023 * 64, 1023 * 64 + 1], dtype=np.uint32)
    block = np.zeros(n, dtype=np.uint32)
    block[:max(1, chunk // 2)] = 64 * 300                                # one class with members in the first chunk and in no other
    words = {"zero": np.zeros(n, dtype=np.uint32),
             "saturated": np.full(n, 0xffffffff, dtype=np.uint32),
             "equal": np.full(n, 64 * 500, dtype=np.uint32),             # every chunk's cursor in one class
             "ramp up": ramp, "ramp down": ramp[::-1].copy(),
             "class edges": edges[np.random.default_rng(5).integers(0, 5, size=n)],
             "two classes": np.where(i % 2 == 0, 64 * 10, 64 * 700).astype(np.uint32),
             "first chunk": block}
    for seed in (1, 2, 3):
        words["random %d" % seed] = np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return words


@pytest.mark.gpu
@pytest.mark.parametrize("gx,gy", [(1, 1), (63, 1), (64, 1), (65, 1),    # the last chunks empty or of one tile
                                   (17, 241), (64, 64), (127, 33),       # 4097 tiles; every chunk full; neither
                                   (0xffff, 1), (1, 0xffff),             # the 16-bit limits of a packed entry
                                   (480, 270)])                          # the 129 600 tiles of a 4K APP_CLOUDS frame
def test_sort_gives_a_permutation_longest_class_first_whatever_the_cost_words_hold(renderer, gx, gy):
    for name, cost in cost_words(gx * gy).items():
        table = renderer.order_build(cost, gx, gy)
        assert table_errors(table, cost, gx, gy) == [], (name, gx, gy)


@pytest.mark.gpu
def test_sort_refuses_grids_a_packed_entry_cannot_hold(renderer):
    import shaderbox_amd
    for gx, gy in [(0, 1), (1, 0), (0x10000, 1), (1, 0x10000), (-1, 1), (1, -1)]:
        cost = np.zeros(max(gx * gy, 1), dtype=np.uint32)
        table = np.zeros_like(cost)
        rc = renderer.lib.sbx_debug_order_build(renderer.ctx, cost.ctypes.data, gx, gy, table.ctypes.data, None)
        assert rc == shaderbox_amd.SBX_ERR_ARG, (gx, gy, rc)


# ---- 2. frames through a table --------------------------------------------------------------------------------------------------
def grid_of(app, w, h):
    tw, th = TILE[FAMILY[app]]
    return (w + tw - 1) // tw, (h + th - 1) // th


POISON = 0x7fc0dead                        # a NaN no kernel computes (APP_VINYL has NaN pixels of its own, the oracle's too: 0x7fc00000)


def poisoned(r, w, h):
    """a frame buffer full of NaN, every channel POISON"""
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.int32, device=r.tdev).view(torch.float32)


def unwritten(frame):
    """#channels of `frame` that still hold the poison"""
    import torch
    return int((frame.view(torch.int32) == POISON).sum().item())


def launch(r, app, w, h, t):
    """one launch into a poisoned buffer, finished"""
    import torch
    out = r.render(app, w, h, t, out=poisoned(r, w, h))
    torch.cuda.synchronize()
    return out


def assert_permutation(table, gx, gy, what):
    assert table is not None and table.size == gx * gy, what
    x, y = (table & 0xffff).astype(np.int64), (table >> 16).astype(np.int64)
    assert (x < gx).all() and (y < gy).all(), what
    assert np.array_equal(np.sort(y * gx + x), np.arange(gx * gy)), what


def frames_through_a_table(r, app, w, h, t, through=2, most=8):
    """Launches of one shape on one stream, each into a poisoned buffer and finished before the next, until `through` of them ran
    under a table (one is there at the latest behind the third launch; `most` launches without one: the test exercised nothing).
    Every frame is launch 1's — which ran in plain order and left no poison — bit for bit; a tile the table lost stays poison.
    -> (launch 1's frame, the table)"""
    gx, gy = grid_of(app, w, h)
    assert gx * gy >= MIN_TILES and (w % TILE[FAMILY[app]][0] or h % TILE[FAMILY[app]][1]), (app, w, h)
    first, ordered, k = None, 0, 0
    while ordered < through:
        built = r.tile_order(app)[0] if first is not None else 0           # (adopts a table whose build has finished)
        assert built >= 1 or k < most, (app, w, h, "no table after %d launches" % k)
        got = launch(r, app, w, h, t)
        k += 1
        if first is None:
            first = got.clone()
            assert r.tile_order(app)[0] == 0, (app, w, h, "launch 1 runs in plain order")
            assert unwritten(first) == 0
        assert bits_differ(got, first) == 0, (app, w, h, "launch", k, "tables built", built)
        ordered += int(built >= 1 and k >= 4)                              # (the table is taken from the fourth launch in a row on a stream)
    built, _, table = r.tile_order(app)
    assert built >= 1
    assert_permutation(table, gx, gy, (app, w, h))
    return first, table


def plain_kernel_frame(r, app, w, h, t):
    """the frame of sbx_set_variant(1): APP_CLOUDS' per-lane kernel, which takes no table; APP_VINYL without culling"""
    r.set_variant(1)
    try:
        return launch(r, app, w, h, t)
    finally:
        r.set_variant(0)


@pytest.mark.gpu
@pytest.mark.parametrize("app,w,h", [("clouds", 520, 501), ("clouds", 543, 483), ("clouds_sky", 520, 501), ("clouds_sky", 543, 483),
                                     ("vinyl", 1000, 1051), ("egg", 500, 515)])
def test_frames_through_a_table_at_shapes_the_grid_does_not_divide(renderer, variant_restored, app, w, h):
    first, _ = frames_through_a_table(renderer, app, w, h, T0)
    if app != "egg":
        assert bits_differ(first, plain_kernel_frame(renderer, app, w, h, T0)) == 0, (app, w, h)
    if (app, w, h) == ("clouds", 520, 501):                              # pinned to the independent restatement too
        from oracle.oracle import APP_IDS
        from tests.model_common import oracle, same_bits
        want = oracle().render(APP_IDS["clouds"], w, h, T0, threads=16)
        assert same_bits(first.cpu().numpy(), want).all()


# ---- 3. the host policy -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_shapes_than_a_context_keeps_tables_for(renderer, variant_restored):
    """ten shapes of APP_CLOUDS round-robin (TILE_ORDER_KEYS = 8: the least recently used entry is replaced, and its buffer grows with
    the tile count), six launches each, twice over"""
    shapes = [(520, 501 + 2 * k) for k in range(10)]
    renderer.set_variant(1)
    want = {s: launch(renderer, "clouds", s[0], s[1], T0) for s in shapes}
    renderer.set_variant(0)
    for rnd in range(2):
        for w, h in shapes:
            for k in range(6):
                assert bits_differ(launch(renderer, "clouds", w, h, T0), want[(w, h)]) == 0, (rnd, w, h, k)
            assert renderer.tile_order("clouds")[0] >= 1, (rnd, w, h)
            assert_permutation(renderer.tile_order("clouds")[2], *grid_of("clouds", w, h), (rnd, w, h))


@pytest.mark.gpu
def test_strips_of_two_ranks_keep_their_own_tables(renderer):
    """in-place strips of ranks 0 and 1 of 2 through one context: each rank's rows are the one-launch frame's, no other row is written,
    and rank 0's table is still rank 0's after rank 1's run"""
    import torch
    from shaderbox_amd import shard
    w, h, br = 520, 1002, 8
    whole = launch(renderer, "clouds", w, h, T0)
    rows = {rank: torch.tensor(shard.rank_row_indices(h, br, rank, 2), device=renderer.tdev) for rank in (0, 1)}
    assert rows[0].numel() + rows[1].numel() == h
    for rank, launches in ((0, 8), (1, 8), (0, 3)):
        gx, gy = grid_of("clouds", w, rows[rank].numel())
        assert gx * gy >= MIN_TILES
        for k in range(launches):
            frame = poisoned(renderer, w, h)
            renderer.render_rank_in_place("clouds", w, h, T0, br, rank, 2, frame)
            torch.cuda.synchronize()
            same_tensor(frame[rows[rank]], whole[rows[rank]], (rank, k, "the rank's rows"))
            assert unwritten(frame[rows[1 - rank]]) == rows[1 - rank].numel() * w * 4, (rank, k, "a write outside the rank's rows")
        built, _, table = renderer.tile_order("clouds")
        assert built >= 1, rank
        assert_permutation(table, gx, gy, rank)


@pytest.mark.gpu
def test_moving_scene_rebuilds_behind_every_launch(renderer, variant_restored):
    """u_time changes with every launch (TILE_SCENE_REFRESH: a rebuild behind every launch, the pending table used at once on the
    stream of its build); launches back to back, nothing looks at a frame before the last one is queued"""
    import torch
    w, h = 520, 501
    for k in range(4):                                                   # (a table is current when the scene starts moving)
        launch(renderer, "clouds", w, h, T0)
    before = renderer.tile_order("clouds")[0]
    assert before >= 1
    times = [T0 + 0.01 * (k + 1) for k in range(12)]
    outs = [poisoned(renderer, w, h) for _ in times]
    torch.cuda.synchronize()
    for t, out in zip(times, outs):
        renderer.render("clouds", w, h, t, out=out)
    torch.cuda.synchronize()
    assert renderer.tile_order("clouds")[0] > before
    assert_permutation(renderer.tile_order("clouds")[2], *grid_of("clouds", w, h), "moving")
    for k in range(len(times)):                                          # (the issue asks for the last three; all twelve cost little more)
        assert bits_differ(outs[k], plain_kernel_frame(renderer, "clouds", w, h, times[k])) == 0, k


@pytest.mark.gpu
def test_per_lane_kernel_of_clouds_takes_no_table(renderer, variant_restored):
    """k_clouds_perlane launches on another grid than the one a table of APP_CLOUDS is built for (kern_clouds.hip launch_clouds_build):
    render_mapped keeps the two apart.  Six launches in a row under sbx_set_variant(1) build no table and count as no launch of the
    shape — in a context of its own, where any table would be theirs, and in the shared one, whose tables stay as they were"""
    w, h = 520, 501
    want = launch(renderer, "clouds", w, h, T0)
    fresh = type(renderer)(0)
    try:
        for r in (fresh, renderer):
            before = r.tile_order("clouds")
            r.set_variant(1)
            for k in range(6):
                assert bits_differ(launch(r, "clouds", w, h, T0), want) == 0, k
            after = r.tile_order("clouds")
            r.set_variant(0)
            assert after[:2] == before[:2]
            if r is fresh:
                assert after == (0, 0, None)
    finally:
        fresh.close()


# ---- 4. the builds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("app,w,h", [("clouds_height", 520, 501), ("clouds_luminance", 543, 483),
                                     ("vinyl_closeup", 1000, 1051), ("vinyl_ridges", 1000, 1051), ("vinyl_noshadow", 1000, 1051),
                                     ("egg_straight", 500, 515), ("egg_oval", 500, 515)])
def test_builds_take_a_table_of_their_own(renderer, variant_restored, app, w, h):
    """the seven builds with an order grid: sbx_debug_tile_order answers for them, a table IS built, frames through it are launch 1's"""
    shipped = FAMILY[app]
    shipped_before = renderer.tile_order(shipped)
    first, _ = frames_through_a_table(renderer, app, w, h, T0)
    after = renderer.tile_order(shipped)
    assert after[:2] == shipped_before[:2], "a build's launches are no launches of the shipped app"
    if shipped != "egg":
        assert bits_differ(first, plain_kernel_frame(renderer, app, w, h, T0)) == 0, (app, w, h)


@pytest.mark.gpu
def test_apps_without_an_order_grid_have_no_table(renderer):
    for app in ("raytracer_phong", "planet_unlit", "atmosphere_ground"):
        for _ in range(5):
            launch(renderer, app, 640, 416, T0)                          # 80 x 52 tiles of 8 x 8 pixels
        assert renderer.tile_order(app) == (0, 0, None), app
