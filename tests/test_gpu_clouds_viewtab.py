"""GPU tests of APP_CLOUDS' view table (csrc/kern_clouds.hip "the context's view table", csrc/sbx_ytab.hip clouds_view_table; DESIGN.md
§5.1): a launch that reads sky colour, phase and horizon weight from the context's per-camera table writes the frame a launch that
computes them per pixel writes, and the table forms, is kept, is given up and is refused exactly where include/sbx.h says.  Every
frame goes into a buffer poisoned with a NaN no kernel computes; every comparison is bit for bit (NaN == NaN) with the first launch of
a fresh context (which can hold no table), which is itself compared once with the per-lane kernel (sbx_set_variant 1) and, for the
shipped build, with the CPU oracle.  Frames of 97 x 55 and 130 x 67: ragged in both directions of the 32 x 2 wave tile, with the
horizon cut (dir.y < .05) inside the frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import aux_sets
from tests import clouds_builds_model as M
from tests.app_checks import assert_same
from tests.model_common import F, get_primary_ray, point_cam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.37
MOUSE = (300.0, 0.0)
SHAPES = [(97, 55), (130, 67)]
YZ = (0.0, 0.6, -0.8)
POISON = 0x7fc0beef
USED, OFF, INELIGIBLE, NEW_KEY, CAP, NO_SLOT, CAPTURE = 0, 1, 2, 3, 4, 5, 6       # include/sbx_test.h SBX_VIEWTAB_*
PIXEL_BYTES = 20


def aux_of(fields):
    import shaderbox_amd
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", dict(fields)).tobytes()) if fields else None


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.int32, device=r.tdev).view(torch.float32)


def launch(r, app, w, h, t, mouse=MOUSE, aux=None):
    """one launch into a poisoned buffer, finished -> the frame as a numpy array (no poison left)"""
    import torch
    out = r.render(app, w, h, t, mouse=mouse, aux=aux_of(aux), out=poisoned(r, w, h))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got.view(np.uint32) == POISON).any(), (app, w, h, t, "pixels left unwritten")
    return got


def state(r):
    """(table in use, refusal) of the context's last launch; the hook and the launch's record agree"""
    entries, built, used, why = r.clouds_viewtab()
    assert (used == 1) == (why == USED)
    return used, why


_REF = {}


def reference(app, w, h, t, mouse=MOUSE, aux=None):
    """the frame of a fresh context's first launch — no table of any kind can exist — checked once against the per-lane kernel and,
    for the shipped build, against the oracle"""
    key = (app, w, h, t, mouse, repr(sorted((aux or {}).items())))
    if key not in _REF:
        import shaderbox_amd
        r = shaderbox_amd.Renderer(0)
        try:
            first = launch(r, app, w, h, t, mouse, aux)
            assert r.clouds_viewtab()[1:3] == (0, 0)
            r.set_variant(1)
            assert_same(first, launch(r, app, w, h, t, mouse, aux), (key, "per-lane kernel"))
        finally:
            r.close()
        if app == "clouds":
            from oracle.oracle import APP_IDS
            from tests.model_common import oracle
            blk = aux_sets.block("clouds", dict(aux)) if aux else None
            assert_same(first, oracle().render(APP_IDS[app], w, h, t, mouse=mouse, aux=blk, threads=8), (key, "oracle"))
        first.setflags(write=False)
        _REF[key] = first
    return _REF[key]


@pytest.fixture
def fresh():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


def form(r, app, w, h, t=T, mouse=MOUSE, aux=None):
    """three launches of one key on a context that holds no table of it: the third builds and reads it"""
    want = reference(app, w, h, t, mouse, aux)
    for k in range(3):
        assert_same(launch(r, app, w, h, t, mouse, aux), want, (app, w, h, "launch", k + 1))
        assert state(r) == ((0, NEW_KEY) if k < 2 else (1, USED)), (app, w, h, k, r.clouds_viewtab())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_frames_hold_marching_and_sky_only_pixels(shape):
    w, h = shape
    fx = np.broadcast_to((np.arange(w, dtype=F) + F(.5))[None, :], (h, w)).ravel()
    fy = np.broadcast_to((np.arange(h, dtype=F) + F(.5))[:, None], (h, w)).ravel()
    pcx, pcy = point_cam(w, h, fx, fy, M.FOV)
    eye, look_at = M.setup_camera(MOUSE)
    marches = ~(get_primary_ray(pcx, pcy, eye, look_at)[1] < F(0.05))
    assert 0.2 * w * h < marches.sum() < 0.8 * w * h
    assert w % 32 and h % 2                                      # ragged in both directions of the wave tile


# ---- (a) formation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_formation(fresh, shape):
    w, h = shape
    form(fresh, "clouds", w, h)
    assert fresh.clouds_viewtab() == (w * h, 1, 1, USED)
    want = reference("clouds", w, h, T)
    for k in range(3):
        assert_same(launch(fresh, "clouds", w, h, T), want, ("later launch", k))
        assert fresh.clouds_viewtab() == (w * h, 1, 1, USED) and fresh.clouds_last_selection()["gt"] == 3
    # a row range reads the same table through its global rows
    import torch
    out = fresh.render("clouds", w, h, T, mouse=MOUSE, rows=(7, h - 5), out=poisoned(fresh, w, h)[7:h - 5])
    torch.cuda.synchronize()
    assert state(fresh) == (1, USED)
    assert_same(out, want[7:h - 5], "row range")


# ---- (b) time moves ------------------------------------------------------------------------------------------------------------------
def test_time_moves_and_the_table_stays(fresh):
    w, h = SHAPES[0]
    for k in range(6):
        t = T + k / 60.0
        assert_same(launch(fresh, "clouds", w, h, t), reference("clouds", w, h, t), ("u_time", t))
        assert state(fresh)[0] == (1 if k >= 2 else 0), k
    assert fresh.clouds_viewtab()[1] == 1
    # wind and the cloud parameters are no part of the key either
    for aux in ({"wind_dir": (0.3, 0.0, -1.0)}, {"cld_coverage": 0.45, "sigma_scattering": 0.2}):
        assert_same(launch(fresh, "clouds", w, h, T, aux=aux), reference("clouds", w, h, T, aux=aux), aux)
        assert state(fresh) == (1, USED) and fresh.clouds_viewtab()[1] == 1


# ---- (c) the key changes -------------------------------------------------------------------------------------------------------------
OTHER_KEYS = {"mouse": dict(mouse=(180.0, 0.0)), "sun_color": dict(aux={"sun_color": (1.0, 0.5, 0.2)}), "resolution": dict(shape=SHAPES[1])}


DRAINING = {(0, NO_SLOT), (1, USED)}       # what a launch of a due key may report while a slot drains: refused for want of a slot, or the table


@pytest.mark.parametrize("what", list(OTHER_KEYS))
def test_key_changes(fresh, what):
    a = dict(shape=SHAPES[0], mouse=MOUSE, aux=None)
    b = dict(a, **OTHER_KEYS[what])
    c = dict(a, mouse=(240.0, 0.0))

    def go(k, n, expect):
        (w, h) = k["shape"]
        for i in range(n):
            assert_same(launch(fresh, "clouds", w, h, T, k["mouse"], k["aux"]), reference("clouds", w, h, T, k["mouse"], k["aux"]), (what, i))
            assert state(fresh) in (expect[i] if isinstance(expect[i], set) else {expect[i]}), (what, i, fresh.clouds_viewtab())
    go(a, 3, [(0, NEW_KEY), (0, NEW_KEY), (1, USED)])
    go(b, 3, [(0, NEW_KEY), (0, NEW_KEY), (1, USED)])           # the first launches under the new key: no table, none of the old values
    assert fresh.clouds_viewtab()[1] == 2
    go(a, 2, [(1, USED), (1, USED)])                            # the first key's table is still there: two slots
    assert fresh.clouds_viewtab()[1] == 2
    # a third key takes the slot used least recently, b's — once the host has seen the events behind b's readers complete (every
    # launch here is finished before the next, so at the latest one launch after the events were recorded)
    go(c, 2, [(0, NEW_KEY), (0, NEW_KEY)])
    for attempt in range(3):
        go(c, 1, [DRAINING])
        if state(fresh) == (1, USED):
            break
    assert state(fresh) == (1, USED) and fresh.clouds_viewtab()[1] == 3
    go(a, 1, [(1, USED)])
    go(b, 1, [(0, NEW_KEY)])


# ---- (d) a camera that moves every launch ----------------------------------------------------------------------------------------------
def test_moving_camera_never_builds_a_table(fresh):
    w, h = SHAPES[0]
    for k in range(7):
        mouse = (300.0 + 4.0 * k, 0.0)
        assert_same(launch(fresh, "clouds", w, h, T + k / 60.0, mouse), reference("clouds", w, h, T + k / 60.0, mouse), ("moving", k))
        assert state(fresh) == (0, NEW_KEY)
    assert fresh.clouds_viewtab()[:2] == (0, 0) and fresh.clouds_hashtab()[3] == 1


# ---- (e) capture ---------------------------------------------------------------------------------------------------------------------
def captured(r, w, h):
    import torch
    out = poisoned(r, w, h)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            r.render("clouds", w, h, T, mouse=MOUSE, out=out)
    return out, g, r.clouds_viewtab()


def test_capture(fresh):
    import torch
    w, h = SHAPES[0]
    want = reference("clouds", w, h, T)
    out, g, st = captured(fresh, w, h)
    assert st[1:3] == (0, 0)                                     # a capture on a fresh context: nothing built, no table
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, want, "captured, fresh")
    form(fresh, "clouds", w, h)
    launch(fresh, "clouds", w, h, T)                            # the host sees the table complete
    out, g, st = captured(fresh, w, h)
    assert st == (w * h, 1, 1, USED)
    for k in range(2):
        out.view(torch.int32).fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        assert_same(out, want, ("replay", k))
    # the graph holds the table's address: two further keys take the other slot, never this one
    for aux in ({"sun_color": (0.9, 0.8, 0.7)}, {"sun_color": (1.0, 0.5, 0.2)}):
        for k in range(3):
            assert_same(launch(fresh, "clouds", w, h, T, aux=aux), reference("clouds", w, h, T, aux=aux), (aux, k))
    out.view(torch.int32).fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, want, "replay after two other keys")


# ---- (f) launches that never take a table ----------------------------------------------------------------------------------------------
def test_never_eligible(fresh):
    import torch
    w, h = SHAPES[0]
    want = reference("clouds", w, h, T)
    form(fresh, "clouds", w, h)
    pts = torch.tensor([[10.5, 40.5], [50.5, 3.5], [96.5, 54.5]], dtype=torch.float32, device=fresh.tdev)
    got = fresh.render_points("clouds", w, h, T, pts, mouse=MOUSE)
    torch.cuda.synchronize()
    assert state(fresh) == (0, INELIGIBLE)
    assert_same(got, np.stack([want[40, 10], want[3, 50], want[54, 96]]), "point list")
    frame = poisoned(fresh, w, h)
    for rank in range(2):                                        # two ranks' strips, in place
        fresh.render_rank_in_place("clouds", w, h, T, 8, rank, 2, frame, mouse=MOUSE)
        assert state(fresh) == (0, INELIGIBLE), rank
    torch.cuda.synchronize()
    assert_same(frame, want, "two ranks' strips")
    frame = poisoned(fresh, w, h)
    fresh.render_span_root("clouds", w, h, T, 8, 2, frame, mouse=MOUSE)      # a span launch
    torch.cuda.synchronize()
    assert state(fresh) == (0, INELIGIBLE)
    sky = launch(fresh, "clouds_sky", w, h, T)
    assert state(fresh) == (0, INELIGIBLE)
    assert_same(sky, reference("clouds_sky", w, h, T), "SKY_SPHERE")
    assert_same(launch(fresh, "clouds", w, h, T), want, "the table is still there")
    assert state(fresh) == (1, USED) and fresh.clouds_viewtab()[1] == 1


# ---- (g) builds and suns -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun", ["z", "yz"])
@pytest.mark.parametrize("app", ["clouds", "clouds_height", "clouds_luminance"])
def test_builds_and_suns(fresh, app, sun):
    w, h = SHAPES[1]
    aux = {"sun_dir": YZ} if sun == "yz" else None
    takes = {o: sun == "z" or o == "clouds_height" for o in ("clouds", "clouds_height", "clouds_luminance")}
    if takes[app]:
        form(fresh, app, w, h, aux=aux)
    else:
        # the y-z light march keeps its kernels: no table, however often the key is seen (profiles/clouds_viewtab_timing.txt)
        for k in range(4):
            assert_same(launch(fresh, app, w, h, T, aux=aux), reference(app, w, h, T, aux=aux), (app, sun, k))
            assert state(fresh) == (0, INELIGIBLE) and fresh.clouds_viewtab()[1] == 0
    rec = fresh.clouds_last_selection()
    assert (rec["gt"], rec["lm"]) == (3, 1 if app == "clouds_height" or sun == "z" else 2)
    # the builds share the table (under the y-z sun only HEIGHT, which has no light march, reads one)
    for other in ("clouds", "clouds_height", "clouds_luminance", "clouds_height"):
        assert_same(launch(fresh, other, w, h, T, aux=aux), reference(other, w, h, T, aux=aux), (app, other))
        if takes[app]:
            assert state(fresh) == ((1, USED) if takes[other] else (0, INELIGIBLE)) and fresh.clouds_viewtab()[1] == 1


# ---- (h) refusals ----------------------------------------------------------------------------------------------------------------------
def test_byte_cap(fresh):
    w, h = SHAPES[0]
    want = reference("clouds", w, h, T)
    fresh.set_clouds_viewtab_cap(w * h * PIXEL_BYTES - 1)
    for k in range(4):
        assert_same(launch(fresh, "clouds", w, h, T), want, ("under the cap", k))
        assert state(fresh) == (0, NEW_KEY if k < 2 else CAP)
    assert fresh.clouds_viewtab()[:2] == (0, 0)
    fresh.set_clouds_viewtab_cap(w * h * PIXEL_BYTES)
    assert_same(launch(fresh, "clouds", w, h, T), want, "at the cap")
    assert fresh.clouds_viewtab() == (w * h, 1, 1, USED)


CHILD = """
import sys
import numpy as np
import torch
import shaderbox_amd
r = shaderbox_amd.Renderer(0)
for k in range(4):
    out = r.render("clouds", %d, %d, %r, mouse=%r)
    torch.cuda.synchronize()
    print("state", r.clouds_viewtab())
np.save(sys.argv[1], out.cpu().numpy())
r.close()
"""


def test_switched_off_in_a_child_process(tmp_path):
    w, h = SHAPES[0]
    path = str(tmp_path / "frame.npy")
    env = dict(os.environ, SBX_CLOUDS_VIEWTAB="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", CHILD % (w, h, T, MOUSE), path], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.count("state (0, 0, 0, %d)" % OFF) == 4, p.stdout
    assert_same(np.load(path), reference("clouds", w, h, T), "SBX_CLOUDS_VIEWTAB=0")


# ---- (i) two streams over one context ------------------------------------------------------------------------------------------------
def test_two_streams_alternating(fresh):
    import torch
    w, h = SHAPES[1]
    keys = [None, {"sun_color": (0.9, 0.8, 0.7)}, {"sun_color": (1.0, 0.5, 0.2)}, None]
    wants = [reference("clouds", w, h, T, aux=a) for a in keys]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [poisoned(fresh, w, h) for _ in range(6 * len(keys))]
    torch.cuda.synchronize()
    frames, states = [], []
    for i, aux in enumerate(keys):                               # no host synchronisation anywhere in here
        for k in range(6):
            out = bufs[6 * i + k]
            with torch.cuda.stream(streams[k % 2]):
                fresh.render("clouds", w, h, T, mouse=MOUSE, aux=aux_of(aux), out=out)
            frames.append((i, k, out))
            states.append((i, k) + state(fresh))
    torch.cuda.synchronize()
    for i, k, out in frames:
        assert_same(out, wants[i], ("two streams", i, k))
    got_table = {}
    for i, k, used, why in states:
        if k < 2:
            # a new key — the returning first key included: its slot, the least recently used, was the one the third key was given
            assert (used, why) == (0, NEW_KEY), (i, k, used, why)
        elif i < 2:
            assert (used, why) == (1, USED), (i, k)              # two free slots for the first two keys
        else:
            # a slot is given up only once the host has SEEN its readers' events complete: until then the launch is refused, and
            # no second slot is sent after the first; once the key has its table it keeps it
            assert (used, why) in DRAINING, (i, k, used, why)
            assert used or not got_table.get(i), (i, k, "lost its table")
            got_table[i] = got_table.get(i) or used
    assert 2 <= fresh.clouds_viewtab()[1] <= 4
