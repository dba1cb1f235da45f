"""GPU tests of sbx_atmosphere_eval (include/sbx.h): the Rayleigh/Mie solver over the caller's rays and the caller's sun, bit for bit
(NaN == NaN) against the oracle's hooks where u_time can make the sun and against tests/atmosphere_eval_model.py where it cannot;
the default kernel (fast forms on the waves whose rays qualify, csrc/sbx_atmosphere.h "CALLER'S RAYS"; the count of such waves is
asserted wherever it is compared) against the plain one; wave composition, ragged sizes, bounds, alignment, the ground app's sky, the argument checks."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import atmosphere_eval_model as M
from tests import atmosphere_ground_model as GM
from tests.app_checks import assert_same, frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu

FNS = ("get_incident_light", "get_sun_light")
# the families with the rays of A and B that lie in the class first: in this order the first wave (64 rays) runs the fast forms under
# every sun the host accepts, and the second one (the rest of the class, then everything outside it) the plain statement.  Every
# comparison below that is about the default kernel asserts that count in the same breath.
_ALL = M.families()
_FIRST = M.in_class(_ALL) & (np.arange(len(_ALL)) < 80)
RAYS = _ALL[np.concatenate([np.flatnonzero(_FIRST), np.flatnonzero(~_FIRST)])]
N_CLASS_AB = int(_FIRST.sum())
assert N_CLASS_AB >= 65 and M.in_class(RAYS[:N_CLASS_AB]).all() and not M.in_class(RAYS[64:128]).all()


@frame_cache
def hook_reference(fn, t):
    from tests.model_common import oracle
    o = oracle()
    return np.stack([o.kat("atmosphere." + fn, [1, 1, 0, 0, t, *r], 3) for r in RAYS])


@frame_cache
def model_reference(sun):
    return M.get_incident_light(RAYS, sun)


def sun_accepted(sun):
    """the host's part of the class (csrc/kern_atmosphere.hip atm_eval_sun_ok), in binary32"""
    s = np.asarray(sun, dtype=F)
    with np.errstate(all="ignore"):
        return bool(np.isfinite(s).all() and np.abs((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2] - F(1)) <= F(1e-4))


def ev(r, fn, rays, sun=(0.0, 1.0, 0.0)):
    return r.atmosphere_eval(fn, to_dev(rays), sun)


def counted(r, fn, rays, sun=(0.0, 1.0, 0.0)):
    """(out, waves that ran the fast forms): the same launch through include/sbx_test.h sbx_debug_atmosphere_eval"""
    return r.atmosphere_eval_counted(fn, to_dev(rays), sun)


def check_default(r, fn, sun, want, what):
    """the entry and its counted twin over RAYS against `want`; the first wave must have run the fast forms iff the sun is accepted"""
    assert differing(ev(r, fn, RAYS, sun), want) == 0, what
    out, waves = counted(r, fn, RAYS, sun)
    assert waves == (1 if fn == FNS[1] or sun_accepted(sun) else 0), (what, waves)
    assert differing(out, want) == 0, what
    return out.cpu().numpy()


def test_against_the_oracle_hooks(renderer):
    for t in M.TIMES:
        sun = tuple(GM.sun_dir(t))
        assert sun_accepted(sun)
        for fn in FNS:
            assert check_default(renderer, fn, sun, hook_reference(fn, t), (fn, t)).shape == (len(RAYS), 3)
    assert 0 <= GM.sun_dir(3.1)[1] < 1e-3 and GM.sun_dir(0.0)[1] == 1    # from the zenith to the horizon (grazing light rays, tau > 80);
    # u_time never puts the sun below it: (0, -1, 0) of M.SUNS does, in the next test


def test_against_the_model_with_suns_no_u_time_makes(renderer):
    assert [sun_accepted(s) for s in M.SUNS] == [True, True, True, False, False, False]
    for sun in M.SUNS:
        check_default(renderer, "get_incident_light", sun, model_reference(sun), sun)


def test_variants_same_bits_and_the_fast_forms_run(renderer, variant_restored):
    """default (a fast wave and a plain one, asserted) against variant 1 (no fast wave, asserted) on every sun of the two sweeps"""
    sweep = [(tuple(GM.sun_dir(t)), hook_reference(FNS[0], t)) for t in M.TIMES] + [(s, model_reference(s)) for s in M.SUNS]
    for fn in FNS:
        for sun, want in (sweep if fn == FNS[0] else [(sweep[0][0], hook_reference(fn, M.TIMES[0]))]):
            renderer.set_variant(0)
            a = check_default(renderer, fn, sun, want, (fn, sun))
            renderer.set_variant(1)
            b, waves = counted(renderer, fn, RAYS, sun)
            assert waves == 0
            assert differing(b, a) == 0 and differing(ev(renderer, fn, RAYS, sun), a) == 0, (fn, sun, "variant 1")
    renderer.set_variant(0)
    # the rays of A and B that satisfy the class's d2 bound ARE the class there: every wave of them, the ragged one too, is fast
    q = RAYS[:N_CLASS_AB]
    for fn in FNS:
        for t in (.37, 3.1):
            out, waves = counted(renderer, fn, q, tuple(GM.sun_dir(t)))
            assert waves == 2, (fn, t, waves)
            assert differing(out, hook_reference(fn, t)[:N_CLASS_AB]) == 0, (fn, t)
    # a sun the host refuses (not a unit vector, not finite) sends the whole launch to the plain kernel
    for bad in [(0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), 1.0, 0.0), (float("inf"), 0.0, 0.0), (1.0, .02, 0.0)]:
        assert counted(renderer, FNS[0], q, bad)[1] == 0, bad


def test_wave_composition_does_not_matter(renderer):
    n = len(RAYS)
    q = M.in_class(RAYS)
    yes, no = np.flatnonzero(q), np.flatnonzero(~q)
    # the two kinds merged evenly (each at its fraction of the way through its own list): every wave holds both
    keys = np.concatenate([np.arange(len(yes)) / len(yes), np.arange(len(no)) / len(no)])
    mixed = np.concatenate([yes, no])[np.argsort(keys, kind="stable")]
    assert sorted(mixed) == list(range(n))
    for w in range(0, n, 64):
        assert q[mixed[w:w + 64]].any() and not q[mixed[w:w + 64]].all()
    below = (0.0, -1.0, 0.0)
    cases = [(t, tuple(GM.sun_dir(t)), fn, hook_reference(fn, t)) for t in (2.0, 3.1) for fn in FNS]      # a high sun, one on the horizon
    cases.append(("below", below, FNS[0], model_reference(below)))                                         # and one below it
    for t, sun, fn, want in cases:
        base = check_default(renderer, fn, sun, want, (fn, t))
        for order in (np.arange(n)[::-1], mixed):
            got, waves = counted(renderer, fn, RAYS[order], sun)
            back = np.empty_like(base)
            back[order] = got.cpu().numpy()
            assert differing(back, base) == 0, (fn, t)
            assert waves == (0 if order is mixed else 1)                # reversed: the ragged last wave is all class
        for i in (0, 39, 63, 64, 80, 100, 103, 106, n - 1):             # one ray per call
            assert differing(ev(renderer, fn, RAYS[i:i + 1], sun), base[i:i + 1]) == 0, (fn, t, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; rays and out 4 bytes off their allocation's alignment"""
    sun = ctypes.cast((ctypes.c_float * 3)(*GM.sun_dir(.37)), ctypes.c_void_p)
    cases = [(fn, (6, 3), np.resize(RAYS, (n, 6)), np.resize(hook_reference(fn, .37), (n, 3))) for fn in FNS]
    check_ragged(renderer, raw_call(renderer, "atmosphere", mid=(sun,)), cases, n)


def test_same_solver_as_the_ground_app(renderer):
    """the sky pixels of a 64x36 atmosphere_ground frame = linear_to_srgb of the entry over the model's primary rays"""
    w, h = 64, 36
    fx = np.tile(np.arange(w, dtype=F) + F(.5), h)
    fy = np.repeat(np.arange(h, dtype=F) + F(.5), w)
    pcx, pcy = GM.point_cam(w, h, fx, fy)
    rd = GM.get_primary_ray(pcx, pcy, GM.EYE, GM.LOOK_AT)
    sky = GM.intersect_plane_t(rd) > GM.MAX_DIST
    assert 0 < sky.sum() < sky.size
    rays = np.concatenate([np.tile(np.array(GM.EYE, dtype=F), (w * h, 1)), np.stack(rd, axis=-1)], axis=1)[sky]
    for t in (.37, 2.0):
        frame = renderer.render("atmosphere_ground", w, h, t).cpu().numpy().reshape(w * h, 4)
        lin = ev(renderer, "get_incident_light", rays, tuple(GM.sun_dir(t))).cpu().numpy()
        assert_same(frame[sky][:, :3], GM.linear_to_srgb(lin), ("sky pixels", t))


def test_inside_a_stream_capture(renderer):
    """the call is one kernel launch and nothing else: recorded into a graph, it is replayed over other rays in the same buffers; the
    counted twin refuses the capturing stream"""
    sun = ctypes.cast((ctypes.c_float * 3)(*GM.sun_dir(.37)), ctypes.c_void_p)
    twin = raw_call(renderer, "atmosphere", mid=(sun,), counts=ctypes.byref(ctypes.c_uint(7)))
    check_capture_replay(renderer, partial(raw_call(renderer, "atmosphere", mid=(sun,)), FNS[0]), RAYS, hook_reference(FNS[0], .37), 3,
                         refused_twin=partial(twin, FNS[1]))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    rays = torch.from_numpy(RAYS[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 3), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr())
    sun = ctypes.cast((ctypes.c_float * 3)(0.0, 1.0, 0.0), ctypes.c_void_p)
    il, sl = b"get_incident_light", b"get_sun_light"
    assert lib.sbx_atmosphere_eval(None, il, rp, sun, op, 4, s) == -1
    bad_args = [(ctx, None, rp, sun, op, 4, s), (ctx, il, None, sun, op, 4, s), (ctx, il, rp, sun, None, 4, s), (ctx, il, rp, None, op, 4, s),
                (ctx, b"get_light", rp, sun, op, 4, s), (ctx, b"", rp, sun, op, 4, s), (ctx, il, rp, sun, op, (1 << 31) + 1, s)]
    check_refusals(renderer, lib.sbx_atmosphere_eval, None, bad_args, out)
    assert lib.sbx_atmosphere_eval(ctx, il, None, None, None, 0, s) == 0      # n == 0 touches nothing
    assert lib.sbx_atmosphere_eval(ctx, sl, None, None, None, 0, s) == 0
    assert lib.sbx_atmosphere_eval(ctx, sl, rp, None, op, 4, s) == 0          # get_sun_light reads no sun
    assert differing(out, M.get_sun_light(RAYS[:4])) == 0
    assert renderer.atmosphere_eval("get_incident_light", torch.zeros((0, 6))).shape == (0, 3)
    with pytest.raises(SbxError):
        renderer.atmosphere_eval("get_light", rays)
    assert lib.sbx_debug_atmosphere_eval(ctx, il, rp, sun, op, 4, None, s) == -1    # the hook needs a place for its count
    # not a render: the launch counter of sbx_stats stays where it is
    before = renderer.stats()["render_launches"]
    renderer.atmosphere_eval("get_incident_light", rays)
    assert renderer.stats()["render_launches"] == before
