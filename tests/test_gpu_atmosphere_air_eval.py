"""GPU tests of sbx_atmosphere_air_eval (include/sbx.h): the Rayleigh/Mie solver over the caller's rays under the
caller's air, bit for bit (NaN == NaN) against tests/atmosphere_air_model.py under each fixture block and, with default solver
numbers, against sbx_atmosphere_eval; the default kernel (the fast body on the waves whose rays are of the class, only under a tame
block: csrc/sbx_atmosphere.h "CALLER'S AIR"; the count of such waves is asserted wherever it is compared) against the plain one; wave
composition, ragged sizes, bounds, alignment, a stream capture, the argument checks."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import atmosphere_air_model as M
from tests import atmosphere_eval_model as E
from tests.app_checks import frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev

pytestmark = pytest.mark.gpu

FNS = ("get_incident_light", "get_sun_light")
# tests/test_gpu_atmosphere_eval.py's order of the four families: the rays of A and B that lie in the class first, so that the first
# wave (64 rays) is all class and the second one is not
_ALL = E.families()
_FIRST = E.in_class(_ALL) & (np.arange(len(_ALL)) < 80)
RAYS = _ALL[np.concatenate([np.flatnonzero(_FIRST), np.flatnonzero(~_FIRST)])]
assert int(_FIRST.sum()) >= 65 and E.in_class(RAYS[:64]).all() and not E.in_class(RAYS[64:128]).all()

BLOCKS = dict(M.AIRS)
BLOCKS["default"] = M.default_air(.37)
BLOCKS["brighter"] = M.air(.37, sun_power=19.)                          # tame, not the literals
BLOCKS["odd_betas"] = M.air(.37, betaR=(5.5e-6, np.inf, 22.4e-6), betaM=(-21e-6, 0., 21e-6), hg_g=1.)   # tame: the betas enter no proof but the ballots'


@frame_cache
def reference(fn, key):
    return (M.get_incident_light if fn == FNS[0] else M.get_sun_light)(BLOCKS[key], RAYS)


def counted(r, fn, rays, key):
    return r.atmosphere_air_eval_counted(fn, to_dev(rays), M.as_aux(BLOCKS[key]))


def check_default(r, fn, key):
    """the entry and its counted twin over RAYS against the model; the first wave ran the fast body iff the block is tame"""
    want = reference(fn, key)
    assert differing(r.atmosphere_air_eval(fn, to_dev(RAYS), M.as_aux(BLOCKS[key])), want) == 0, (fn, key)
    out, waves = counted(r, fn, RAYS, key)
    assert waves == (1 if M.tame(BLOCKS[key]) else 0), (fn, key, waves)
    assert differing(out, want) == 0, (fn, key)
    return out.cpu().numpy()


@pytest.mark.parametrize("key", sorted(BLOCKS))
def test_against_the_model_and_variant_1(renderer, variant_restored, key):
    assert M.tier_of(BLOCKS[key], app=False) == (M.RUNTIME if key in ("sunset", "aloft", "default", "brighter", "odd_betas") else M.PLAIN)
    for fn in FNS:
        renderer.set_variant(0)
        a = check_default(renderer, fn, key)
        renderer.set_variant(1)
        b, waves = counted(renderer, fn, RAYS, key)
        assert waves == 0
        assert differing(b, a) == 0, (fn, key, "variant 1")
    renderer.set_variant(0)


def test_default_solver_numbers_are_sbx_atmosphere_eval(renderer):
    """the camera fields are not read; the sun is the block's"""
    for sun in E.SUNS + (M.sun(2., 40.),):
        A = M.air(0., sun_dir=sun, view=1, eye=(1., 2., 3.), fov=7., look_at=(0., 0., 0.))
        for fn in FNS:
            want = renderer.atmosphere_eval(fn, to_dev(RAYS), tuple(float(c) for c in A["sun_dir"])).cpu().numpy()
            got, waves = renderer.atmosphere_air_eval_counted(fn, to_dev(RAYS), M.as_aux(A))
            assert differing(got, want) == 0, (fn, sun)
            assert waves == (1 if M.sun_ok(sun) else 0), (fn, sun, waves)


def test_wave_composition_does_not_matter(renderer):
    n = len(RAYS)
    q = E.in_class(RAYS)
    yes, no = np.flatnonzero(q), np.flatnonzero(~q)
    keys = np.concatenate([np.arange(len(yes)) / len(yes), np.arange(len(no)) / len(no)])
    mixed = np.concatenate([yes, no])[np.argsort(keys, kind="stable")]          # every wave holds both kinds
    assert sorted(mixed) == list(range(n))
    for key in ("brighter", "sunset", "thin"):
        for fn in FNS:
            base = check_default(renderer, fn, key)
            for order in (np.arange(n)[::-1], mixed):
                got, waves = counted(renderer, fn, RAYS[order], key)
                back = np.empty_like(base)
                back[order] = got.cpu().numpy()
                assert differing(back, base) == 0, (fn, key)
                assert waves == (1 if order is not mixed and M.tame(BLOCKS[key]) else 0)      # reversed: the ragged last wave is all class


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; rays and out 4 bytes off their allocation's alignment"""
    for key in ("brighter", "coarse"):
        a = M.as_aux(BLOCKS[key])
        cases = [(fn, (6, 3), np.resize(RAYS, (n, 6)), np.resize(reference(fn, key), (n, 3))) for fn in FNS]
        check_ragged(renderer, raw_call(renderer, "atmosphere_air", lead=(ctypes.byref(a),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """the call is one kernel launch and nothing else: recorded into a graph, it is replayed over other rays in the same buffers; the
    counted twin refuses the capturing stream"""
    a = ctypes.byref(M.as_aux(BLOCKS["brighter"]))
    twin = raw_call(renderer, "atmosphere_air", lead=(a,), counts=ctypes.byref(ctypes.c_uint(7)))
    check_capture_replay(renderer, partial(raw_call(renderer, "atmosphere_air", lead=(a,)), FNS[0]), RAYS, reference(FNS[0], "brighter"), 3,
                         refused_twin=partial(twin, FNS[1]))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    rays = torch.from_numpy(RAYS[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 3), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr())
    good = M.as_aux(BLOCKS["brighter"])
    a = ctypes.byref(good)
    il, sl = b"get_incident_light", b"get_sun_light"
    assert lib.sbx_atmosphere_air_eval(None, il, a, rp, op, 4, s) == -1
    bad_args = [(ctx, None, a, rp, op, 4, s), (ctx, il, None, rp, op, 4, s), (ctx, il, a, None, op, 4, s), (ctx, il, a, rp, None, 4, s),
                (ctx, b"get_light", a, rp, op, 4, s), (ctx, b"", a, rp, op, 4, s), (ctx, il, a, rp, op, (1 << 31) + 1, s)]
    check_refusals(renderer, lib.sbx_atmosphere_air_eval, None, bad_args, out)
    for bad in (M.air(num_samples=0), M.air(num_samples=65), M.air(num_samples_light=0), M.air(num_samples_light=33), M.air(reserved0=1),
                M.air(reserved=(0., 0., 1., 0., 0., 0.))):
        assert M.refused(bad, app=False) is not None
        for fn in (il, sl):
            assert lib.sbx_atmosphere_air_eval(ctx, fn, ctypes.byref(M.as_aux(bad)), rp, op, 4, s) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()), "a refused call writes nothing"
    assert lib.sbx_atmosphere_air_eval(ctx, il, a, None, None, 0, s) == 0      # n == 0 touches nothing
    view9 = M.as_aux(M.air(.37, view=9, sun_power=19.))                        # `view` is not read
    assert lib.sbx_atmosphere_air_eval(ctx, sl, ctypes.byref(view9), rp, op, 4, s) == 0
    assert differing(out, M.get_sun_light(BLOCKS["brighter"], RAYS[:4])) == 0
    assert renderer.atmosphere_air_eval("get_incident_light", torch.zeros((0, 6)), good).shape == (0, 3)
    with pytest.raises(SbxError):
        renderer.atmosphere_air_eval("get_light", rays, good)
    assert lib.sbx_debug_atmosphere_air_eval(ctx, il, a, rp, op, 4, None, s) == -1    # the hook needs a place for its count
    before = renderer.stats()["render_launches"], renderer.atmosphere_air_launches()
    renderer.atmosphere_air_eval("get_incident_light", rays, good)
    assert (renderer.stats()["render_launches"], renderer.atmosphere_air_launches()) == before      # not a render
