"""The kernels against the reference TEXT under non-default aux uniform blocks, bit for bit.

The aux block (cbuffer b1) picks most of the paths the clouds kernels have: the z-only, y-z-plane and general light marches
(sun_dir), the y table and the table-less kernels beyond it (cld_march_steps), the table key (wind_dir.y), exp_small_ against
exp_reg64_ (sigma_scattering), the staged main sample's cut-offs and the div3_ smoothstep (cld_coverage), the SKY_SPHERE sphere and
noise factor (atm_radius, atm_ground_y); and APP_SDF_AO's fog.  The other GPU tests hold those paths equal to the oracle, a
restatement written by hand.  Here they are held equal to the reference's own headers: oracle/_ref holds one build per (header,
set of tests/golden/reference_aux_sets.json) with the set's values compiled in where the reference compiles its defaults
(oracle/aux_sets.py, oracle/README.md), and `Reference.render(..., aux=)` is answered by the build whose set equals the block.

Only the builds that travelled with the tree are used; the reference tree itself is not read.  A reference frame is rendered once
and shared by every test that compares with it.
"""
import numpy as np
import pytest

from oracle import aux_sets
from oracle.oracle import Reference
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

MOUSE = (300.0, 120.0)

SETS = aux_sets.load()
CASES = [(b, name) for kind, by_name in SETS.items() for b, _, _ in aux_sets.BUILDS[kind] for name in by_name]
SIZES = [(96, 54), (97, 61)]
TIMES = [0.37, 9.25]
# the order of the back-to-back test: exp_small_ / exp_reg64_ / the y-z march / the default (z-only) kernels / beyond the y table /
# the general march with every field live (None = no aux block, the defaults)
BACK_TO_BACK = ["exp_on", "exp_off", "yz", None, "long", "steer"]


def assert_same(got, want, what):
    """over the bits of all four channels, NaN equal to NaN: no tolerance, no excluded pixel"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        i = np.argwhere(~ok)
        raise AssertionError("%s: %d of %d channels differ, first at %s: kernel %r, reference build %r"
                             % (what, len(i), ok.size, i[0].tolist(), got[tuple(i[0])], want[tuple(i[0])]))


def mouse_of(app, t):
    """u_mouse is read by the clouds headers (app_clouds.h:28): the camera turned at one of the two times"""
    return MOUSE if (app != "sdf_ao" and t == 9.25) else (0.0, 0.0)


def block(app, name):
    kind = aux_sets.KIND_OF[app]
    return aux_sets.block(kind, SETS[kind][name]) if name else None


def device_block(app, name):
    """the same bytes as the structure the library takes"""
    import shaderbox_amd
    if name is None:
        return None
    cls = {"clouds": shaderbox_amd.AuxClouds, "sdf_ao": shaderbox_amd.AuxSdfAo}[aux_sets.KIND_OF[app]]
    return cls.from_buffer_copy(block(app, name).tobytes())


@pytest.fixture(scope="module")
def ref():
    if not Reference.available_aux():
        pytest.skip("oracle/_ref holds no aux-set build")
    return Reference()


_frames = {}


def want(ref, app, name, w, h, t):
    """the reference build's frame: rendered once, shared, never written to"""
    key = (app, name, w, h, t)
    if key not in _frames:
        build = "%s@%s" % (app, name) if name else app
        if build not in ref.available_aux() + ref.available():
            pytest.skip("no reference build %s under oracle/_ref" % build)
        f = ref.render(app, w, h, t, mouse=mouse_of(app, t), aux=block(app, name))
        f.setflags(write=False)
        _frames[key] = f
    return _frames[key]


def render(r, app, name, w, h, t):
    return r.render(app, w, h, t, mouse=mouse_of(app, t), aux=device_block(app, name))


def points(w, h):
    """fragCoords that are no pixel centres: inside the frame, around it, on its corners and edges"""
    rng = np.random.default_rng(11)
    return np.concatenate([
        rng.uniform(0, 1, size=(300, 2)) * [w, h],
        rng.uniform(-3, 4, size=(200, 2)) * [w, h],
        [[0, 0], [w, h], [-.5, -.5], [w - .5, h - .5], [-1, 7], [w / 2, h / 2], [w / 2, 0], [0, h / 2]],
    ]).astype(np.float32)


def test_the_aux_builds_travelled(ref):
    """all of them or none: a tree that brought some aux-set builds brought every one the fixture names"""
    assert list(ref.available_aux()) == aux_sets.build_names()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("app,name", CASES)
def test_default_kernels_equal_the_aux_set_build(renderer, ref, app, name, w, h):
    for t in TIMES:
        assert_same(render(renderer, app, name, w, h, t).cpu().numpy(), want(ref, app, name, w, h, t), (app, name, w, h, t))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("app,name", CASES)
def test_plain_kernels_equal_the_aux_set_build(renderer, ref, app, name, w, h):
    """sbx_set_variant 1: the per-lane clouds kernel (no cache, no staging, no tables), SDF_AO without culling"""
    try:
        renderer.set_variant(1)
        for t in TIMES:
            assert_same(render(renderer, app, name, w, h, t).cpu().numpy(), want(ref, app, name, w, h, t),
                        (app, name, "variant 1", w, h, t))
    finally:
        renderer.set_variant(0)


@pytest.mark.parametrize("app,name", CASES)
def test_points_equal_the_aux_set_build(renderer, ref, app, name):
    import torch
    if "%s@%s" % (app, name) not in ref.available_aux():
        pytest.skip("no reference build %s@%s under oracle/_ref" % (app, name))
    w, h, t = 97, 61, 9.25
    pts = points(w, h)
    aux = block(app, name)
    b = np.stack([ref.main_image(app, w, h, t, x, y, mouse=mouse_of(app, t), aux=aux) for x, y in pts])
    got = renderer.render_points(app, w, h, t, torch.from_numpy(pts), mouse=mouse_of(app, t), aux=device_block(app, name))
    assert_same(got.cpu().numpy(), b, (app, name, "render_points", t))


@pytest.mark.parametrize("app", ["clouds", "clouds_sky"])
def test_back_to_back_launches_keep_their_own_aux(ref, app):
    """one context, the sets one after the other in an order that alternates the kernels' paths, nothing read back in between,
    then the same once more: every frame is its own build's.  A kernel selection, a y table, a span table or a frame cache keyed
    by less than the whole aux block would hand one launch what belongs to another."""
    import shaderbox_amd
    w, h, t = 96, 54, 0.37
    r = shaderbox_amd.Renderer(0)
    try:
        order = BACK_TO_BACK + BACK_TO_BACK
        got = [render(r, app, name, w, h, t) for name in order]
        for name, g in zip(order, got):
            assert_same(g.cpu().numpy(), want(ref, app, name, w, h, t), (app, name, "back to back"))
    finally:
        r.close()


@pytest.mark.parametrize("app,a,b", [("clouds", "exp_on", "yz"), ("clouds", "long", None), ("clouds_sky", "steer", "small_sphere"),
                                     ("sdf_ao", "fog_mid", "fog_negative")])
def test_main_image_alternating_sets_returns_each_sets_pixel(ref, app, a, b):
    """sbx_main_image keeps the frame of its last call on the host (include/sbx.h): two aux blocks in alternation, at pixel centres
    of one frame, must each get their own frame's pixel"""
    import shaderbox_amd
    w, h, t = 96, 54, 0.37
    r = shaderbox_amd.Renderer(0)
    try:
        for i, (x, y) in enumerate([(10, 20), (11, 20), (95, 53), (0, 0), (10, 20), (48, 30)]):
            for name in ((a, b) if i % 2 == 0 else (b, a)):
                px = r.main_image(app, w, h, t, (x + .5, y + .5), mouse=mouse_of(app, t), aux=device_block(app, name))
                assert_same(np.array(px, np.float32), want(ref, app, name, w, h, t)[y, x], (app, name, "main_image", x, y))
    finally:
        r.close()
