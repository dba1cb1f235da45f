"""The restatement pinned to the reference TEXT, bit for bit.

oracle/ref_apps.h and ref_lib.h restate the reference's shader headers by hand, and every GPU test compares a kernel with that
restatement: a wrong term in it is copied faithfully and seen by nobody.  oracle/_ref/libsbx_ref_<name>.so are the reference's own
headers, compiled verbatim over oracle/glsl_env.h (oracle/Makefile `ref`, oracle/README.md "How it is pinned"); this file compares
the two: whole frames at three sizes, several times and mouse positions, off-centre and out-of-frame fragCoords, the noise
library, the committed golden frames, and the two Python models that stand in for the oracle (tests/app2d_model.py,
tests/atmosphere_ground_model.py); and, for the aux uniform block (cbuffer b1), every set of tests/golden/reference_aux_sets.json
against the build that has the set compiled in ("the aux sets" below).  Every comparison is over the bits of all four channels,
NaN equal to NaN: no tolerance, no excluded pixel.

Where the reference tree is on the machine the builds are (re)made first, and all of them must then exist; elsewhere the tests
use what oracle/_ref holds (it travels with the tree to the GPU machine) and skip only when it holds no library.
"""
import glob
import os

import numpy as np
import pytest

from oracle import aux_sets
from oracle.oracle import APP_IDS, REF_NAMES, Reference, build_reference, reference_root
from tests import app2d_model as M2
from tests import atmosphere_ground_model as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the apps the oracle renders and the reference builds compile
ORACLE_APPS = ["planet", "clouds", "clouds_sky", "vinyl", "egg", "raytracer", "atmosphere", "sdf_ao", "clouds_best"]
# the apps whose headers read u_mouse (src/app_clouds.h:28, app_raytracer.h:40; app_vinyl.h:422-423 reads u_mouse.z and .y, and
# .z is 0 on this path: the oracle's and the kernels' u_mouse is a vec2)
MOUSE_APPS = {"clouds", "clouds_sky", "raytracer", "vinyl"}
MOUSE = (300.0, 120.0)
SIZES = [(64, 36), (256, 144), (97, 61)]
# 0, 0.37 and 9.25; 2.0 and 100.5 lie in other periods of every animation the headers have (EGG's wheel and pedals
# rotate_around_y(-100 t) / rotate_around_z(-t pedal_speed), app_egg.h:40,73-76, and its IK pose; PLANET's rotate_around_x(-12 t)
# and (8 t), app_planet.h:308-309; SDF_AO's rotate_around_y(50 t), app_sdf_ao.h:47; VINYL's 200 t and sin(3.6758 t),
# app_vinyl.h:142,419; RAYTRACER's sin/cos(t), app_raytracer.h:30-31); ATMOSPHERE's -abs(sin(t / 2)) (app_atmosphere.h:179) has
# sin > 0 at 0.37, 2.0 and 100.5 and sin < 0 at 9.25 and 7.0, and is 0 at 0; -3.1 is a negative time
TIMES = [0.0, 0.37, 9.25, 2.0, 7.0, 100.5, -3.1]
# app_2d.h:79-104: t = mod(u_time, 16) against 4, 8, 12 with strict inequalities — every phase, every edge, a wrapped time
TIMES_2D = [0.0, 0.37, 2.0, 4.0, 5.5, 8.0, 9.25, 12.0, 13.0, 14.0, 16.0 + 4.0, 100.5, 1000.9, -3.1]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)
        raise AssertionError("%s: %d of %d channels differ, first at %s: restatement %r, reference build %r"
                             % (what, len(i), ok.size, i[0].tolist(), got[tuple(i[0])], want[tuple(i[0])]))


@pytest.fixture(scope="module")
def ref():
    if os.path.isdir(os.path.join(reference_root(), "src")):
        have = build_reference()
        assert set(have) == set(REF_NAMES), "make ref left builds out: %s" % sorted(set(REF_NAMES) - set(have))
    if not Reference.available():
        pytest.skip("oracle/_ref holds no reference build and the reference tree is not on this machine")
    return Reference()


def need(ref, name):
    if name not in ref.available():
        pytest.skip("no reference build of %s under oracle/_ref" % name)


def points(w, h):
    """fragCoords that are no pixel centres: inside the frame, around it, far outside, and beyond 2^24 W where the quotients of
    main.h:40 round.  No inf and NaN rows: a shader's float-to-int conversions and comparisons of them are not defined alike on
    both sides."""
    rng = np.random.default_rng(11)
    big = float(2 ** 24) * w
    return np.concatenate([
        rng.uniform(0, 1, size=(300, 2)) * [w, h],
        rng.uniform(-3, 4, size=(200, 2)) * [w, h],
        rng.uniform(-1, 1, size=(30, 2)) * [big, big * 16],
        [[0, 0], [w, h], [-.5, -.5], [w - .5, h - .5], [-1, 7], [big, 3], [3, -big], [w / 2, h / 2], [w / 2, 0], [0, h / 2]],
    ]).astype(np.float32)


# ---- whole frames ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("app", ORACLE_APPS)
def test_frames_equal_the_reference_build(oracle, ref, app):
    need(ref, app)
    seen = {}
    for w, h in SIZES:
        for t in TIMES:
            for mouse in [(0.0, 0.0)] + ([MOUSE] if app in MOUSE_APPS else []):
                a = oracle.render(APP_IDS[app], w, h, t, mouse=mouse)
                assert_same(a, ref.render(app, w, h, t, mouse=mouse), (app, w, h, t, mouse))
                seen[(w, h, t, mouse)] = a
    # the cases are different frames, not one frame many times: time moves every app but clouds_best's sky far from the wind
    # (its frames still differ), and the mouse moves the apps that read u_mouse.x or .y
    w, h = SIZES[0]
    zero = (0.0, 0.0)
    assert not same_bits(seen[(w, h, 0.37, zero)], seen[(w, h, 9.25, zero)]).all(), (app, "time does not enter")
    if app in MOUSE_APPS - {"vinyl"}:
        assert not same_bits(seen[(w, h, 0.37, zero)], seen[(w, h, 0.37, MOUSE)]).all(), (app, "the mouse does not enter")


def test_row_lists_and_threads_do_not_matter(oracle, ref):
    """render_rows of a row list, in any order and on one thread, is the same rows of the frame: the per-pixel reset of the
    mutated globals (`depth`, `sun_dir`: SURVEY.md Appendix B1) holds whatever ran on the thread before"""
    for app in ("egg", "atmosphere"):
        need(ref, app)
        w, h, t = 97, 61, 9.25
        frame = ref.render(app, w, h, t)
        rows = [60, 0, 33, 34, 7, 33]
        assert_same(ref.render_rows(app, w, h, t, rows, threads=1), frame[rows], (app, "rows, one thread"))
        assert_same(ref.render_rows(app, w, h, t, rows, threads=5), oracle.render_rows(APP_IDS[app], w, h, t, rows), (app, "rows"))


# ---- single fragCoords -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("app", ORACLE_APPS)
def test_main_image_off_centre_and_out_of_frame(oracle, ref, app):
    need(ref, app)
    w, h = 1920, 1080
    pts = points(w, h)
    for t, mouse in [(9.25, (0.0, 0.0)), (0.37, MOUSE if app in MOUSE_APPS else (0.0, 0.0))]:
        a = np.stack([oracle.main_image(APP_IDS[app], w, h, t, x, y, mouse=mouse) for x, y in pts])
        b = np.stack([ref.main_image(app, w, h, t, x, y, mouse=mouse) for x, y in pts])
        assert_same(a, b, (app, "main_image", t, mouse))
    # and a pixel centre through main_image is the frame's pixel
    assert_same(ref.main_image(app, 64, 36, 0.37, 10.5, 20.5), ref.render(app, 64, 36, 0.37)[20, 10], (app, "centre"))


# ---- the noise library -------------------------------------------------------------------------------------------------

def noise_points():
    rng = np.random.default_rng(5)
    return np.concatenate([
        rng.uniform(0, 1, size=(1500, 3)),
        rng.uniform(-8, 8, size=(1500, 3)),
        rng.uniform(-2000, 2000, size=(800, 3)),
        rng.uniform(-1e5, 1e5, size=(400, 3)),
        rng.integers(-40, 40, size=(300, 3)) * .5,                          # lattice points and cell centres
        [[0, 0, 0], [1, 1, 1], [-1, -1, -1], [.5, .5, .5], [1e-30, -1e-30, 0], [127.5, -0.125, 3e6], [-0.0, 7, 1e7]],
    ]).astype(np.float32)


def test_noise_library_equals_the_reference_build(oracle, ref):
    need(ref, "noise")
    p = noise_points()
    assert len(p) > 4000
    assert_same(oracle.noise("noise_iq", p)[:, 0], ref.noise("noise_iq", p)[:, 0], "noise_iq")
    assert_same(oracle.noise("hash_w", p), ref.noise("hash_w", p), "hash_w")
    for rep in (1.0, 4.0, 7.0, 8.0, 128.0):
        assert_same(oracle.noise("noise_w", p, (rep, 0, 0)), ref.noise("noise_w", p, (rep, 0, 0)), ("noise_w", rep))
    for par in [(2.0, 1.0, .5), (4.0, 1.0, .5), (7.0, 1.0, .5), (2.64, .5, .5)]:
        assert_same(oracle.noise("fbm_worley_tile", p, par)[:, 0], ref.noise("fbm_worley_tile", p, par)[:, 0], ("fbm_worley_tile", par))
    # noise_iq.h's scalar hash: the oracle states it through its known-answer hook
    xs = np.concatenate([np.arange(-300, 300, dtype=np.float32), p[:600, 0] * np.float32(37)]).astype(np.float32)
    want = ref.noise("hash", np.stack([xs, xs, xs], axis=1))[:, 0]
    got = np.array([oracle.kat("hash", [x], 1)[0] for x in xs], dtype=np.float32)
    assert_same(got, want, "hash")


# ---- the committed golden frames ---------------------------------------------------------------------------------------

# golden frames of apps that are no build of one reference header, with the reason: the volumes of APP_CLOUDS' USE_NOISE_TEX
# text are HLSL declarations (src/app_clouds.h:52-55) that no C++ compiler takes; clouds_ue4 is the .usf under ue4/; vinyl_gpu
# is the march length of app_vinyl.h's non-C++ branch (:412-416); planet_atmosphere is this project's composite
GOLDEN_WITHOUT_BUILD = {"clouds_tex", "clouds_ue4", "vinyl_gpu", "planet_atmosphere"}


def golden_cases():
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        app, res = os.path.basename(path)[:-4].rsplit("_", 1)
        w, h = (int(v) for v in res.split("x"))
        yield path, app, w, h


def test_every_golden_is_classified():
    apps = {c[1] for c in golden_cases()}
    assert apps - GOLDEN_WITHOUT_BUILD == set(ORACLE_APPS)
    assert GOLDEN_WITHOUT_BUILD <= apps


@pytest.mark.parametrize("path,app,w,h", [c for c in golden_cases() if c[1] not in GOLDEN_WITHOUT_BUILD])
def test_reference_build_reproduces_golden(ref, path, app, w, h):
    need(ref, app)
    z = np.load(path)
    assert len(z.files) >= 3
    for key in z.files:
        assert_same(z[key], ref.render(app, w, h, float(key[1:])), (app, key))


# ---- the Python models that stand in for the oracle ----------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 36), (256, 144), (97, 61), (16, 8)])
def test_app2d_model_equals_the_reference_build(ref, w, h):
    need(ref, "2d")
    need(ref, "2d_tex")
    tex = M2.decode_unorm8(M2.checkerboard_texture())
    ref.set_texture2d(tex)
    for t in TIMES_2D:
        assert_same(M2.frame(w, h, t), ref.render("2d", w, h, t), ("2d", w, h, t))
        assert_same(M2.frame(w, h, t, tex), ref.render("2d_tex", w, h, t), ("2d_tex", w, h, t))
    assert {M2.phase(t)[0] for t in TIMES_2D} == {0, 1, 2, 3, 4}


def test_app2d_model_points_and_other_textures(ref):
    need(ref, "2d")
    need(ref, "2d_tex")
    w, h = 1920, 1080
    pts = points(w, h)
    rng = np.random.default_rng(3)
    texf = rng.uniform(-2, 2, size=(61, 97, 4)).astype(np.float32)          # not square, not a power of two, any float
    for tex in (M2.decode_unorm8(M2.checkerboard_texture()), texf, texf[:1, :1]):
        ref.set_texture2d(tex)
        for t in (0.37, 5.5, 9.25, 13.0):
            b = np.stack([ref.main_image("2d_tex", w, h, t, x, y) for x, y in pts])
            assert_same(M2.main_image(w, h, t, pts[:, 0], pts[:, 1], tex), b, ("2d_tex points", tex.shape, t))
    for t in (0.37, 5.5, 9.25, 13.0):
        b = np.stack([ref.main_image("2d", w, h, t, x, y) for x, y in pts])
        assert_same(M2.main_image(w, h, t, pts[:, 0], pts[:, 1]), b, ("2d points", t))
    # the grid tests/test_app2d_cpu.py uses, at its size
    fx, fy = np.meshgrid(np.arange(0, w, 7, dtype=np.float32) + .5, np.arange(0, h, 5, dtype=np.float32) + .5)
    rows = np.arange(0, h, 5)
    for t in (0.37, 5.5, 9.25, 14.0, -3.1, 1000.9):
        assert_same(M2.main_image(w, h, t, fx, fy), ref.render_rows("2d", w, h, t, rows)[:, ::7], ("2d grid", t))


@pytest.mark.parametrize("w,h", [(96, 54), (64, 36), (97, 61)])
def test_atmosphere_ground_model_equals_the_reference_build(ref, w, h):
    need(ref, "atmosphere_ground")
    for t in (0.0, 0.37, 2.0, 3.1, 9.25, 100.5):
        assert_same(MG.frame(w, h, t), ref.render("atmosphere_ground", w, h, t), ("atmosphere_ground", w, h, t))


def test_atmosphere_ground_model_points(ref):
    need(ref, "atmosphere_ground")
    w, h = 1920, 1080
    pts = points(w, h)[::3]
    for t in (0.37, 9.25):
        b = np.stack([ref.main_image("atmosphere_ground", w, h, t, x, y) for x, y in pts])
        assert_same(MG.main_image(w, h, t, pts[:, 0], pts[:, 1]), b, ("atmosphere_ground points", t))


# ---- the aux sets ------------------------------------------------------------------------------------------------------
# In the reference's C++ form an aux uniform is a compile-time constant (src/uniform_buffer.h:13), so the builds above hold the
# defaults and only the defaults.  tests/golden/reference_aux_sets.json names aux blocks that move the kernels onto their other
# paths (light marches, y table, exp forms, stage cut-offs, the SKY_SPHERE sphere); `make ref` compiles one build per (header,
# set) with the set's binary32 values in place of the defaults (oracle/aux_sets.py), and Reference answers `aux=` with the build
# whose set equals the block field for field.

AUX_SETS = aux_sets.load()
AUX_CASES = [(b, name) for kind, by_name in AUX_SETS.items() for b, _, _ in aux_sets.BUILDS[kind] for name in by_name]
AUX_SIZES = [(96, 54), (97, 61)]
AUX_TIMES = [0.37, 9.25, -3.1]


def aux_block(build, name=None):
    kind = aux_sets.KIND_OF[build]
    return aux_sets.block(kind, AUX_SETS[kind][name] if name else None)


def need_aux(ref, build, name):
    if "%s@%s" % (build, name) not in ref.available_aux():
        pytest.skip("no reference build %s@%s under oracle/_ref" % (build, name))


def test_every_aux_set_has_its_builds(ref):
    """wherever the reference tree is, `make ref` (the `ref` fixture ran it) made <build>@<set> for every set of the fixture"""
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        pytest.skip("the reference tree is not on this machine")
    want = aux_sets.build_names()
    assert len(want) == len(set(want)) == len(AUX_CASES) and len(want) >= 28
    assert list(ref.available_aux()) == want
    # the sets the project's paths need, under the names the other tests use
    assert {"steer", "yz", "exp_on", "exp_off", "long", "cov_hi", "cov_lo", "wind_y", "zero", "degenerate", "outside",
            "small_sphere"} <= set(AUX_SETS["clouds"])
    fog = {(v["fog_density"], v["fog_falloff"]) for v in AUX_SETS["sdf_ao"].values() if len(v) == 2}
    assert {(.25, .3), (0, .5), (2.5, 0), (-.1, 4)} <= fog


def test_aux_literals_and_blocks_hold_the_same_binary32():
    """what the build compiles and what the oracle and the kernels are handed: one binary32 per field.  The literal is %.9g of it
    (read back as binary32 under -fsingle-precision-constant), with a decimal point or an exponent; integers are integers; and a
    block of defaults is the block the library's own defaults call fills"""
    import shaderbox_amd
    from shaderbox_amd import build
    build.build(verbose=False)
    assert aux_block("clouds").tobytes() == bytes(shaderbox_amd.clouds_defaults())
    assert aux_block("sdf_ao").tobytes() == bytes(shaderbox_amd.sdf_ao_defaults())
    for kind, by_name in AUX_SETS.items():
        for name, over in by_name.items():
            b = aux_sets.block(kind, over)
            for field in over:
                text = aux_sets.literal(b[field])
                if b.dtype[field].kind == "i":
                    assert text == "(%d)" % over[field]
                    continue
                nums = text[text.index("(") + 1:-1].split(",")
                assert len(nums) == (3 if b.dtype[field].shape else 1) and text.startswith("vec3(" if b.dtype[field].shape else "(")
                assert all("." in n or "e" in n for n in nums), (name, field, text)
                # decimal -> binary32 in one rounding, as the compiler reads a float literal
                got = np.array([np.float32(n) for n in nums], dtype=np.float32)
                assert got.tobytes() == np.asarray(b[field], dtype=np.float32).tobytes(), (name, field, text)
                assert got.tobytes() == np.asarray(over[field], dtype=np.float32).tobytes()


def test_exp_sets_lie_on_either_side_of_the_exp_small_bound():
    """launch_clouds (kern_clouds.hip) takes the exp_small_ kernels when sigma, dt >= 0 and .94 sigma dt <= .2049 in binary64, with
    dt = cld_thick / cld_march_steps in binary32 (build_clouds, sbx_frames.hip).  With the default dt = 1.25 the edge is
    sigma = .17438...; .1744 and .1746 both lie beyond it (.204920, .205155), so the pair is .1743 (.204803) and .1745 (.205038)."""
    def product(name):
        b = aux_block("clouds", name)
        dt = np.float32(b["cld_thick"]) / np.float32(b["cld_march_steps"])
        return .94 * float(b["sigma_scattering"]) * float(dt)
    assert set(AUX_SETS["clouds"]["exp_on"]) == set(AUX_SETS["clouds"]["exp_off"]) == {"sigma_scattering"}
    assert 0 < product("exp_on") <= .2049 < product("exp_off")
    assert abs(product("exp_on") - .2049) < 2e-4 and abs(product("exp_off") - .2049) < 2e-4      # both next to the edge


@pytest.mark.parametrize("build,name", AUX_CASES)
def test_aux_frames_equal_the_aux_set_build(oracle, ref, build, name):
    need_aux(ref, build, name)
    aux = aux_block(build, name)
    for w, h in AUX_SIZES:
        for t in AUX_TIMES:
            for mouse in [(0.0, 0.0)] + ([MOUSE] if build in MOUSE_APPS else []):
                assert_same(oracle.render(APP_IDS[build], w, h, t, mouse=mouse, aux=aux),
                            ref.render(build, w, h, t, mouse=mouse, aux=aux), (build, name, w, h, t, mouse))


@pytest.mark.parametrize("build", ["clouds", "clouds_sky", "sdf_ao"])
def test_aux_defaults_block_is_the_default_build(oracle, ref, build):
    """a block of defaults is answered by the default build, and is what aux=None means on the oracle's side"""
    need(ref, build)
    aux = aux_block(build)
    assert Reference.build_for(build, aux) == build
    w, h, t = 97, 61, 9.25
    want = ref.render(build, w, h, t)
    assert_same(ref.render(build, w, h, t, aux=aux), want, (build, "defaults block, reference"))
    assert_same(oracle.render(APP_IDS[build], w, h, t, aux=aux), want, (build, "defaults block"))
    assert_same(oracle.render(APP_IDS[build], w, h, t), want, (build, "no block"))


@pytest.mark.parametrize("build", ["clouds", "clouds_sky"])
@pytest.mark.parametrize("name", ["steer", "yz"])
def test_aux_main_image_off_centre_and_out_of_frame(oracle, ref, build, name):
    need_aux(ref, build, name)
    aux = aux_block(build, name)
    w, h = 1920, 1080
    pts = points(w, h)
    for t, mouse in [(9.25, (0.0, 0.0)), (0.37, MOUSE)]:
        a = np.stack([oracle.main_image(APP_IDS[build], w, h, t, x, y, mouse=mouse, aux=aux) for x, y in pts])
        b = np.stack([ref.main_image(build, w, h, t, x, y, mouse=mouse, aux=aux) for x, y in pts])
        assert_same(a, b, (build, name, "main_image", t, mouse))
    assert_same(ref.main_image(build, 96, 54, 0.37, 10.5, 20.5, aux=aux), ref.render(build, 96, 54, 0.37, aux=aux)[20, 10],
                (build, name, "centre"))


# field -> (a set that changes this field and no other, the builds whose text reads the field, the builds whose text does not).
# wind_dir: app_clouds.h:167 is compiled out under SKY_SPHERE; atm_radius and atm_ground_y: read only under SKY_SPHERE (:14-19).
BOTH = ("clouds", "clouds_sky")
AUX_FIELD_WITNESS = {
    "wind_dir": ("wind_y", ("clouds",), ("clouds_sky",)),
    "sun_dir": ("yz", BOTH, ()),
    "sun_color": ("one_sun_color", BOTH, ()),
    "sun_power": ("one_sun_power", BOTH, ()),
    "cld_march_steps": ("zero", BOTH, ()),
    "illum_march_steps": ("one_illum_steps", BOTH, ()),
    "sigma_scattering": ("exp_off", BOTH, ()),
    "cld_coverage": ("cov_lo", BOTH, ()),
    "cld_thick": ("one_thick", BOTH, ()),
    "atm_radius": ("outside", ("clouds_sky",), ("clouds",)),
    "atm_ground_y": ("one_ground_y", ("clouds_sky",), ("clouds",)),
    "fog_density": ("fog_none", ("sdf_ao",), ()),
    "fog_falloff": ("one_falloff", ("sdf_ao",), ()),
}


def test_every_aux_field_has_a_witness():
    assert set(AUX_FIELD_WITNESS) == set(aux_sets.fields("clouds")) | set(aux_sets.fields("sdf_ao")) and len(AUX_FIELD_WITNESS) == 13
    for field, (name, reads, ignores) in AUX_FIELD_WITNESS.items():
        kind = aux_sets.KIND_OF[reads[0]]
        b, d = aux_block(reads[0], name), aux_block(reads[0])
        assert {f for f in aux_sets.fields(kind) if np.asarray(b[f]).tobytes() != np.asarray(d[f]).tobytes()} == {field}, (field, name)
        assert set(reads) | set(ignores) == {b for b, _, _ in aux_sets.BUILDS[kind]}


@pytest.mark.parametrize("field", sorted(AUX_FIELD_WITNESS))
def test_every_aux_field_is_read_where_the_text_reads_it(ref, field):
    """reference build against reference build: a set that changes ONE field changes the frame of every header that reads the
    field (more than a thousand of 5 184 pixels), and no bit of a header that does not"""
    name, reads, ignores = AUX_FIELD_WITNESS[field]
    w, h, t = 96, 54, 0.37
    for build in reads + ignores:
        need(ref, build)
        need_aux(ref, build, name)
        a, d = ref.render(build, w, h, t, aux=aux_block(build, name)), ref.render(build, w, h, t)
        changed = int((~same_bits(a, d)).any(axis=-1).sum())
        if build in reads:
            assert changed > 1000, (field, build, name, changed)
        else:
            assert changed == 0, (field, build, name, changed)


def test_sets_the_text_does_not_read_equal_the_default_build(ref):
    """wind_y under SKY_SPHERE, outside and small_sphere without it: every bit of the default build's frame, at every size, time and
    mouse position of the frame test"""
    for build, name in [("clouds_sky", "wind_y"), ("clouds", "outside"), ("clouds", "small_sphere")]:
        need(ref, build)
        need_aux(ref, build, name)
        for w, h in AUX_SIZES:
            for t in AUX_TIMES:
                for mouse in [(0.0, 0.0), MOUSE]:
                    assert_same(ref.render(build, w, h, t, mouse=mouse, aux=aux_block(build, name)),
                                ref.render(build, w, h, t, mouse=mouse), (build, name, "is not read", w, h, t, mouse))


def test_outside_set_pins_the_nan_sky(oracle, ref):
    """atm_radius 100 around a centre 4750 below the eye: the eye is outside the sphere, and every sky pixel of the SKY_SPHERE
    build is NaN in the reference build; the oracle has NaN in the same pixels (the frame test compares them all)"""
    need_aux(ref, "clouds_sky", "outside")
    aux = aux_block("clouds_sky", "outside")
    a = ref.render("clouds_sky", 96, 54, 0.37, aux=aux)
    nan = np.isnan(a).any(axis=-1)
    assert nan.sum() > 1000 and not nan.all()
    assert not np.isnan(ref.render("clouds_sky", 96, 54, 0.37)).any()
    assert (np.isnan(oracle.render(APP_IDS["clouds_sky"], 96, 54, 0.37, aux=aux)).any(axis=-1) == nan).all()


def test_a_block_without_a_build_is_an_error(ref):
    """never the defaults: a block that equals no set, a block of another layout, an aux block for an app that has none"""
    need(ref, "clouds")
    odd = aux_block("clouds")
    odd["cld_coverage"] = np.nextafter(np.float32(AUX_SETS["clouds"]["steer"]["cld_coverage"]), np.float32(1))
    for call in (lambda: ref.render("clouds", 16, 9, 0.37, aux=odd),
                 lambda: ref.render_rows("clouds_sky", 16, 9, 0.37, [0], aux=odd),
                 lambda: ref.main_image("clouds", 16, 9, 0.37, .5, .5, aux=odd),
                 lambda: ref.render("sdf_ao", 16, 9, 0.37, aux=aux_block("clouds", "yz")),     # a clouds block is no fog block
                 lambda: ref.render("clouds", 16, 9, 0.37, aux=aux_block("sdf_ao", "fog_mid")),
                 lambda: ref.render("egg", 16, 9, 0.37, aux=aux_block("sdf_ao"))):
        with pytest.raises(ValueError):
            call()
    # one field of a set alone is not the set
    part = aux_block("clouds")
    part["sun_dir"] = AUX_SETS["clouds"]["steer"]["sun_dir"]
    with pytest.raises(ValueError):
        ref.render("clouds", 16, 9, 0.37, aux=part)
    # -0 is not 0: the literal would differ
    neg = aux_block("sdf_ao", "fog_none")
    neg["fog_density"] = -0.0
    with pytest.raises(ValueError):
        ref.render("sdf_ao", 16, 9, 0.37, aux=neg)


# ---- the kernels -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_kernels_equal_the_reference_build():
    """one 256x144 frame of every app with a reference build, at a time and (where it is read) a mouse position no other GPU
    test uses, straight against the reference text: Renderer.render == Reference.render in every bit.  Uses the builds that
    travelled with the tree; the reference tree itself is not read."""
    have = Reference.available()
    if not have:
        pytest.skip("oracle/_ref holds no reference build")
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    ref = Reference()
    w, h, t = 256, 144, 9.25
    try:
        if "2d_tex" in have:
            ref.set_texture2d(M2.decode_unorm8(M2.checkerboard_texture()))   # the renderer's default t0
        for app in [a for a in ORACLE_APPS + ["atmosphere_ground", "2d", "2d_tex"] if a in have]:
            mouse = MOUSE if app in MOUSE_APPS else (0.0, 0.0)
            got = r.render(app, w, h, t, mouse=mouse).cpu().numpy()
            assert_same(got, ref.render(app, w, h, t, mouse=mouse), (app, w, h, t, mouse))
    finally:
        r.close()
