"""CPU checks of APP_CLOUDS' view table (csrc/sbx_ytab.hip clouds_viewtab_key, csrc/kern_clouds.hip clouds_select):
the key of a table is the camera, the sun and the frame size, field by field — never u_time, the wind, a cloud parameter or a pad of
either block — and the selection yields the view-table instantiation only where it yields a hash-table one.  Host code only."""
import ctypes

import numpy as np
import pytest

import shaderbox_amd
from tests import clouds_selection_cases as C

W, H, T = 97, 55, 0.37
MOUSE = (300.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    from shaderbox_amd import build
    build.build(verbose=False)
    return shaderbox_amd.load_library()


def aux_of(fields=None):
    """an aux block of its own (the defaults with `fields` on top)"""
    from oracle import aux_sets
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", dict(fields or {})).tobytes())


def key(lib, w=W, h=H, t=T, mouse=MOUSE, aux=None, app="clouds", u=None):
    u = u or shaderbox_amd.uniforms(w, h, t, mouse)
    return shaderbox_amd.clouds_viewtab_key(app, u, aux, lib=lib)


def test_key_ignores_time_wind_and_the_cloud_parameters(lib):
    base = key(lib)
    assert base.shape == (shaderbox_amd.VIEWTAB_KEY_WORDS,) and np.array_equal(base, key(lib, aux=aux_of()))
    for t in (0.0, 1.0 / 60.0, 200.0, 1e9, float("inf")):
        assert np.array_equal(base, key(lib, t=t)), t
    for fields in ({"wind_dir": (0.3, 0.1, -2.0)}, {"cld_coverage": 0.4}, {"sigma_scattering": 0.7}, {"cld_march_steps": 37},
                   {"illum_march_steps": 3}, {"cld_thick": 333.0}, {"sun_power": 55.0}):
        assert np.array_equal(base, key(lib, aux=aux_of(fields))), fields
    for app in ("clouds_height", "clouds_luminance"):        # the builds share the tables
        assert np.array_equal(base, key(lib, app=app))


def test_key_ignores_the_pads_of_both_blocks(lib):
    base = key(lib)
    u = shaderbox_amd.uniforms(W, H, T, MOUSE)
    a = aux_of()
    for k, garbage in enumerate((float("nan"), -1e30, 7.0)):
        u._pad[k] = garbage
    a._pad0, a._pad1, a._pad2 = 3.5, float("nan"), -2e-40
    raw = (ctypes.c_uint32 * (ctypes.sizeof(a) // 4)).from_buffer(a)
    named = sum(ctypes.sizeof(t) for n, t in a._fields_) // 4
    assert named == len(raw)                                 # (every word of the block is a named field: the three pads are its only ones)
    assert np.array_equal(base, key(lib, u=u, aux=a))


def test_every_key_field_changes_the_key(lib):
    base = key(lib)
    changed = {
        "width (res_x, aspect_x, rres_x)": key(lib, w=W + 1),
        "height (res_y, aspect_x, rres_y)": key(lib, h=H + 1),
        "mouse x (eye, fwd, right, up)": key(lib, mouse=(301.0, 0.0)),
        "sun_dir": key(lib, aux=aux_of({"sun_dir": (0.0, 0.6, -0.8)})),
        "sun_color": key(lib, aux=aux_of({"sun_color": (1.0, 0.7, 0.56)})),
    }
    for what, k in changed.items():
        assert not np.array_equal(base, k), what
    # word by word: the words that differ are the ones the changed input feeds (csrc/sbx_ytab.hip clouds_viewtab_key's order:
    # res_x res_y aspect fov | eye fwd up right | sun_dir sun_color | rres_x rres_y | width height)
    diff = lambda k: set(np.nonzero(base != k)[0].tolist())   # noqa: E731
    assert diff(changed["sun_dir"]) <= {16, 17, 18} and diff(changed["sun_dir"])
    assert diff(changed["sun_color"]) <= {19, 20, 21} and diff(changed["sun_color"])
    assert {0, 2, 26} <= diff(changed["width (res_x, aspect_x, rres_x)"]) <= {0, 2, 22, 23, 26}
    assert {1, 2, 27} <= diff(changed["height (res_y, aspect_x, rres_y)"]) <= {1, 2, 24, 25, 27}
    assert diff(changed["mouse x (eye, fwd, right, up)"]) <= set(range(4, 16)) and diff(changed["mouse x (eye, fwd, right, up)"])
    # fov is a constant of the app's camera (word 3): the same under every input above
    assert all(k[3] == base[3] for k in changed.values())


def expected_key(w, h, mouse, aux):
    """the 28 words from the model's camera (tests/clouds_builds_model.py setup_camera; make_camera's operations of csrc/sbx_frame.h in
    binary32) and the aux block's sun: every field at its place, so a key that dropped or misplaced one differs"""
    from tests import clouds_builds_model as M
    from tests.model_common import F, ONE, ZERO, cross, normalize
    eye, look_at = M.setup_camera(mouse)
    eye, look_at = tuple(map(F, eye)), tuple(map(F, look_at))
    fwd = normalize(tuple(look_at[k] - eye[k] for k in range(3)))
    right = cross((ZERO, ONE, ZERO), fwd)
    up = cross(fwd, right)
    A = M.aux_block(aux)
    f = [F(w), F(h), F(w) / F(h), M.FOV, *eye, *fwd, *up, *right, *A["sun_dir"], *A["sun_color"]]
    words = np.array([np.asarray(v, dtype=np.float32).reshape(-1)[0] for v in f], dtype=np.float32).view(np.uint32)
    rres = np.array([1.0 / float(w), 1.0 / float(h)], dtype=np.float64).view(np.uint32)
    return np.concatenate([words, rres, np.array([w, h], dtype=np.uint32)])


@pytest.mark.parametrize("mouse", [(0.0, 0.0), MOUSE, (37.0, 11.0), (1234.5, 0.0)])
@pytest.mark.parametrize("aux", [None, {"sun_dir": (0.0, 0.6, -0.8), "sun_color": (1.0, 0.5, 0.25)}], ids=["default_sun", "other_sun"])
def test_key_is_the_camera_the_sun_and_the_size_word_for_word(lib, mouse, aux):
    for w, h in ((W, H), (130, 67), (3840, 2160)):
        got = key(lib, w=w, h=h, mouse=mouse, aux=aux_of(aux))
        want = expected_key(w, h, mouse, aux)
        assert np.array_equal(got, want), (w, h, np.nonzero(got != want)[0].tolist())
        assert len(want) == shaderbox_amd.VIEWTAB_KEY_WORDS


def select(lib, app="clouds", aux=None, table_range=1 << 18, view_table=True, **kw):
    return shaderbox_amd.clouds_select_vt(app, W, H, T, MOUSE, C.aux_struct(aux), table_range=table_range, view_table=view_table, lib=lib, **kw)


def test_selection_yields_vt_only_on_hash_table_forms(lib):
    for app in ("clouds", "clouds_height", "clouds_luminance"):
        for aux in (None, C.YZ):
            r = select(lib, app, aux)
            # the z-only light march (and HEIGHT, which has none) only: the y-z forms keep their kernels
            assert (r["gt"], r["vt"]) == (3, 1 if aux is None or app == "clouds_height" else 0), (app, aux, r)
            assert select(lib, app, aux, view_table=False)["vt"] == 0
            # without a ready hash table: the cache kernel, and no view table either
            r = select(lib, app, aux, table_range=0)
            assert (r["gt"], r["vt"]) == (0, 0), (app, aux, r)
    assert select(lib, aux={"sun_dir": (0.3, 0.2, -0.9)})["vt"] == 0          # the general light march takes no table kernel
    assert select(lib, variant=1)["vt"] == 0 and select(lib, variant=1)["perlane"] == 1
    assert select(lib, point_list=True)["vt"] == 0
    assert select(lib, "clouds_sky")["vt"] == 0
    assert select(lib, ytab_rows=0)["vt"] == 0                                # the table-less kernels
    # every other field is sbx_debug_clouds_select's
    for aux in (None, C.YZ):
        want = shaderbox_amd.clouds_select("clouds", W, H, T, MOUSE, C.aux_struct(aux), table_range=1 << 18, lib=lib)
        got = select(lib, aux=aux)
        assert {k: v for k, v in got.items() if k != "vt"} == want
