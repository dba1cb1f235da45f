"""CPU tests of SBX_APP_FUNC (src/app_func.h's 2D branch): the pure-numpy hash_w / noise_w against the oracle on every table cell
and frame grid position, the restatement (tests/appfunc_model.py) against a float64 combination, the header, the Python surface,
the C++ drop-in's selection and the span table."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import appfunc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 3), (257, 2), (640, 360)]


def test_table_cells_hash_matches_oracle():
    cells = M.table_cells()
    assert cells.shape == (18096, 3) == (3 * sum(L * L for L in M.PERIODS), 3)
    # the z cells of pos.z = 0 are mod(-1, 0, 1; L) = L - 1, 0, 1
    assert sorted(set(cells[:48, 2].tolist())) == [0.0, 1.0, 3.0]
    got, want = M.hash_w(cells), M.oracle().noise("hash_w", cells)
    assert M.same_bits(got, want).all(), int((~M.same_bits(got, want)).sum())


def _grid_t(w, h):
    fx, fy = np.meshgrid(np.arange(w, dtype=np.float32) + .5, np.arange(h, dtype=np.float32) + .5)
    tx, ty = M.t_of(w, h, fx, fy)
    return tx, ty


@pytest.mark.parametrize("w,h", SIZES)
def test_numpy_noise_w_matches_oracle_on_frame_grid(w, h):
    tx, ty = _grid_t(w, h)
    assert tx[0, -1] == 1.0 and ty[-1, 0] == 1.0               # the t = 1 column and row: (W - 1 + .5 + .5) / W
    mine = M.f1_of(tx, ty, M.noise_w_numpy)
    ref = M.f1_of(tx, ty)
    for L in M.PERIODS:
        assert M.same_bits(mine[L], ref[L]).all(), (w, h, L)


@pytest.mark.parametrize("w,h", [(640, 360), (257, 2)])
def test_restatement_matches_float64_combination(w, h):
    tx, ty = _grid_t(w, h)
    f1 = M.f1_of(tx, ty)
    n = M.frame(w, h)
    assert n.shape == (h, w, 4) and (n[..., 3] == 1).all() and (n[..., 0] == n[..., 1]).all() and (n[..., 1] == n[..., 2]).all()
    w64 = {L: 1 - (f1[L].astype(np.float64) + .015) for L in M.PERIODS}
    left = w64[4] * .625 + w64[8] * .25 + w64[16] * .125
    middle = w64[8] * .625 + w64[16] * .25 + w64[32] * .125
    right = w64[24] * .625 + w64[32] * .25 + w64[64] * .125
    want = left * .625 + middle * .25 + right * .125
    # a dozen binary32 roundings of values below 2 in magnitude: well inside 1e-6
    assert np.abs(n[..., 0].astype(np.float64) - want).max() < 1e-6


def test_nan_frag_coord_gives_f1_of_100():
    c = M.main_image(640, 360, np.float32("nan"), np.float32(3.5))
    want = np.float32(1) - (np.float32(10) + np.float32(.015))     # every d is NaN: F1 stays 100, sqrt = 10, for every period
    assert c[0] == c[1] == c[2] == want and c[3] == 1


def test_header_declares_app_func():
    h = open(os.path.join(ROOT, "include", "sbx.h")).read()
    m = re.search(r"SBX_APP_FUNC\s*=\s*(\d+)\b", h)
    assert m and int(m.group(1)) == 15
    assert "#define SBX_ABI_VERSION 2" in h
    assert '"worley_fbm"' in h


def test_python_names():
    import shaderbox_amd
    assert shaderbox_amd.APP_FUNC == 15 == shaderbox_amd.APPS["APP_FUNC"]
    assert shaderbox_amd.app_id("func") == shaderbox_amd.app_id("APP_FUNC") == shaderbox_amd.app_id("app_func") == 15


def test_dropin_selects_app_func(tmp_path):
    src = tmp_path / "sel.cpp"
    src.write_text('#include "sbx_mainimage.hpp"\nint selected_app = SBX_SELECTED_APP;\n')
    out = subprocess.run(["g++", "-std=c++17", "-E", "-DAPP_FUNC", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, check=True).stdout
    assert "int selected_app = SBX_APP_FUNC;" in out
    r = subprocess.run(["g++", "-std=c++17", "-E", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "APP_FUNC" in r.stderr                   # the #error list names it


def test_span_table_whole_rows():
    import shaderbox_amd
    w, h, br, n = 1280, 720, 8, 3
    table, pix, mw = shaderbox_amd.span_table("func", w, h, 0.37, br, n)
    assert (table[:, 0] == 0).all() and (table[:, 1] == w).all()
    assert int(pix.sum()) == w * h and mw == w


def test_library_exports_app_func_names():
    lib = open(os.path.join(ROOT, "shaderbox_amd", "lib", "libsbx.so"), "rb").read()
    assert b"worley_fbm" in lib
