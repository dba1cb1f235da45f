"""SBX_APP_CLOUDS_HEIGHT and SBX_APP_CLOUDS_LUMINANCE without a GPU: the numpy definition of the three builds of
src/app_clouds.h's illuminate_volume (tests/clouds_builds_model.py) pinned from two sides — its shipped build against the CPU oracle,
its other two against what the edited reference header itself rendered (tests/golden/clouds_builds/) — the conditions those
fixtures were recorded under (tests/build_families.py), and the host-only span table.  The name tables: tests/test_build_families_cpu.py."""
import os

import numpy as np
import pytest

from oracle import aux_sets
from tests import clouds_builds_model as M
from tests.build_families import FAMILIES, fixture_path, frame_keys
from tests.model_common import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = FAMILIES["clouds"]
CAPS = FAMILY["builds"]                             # per build: the caps that keep a fixture from saying nothing (tests/build_families.py)
NEW = tuple(CAPS)
W, H = FAMILY["size"]
POINTS = FAMILY["points"]


def assert_bits(got, want, what):
    ok = same_bits(got, want)
    assert got.shape == want.shape and ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


@pytest.mark.parametrize("t,aux_set", [(0.0, None), (1.5, None), (1.5, "steer"), (1.5, "yz")])
def test_shipped_build_of_the_model_is_the_oracle(oracle, t, aux_set):
    over = None if aux_set is None else aux_sets.load()["clouds"][aux_set]
    want = oracle.render(1, 96, 54, t, aux=None if over is None else aux_sets.block("clouds", over))
    assert_bits(M.frame("default", 96, 54, t, aux=over), want, (t, aux_set))


@pytest.mark.parametrize("build", NEW)
def test_model_equals_the_reference_headers_frames(build):
    fx = M.fixture(build)
    assert [f[0] for f in fx["frames"]] == [k[2:] for k in frame_keys(FAMILY["keys"], FAMILY["uniforms"])] + ["aux_" + s for s in FAMILY["aux_sets"]]
    for name, t, aux_set, want in fx["frames"]:
        over = None if aux_set is None else aux_sets.load()["clouds"][aux_set]
        assert want.shape == (H, W, 4)
        assert_bits(M.frame(build, W, H, t, aux=over), want, (build, name))


@pytest.mark.parametrize("build", NEW)
def test_model_equals_the_reference_headers_points(build):
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    assert pts.shape == (POINTS["count"], 2) and (int(u[0]), int(u[1]), float(u[4])) == POINTS["size"] + (POINTS["time"],)
    assert_bits(M.main_image(build, int(u[0]), int(u[1]), float(u[4]), pts[:, 0], pts[:, 1]), fx["points_out"], (build, "points"))
    assert_bits(M.main_image("default", int(u[0]), int(u[1]), float(u[4]), pts[:, 0], pts[:, 1]), fx["points_shipped"], (build, "shipped points"))


@pytest.mark.parametrize("build", NEW)
def test_fixture_conditions(build, oracle):
    """what tools/make_golden_builds.py asserted when it recorded the files, of the committed files"""
    path = fixture_path(os.path.join(ROOT, "tests"), "clouds", build)
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz"))
    assert FAMILY["max_bytes"] == "largest" and os.path.getsize(path) <= largest
    fx = M.fixture(build)
    for name, t, aux_set, frame in fx["frames"]:
        assert not np.isnan(frame).any() and (frame[..., 3] == 1).all()
        over = None if aux_set is None else aux_sets.load()["clouds"][aux_set]
        shipped = oracle.render(1, W, H, t, aux=None if over is None else aux_sets.block("clouds", over))
        n = int((~same_bits(frame, shipped).all(axis=-1)).sum())
        if aux_set is None:
            assert n >= CAPS[build]["min_pixels"], (build, name, n)
        else:
            assert n == fx["aux_counts"][aux_set] and ((n == 0) if aux_set == "zero" else (n > 0)), (build, name, n)
    pts = fx["points"]
    assert (pts[:, 1] >= POINTS["rect"][1]).all() and (pts != np.floor(pts) + .5).any(axis=1).all()      # above the horizon cut, off-centre
    assert FAMILY["no_nan"] and not np.isnan(fx["points_out"]).any()
    assert int((~same_bits(fx["points_out"], fx["points_shipped"]).all(axis=-1)).sum()) >= CAPS[build]["min_points"]


def test_the_two_builds_differ_from_each_other():
    a, b = M.fixture("height"), M.fixture("luminance")
    assert not same_bits(a["frames"][1][3], b["frames"][1][3]).all()


@pytest.mark.parametrize("app", ["clouds_height", "clouds_luminance"])
def test_span_table_is_app_clouds(app):
    """sbx_span_table is host only: the horizon exit of :212 is the same in every build, so are the intervals"""
    import shaderbox_amd
    for t, aux in [(1.5, None), (0.0, shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", aux_sets.load()["clouds"]["steer"]).tobytes()))]:
        got = shaderbox_amd.span_table(app, 256, 144, t, 8, 4, aux=aux)
        want = shaderbox_amd.span_table("clouds", 256, 144, t, 8, 4, aux=aux)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert (want[0][:, 1] - want[0][:, 0] < 256).any()                  # the model cuts something: rows below the horizon
