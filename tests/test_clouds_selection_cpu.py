"""CPU tests of APP_CLOUDS' kernel selection through sbx_debug_clouds_select (include/sbx_test.h; csrc/kern_clouds.hip clouds_select):
host code of libsbx.so, no GPU.  The table of tests/clouds_selection_cases.py selects what it states and reaches every instantiation
of k_clouds / k_clouds_perlane the launcher holds; each of the host's predicates is stepped across its edge and compared with the
restatement of that module (binary64 over the binary32 frame constants); and a seeded fuzz of 10^4 uniforms and aux blocks, non-finite
fields included, compares the whole record.

Two of the issue's edge values cannot be produced through sbx_uniforms and sbx_aux_clouds and are therefore not stepped here: a camera
entry of 4 (the camera of app_clouds.h:23-30 is orthonormal: its entries are at most 1 or NaN) and a fov of 1e6 (app_clouds.h:219 fixes
FOV at 1.; the other product the host bounds by 1e6, aspect * fov, is stepped through u_res), and cov_rd == 0 (cov_hi - cov cannot be
infinite: it is 0, NaN or about .0135)."""
import os
import re

import numpy as np
import pytest

import shaderbox_amd
from tests import clouds_selection_cases as C
from tests.model_common import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = C.INF, C.NAN
UNIT = C.UNIT                                                  # dt = 1 exactly


@pytest.fixture(scope="module")
def lib():
    from shaderbox_amd import build
    build.build(verbose=False)
    return shaderbox_amd.load_library()


def hook(lib, app="clouds", aux=None, t=C.T, mouse=(0.0, 0.0), w=C.W, h=C.H, variant=0, ytab_rows=C.YTAB_ROWS, table_range=0, point_list=False):
    got = shaderbox_amd.clouds_select(app, w, h, t, mouse, C.aux_struct(aux), variant, ytab_rows, table_range, point_list, lib=lib)
    assert got.pop("launches") == 0
    return got


def both(lib, app="clouds", aux=None, t=C.T, mouse=(0.0, 0.0), w=C.W, h=C.H, variant=0, ytab_rows=C.YTAB_ROWS, table_range=0, point_list=False):
    """the hook's record, after asserting that it is the restatement's"""
    got = hook(lib, app, aux, t, mouse, w, h, variant, ytab_rows, table_range, point_list)
    f = C.frame_of(app, w, h, t, mouse, aux)
    want = C.select(f, C.BUILD_OF[app], variant, ytab_rows, table_range, point_list)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    return got


def up(x):
    return float(np.nextafter(F(x), F(INF)))


def down(x):
    return float(np.nextafter(F(x), F(-INF)))


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in C.CASES])
def test_case_selects_what_it_states(lib, name):
    c = C.BY_NAME[name]
    rows, kind, table = C.launch_context(c)
    got = both(lib, c["app"], c["aux"], c["t"], c["mouse"], c["w"], c["h"], c["variant"], rows, table)
    assert C.kernel_of(got) == c["kernel"], (name, got)
    assert got["build"] == C.BUILD_OF[c["app"]] and got["sky"] == (c["app"] == "clouds_sky")
    # (the hook has no context: it reports a ring table for the capture ring's slot)
    assert got["ytab"] == {0: 0, 1: 1, 2: 2, 3: 1}[c["ytab"]] and kind == c["ytab"]
    assert (got["gt"] != 0) == (0 < got["need_range"] <= got["table_range"] and got["ytab_used"] == 1 and not got["perlane"])


def launcher_forms():
    """the CL_FORM list of kern_clouds.hip's launch_clouds_build, as written there"""
    src = open(os.path.join(ROOT, "shaderbox_amd", "csrc", "kern_clouds.hip")).read()
    body = src[src.index("static bool launch_clouds_build("):src.index("#undef CL_FORM")]
    forms = re.findall(r"CL_FORM\((\d), (\d), (\d), (\d), (G|0)\)", body)
    assert "constexpr int G = CL_GTAB_OCT + 1;" in body and re.search(r"#define CL_GTAB_OCT 2\b", src)
    assert body.count("CL_FORM(") == len(forms) + 1                # + the macro's definition: no call in another spelling
    return [tuple(int(v) for v in f[:4]) + (C.G if f[4] == "G" else 0,) for f in forms]


def test_table_reaches_exactly_the_launchers_instantiations(lib):
    forms = launcher_forms()
    assert len(forms) == len(set(forms)) == 19 and set(forms) == set(C.FORMS)
    src = open(os.path.join(ROOT, "shaderbox_amd", "csrc", "kern_clouds.hip")).read()
    # every launch of the two kernels is the launcher's: one hipLaunchKernelGGL each, and HEIGHT is kept to LM == 1 there
    assert len(re.findall(r"hipLaunchKernelGGL\(\(?k_clouds<", src)) == 1 and len(re.findall(r"hipLaunchKernelGGL\(k_clouds_perlane<", src)) == 1
    assert "if constexpr ((LMV) == 1 || !HT)" in src
    reached = set()
    for c in C.CASES:
        rows, _, table = C.launch_context(c)
        got = hook(lib, c["app"], c["aux"], c["t"], c["mouse"], c["w"], c["h"], c["variant"], rows, table)
        reached.add((got["build"], C.kernel_of(got)))
    assert reached == C.INSTANTIATIONS, (sorted(map(str, C.INSTANTIATIONS - reached)), sorted(map(str, reached - C.INSTANTIATIONS)))


# ---- 2. the predicates at their edges ----------------------------------------------------------------------------------------------
def test_regular_edges(lib):
    """|sigma| |dt| = 80 and the next value up (dt = 1); a reciprocal of cov_hi - cov that is inf or NaN"""
    for sign in (1.0, -1.0):
        a = both(lib, aux=dict(UNIT, sigma_scattering=sign * 80.0))
        b = both(lib, aux=dict(UNIT, sigma_scattering=sign * up(80.0)))
        assert (a["regular"], a["reg"]) == (1, 1) and (b["regular"], b["reg"]) == (0, 0)
    a = both(lib, aux=dict(cld_thick=-100.0, cld_march_steps=100, sigma_scattering=80.0))     # |dt|: dt = -1
    b = both(lib, aux=dict(cld_thick=-100.0, cld_march_steps=100, sigma_scattering=up(80.0)))
    assert (a["regular"], b["regular"]) == (1, 0)
    for cov, why in ((-1e10, "cov_hi == cov: 1 / 0 = inf"), (-INF, "inf - inf"), (NAN, "NaN"), (INF, "cov = -inf")):
        r = both(lib, aux={"cld_coverage": cov})
        assert (r["regular"], r["reg"], r["sm"], r["need_range"]) == (0, 0, 0, 0), why
    for field in ("sigma_scattering", "cld_thick"):
        for v in (INF, -INF, NAN):
            assert both(lib, aux={field: v})["regular"] == 0, (field, v)
    assert both(lib, aux={"cld_march_steps": 0})["regular"] == 0                                # dt = 125 / 0


def test_exp_small_edges(lib):
    """.94 sigma dt against .2049 one float either side (dt = 1); sigma or dt -0, negative, NaN"""
    s, s_up = C.exp_small_edge()
    assert s_up == up(s) and .94 * s <= .2049 < .94 * s_up and float(F(s)) == s
    a = both(lib, aux=dict(UNIT, sigma_scattering=s))
    b = both(lib, aux=dict(UNIT, sigma_scattering=up(s)))
    assert (a["exp_small"], a["sm"]) == (1, 1) and (b["exp_small"], b["sm"], b["reg"]) == (0, 0, 1)
    assert C.kernel_of(a) != C.kernel_of(b)
    for aux, want in ((dict(UNIT, sigma_scattering=-0.0), 1), (dict(UNIT, sigma_scattering=-.01), 0), (dict(UNIT, sigma_scattering=NAN), 0),
                      (dict(cld_thick=-0.0, cld_march_steps=100), 1), (dict(cld_thick=-1.0, cld_march_steps=100), 0),
                      (dict(cld_thick=NAN, cld_march_steps=100), 0), (dict(UNIT, sigma_scattering=0.0), 1)):
        r = both(lib, aux=aux)
        assert r["exp_small"] == want and (r["sm"] == 1) == (want == 1 and r["regular"] == 1), aux
    # the two sides as the aux sets exp_on / exp_off place them (dt = 1.25)
    assert both(lib, aux={"sigma_scattering": 0.1743})["sm"] == 1 and both(lib, aux={"sigma_scattering": 0.1745})["sm"] == 0


def test_div3_edges(lib):
    """|cov| at 2^-20 and 2^-21; cov 0; a coverage so large that cov_hi == cov"""
    a = both(lib, aux={"cld_coverage": 1.0 - 2.0 ** -20})
    b = both(lib, aux={"cld_coverage": 1.0 - 2.0 ** -21})
    assert (a["div3_domain"], a["sm"]) == (1, 1) and (b["div3_domain"], b["sm"], b["reg"], b["exp_small"]) == (0, 0, 1, 1)
    assert both(lib, aux={"cld_coverage": 1.0 + 2.0 ** -20})["sm"] == 1 and both(lib, aux={"cld_coverage": 1.0 + 2.0 ** -21})["sm"] == 0
    z = both(lib, aux={"cld_coverage": 1.0})
    assert (z["div3_domain"], z["sm"], z["reg"]) == (0, 0, 1)
    big = both(lib, aux={"cld_coverage": -1e10})
    assert (big["div3_domain"], big["sm"]) == (0, 0)
    # cov = 2^17: .0135 rounds to one ulp, cov_hi - cov = 2^-6; cov = 2^18: to none, cov_hi == cov (the divisor 0, well before |cov| = 2^20)
    assert both(lib, aux={"cld_coverage": 1.0 - 2.0 ** 17})["div3_domain"] == 1
    assert both(lib, aux={"cld_coverage": 1.0 - 2.0 ** 18})["div3_domain"] == 0


def test_lip_edges(lib):
    """far = |eye| + |wind_off| + reach against 131072: times 620 / 630 with the default wind, and the two adjacent times at the edge"""
    assert both(lib, t=620.0)["lip_ok"] == 1 and both(lib, t=630.0)["lip_ok"] == 0
    far = lambda t: C.lip_far(C.frame_of("clouds", C.W, C.H, t, (0.0, 0.0), None))   # noqa: E731
    lo, hi = 620.0, 630.0
    while up(lo) < hi:
        mid = float(F((lo + hi) / 2))
        lo, hi = (mid, hi) if far(mid) <= 131072.0 else (lo, mid)
    assert far(lo) <= 131072.0 < far(hi) and hi == up(lo)
    assert both(lib, t=lo)["lip_ok"] == 1 and both(lib, t=hi)["lip_ok"] == 0
    for wind in ((NAN, 0.0, 0.2), (0.0, INF, 0.2)):
        assert both(lib, aux={"wind_dir": wind})["lip_ok"] == 0


def test_index_domain_edge(lib):
    """the index bound at 2^39: the SM kernels' sin_b40_ on one side only"""
    bound = lambda t: C.index_bound(C.frame_of("clouds", C.W, C.H, t, (0.0, 0.0), None))   # noqa: E731
    lo, hi = C._bits(1e6), C._bits(1e12)
    assert bound(C._from_bits(lo)) <= 2.0 ** 39 < bound(C._from_bits(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if bound(C._from_bits(mid)) <= 2.0 ** 39 else (lo, mid)
    a, b = both(lib, t=C._from_bits(lo)), both(lib, t=C._from_bits(hi))
    assert (a["index_domain"], a["sm"]) == (1, 1) and (b["index_domain"], b["sm"], b["reg"]) == (0, 0, 1)
    assert a["need_range"] == b["need_range"] == 0 and a["lip_ok"] == 0


@pytest.mark.parametrize("sun", ["z", "yz"])
def test_hashtab_range_edges(lib, sun):
    """the bound one binary32 time either side of 2^18 ... 2^22: the range doubles at each edge and is 0 beyond the cap"""
    for e, inside, beyond in C.range_edge_cases(sun):
        a = both(lib, aux=inside["aux"], t=inside["t"], table_range=C.MAX_RANGE)
        b = both(lib, aux=beyond["aux"], t=beyond["t"], table_range=C.MAX_RANGE)
        assert a["need_range"] == max(e, C.MIN_RANGE) and b["need_range"] == (2 * e if e < C.MAX_RANGE else 0)
        assert C.kernel_of(a) == inside["kernel"] and C.kernel_of(b) == beyond["kernel"]
        # a table one size too small is not taken
        assert both(lib, aux=beyond["aux"], t=beyond["t"], table_range=e)["gt"] == 0
        assert both(lib, aux=inside["aux"], t=inside["t"], table_range=e)["gt"] == (C.G if e >= C.MIN_RANGE else 0)


def test_hashtab_range_other_conditions(lib):
    R = C.MIN_RANGE
    assert both(lib, table_range=R)["gt"] == C.G
    # aspect * fov at 1e6 and just above
    assert both(lib, w=1e6, h=1.0, table_range=R)["need_range"] == R and both(lib, w=1000001.0, h=1.0, table_range=R)["need_range"] == 0
    assert both(lib, w=C.W, h=0.0, table_range=R)["need_range"] == 0 and both(lib, w=0.0, h=0.0, table_range=R)["need_range"] == 0
    for mouse in ((NAN, 0.0), (INF, 0.0), (-INF, 5.0)):
        r = both(lib, mouse=mouse, table_range=R)
        assert (r["need_range"], r["gt"], r["reg"], r["lm"]) == (0, 0, 1, 1), mouse
    assert both(lib, mouse=(0.0, NAN), table_range=R)["gt"] == C.G                         # u_mouse.y is not read (app_clouds.h:26)
    # no march: steps 0; negative steps are refused before any choice is made
    z = both(lib, aux={"cld_march_steps": 0}, table_range=R)
    assert (z["need_range"], z["ytab_used"], z["gt"]) == (0, 0, 0)
    with pytest.raises(shaderbox_amd.SbxError):
        hook(lib, aux={"cld_march_steps": -1})
    with pytest.raises(shaderbox_amd.SbxError):
        hook(lib, aux={"illum_march_steps": -1})
    with pytest.raises(shaderbox_amd.SbxError):
        hook(lib, app="egg")
    # a point list, SKY_SPHERE, the general sun, no regular frame, the per-lane variant: no table kernel
    assert both(lib, point_list=True, table_range=R)["need_range"] == 0
    assert both(lib, app="clouds_sky", table_range=R)["need_range"] == 0
    assert both(lib, aux=C.GEN, table_range=R)["need_range"] == 0 and both(lib, app="clouds_height", aux=C.GEN, table_range=R)["gt"] == C.G
    assert both(lib, aux=C.NOREG, table_range=R)["need_range"] == 0
    p = both(lib, variant=1, table_range=R)
    assert (p["perlane"], p["gt"], p["need_range"]) == (1, 0, R)


def test_ytab_row_edges(lib):
    """4096 / 4097 steps against a ring table; 2^20 / 2^20 + 1 against the big table's cap (the hook only: never rendered)"""
    for steps, rows, used, kind in ((4096, 4096, 1, 1), (4097, 4096, 0, 0), (4097, 8192, 1, 2), (8192, 8192, 1, 2), (8193, 8192, 0, 0),
                                    (1 << 20, 1 << 20, 1, 2), ((1 << 20) + 1, 1 << 20, 0, 0), (100, 0, 0, 0)):
        r = both(lib, aux={"cld_march_steps": steps, "cld_thick": 137.5}, ytab_rows=rows)
        assert (r["ytab_used"], r["ytab"]) == (used, kind), (steps, rows)
    # what render_clouds hands the launch at those step counts (csrc/sbx_ytab.hip), restated in launch_context
    for steps, mode, want in ((4096, "eager", (4096, 1)), (4097, "eager", (8192, 2)), (4096, "captured_fresh", (4096, 3)),
                              (4097, "captured_fresh", (0, 0)), (1 << 20, "eager", (1 << 20, 2)), ((1 << 20) + 1, "eager", (0, 0))):
        c = C._c("x", "clouds", None, 0, {"cld_march_steps": steps, "cld_thick": 137.5}, mode=mode)
        assert C.launch_context(c)[:2] == want, (steps, mode)


def test_light_march_forms(lib):
    """sun_dir * dt with an x of +-0, a denormal x (which a small dt rounds to 0: the march runs on the product), NaN"""
    den = float(np.float32(1e-45))
    for sun, aux, light in (((0.0, 0.0, -1.0), {}, 1), ((-0.0, -0.0, -1.0), {}, 1), ((-0.0, 0.6, -0.8), {}, 2), ((0.0, 0.6, -0.8), {}, 2),
                            ((den, 0.0, -1.0), {}, 0), ((den, 0.6, -0.8), {}, 0), ((den, 0.0, -1.0), C.LONG, 1), ((den, 0.6, -0.8), C.LONG, 2),
                            ((0.0, den, -1.0), C.LONG, 1), ((NAN, 0.0, -1.0), {}, 0), ((0.0, NAN, -1.0), {}, 2), ((0.3, 0.2, -0.9), {}, 0)):
        r = both(lib, aux=dict(aux, sun_dir=sun), ytab_rows=8192)
        assert (r["light"], r["lm"]) == (light, light), (sun, aux)
        h = both(lib, app="clouds_height", aux=dict(aux, sun_dir=sun), ytab_rows=8192)
        assert (h["light"], h["lm"]) == (light, 1)
    # dt = NaN or inf: 0 * NaN
    assert both(lib, aux={"cld_thick": NAN})["light"] == 0 and both(lib, aux={"cld_thick": INF})["light"] == 0


# ---- 3. fuzz ------------------------------------------------------------------------------------------------------------------------
SPECIAL = [0.0, -0.0, INF, -INF, NAN, 1e-45, -1e-45, 1.0, -1.0, 3.4e38]


def _value(rng, lo, hi):
    k = rng.integers(0, 10)
    if k == 0:
        return float(rng.choice(SPECIAL))
    if k == 1:
        return float(F(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-12, 12)))
    return float(F(rng.uniform(lo, hi)))


def test_fuzz_hook_equals_restatement(lib):
    rng = np.random.default_rng(20261019)
    apps = list(C.BUILD_OF)
    kernels = set()
    for i in range(10000):
        aux = {"wind_dir": tuple(_value(rng, -.3, .3) for _ in range(3)),
               "sun_dir": tuple(float(rng.choice([0.0, -0.0])) if rng.integers(0, 3) == 0 else _value(rng, -1, 1) for _ in range(3)),
               "sigma_scattering": _value(rng, 0, .4), "cld_coverage": _value(rng, 0, 1.1), "cld_thick": _value(rng, 50, 200),
               "atm_radius": _value(rng, 50, 6000), "atm_ground_y": _value(rng, 20, 6000),
               "cld_march_steps": int(rng.choice([0, 1, 40, 100, 4096, 4097, 4200, 1 << 20, (1 << 20) + 1, int(rng.integers(0, 6000))])),
               "illum_march_steps": int(rng.choice([0, 6, 9, int(rng.integers(0, 2000))]))}
        t = _value(rng, 0, 4000) if rng.integers(0, 4) else float(F(10.0 ** rng.uniform(-3, 10)))
        mouse = (_value(rng, -2000, 2000), _value(rng, -100, 100))
        w, h = (float(rng.integers(1, 4000)), float(rng.integers(1, 3000))) if rng.integers(0, 8) else (_value(rng, 0, 1e7), _value(rng, 0, 4))
        app = apps[int(rng.integers(0, 4))]
        got = both(lib, app, aux, t, mouse, w, h, variant=int(rng.integers(0, 5) == 0), ytab_rows=int(rng.choice([0, 4096, 8192, 1 << 20])),
                   table_range=int(rng.choice([0, 0, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22])), point_list=bool(rng.integers(0, 6) == 0))
        kernels.add((got["build"], C.kernel_of(got)))
        assert (got["build"], C.kernel_of(got)) in C.INSTANTIATIONS, (i, got)
    assert len(kernels) >= 40                        # the fuzz is no idle one: it walks most of the launcher


def test_rendered_predicate_edges_differ_in_their_field(lib):
    """the pairs tests/test_gpu_clouds_selection.py renders: one record field apart, and another kernel on either side"""
    for name, field, inside, outside in C.PREDICATE_EDGES:
        a, b = both(lib, aux=inside, table_range=C.MIN_RANGE), both(lib, aux=outside, table_range=C.MIN_RANGE)
        assert (a[field], b[field]) == (1, 0) and C.kernel_of(a) != C.kernel_of(b), name
