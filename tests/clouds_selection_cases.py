"""Which kernel a launch of APP_CLOUDS takes (csrc/kern_clouds.hip clouds_select / launch_form, csrc/sbx_ytab.hip render_clouds;
DESIGN.md §5.1): ONE table of named cases that the CPU tests (tests/test_clouds_selection_cpu.py, tests/test_clouds_hashtab_cpu.py)
and the GPU tests (tests/test_gpu_clouds_selection.py) share, and a restatement of the host's nine predicates and of the choice they
make, written from the documented domains (the comments above each predicate in kern_clouds.hip) in binary64 over the
frame constants in binary32 — as the host evaluates them.

A case states the app, the uniforms, the aux fields that differ from the defaults, how it is launched and the kernel it MUST take:
    kernel = (YTAB, REG, LM, SM, GT) of k_clouds<YTAB, REG, LM, SM, BUILD, GT>, or "perlane"
    ytab   = the y table read: 0 none, 1 a slot of the eager ring, 2 the context's big table, 3 a slot of the capture ring
    mode   = "eager"           an ordinary launch (a hash table is built on demand)
             "captured_fresh"  recorded into a graph on a context that has no hash table: nothing is built inside a capture
             "captured_warm"   recorded after two eager launches of the frame, the second of which saw the table complete
Every frame is 96 x 54: marching lanes, straight-up lanes and tile rows cut by the horizon."""
import math

import numpy as np

from tests import clouds_builds_model as M
from tests.model_common import F, ONE, ZERO, cross, normalize

W, H, T = 96, 54, 0.37
MIN_RANGE, MAX_RANGE = 1 << 18, 1 << 22             # csrc/sbx_device.h CLOUDS_HASHTAB_MIN_RANGE / _MAX_RANGE
YTAB_ROWS, YTAB_BIG_MAX = 4096, 1 << 20             # csrc/sbx_device.h CLOUDS_YTAB_ROWS / CLOUDS_YTAB_BIG_MAX
G = 3                                               # GT of the hash-table kernels: 1 + CL_GTAB_OCT (kern_clouds.hip)
BUILD_OF = {"clouds": 0, "clouds_sky": 0, "clouds_height": 1, "clouds_luminance": 2}
INF, NAN = float("inf"), float("nan")

# ---- the kernels that exist: kern_clouds.hip launch_clouds_build, its CL_FORM list line by line ---------------------------------------
#   CL_FORM(1, 1, 1, 1, G) CL_FORM(1, 1, 1, 0, G) CL_FORM(1, 1, 2, 1, G) CL_FORM(1, 1, 2, 0, G)                the hash-table kernels
#   CL_FORM(1, 1, 1, 1, 0) CL_FORM(1, 1, 1, 0, 0) CL_FORM(1, 0, 1, 0, 0)                                        y table + LDS cache
#   CL_FORM(1, 1, 2, 1, 0) CL_FORM(1, 1, 2, 0, 0) CL_FORM(1, 1, 0, 1, 0) CL_FORM(1, 1, 0, 0, 0) CL_FORM(1, 0, 2, 0, 0) CL_FORM(1, 0, 0, 0, 0)
#   CL_FORM(0, 1, 1, 1, 0) CL_FORM(0, 1, 1, 0, 0) CL_FORM(0, 0, 1, 0, 0)                                        table-less
#   CL_FORM(0, 1, 0, 1, 0) CL_FORM(0, 1, 0, 0, 0) CL_FORM(0, 0, 0, 0, 0)
# each instantiated for the shipped build and for LUMINANCE (19 + 19); for HEIGHT only those with LM == 1 (8); and
# k_clouds_perlane<BUILD> for the three builds.
FORMS = [(1, 1, 1, 1, G), (1, 1, 1, 0, G), (1, 1, 2, 1, G), (1, 1, 2, 0, G),
         (1, 1, 1, 1, 0), (1, 1, 1, 0, 0), (1, 0, 1, 0, 0),
         (1, 1, 2, 1, 0), (1, 1, 2, 0, 0), (1, 1, 0, 1, 0), (1, 1, 0, 0, 0), (1, 0, 2, 0, 0), (1, 0, 0, 0, 0),
         (0, 1, 1, 1, 0), (0, 1, 1, 0, 0), (0, 0, 1, 0, 0),
         (0, 1, 0, 1, 0), (0, 1, 0, 0, 0), (0, 0, 0, 0, 0)]
INSTANTIATIONS = ({(b, k) for b in (0, 2) for k in FORMS} | {(1, k) for k in FORMS if k[2] == 1} | {(b, "perlane") for b in (0, 1, 2)})
assert len(FORMS) == 19 and len(INSTANTIATIONS) == 19 + 19 + 8 + 3

# ---- aux fields ---------------------------------------------------------------------------------------------------------------------
YZ = {"sun_dir": (0.0, 0.6, -0.8)}                  # sun_dir * dt has x == 0: the y-z light march
GEN = {"sun_dir": (0.3, 0.2, -0.9)}                 # the general one
NOSM = {"sigma_scattering": 0.3}                    # .94 * .3 * 1.25 = .3525 > .2049: outside exp_small_'s domain
COV1 = {"cld_coverage": 1.0}                        # cov = 0: outside div3_'s domain, so no SM kernel either
NOREG = {"sigma_scattering": 100.0}                 # |sigma dt| = 125 > 80: no regular frame
SIGINF = {"sigma_scattering": INF}                  # nor this
LONG = {"cld_march_steps": 4200, "cld_thick": 137.5}   # more steps than a ring table has rows; dt = .0327: SM up to sigma 6.66, REG up to 2443
LONG_NOSM = dict(LONG, sigma_scattering=30.0)
LONG_NOREG = dict(LONG, sigma_scattering=3000.0)
T_CAP = 3000.0                                      # wind_off.z = 6e5: an index bound of 6.1e6, beyond the largest table's 2^22


def _c(name, app, kernel, ytab, aux=None, t=T, mode="eager", variant=0, mouse=(0.0, 0.0)):
    return dict(name=name, app=app, kernel=kernel, ytab=ytab, aux=dict(aux or {}), t=t, mode=mode, variant=variant, mouse=mouse,
                w=W, h=H)


def _build_cases(p, app, lm_forms):
    """the y-table kernels of one build, reached the same way in each"""
    c = [_c(p + "_gt_z_sm", app, (1, 1, 1, 1, G), 1),
         _c(p + "_gt_z", app, (1, 1, 1, 0, G), 1, NOSM),
         _c(p + "_cache_z_sm", app, (1, 1, 1, 1, 0), 3, mode="captured_fresh"),
         _c(p + "_cache_z", app, (1, 1, 1, 0, 0), 1, NOSM, t=T_CAP),
         _c(p + "_cache_z_noreg", app, (1, 0, 1, 0, 0), 1, SIGINF),
         _c(p + "_capture_gt", app, (1, 1, 1, 1, G), 3, mode="captured_warm"),
         _c(p + "_big_gt", app, (1, 1, 1, 1, G), 2, LONG)]
    if lm_forms:
        c += [_c(p + "_gt_yz_sm", app, (1, 1, 2, 1, G), 1, YZ),
              _c(p + "_gt_yz", app, (1, 1, 2, 0, G), 1, dict(YZ, **NOSM)),
              _c(p + "_cache_yz_sm", app, (1, 1, 2, 1, 0), 1, YZ, t=T_CAP),
              _c(p + "_cache_yz", app, (1, 1, 2, 0, 0), 3, dict(YZ, **NOSM), mode="captured_fresh"),
              _c(p + "_cache_yz_noreg", app, (1, 0, 2, 0, 0), 1, dict(YZ, **NOREG)),
              _c(p + "_cache_gen_sm", app, (1, 1, 0, 1, 0), 1, GEN),
              _c(p + "_cache_gen", app, (1, 1, 0, 0, 0), 1, dict(GEN, **COV1)),
              _c(p + "_cache_gen_noreg", app, (1, 0, 0, 0, 0), 1, dict(GEN, **SIGINF))]
    return c


def _notab_cases(p, app, lm_forms):
    """the table-less kernels through a captured march of 4200 steps (the big table is never allocated inside a capture)"""
    c = [_c(p + "_notab_z_sm", app, (0, 1, 1, 1, 0), 0, LONG, mode="captured_fresh"),
         _c(p + "_notab_z", app, (0, 1, 1, 0, 0), 0, LONG_NOSM, mode="captured_fresh"),
         _c(p + "_notab_z_noreg", app, (0, 0, 1, 0, 0), 0, LONG_NOREG, mode="captured_fresh")]
    if lm_forms:
        c += [_c(p + "_notab_gen_sm", app, (0, 1, 0, 1, 0), 0, dict(LONG, **GEN), mode="captured_fresh"),
              _c(p + "_notab_gen", app, (0, 1, 0, 0, 0), 0, dict(LONG_NOSM, **GEN), mode="captured_fresh"),
              _c(p + "_notab_gen_noreg", app, (0, 0, 0, 0, 0), 0, dict(LONG_NOREG, **GEN), mode="captured_fresh")]
    return c


CASES = (
    _build_cases("d", "clouds", True) +
    # the shipped build's table-less kernels: CLOUDS_SKY (SKY_SPHERE never reads a y table) ...
    [_c("sky_z_sm", "clouds_sky", (0, 1, 1, 1, 0), 0),
     _c("sky_z", "clouds_sky", (0, 1, 1, 0, 0), 0, NOSM),
     _c("sky_z_noreg", "clouds_sky", (0, 0, 1, 0, 0), 0, NOREG),
     _c("sky_gen_sm", "clouds_sky", (0, 1, 0, 1, 0), 0, GEN),
     _c("sky_gen", "clouds_sky", (0, 1, 0, 0, 0), 0, dict(GEN, **COV1)),
     _c("sky_gen_noreg", "clouds_sky", (0, 0, 0, 0, 0), 0, dict(GEN, **SIGINF)),
     # ... and, with a y-z sun, a captured long march (table-less kernels have no y-z form: the general march)
     _c("d_notab_yz_is_gen", "clouds", (0, 1, 0, 1, 0), 0, dict(LONG, **YZ), mode="captured_fresh")] +
    _build_cases("l", "clouds_luminance", True) + _notab_cases("l", "clouds_luminance", True) +
    _build_cases("h", "clouds_height", False) + _notab_cases("h", "clouds_height", False) +
    # HEIGHT has no light march: a general sun still takes the z forms, the hash table included
    [_c("h_gt_general_sun", "clouds_height", (1, 1, 1, 1, G), 1, GEN),
     _c("d_perlane", "clouds", "perlane", 0, variant=1),
     _c("sky_perlane", "clouds_sky", "perlane", 0, variant=1),
     _c("l_perlane", "clouds_luminance", "perlane", 0, variant=1),
     _c("h_perlane", "clouds_height", "perlane", 0, variant=1)])
assert len({c["name"] for c in CASES}) == len(CASES)
BY_NAME = {c["name"]: c for c in CASES}
# one ragged frame (33 x 3) per (LM, SM, GT) of the shipped build: the cases that reach them
RAGGED = ["d_gt_z_sm", "d_gt_z", "d_gt_yz_sm", "d_gt_yz", "d_cache_z_sm", "d_cache_z", "d_cache_yz_sm", "d_cache_yz", "d_cache_gen_sm",
          "d_cache_gen", "sky_z_sm", "sky_z", "sky_gen_sm", "sky_gen"]
RAGGED_GT = [n for n in RAGGED if BY_NAME[n]["kernel"][4]]


def aux_struct(fields):
    """the aux block the C API takes: the defaults with `fields` on top (None for no fields: the library's own defaults)"""
    import shaderbox_amd
    from oracle import aux_sets
    if not fields:
        return None
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", dict(fields)).tobytes())


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def frame_of(app, width, height, time, mouse, aux):
    """FrameClouds' constants (csrc/sbx_frames.hip build_clouds; src/app_clouds.h:23-30, :83-84, :98, :167) in binary32"""
    A = M.aux_block(aux if aux else None)
    sky = app == "clouds_sky"
    f = {"sky": sky, "steps": int(A["cld_march_steps"]), "lsteps": int(A["illum_march_steps"])}
    with np.errstate(all="ignore"):
        f["sigma"] = F(A["sigma_scattering"])
        f["dt"] = F(A["cld_thick"]) / F(f["steps"])
        f["cov"] = ONE - F(A["cld_coverage"])
        f["cov_hi"] = f["cov"] + F(.0135)
        f["cov_d"] = f["cov_hi"] - f["cov"]
        f["cov_r"] = ONE / f["cov_d"]
        f["cov_rd"] = np.float64(1.0) / np.float64(f["cov_d"])
        f["wind"] = [(F(A["wind_dir"][k]) * F(time)) * (ONE / M.NOISE_FACTOR) for k in range(3)]
        f["sun"] = [F(A["sun_dir"][k]) for k in range(3)]
        f["eye"], look_at = M.setup_camera(mouse)
        fwd = normalize(tuple(look_at[k] - f["eye"][k] for k in range(3)))
        right = cross((ZERO, ONE, ZERO), fwd)
        up = cross(fwd, right)
        f["cam"] = [F(v) for v in fwd + up + right]
        f["fov"] = F(1.0)
        f["aspect_fov"] = (F(width) / F(height)) * f["fov"]
        f["nf"] = (ONE / F(A["atm_radius"])) * F(10.0) if sky else F(.001)
        f["atm_r"], f["atm_y"] = F(A["atm_radius"]), F(A["atm_ground_y"])
    return f


def _fin(*v):
    return all(math.isfinite(float(x)) for x in v)


def _m3(v):
    """the largest magnitude of a vector; NaN if any component is (the bound is "inf / NaN if anything it is made of is")"""
    v = [abs(float(x)) for x in v]
    return NAN if any(math.isnan(x) for x in v) else max(v)


def regular(f):
    """the REG shortcuts' frame: finite cov, a finite positive reciprocal of cov_hi - cov, finite sigma and dt, |sigma| |dt| <= 80"""
    return _fin(f["cov"], f["cov_rd"], f["sigma"], f["dt"]) and float(f["cov_rd"]) > 0.0 and abs(float(f["sigma"])) * abs(float(f["dt"])) <= 80.0


def exp_small(f):
    """exp_small_'s domain: sigma, dt >= 0 and .94 sigma dt <= .2049 (NaN: no)"""
    s, d = float(f["sigma"]), float(f["dt"])
    return s >= 0.0 and d >= 0.0 and .94 * s * d <= .2049


def div3_domain(f):
    """div3_'s domain: 2^-20 <= |cov| <= 2^20, the divisor cov_hi - cov within 2^+-60, and its binary32 reciprocal"""
    c, d = abs(float(f["cov"])), abs(float(f["cov_d"]))
    with np.errstate(all="ignore"):
        return (_fin(f["cov"], f["cov_d"], f["cov_r"]) and 2.0 ** -20 <= c <= 2.0 ** 20 and 2.0 ** -60 <= d <= 2.0 ** 60 and
                f["cov_d"] == f["cov_hi"] - f["cov"] and f["cov_r"] == ONE / f["cov_d"])


def reach(f):
    return 21.0 * 150.0 + 22.0 * abs(float(f["dt"])) * float(f["steps"])


def lip_far(f):
    return _m3(f["eye"]) + _m3(f["wind"]) + reach(f)


def lip_domain(f):
    """the Lipschitz skip's domain: every coordinate of every main march position within 2^17"""
    return _fin(*f["wind"]) and lip_far(f) <= 131072.0


def index_bound(f):
    """every lattice index of every main and light sample of the frame is below this in magnitude"""
    light = (f["lsteps"] + 1.0) * _m3(f["sun"]) * abs(float(f["dt"]))
    sky = abs(float(f["atm_r"])) + abs(float(f["atm_y"])) if f["sky"] else 0.0
    P = _m3(f["eye"]) + _m3(f["wind"]) + reach(f) + light + sky
    return 271.0 * (P * abs(float(f["nf"])) * 2.03 * 18.4 + 2.0)


def index_domain(f):
    """sin_b40_'s domain: the bound at most 2^39"""
    return index_bound(f) <= 2.0 ** 39              # NaN compares false


def light_form(f):
    """sun_dir * dt in binary32: 1 z-only, 2 y-z, 0 general (NaN compares false)"""
    with np.errstate(all="ignore"):
        x, y = f["sun"][0] * f["dt"], f["sun"][1] * f["dt"]
    return 1 if (x == 0 and y == 0) else 2 if x == 0 else 0


def hashtab_range(f, build, point_list=False):
    """the range R of the hash table the frame needs (the table holds the indices [-R, R + 271]); 0: no table kernel"""
    if f["sky"] or point_list or f["steps"] <= 0 or not regular(f):
        return 0
    if not (build == 1 or light_form(f) in (1, 2)):
        return 0
    if not all(abs(float(v)) <= 4.0 for v in f["cam"]):            # NaN compares false
        return 0
    if not (abs(float(f["fov"])) <= 1e6 and abs(float(f["aspect_fov"])) <= 1e6):
        return 0
    n = index_bound(f)
    if not n <= MAX_RANGE:
        return 0
    R = MIN_RANGE
    while R < n:
        R *= 2
    return R


def select(f, build, variant=0, ytab_rows=YTAB_ROWS, table_range=0, point_list=False):
    """the record of sbx_debug_clouds_select (without `launches`), from the predicates above"""
    S = dict(build=build, perlane=0, ytab_used=0, reg=0, lm=0, sm=0, gt=0, ytab=0, sky=int(f["sky"]),
             regular=int(regular(f)), exp_small=int(exp_small(f)), index_domain=int(index_domain(f)), div3_domain=int(div3_domain(f)),
             lip_ok=int(lip_domain(f)), light=light_form(f), need_range=hashtab_range(f, build, point_list),
             table_range=max(int(table_range), 0))
    if f["sky"]:
        ytab_rows, S["table_range"] = 0, 0
    reg = bool(S["regular"])
    sm = bool(S["exp_small"] and S["index_domain"] and S["div3_domain"])
    zl = build == 1 or S["light"] == 1
    yz = not zl and S["light"] == 2
    if variant == 1:
        S["perlane"] = 1
        return S
    if ytab_rows > 0 and 0 < f["steps"] <= ytab_rows:
        S["ytab_used"], S["ytab"] = 1, 1 if ytab_rows <= YTAB_ROWS else 2
        if 0 < S["need_range"] <= S["table_range"]:
            S.update(reg=1, lm=1 if zl else 2, sm=int(sm), gt=G)
        elif zl:
            S.update(reg=int(reg), lm=1, sm=int(reg and sm))
        elif reg:
            S.update(reg=1, lm=2 if yz else 0, sm=int(sm))
        else:
            S.update(reg=0, lm=2 if yz else 0, sm=0)
    else:
        S.update(reg=int(reg), lm=1 if zl else 0, sm=int(reg and sm))
    return S


def launch_context(case, f=None):
    """what sbx_ytab.hip's render_clouds hands the launch of `case`: (rows of the y table at hand, its kind, range of the ready hash table)"""
    f = f or frame_of(case["app"], case["w"], case["h"], case["t"], case["mouse"], case["aux"])
    if f["sky"] or case["variant"] == 1:
        return 0, 0, 0
    steps, captured = f["steps"], case["mode"] != "eager"
    if 0 < steps <= YTAB_ROWS:
        rows, kind = YTAB_ROWS, 3 if captured else 1
    elif YTAB_ROWS < steps <= YTAB_BIG_MAX and not captured:
        rows, kind = (steps + 4095) // 4096 * 4096, 2
    else:
        return 0, 0, 0
    need = hashtab_range(f, BUILD_OF[case["app"]])
    return rows, kind, 0 if case["mode"] == "captured_fresh" else need


def kernel_of(rec):
    return "perlane" if rec["perlane"] else (rec["ytab_used"], rec["reg"], rec["lm"], rec["sm"], rec["gt"])


# ---- the table-range edges: u_time by bisection on the restated bound ----------------------------------------------------------------------
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _from_bits(b):
    return float(np.uint32(b).view(np.float32))


def time_at_bound(limit, app="clouds", aux=None):
    """(t_lo, t_hi): adjacent binary32 times with index_bound(t_lo) <= limit < index_bound(t_hi); default wind, growing with t"""
    bound = lambda t: index_bound(frame_of(app, W, H, t, (0.0, 0.0), aux))   # noqa: E731
    lo, hi = _bits(0.0), _bits(1e5)
    assert bound(_from_bits(lo)) <= limit < bound(_from_bits(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bound(_from_bits(mid)) <= limit:
            lo = mid
        else:
            hi = mid
    return _from_bits(lo), _from_bits(hi)


RANGE_EDGES = [1 << k for k in range(18, 23)]


def range_edge_cases(sun="z"):
    """per edge 2^k: the frame just inside (its table has range 2^k) and the frame just beyond (2^(k+1); beyond 2^22: none, GT == 0)"""
    aux = YZ if sun == "yz" else {}
    lm = 2 if sun == "yz" else 1
    out = []
    for e in RANGE_EDGES:
        lo, hi = time_at_bound(float(e), aux=aux)
        beyond = (1, 1, lm, 1, G) if e < MAX_RANGE else (1, 1, lm, 1, 0)
        out.append((e, _c("edge_%s_2p%d_in" % (sun, e.bit_length() - 1), "clouds", (1, 1, lm, 1, G), 1, aux, t=lo),
                    _c("edge_%s_2p%d_out" % (sun, e.bit_length() - 1), "clouds", beyond, 1, aux, t=hi)))
    return out


# ---- the predicate edges whose two sides are rendered (tests/test_gpu_clouds_selection.py) ---------------------------------------------
UNIT = {"cld_thick": 100.0, "cld_march_steps": 100}            # dt = 1 exactly


def _up(x):
    return float(np.nextafter(F(x), F(INF)))


def exp_small_edge():
    """adjacent binary32 sigmas (s, next up) with .94 s <= .2049 < .94 next, for dt = 1"""
    s = float(F(.2049 / .94))
    while .94 * s > .2049:
        s = float(np.nextafter(F(s), F(-INF)))
    while .94 * _up(s) <= .2049:
        s = _up(s)
    return s, _up(s)


# (name, the record field that differs, aux inside the domain, aux just outside)
PREDICATE_EDGES = [("exp_small", "exp_small", dict(UNIT, sigma_scattering=exp_small_edge()[0]), dict(UNIT, sigma_scattering=exp_small_edge()[1])),
                   ("regular", "regular", dict(UNIT, sigma_scattering=80.0), dict(UNIT, sigma_scattering=_up(80.0))),
                   ("div3", "div3_domain", {"cld_coverage": 1.0 - 2.0 ** -20}, {"cld_coverage": 1.0 - 2.0 ** -21})]
