"""CPU check of the index bound behind APP_CLOUDS' lattice-hash table (csrc/kern_clouds.hip clouds_index_bound / clouds_hashtab_range,
GTab): the table holds hash(n) for the lattice indices [-R, R + 271], a lookup is unchecked, so every index a lane of a table kernel
can form must lie strictly inside that range.  The bound is restated here and every index is enumerated with the numpy march model
(tests/clouds_builds_model.py: camera, ray, origin, wind, step — binary32, the kernel's operation order): every main sample of every
marching pixel for the WHOLE march (a lane goes on sampling after its own pixel is opaque, as long as its wave marches), every light
sample of every main sample (lit or not: a lane runs the light march of its wave's lit lanes), all four octaves, all eight corners —
and the straight-up ray the kernel gives the lanes that do not march."""
import numpy as np
import pytest

from tests import clouds_builds_model as M
from tests import clouds_selection_cases as C
from tests.model_common import F, ONE, ZERO, _f, get_primary_ray, point_cam

MIN_RANGE, MAX_RANGE = 1 << 18, 1 << 22             # csrc/sbx_device.h CLOUDS_HASHTAB_MIN_RANGE / _MAX_RANGE
CORNERS = (0.0, 1.0, 157.0, 158.0, 113.0, 114.0, 270.0, 271.0)


def index_bound(eye, wind, sun_dir, dt, steps, lsteps):
    """clouds_index_bound (no SKY_SPHERE, noise factor .001), in binary64 like the host"""
    m3 = lambda v: max(abs(float(c)) for c in v)    # noqa: E731
    reach = 21.0 * 150.0 + 22.0 * abs(float(dt)) * steps
    light = (lsteps + 1.0) * m3(sun_dir) * abs(float(dt))
    P = m3(eye) + m3(wind) + reach + light
    return 271.0 * (P * 0.001 * 2.03 * 18.4 + 2.0)


def table_range(bound):
    """clouds_hashtab_range's R: the power of two at or above the bound, at least MIN_RANGE; 0 beyond the cap"""
    if not bound <= MAX_RANGE:
        return 0
    R = MIN_RANGE
    while R < bound:
        R *= 2
    return R


def lattice_extremes(pos):
    """(min, max) over the four octaves of the lattice index n = px + 157 py + 113 pz of the samples `pos` (three binary32 arrays),
    in the kernel's operations: q = (pos * .001) * 2.03, then q *= 2.64 per octave"""
    q = [(_f(c) * M.NOISE_FACTOR) * F(2.03) for c in pos]
    lo, hi = np.inf, -np.inf
    for _ in range(4):
        p = [np.floor(c) for c in q]
        n = (p[0] + p[1] * F(157.0)) + F(113.0) * p[2]
        assert n.dtype == F and np.isfinite(n).all()
        lo, hi = min(lo, float(n.min())), max(hi, float(n.max()))
        q = [c * F(2.64) for c in q]
    return lo, hi


def frame_extremes(width, height, u_time, mouse, aux=None):
    """(lowest index, highest index + 271, bound) over every sample the table kernels' lanes of the frame can evaluate"""
    A = M.aux_block(aux)
    steps, lsteps = int(A["cld_march_steps"]), int(A["illum_march_steps"])
    fx = np.broadcast_to((np.arange(width, dtype=F) + F(.5))[None, :], (height, width)).ravel()
    fy = np.broadcast_to((np.arange(height, dtype=F) + F(.5))[:, None], (height, width)).ravel()
    pcx, pcy = point_cam(width, height, fx, fy, M.FOV)
    eye, look_at = M.setup_camera(mouse)
    d = get_primary_ray(pcx, pcy, eye, look_at)
    marching = ~(d[1] < F(0.05))
    assert marching.any() and not marching.all()    # the frame has both kinds of lanes
    wind = [(A["wind_dir"][k] * F(u_time)) * (ONE / M.NOISE_FACTOR) for k in range(3)]
    dt = A["cld_thick"] / F(steps)
    proj = [np.append(d[k][marching] / d[1][marching], F(1.0 if k == 1 else 0.0)) for k in range(3)]   # + the straight-up ray
    origin = [(eye[k] + proj[k] * F(150.)) + wind[k] for k in range(3)]
    lstep = [A["sun_dir"][k] * dt for k in range(3)]
    lo, hi = np.inf, -np.inf
    t = ZERO
    for _ in range(steps):
        pos = [origin[k] + t * proj[k] for k in range(3)]
        t = t + dt
        samples = [pos]
        lp = [pos[k] + lstep[k] for k in range(3)]
        for _ in range(lsteps):
            samples.append(lp)
            lp = [lp[k] + lstep[k] for k in range(3)]
        a, b = lattice_extremes([np.concatenate([s[k] for s in samples]) for k in range(3)])
        lo, hi = min(lo, a), max(hi, b)
    return lo, hi + max(CORNERS), index_bound(eye, wind, A["sun_dir"], dt, steps, lsteps)


FRAMES = [(96, 54, 0.37, (0.0, 0.0)), (33, 3, 0.37, (0.0, 0.0)), (96, 54, 200.0, (0.0, 0.0)), (33, 3, 200.0, (0.0, 0.0)),
          (96, 54, 0.37, (300.0, 40.0)), (96, 54, 200.0, (1234.5, 7.0)), (33, 3, 0.37, (1234.5, 7.0)), (33, 3, 200.0, (300.0, 40.0))]


@pytest.mark.parametrize("sun", [None, (0.0, 0.6, -0.8)], ids=["z_sun", "yz_sun"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d_t%g_m%g" % (f[0], f[1], f[2], f[3][0]))
def test_every_lattice_index_lies_inside_the_table(frame, sun):
    w, h, t, mouse = frame
    lo, hi, bound = frame_extremes(w, h, t, mouse, None if sun is None else {"sun_dir": sun})
    R = table_range(bound)
    assert R >= MIN_RANGE and bound <= R            # these frames take a table
    # strictly inside the host's bound itself — hence inside the table's [-R, R + 271], guards untouched
    assert -bound < lo and hi < bound, (lo, hi, bound)
    assert -R < lo and hi < R + 271


def test_default_frame_and_grown_frame_ranges():
    """the default frame fits the smallest table; u_time = 200 (wind_off.z = 4e4) needs the next one; a wind beyond the cap, none"""
    b0 = frame_extremes(33, 3, 0.37, (0.0, 0.0))[2]
    b1 = frame_extremes(33, 3, 200.0, (0.0, 0.0))[2]
    assert 6.0e4 < b0 < 7.0e4 and table_range(b0) == MIN_RANGE
    assert table_range(b1) == 2 * MIN_RANGE
    assert table_range(index_bound((0, -.5, 0), (0, 0, .2 * 3000.0 * 1000.0), (0, 0, -1), 1.25, 100, 6)) == 0
    assert table_range(float("inf")) == 0 and table_range(float("nan")) == 0


# ---- every frame the GPU suite sends through a hash-table kernel (tests/clouds_selection_cases.py) --------------------------------------
# No case goes to the GPU that has not passed this enumeration: tests/test_gpu_clouds_selection.py renders exactly these frames (the
# table's GT cases, the frames either side of every table-range edge, the ragged frames of the default build's GT forms and the
# sides of the predicate edges that take a table).
GT_FRAMES = ([c for c in C.CASES if c["kernel"] != "perlane" and c["kernel"][4]] +
             [c for sun in ("z", "yz") for _, a, b in C.range_edge_cases(sun) for c in (a, b) if c["kernel"][4]] +
             [dict(c, name=c["name"] + "_33x3", w=33, h=3) for c in C.CASES if c["name"] in C.RAGGED_GT] +
             [C._c("%s_%s" % (e[0], side), "clouds", None, 1, aux) for e in C.PREDICATE_EDGES for side, aux in (("in", e[2]), ("out", e[3]))
              if C.hashtab_range(C.frame_of("clouds", C.W, C.H, C.T, (0.0, 0.0), aux), 0)])


@pytest.mark.parametrize("case", GT_FRAMES, ids=lambda c: c["name"])
def test_selection_cases_stay_inside_their_table(case):
    f = C.frame_of(case["app"], case["w"], case["h"], case["t"], case["mouse"], case["aux"])
    R = C.hashtab_range(f, C.BUILD_OF[case["app"]])
    lo, hi, bound = frame_extremes(case["w"], case["h"], case["t"], case["mouse"], case["aux"] or None)
    # (index_bound above takes the noise factor as .001; the host, and C.index_bound, as the binary32 nearest to it: 5e-8 apart)
    host = C.index_bound(f)
    assert abs(bound - host) <= 1e-7 * host and R == table_range(host) and R >= MIN_RANGE, (bound, host, R)
    bound = min(bound, host)
    assert -bound < lo and hi < bound, (lo, hi, bound)
    assert -R < lo and hi < R + 271
