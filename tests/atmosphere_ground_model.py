"""numpy restatement of SBX_APP_ATMOSPHERE_GROUND (src/app_atmosphere.h built without FROM_SPACE; include/sbx.h).

The CPU oracle renders the FROM_SPACE build only, so the GPU tests compare against this module, and this module is compared bit
for bit with src/app_atmosphere.h compiled without its FROM_SPACE line (oracle/_ref/libsbx_ref_atmosphere_ground.so;
tests/test_oracle_vs_reference.py).  What it adds to
the oracle is little: mainImage's camera part (oracle/ref_apps.h:29-40), get_primary_ray and intersect_plane (oracle/ref_lib.h),
restated in binary32 step by step in the oracle's operation order (oracle/ovec.h: dot = (x x + y y) + z z, normalize = divide by
sqrtf, cross) with explicit np.float32 values so that nothing widens to float64 — tests/test_atmosphere_ground_cpu.py pins that
algebra against the oracle's compiled `primary_ray` hook.  The sky itself is the oracle's own get_incident_light
(`atmosphere.get_incident_light`, one call per sky point) and the epilogue the oracle's pow.
"""
import numpy as np

from tests import model_common as C
from tests.model_common import F, ZERO, _f, dot, get_primary_ray, oracle, same_bits

EARTH_RADIUS = F(6360e3)                            # src/app_atmosphere.h:37
EYE = (F(0), EARTH_RADIUS + F(1.0), F(0))           # :172
LOOK_AT = (F(0), EARTH_RADIUS + F(1.5), F(-1))      # :173
FOV = F(1.0)                                        # :230
MAX_DIST = F(1e8)                                   # src/def.h:77
NO_HIT_T = MAX_DIST + F(1e1)                        # src/def.h:78-83
GROUND = F(.33)                                     # :223


def point_cam(width, height, fx, fy, fov=FOV):      # main.h:44-46 with this header's FOV
    return C.point_cam(width, height, fx, fy, fov)


def intersect_plane_t(rd, origin=EYE, direction=(ZERO, F(-1), ZERO), distance=EARTH_RADIUS):
    """hit.t after intersect_plane(ray, plane, no_hit) (oracle/ref_lib.h:245-255, intersect.h:61-77): NO_HIT_T where it returns
    early, t where the hit is recorded — a NaN t included."""
    with np.errstate(all="ignore"):
        denom = dot(direction, rd)
        p0o = (distance - origin[0], distance - origin[1], distance - origin[2])
        t = dot(p0o, direction) / denom
        early = (denom < F(1e-6)) | (t < ZERO) | (t > NO_HIT_T)
        return np.where(early, NO_HIT_T, t).astype(F)


def sun_dir(u_time):                                # the oracle's setup_scene (:177-181)
    return oracle().kat("atmosphere.sun_dir", [1, 1, 0, 0, u_time], 3)


def linear_to_srgb(c):                              # oracle/ref_lib.h:91-94
    c = _f(c)
    return oracle().math("pow", c.ravel(), F(1) / F(2.2)).reshape(c.shape)


def main_image(width, height, u_time, fx, fy):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel())
    rd = get_primary_ray(pcx, pcy, EYE, LOOK_AT)
    sky = intersect_plane_t(rd) > MAX_DIST          # :220
    col = np.full((fx.size, 3), GROUND, dtype=F)    # :223
    o = oracle()
    for i in np.flatnonzero(sky):                   # :221
        col[i] = o.kat("atmosphere.get_incident_light",
                       [width, height, 0, 0, u_time, EYE[0], EYE[1], EYE[2], rd[0][i], rd[1][i], rd[2][i]], 3)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = linear_to_srgb(col)
    return out.reshape(shape + (4,))


def frame(width, height, u_time, rows=None):
    """float32 [rows, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre)"""
    ys = np.arange(height) if rows is None else np.asarray(list(rows))
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (ys.astype(F) + F(.5))[:, None]
    return main_image(width, height, u_time, fx, fy)


def horizon_row(width, height):
    """the first row (from the bottom) whose pixel centres are sky; the camera has no roll, so a row is one or the other"""
    pcx, pcy = point_cam(width, height, np.full(height, F(.5)), np.arange(height, dtype=F) + F(.5))
    sky = intersect_plane_t(get_primary_ray(pcx, pcy, EYE, LOOK_AT)) > MAX_DIST
    return int(np.argmax(sky)) if sky.any() else height
