"""The binary32 toolkit the numpy models of tests/*_model.py share: the oracle's vector algebra (oracle/ovec.h), its min / max and
GLSL's mod, the camera of main.h and util.h, and the bit comparison every test of a model or a kernel rests on
(tests/test_model_common.py).  Every value is an explicit np.float32 so that nothing widens to float64; a model imports what it
uses from here and states only its own scene."""
import numpy as np

F = np.float32
ZERO, ONE, TWO = F(0), F(1), F(2)
RADIANS = F(0.017453292519943295)                   # oracle/sbx_math_ref.h m_radians

_ORACLE = None


def oracle():
    """the CPU oracle, built on first use"""
    global _ORACLE
    if _ORACLE is None:
        from oracle.oracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


def same_bits(a, b):
    """per-element bit equality with NaN == NaN (any NaN)"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _f(x):
    return np.asarray(x, dtype=F)


def _const(v, like):
    return np.full(like.shape, v, dtype=F)


def dot(a, b):                                      # oracle/ovec.h:67
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalize(v):                                   # oracle/ovec.h:69-70
    n = np.sqrt(dot(v, v))
    return (v[0] / n, v[1] / n, v[2] / n)


def cross(a, b):                                    # oracle/ovec.h:71-73
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def fmax(a, b):                                     # m_max: (a < b) ? b : a
    return np.where(a < b, b, a)


def fmin(a, b):                                     # m_min: (b < a) ? b : a
    return np.where(b < a, b, a)


def mod(x, y):                                      # GLSL mod: x - y * floor(x / y)
    return x - y * np.floor(x / y)


def op_add2(a, b):                                  # sdf.h:5-11: d1.x < d2.x ? d1 : d2
    k = a[0] < b[0]
    return np.where(k, a[0], b[0]), np.where(k, a[1], b[1])


def _sincos(deg):
    """(sin, cos) of an angle in degrees: the oracle's binary32 sin and cos of deg * m_radians"""
    a = _f(F(deg) * RADIANS).reshape(1)
    o = oracle()
    return o.math("sin", a)[0], o.math("cos", a)[0]


def point_cam(width, height, fx, fy, fov):          # oracle/ref_apps.h:31,35-36 (main.h:33,40,44-46); point_cam.z = -1
    """fov: the FOV that the app's header defines for main.h, binary32; no default, each model states its own"""
    fx, fy = _f(fx), _f(fy)
    w, h = F(width), F(height)
    with np.errstate(all="ignore"):
        aspect = w / h
        return ((TWO * (fx / w) - ONE) * aspect) * fov, ((TWO * (fy / h) - ONE) * ONE) * fov


def get_primary_ray(pcx, pcy, eye, look_at):        # oracle/ref_lib.h:56-65 (util.h:5-20); the point's z is not read
    eye, look_at = tuple(map(F, eye)), tuple(map(F, look_at))
    pcx, pcy = _f(pcx), _f(pcy)
    with np.errstate(all="ignore"):
        fwd = normalize((look_at[0] - eye[0], look_at[1] - eye[1], look_at[2] - eye[2]))
        up = (ZERO, ONE, ZERO)
        right = cross(up, fwd)
        up = cross(fwd, right)
        v = tuple((fwd[k] + up[k] * pcy) + right[k] * pcx for k in range(3))
        return normalize(v)
