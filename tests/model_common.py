"""The binary32 toolkit the numpy models of tests/*_model.py share: the oracle's vector algebra (oracle/ovec.h), its min / max and
GLSL's mod, the camera of main.h and util.h, and the bit comparison every test of a model or a kernel rests on
(tests/test_model_common.py).  Every value is an explicit np.float32 so that nothing widens to float64; a model imports what it
uses from here and states only its own scene.  builds_fixture() is the one decoder of the build families' fixtures
(tests/build_families.py, tools/make_golden_builds.py)."""
import os

import numpy as np

from tests.build_families import FAMILIES, fixture_path, frame_keys

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


# ---- the fixtures of the build families ------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)[..., :3]).view(np.uint32)


def _rgba(bits):
    out = np.ones(bits.shape[:-1] + (4,), dtype=F)
    out[..., :3] = np.ascontiguousarray(bits).view(F)
    return out


_FIXTURES = {}


def builds_fixture(family, build):
    """tests/golden/<family>_builds/<file of the build> decoded, as tests/build_families.py describes it and tools/make_golden_builds.py
    wrote it: a dict with
        uniforms [n, 5] (u_res, u_mouse, u_time per frame) and frames, a list with one float32 [H, W, 4] per frame or, by the family's
        `frames_as`, one (w, h, u_time, u_mouse, frame) or one (name, u_time, aux set or None, frame), clouds' aux-set frames behind
        the others, with aux_counts {set: pixels that differ from the shipped build's};
        big_uniforms, big_frames: the larger set, empty for a build without one;
        points [n, 2], points_uniforms [5], points_out and points_shipped [n, 4], where the family records points.
    Where the file holds the XOR of every frame's rgb bits with the shipped build's frame, that frame is the oracle's under the same
    uniforms, and alpha is 1.  The file's keys and uniforms are asserted to be the table's."""
    if (family, build) in _FIXTURES:
        return _FIXTURES[(family, build)]
    fam = FAMILIES[family]
    z = np.load(fixture_path(os.path.dirname(os.path.abspath(__file__)), family, build))
    name, app = fam["shipped"]
    xor, keys = fam["storage"] == "xor", {"uniforms"}

    def decode(key, shipped):
        keys.add(key)
        if not xor:
            return z[key]
        shipped = shipped()
        assert (shipped[..., 3] == 1).all()
        return _rgba(z[key] ^ _bits(shipped))

    def frame_set(size, uniforms, pattern, name_of_uniforms):
        u = np.array([[size[0], size[1], m[0], m[1], t] for t, m in uniforms], dtype=F)
        assert np.array_equal(z[name_of_uniforms], u), (family, build, name_of_uniforms)
        return u, [decode(k, lambda: oracle().render(app, size[0], size[1], t, mouse=m)) for k, (t, m) in zip(frame_keys(pattern, uniforms), uniforms)]

    fx = {}
    fx["uniforms"], frames = frame_set(fam["size"], fam["uniforms"], fam["keys"], "uniforms")
    if fam["frames_as"] == "whtm":
        frames = [(int(u[0]), int(u[1]), float(u[4]), (float(u[2]), float(u[3])), f) for u, f in zip(fx["uniforms"], frames)]
    elif fam["frames_as"] == "named":
        frames = [(k[2:], float(u[4]), None, f) for k, u, f in zip(frame_keys(fam["keys"], fam["uniforms"]), fx["uniforms"], frames)]
    if "aux_sets" in fam:
        from oracle import aux_sets
        (w, h), t = fam["size"], fam["aux_time"]
        assert tuple(map(str, z["aux_sets"])) == fam["aux_sets"] and tuple(z["aux_uniforms"]) == (w, h, 0, 0, t)
        for s in fam["aux_sets"]:
            block = aux_sets.block(name, aux_sets.load()[name][s])
            frames.append(("aux_" + s, float(z["aux_uniforms"][4]), s, decode("x_aux_" + s, lambda: oracle().render(app, w, h, t, aux=block))))
        fx["aux_counts"] = dict(zip(fam["aux_sets"], map(int, z["aux_counts"])))
        keys.update(("aux_sets", "aux_uniforms", "aux_counts"))
    fx["frames"], fx["big_uniforms"], fx["big_frames"] = frames, np.zeros((0, 5), dtype=F), []
    if "min_big" in fam["builds"][build]:
        fx["big_uniforms"], fx["big_frames"] = frame_set(fam["big"]["size"], fam["big"]["uniforms"], fam["big_keys"], "big_uniforms")
        keys.add("big_uniforms")
    if fam["points"]:
        p = fam["points"]
        assert z["points"].shape == (p["count"], 2) and tuple(z["points_uniforms"]) == p["size"] + (0, 0, p["time"])
        shipped = np.ones((p["count"], 4), dtype=F)
        shipped[:, :z["points_shipped"].shape[1]] = z["points_shipped"]
        fx.update(points=z["points"], points_uniforms=z["points_uniforms"], points_shipped=shipped,
                  points_out=decode("points_xor" if xor else "points_out", lambda: shipped))
        keys.update(("points", "points_uniforms", "points_shipped"))
    assert set(z.files) == keys, (family, build, sorted(set(z.files) ^ keys))
    _FIXTURES[(family, build)] = fx
    return fx
