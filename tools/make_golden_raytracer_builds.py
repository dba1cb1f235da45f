#!/usr/bin/env python3
"""Generate tests/golden/raytracer_builds/raytracer_{phong,noshadow,static}.npz: frames and points of src/app_raytracer.h rendered by
the reference header ITSELF with one of its three compile-time switches the other way (SBX_APP_RAYTRACER_PHONG,
SBX_APP_RAYTRACER_NOSHADOW, SBX_APP_RAYTRACER_STATIC).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes three edited copies of the generated app_raytracer.h next to it —
    app_raytracer_phong.h      the `#if 0` of illuminate at :61 turned to `#if 1` (illum_blinn_phong, light.h:44-62)
    app_raytracer_noshadow.h   the `#if 1 // shadow ray` of render at :107 turned to `#if 0` (:108-121 gone)
    app_raytracer_static.h     the `#if 1` of setup_scene at :29 turned to `#if 0` (the scene of cornell_box.h:71-85, no u_time)
each edit asserted to change exactly that line, from exactly the text expected there — and builds them with the oracle's own pattern
rule, the header and the defines given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_raytracer_phong.so REF_HDR=app_raytracer_phong.h REF_DEFS=-DAPP_RAYTRACER
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are recorded results, per build:
    uniforms, x_frame0 .. x_frame3
                            64x64 frames at u_time 0, 0.37 and 2.5 with u_mouse (0, 0) and one at u_time 1.5 with u_mouse (40, 20)
                            (the camera turned by 66 degrees); `uniforms` holds u_res, u_mouse, u_time per frame
    points, points_uniforms, points_xor, points_shipped
                            2048 fragCoords at u_res 1920x1080 and u_time 1.5, drawn with a fixed seed from the whole frame,
                            off-centre; the edited header's sbxr_main_image answers and the shipped header's
ENCODING.  Four float frames and the points do not fit the size that a fixture under tests/golden/ may have (the largest .npz
directly under it), so every frame and points_out are recorded as the XOR of their rgb bit patterns with the SHIPPED build's under the
same uniforms (`x_frame<i>`, `points_xor`, uint32: zero where the builds agree); alpha is 1 in every pixel, asserted here.  The shipped
build's frames are not stored: they are the CPU oracle's SBX_APP_RAYTRACER frames, which this tool asserts equal to the reference's
shipped build bit for bit before it encodes against them.  tests/raytracer_builds_model.py fixture() decodes.

Conditions, asserted here and again by tests/test_raytracer_builds_cpu.py (caps that keep a fixture from saying nothing; the
reference alone meets them): no NaN, alpha 1; pixels of a 4096-pixel frame that differ from the shipped build's: phong >= 1500,
noshadow >= 250, static >= 3500; the three u_mouse (0, 0) frames of static are bit-identical; points of the 2048 that differ from the
shipped build's: phong >= 500, noshadow >= 100, static >= 1500.

    python tools/make_golden_raytracer_builds.py
"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import APP_RAYTRACER, Oracle, REF_DIR, reference_root  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "raytracer_builds")
W, H = 64, 64
UNIFORMS = [(0.0, (0.0, 0.0)), (0.37, (0.0, 0.0)), (2.5, (0.0, 0.0)), (1.5, (40.0, 20.0))]      # (u_time, u_mouse) per frame
PW, PH, P_TIME, NPOINTS, SEED = 1920, 1080, 1.5, 2048, 23
# build -> (line number, the line as it is, the line as it becomes)
EDITS = {"phong": (61, "#if 0", "#if 1"), "noshadow": (107, "#if 1 // shadow ray", "#if 0 // shadow ray"), "static": (29, "#if 1", "#if 0")}
MIN_PIXELS = {"phong": 1500, "noshadow": 250, "static": 3500}
MIN_POINTS = {"phong": 500, "noshadow": 100, "static": 1500}


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_raytracer.h")
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = EDITS[build]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + [lines[at - 1].replace(old, new, 1)] + lines[at:]
    assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "app_raytracer_%s.h" % build
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(out)
    return name


def load(target):
    lib = ctypes.CDLL(os.path.join(ORACLE_DIR, target))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.sbxr_render_rows.argtypes = [fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, fp, ctypes.c_int]
    lib.sbxr_main_image.argtypes = [fp, ctypes.c_float, ctypes.c_float, fp]
    return lib


def build_library(build):
    name = edited_header(build)
    target = "_ref/libsbx_ref_raytracer_%s.so" % build
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, "REF_DEFS=-DAPP_RAYTRACER"], check=True)
    return load(target)


def render(lib, w, h, t, mouse):
    u = Oracle._uni(w, h, t, mouse)
    rows = np.arange(h, dtype=np.int32)
    out = np.zeros((h, w, 4), dtype=np.float32)
    lib.sbxr_render_rows(Oracle._fp(u), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), h, Oracle._fp(out), 8)
    return out


def points_of(lib, pts, t):
    u = Oracle._uni(PW, PH, t, (0.0, 0.0))
    out = np.zeros((len(pts), 4), dtype=np.float32)
    for i, (x, y) in enumerate(pts):
        lib.sbxr_main_image(Oracle._fp(u), float(x), float(y), Oracle._fp(out[i]))
    return out


def differ(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(axis=-1)


def rgb_bits(a):
    assert (a[..., 3] == 1).all()
    return np.ascontiguousarray(a[..., :3]).view(np.uint32)


def size_bound():
    """the largest .npz directly under tests/golden/"""
    return max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    shipped = load("_ref/libsbx_ref_raytracer.so")
    oracle = Oracle()
    os.makedirs(OUT_DIR, exist_ok=True)
    base = []
    for t, mouse in UNIFORMS:                       # the shipped frames: the oracle's, asserted to be the reference's
        base.append(render(shipped, W, H, t, mouse))
        assert not differ(base[-1], oracle.render(APP_RAYTRACER, W, H, t, mouse=mouse)).any(), ("the oracle's APP_RAYTRACER is not the reference's", t, mouse)
    rng = np.random.default_rng(SEED)
    pts = (rng.uniform(0, 1, size=(NPOINTS, 2)) * [PW, PH]).astype(np.float32)
    pbase = points_of(shipped, pts, P_TIME)
    for build in ("phong", "noshadow", "static"):
        lib = build_library(build)
        frames = [render(lib, W, H, t, mouse) for t, mouse in UNIFORMS]
        assert all(not np.isnan(f).any() and (f[..., 3] == 1).all() for f in frames)
        counts = [int(differ(f, b).sum()) for f, b in zip(frames, base)]
        assert min(counts) >= MIN_PIXELS[build], (build, counts)
        if build == "static":
            assert not differ(frames[0], frames[1]).any() and not differ(frames[0], frames[2]).any()
        got = points_of(lib, pts, P_TIME)
        assert not np.isnan(got).any() and (got[:, 3] == 1).all()
        n = int(differ(got, pbase).sum())
        assert n >= MIN_POINTS[build], (build, n, "choose another seed")
        uniforms = np.array([[W, H, m[0], m[1], t] for t, m in UNIFORMS], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        path = os.path.join(OUT_DIR, "raytracer_%s.npz" % build)
        np.savez_compressed(path, uniforms=uniforms, points=pts, points_uniforms=np.array([PW, PH, 0.0, 0.0, P_TIME], dtype=np.float32),
                            points_xor=rgb_bits(got) ^ rgb_bits(pbase), points_shipped=np.ascontiguousarray(pbase[:, :3]),
                            **{"x_frame%d" % i: rgb_bits(f) ^ rgb_bits(b) for i, (f, b) in enumerate(zip(frames, base))})
        assert os.path.getsize(path) <= size_bound(), (build, os.path.getsize(path), size_bound())
        print(build, os.path.getsize(path), "bytes (bound %d); frames differ from the shipped build's in" % size_bound(), counts,
              "pixels, the points in", n)
