#!/usr/bin/env python3
"""Generate tests/golden/planet_builds/planet_{closeup,cloudless,unlit}.npz: frames and points of src/app_planet.h rendered by the
reference header ITSELF with one of three compile-time switches the other way (SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS,
SBX_APP_PLANET_UNLIT).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes three edited copies of the generated app_planet.h next to it —
    app_planet_closeup.h     the `#if 0` of setup_camera at :51 turned to `#if 1` (eye and look_at of :52-53)
    app_planet_cloudless.h   the `#define CLOUDS` at :63 turned into a comment (:344-347 and :355-361 gone: no cloud march, no
                             cloud shadow march; `cloud` is never written and stays the zeros of the static object)
    app_planet_unlit.h       the `#define LIGHT` at :249 turned into a comment (N = w_normal.y, ocean = water, no setup_lights)
each edit asserted to change exactly that line, from exactly the text expected there — and builds them with the oracle's own pattern
rule, the header and the defines given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_planet_unlit.so REF_HDR=app_planet_unlit.h REF_DEFS=-DAPP_PLANET
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are recorded results, per build:
    uniforms, x_frame0 .. x_frame3
                            64x36 frames at u_time 0.37, 2.5, -3.7 and 7.25 (u_mouse is not read); `uniforms` holds u_res, u_mouse,
                            u_time per frame
    big_uniforms, x_big0, x_big1
                            cloudless and unlit only: 128x72 frames at u_time -3.7 and 7.25 (closeup differs from the shipped build
                            in every pixel, so its XOR does not compress: it gets none)
    points, points_uniforms, points_xor, points_shipped
                            2048 fragCoords at u_res 1920x1080 and u_time 2.5, drawn with a fixed seed from the whole frame,
                            off-centre; the edited header's sbxr_main_image answers and the shipped header's
ENCODING.  Every frame and points_out are recorded as the XOR of their rgb bit patterns with the SHIPPED build's under the same
uniforms (`x_frame<i>`, `x_big<i>`, `points_xor`, uint32: zero where the builds agree); alpha is 1 in every pixel, asserted here.
The shipped build's frames are not stored: they are the CPU oracle's SBX_APP_PLANET frames, which this tool asserts equal to the
reference's shipped build bit for bit before it encodes against them.  tests/planet_builds_model.py fixture() decodes.  Each file
stays within the size of the largest .npz directly under tests/golden/.

NaN pixels are data here: smoothstep(1 - .3 s, 1 - .2 s, N) with s = 0 is 0/0 where N == 1 (:270-273), and a zero normal of the
central differences normalises to NaN (:206); `differ` counts NaN == NaN as equal, like every comparison of this project.  The unlit
build takes N = w_normal.y, which is 1 for no hit point of a recorded frame: it has no NaN pixel.

Conditions, asserted here and again by tests/test_planet_builds_cpu.py (caps that keep a fixture from saying nothing; the reference
alone meets them): alpha 1; pixels that differ from the shipped build's — closeup >= 2250 of a 64x36 frame, cloudless >= 750 and
>= 3000 of a 128x72 frame, unlit >= 580 and >= 2300; NaN pixels per frame — closeup <= 150, cloudless <= 100 of 2304 and <= 300 of
9216, unlit exactly 0.  The points that differ from the shipped build's are printed; the test asks for 80 % of what was printed:
    closeup 2047, cloudless 796, unlit 659
(and, as printed with them: 64x36 frames differ in 2304 each (closeup), 873 / 842 / 885 / 865 (cloudless), 672 / 684 / 649 / 665
(unlit); 128x72 frames in 3468 / 3451 and 2583 / 2662; NaN pixels 9 / 32 / 88 / 12 (closeup), 25 / 21 / 50 / 20 and 212 / 75
(cloudless), none (unlit))

    python tools/make_golden_planet_builds.py
"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import APP_PLANET, Oracle, REF_DIR, reference_root  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "planet_builds")
BUILDS = ("closeup", "cloudless", "unlit")
W, H = 64, 36
TIMES = (0.37, 2.5, -3.7, 7.25)                     # u_time per 64x36 frame
BW, BH = 128, 72
BIG_TIMES = (-3.7, 7.25)                            # u_time per 128x72 frame (cloudless, unlit)
PW, PH, P_TIME, NPOINTS, SEED = 1920, 1080, 2.5, 2048, 23
REF_DEFS = "-DAPP_PLANET"                           # oracle/Makefile's own for app_planet.h
# build -> (line number, the line as it is, the line as it becomes)
EDITS = {"closeup": (51, "#if 0", "#if 1"), "cloudless": (63, "#define CLOUDS", "//#define CLOUDS"),
         "unlit": (249, "#define LIGHT", "//#define LIGHT")}
MIN_PIXELS = {"closeup": 2250, "cloudless": 750, "unlit": 580}     # per 64x36 frame
MIN_BIG = {"cloudless": 3000, "unlit": 2300}                       # per 128x72 frame
MAX_NAN = {"closeup": 150, "cloudless": 100, "unlit": 0}
MAX_NAN_BIG = {"cloudless": 300, "unlit": 0}


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_planet.h")
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = EDITS[build]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + [lines[at - 1].replace(old, new, 1)] + lines[at:]
    assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "app_planet_%s.h" % build
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
    target = "_ref/libsbx_ref_planet_%s.so" % build
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, "REF_DEFS=%s" % REF_DEFS], check=True)
    return load(target)


def render(lib, w, h, t):
    u = Oracle._uni(w, h, t, (0.0, 0.0))
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


def nan_pixels(a):
    return int(np.isnan(a).any(axis=-1).sum())


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
    shipped = load("_ref/libsbx_ref_planet.so")
    oracle = Oracle()
    os.makedirs(OUT_DIR, exist_ok=True)
    base, big_base = [], []
    for (w, h, times, into) in ((W, H, TIMES, base), (BW, BH, BIG_TIMES, big_base)):
        for t in times:                             # the shipped frames: the oracle's, asserted to be the reference's
            into.append(render(shipped, w, h, t))
            assert not differ(into[-1], oracle.render(APP_PLANET, w, h, t)).any(), ("the oracle's APP_PLANET is not the reference's", w, h, t)
    rng = np.random.default_rng(SEED)
    pts = (rng.uniform(0, 1, size=(NPOINTS, 2)) * [PW, PH]).astype(np.float32)
    pbase = points_of(shipped, pts, P_TIME)
    for build in BUILDS:
        lib = build_library(build)
        frames = [render(lib, W, H, t) for t in TIMES]
        assert all((f[..., 3] == 1).all() for f in frames)
        assert all(not differ(f, render(lib, W, H, t)).any() for f, t in zip(frames, TIMES)), (build, "a second render differs")
        nans = [nan_pixels(f) for f in frames]
        assert max(nans) <= MAX_NAN[build], (build, nans)
        counts = [int(differ(f, b).sum()) for f, b in zip(frames, base)]
        assert min(counts) >= MIN_PIXELS[build], (build, counts)
        extra, big_counts, big_nans = {}, [], []
        if build in MIN_BIG:
            bigs = [render(lib, BW, BH, t) for t in BIG_TIMES]
            assert all((f[..., 3] == 1).all() for f in bigs)
            big_nans = [nan_pixels(f) for f in bigs]
            assert max(big_nans) <= MAX_NAN_BIG[build], (build, big_nans)
            big_counts = [int(differ(f, b).sum()) for f, b in zip(bigs, big_base)]
            assert min(big_counts) >= MIN_BIG[build], (build, big_counts)
            extra["big_uniforms"] = np.array([[BW, BH, 0.0, 0.0, t] for t in BIG_TIMES], dtype=np.float32)
            extra.update({"x_big%d" % i: rgb_bits(f) ^ rgb_bits(b) for i, (f, b) in enumerate(zip(bigs, big_base))})
        got = points_of(lib, pts, P_TIME)
        assert (got[:, 3] == 1).all()
        n = int(differ(got, pbase).sum())
        uniforms = np.array([[W, H, 0.0, 0.0, t] for t in TIMES], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        path = os.path.join(OUT_DIR, "planet_%s.npz" % build)
        np.savez_compressed(path, uniforms=uniforms, points=pts, points_uniforms=np.array([PW, PH, 0.0, 0.0, P_TIME], dtype=np.float32),
                            points_xor=rgb_bits(got) ^ rgb_bits(pbase), points_shipped=np.ascontiguousarray(pbase[:, :3]),
                            **{"x_frame%d" % i: rgb_bits(f) ^ rgb_bits(b) for i, (f, b) in enumerate(zip(frames, base))}, **extra)
        assert os.path.getsize(path) <= size_bound(), (build, os.path.getsize(path), size_bound())
        print(build, os.path.getsize(path), "bytes (bound %d); 64x36 frames differ from the shipped build's in" % size_bound(), counts,
              "pixels (NaN pixels", nans, "), 128x72 frames in", big_counts, "(NaN", big_nans, "), the points in", n)
