#!/usr/bin/env python3
"""Generate tests/golden/vinyl_builds/vinyl_{closeup,ridges,noshadow}.npz: frames and points of src/app_vinyl.h rendered by the
reference header ITSELF with one of three compile-time switches the other way (SBX_APP_VINYL_CLOSEUP, SBX_APP_VINYL_RIDGES,
SBX_APP_VINYL_NOSHADOW).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes three edited copies of the generated app_vinyl.h next to it —
    app_vinyl_closeup.h    the `#if 1` of setup_camera at :60 turned to `#if 0` (eye and look_at of :64-65)
    app_vinyl_ridges.h     the `#if 0` of illuminate at :357 turned to `#if 1` (the ridge of :358-363 on label and logo hits)
    app_vinyl_noshadow.h   the `#if 1` of render at :445 turned to `#if 0` (:446-449 gone, sh stays 1.)
each edit asserted to change exactly that line, from exactly the text expected there — and builds them with the oracle's own pattern
rule, the header and the defines given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_vinyl_ridges.so REF_HDR=app_vinyl_ridges.h "REF_DEFS=-DAPP_VINYL -DSBX_ENV_REFLECT"
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are recorded results, per build:
    uniforms, x_frame0 .. x_frame3
                            64x36 frames at u_time 0.37, 2.5, -3.7 and 7.25 (u_mouse is not read); `uniforms` holds u_res, u_mouse,
                            u_time per frame
    big_uniforms, x_big0, x_big1
                            ridges and noshadow only: 128x72 frames at u_time -3.7 and 7.25 (closeup differs from the shipped build
                            almost everywhere, so its XOR does not compress: it gets none)
    points, points_uniforms, points_xor, points_shipped
                            2048 fragCoords at u_res 1920x1080 and u_time 2.5, drawn with a fixed seed from the whole frame,
                            off-centre; the edited header's sbxr_main_image answers and the shipped header's
ENCODING.  Every frame and points_out are recorded as the XOR of their rgb bit patterns with the SHIPPED build's under the same
uniforms (`x_frame<i>`, `x_big<i>`, `points_xor`, uint32: zero where the builds agree); alpha is 1 in every pixel, asserted here.
The shipped build's frames are not stored: they are the CPU oracle's SBX_APP_VINYL frames, which this tool asserts equal to the
reference's shipped build bit for bit before it encodes against them.  tests/vinyl_builds_model.py fixture() decodes.  Each file
stays within the size of the largest .npz directly under tests/golden/.

NaN pixels are data here: sqrt of a negative dotLN * dot(V, N) in the groove shading (:339) gives 1-2 per shipped 64x36 frame and
some tens from the close-up camera; `differ` counts NaN == NaN as equal, like every comparison of this project.

Conditions, asserted here and again by tests/test_vinyl_builds_cpu.py (caps that keep a fixture from saying nothing; the reference
alone meets them): alpha 1; pixels that differ from the shipped build's — closeup >= 1400 of a 64x36 frame and >= 1200 of the
points; noshadow >= 50 per 64x36 frame, >= 200 per 128x72 frame, >= 50 points; ridges >= 60 per 64x36 frame at u_time 2.5, -3.7 and
7.25 and >= 10 at 0.37, >= 300 per 128x72 frame, >= 60 points (the ridge's share depends strongly on the platter angle: at u_time
1.0, 1.5 and 4.0 it is 3-6 pixels, which is why these times are recorded); NaN pixels per frame <= 100 of 2304 (closeup), <= 4 of 2304
and <= 20 of 9216 (ridges, noshadow).

    python tools/make_golden_vinyl_builds.py
"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import APP_VINYL, Oracle, REF_DIR, reference_root  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "vinyl_builds")
BUILDS = ("closeup", "ridges", "noshadow")
W, H = 64, 36
TIMES = (0.37, 2.5, -3.7, 7.25)                     # u_time per 64x36 frame
BW, BH = 128, 72
BIG_TIMES = (-3.7, 7.25)                            # u_time per 128x72 frame (ridges, noshadow)
PW, PH, P_TIME, NPOINTS, SEED = 1920, 1080, 2.5, 2048, 23
REF_DEFS = "-DAPP_VINYL -DSBX_ENV_REFLECT"          # oracle/Makefile's own for app_vinyl.h
# build -> (line number, the line as it is, the line as it becomes)
EDITS = {"closeup": (60, "#if 1", "#if 0"), "ridges": (357, "#if 0", "#if 1"), "noshadow": (445, "#if 1", "#if 0")}
MIN_PIXELS = {"closeup": (1400, 1400, 1400, 1400), "ridges": (10, 60, 60, 60), "noshadow": (50, 50, 50, 50)}   # per frame of TIMES
MIN_BIG = {"ridges": 300, "noshadow": 200}
MIN_POINTS = {"closeup": 1200, "ridges": 60, "noshadow": 50}
MAX_NAN = {"closeup": 100, "ridges": 4, "noshadow": 4}
MAX_NAN_BIG = 20


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_vinyl.h")
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = EDITS[build]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + [lines[at - 1].replace(old, new, 1)] + lines[at:]
    assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "app_vinyl_%s.h" % build
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
    target = "_ref/libsbx_ref_vinyl_%s.so" % build
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
    shipped = load("_ref/libsbx_ref_vinyl.so")
    oracle = Oracle()
    os.makedirs(OUT_DIR, exist_ok=True)
    base, big_base = [], []
    for (w, h, times, into) in ((W, H, TIMES, base), (BW, BH, BIG_TIMES, big_base)):
        for t in times:                             # the shipped frames: the oracle's, asserted to be the reference's
            into.append(render(shipped, w, h, t))
            assert not differ(into[-1], oracle.render(APP_VINYL, w, h, t)).any(), ("the oracle's APP_VINYL is not the reference's", w, h, t)
    rng = np.random.default_rng(SEED)
    pts = (rng.uniform(0, 1, size=(NPOINTS, 2)) * [PW, PH]).astype(np.float32)
    pbase = points_of(shipped, pts, P_TIME)
    for build in BUILDS:
        lib = build_library(build)
        frames = [render(lib, W, H, t) for t in TIMES]
        assert all((f[..., 3] == 1).all() for f in frames)
        nans = [nan_pixels(f) for f in frames]
        assert max(nans) <= MAX_NAN[build], (build, nans)
        counts = [int(differ(f, b).sum()) for f, b in zip(frames, base)]
        assert all(c >= m for c, m in zip(counts, MIN_PIXELS[build])), (build, counts)
        extra, big_counts, big_nans = {}, [], []
        if build in MIN_BIG:
            bigs = [render(lib, BW, BH, t) for t in BIG_TIMES]
            assert all((f[..., 3] == 1).all() for f in bigs)
            big_nans = [nan_pixels(f) for f in bigs]
            assert max(big_nans) <= MAX_NAN_BIG, (build, big_nans)
            big_counts = [int(differ(f, b).sum()) for f, b in zip(bigs, big_base)]
            assert min(big_counts) >= MIN_BIG[build], (build, big_counts)
            extra["big_uniforms"] = np.array([[BW, BH, 0.0, 0.0, t] for t in BIG_TIMES], dtype=np.float32)
            extra.update({"x_big%d" % i: rgb_bits(f) ^ rgb_bits(b) for i, (f, b) in enumerate(zip(bigs, big_base))})
        got = points_of(lib, pts, P_TIME)
        assert (got[:, 3] == 1).all()
        n = int(differ(got, pbase).sum())
        assert n >= MIN_POINTS[build], (build, n, "choose another seed")
        uniforms = np.array([[W, H, 0.0, 0.0, t] for t in TIMES], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        path = os.path.join(OUT_DIR, "vinyl_%s.npz" % build)
        np.savez_compressed(path, uniforms=uniforms, points=pts, points_uniforms=np.array([PW, PH, 0.0, 0.0, P_TIME], dtype=np.float32),
                            points_xor=rgb_bits(got) ^ rgb_bits(pbase), points_shipped=np.ascontiguousarray(pbase[:, :3]),
                            **{"x_frame%d" % i: rgb_bits(f) ^ rgb_bits(b) for i, (f, b) in enumerate(zip(frames, base))}, **extra)
        assert os.path.getsize(path) <= size_bound(), (build, os.path.getsize(path), size_bound())
        print(build, os.path.getsize(path), "bytes (bound %d); 64x36 frames differ from the shipped build's in" % size_bound(), counts,
              "pixels (NaN pixels", nans, "), 128x72 frames in", big_counts, "(NaN", big_nans, "), the points in", n)
