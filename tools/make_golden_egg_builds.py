#!/usr/bin/env python3
"""Generate tests/golden/egg_builds/egg_{straight,oval}.npz: frames and points of src/app_egg.h rendered by the reference header
ITSELF with one of the two switches of its sdf() the other way (SBX_APP_EGG_STRAIGHT, SBX_APP_EGG_OVAL).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes two edited copies of the generated app_egg.h next to it —
    app_egg_straight.h   the `#define BEZIER` line at :37 removed (the four sd_cylinder legs of :86-109)
    app_egg_oval.h       the `#if 1` at :46 turned to `#if 0` (the one scaled sphere of :53-66)
each edit asserted to change exactly one line, at that line number — and builds them with the oracle's own pattern rule, the header
and the defines given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_egg_straight.so REF_HDR=app_egg_straight.h "REF_DEFS=-DAPP_EGG '-DSBX_REF_RESET=depth = -max_dist'"
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are recorded results, the
fixtures that pin tests/egg_builds_model.py, per build:
    t0.0037, t0.02, t0.2   96x54 frames (sbxr_render_rows) with their `uniforms` (u_res, u_mouse, u_time per frame)
    points, points_uniforms, points_out, points_shipped
                           4096 fragCoords at u_res 1920x1080 and u_time 0.02, drawn with a fixed seed from the screen rectangle of
                           the figure and its shadow (RECT below), what the edited header's sbxr_main_image answers there and, beside
                           it, what the SHIPPED header's answers.  The scene is flat-shaded, so a whole frame is a weak pin of a thin
                           member: most of its pixels are ground and sky in every build.  The points carry most of the evidence.
They live in a directory of their own because tests/golden/*.npz is the set of oracle-rendered app fixtures (tests/test_golden.py).

Conditions, asserted here and again by tests/test_egg_builds_cpu.py; the counts of the committed fixtures:
    pixels of a 96x54 frame that differ from the shipped build's      straight >= 90: 128, 135, 100    oval >= 15: 20, 21, 20
    points that differ from the shipped build's answers (>= 200)       straight: 985                    oval: 297
The rectangles were chosen from the reference alone, from the pixels in which the edited header's 1920x1080 frame at u_time 0.02
differs from the shipped header's (--find-rects prints their bounding box; 50649 pixels for straight, 7322 for oval):
    straight   the box between the 5th and the 95th percentile of those pixels' x and of their y: legs, knees and their shadow
    oval       the differences are a ring a pixel or two wide around the egg's outline, which reaches the top of the frame, and the
               shadow of its taller top (rows 237-363, 4123 of the pixels).  The ring's bounding box gives 114 of 4096, so the
               rectangle is the shadow's difference and the lower left of the outline above it, up to row 700

    python tools/make_golden_egg_builds.py [--find-rects]
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle, REF_DIR, reference_root  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "egg_builds")
W, H = 96, 54
TIMES = (0.0037, 0.02, 0.2)                     # the turntable (100 degrees per unit, :40) carries the figure out of view for |t| > 0.5
PW, PH, P_TIME, NPOINTS, SEED = 1920, 1080, 0.02, 4096, 20
REF_DEFS = "REF_DEFS=-DAPP_EGG '-DSBX_REF_RESET=depth = -max_dist'"
# build -> (line number, the line as it is, the line as it becomes; None: removed)
EDITS = {"straight": (37, "#define BEZIER", None), "oval": (46, "#if 1", "#if 0")}
MIN_PIXELS = {"straight": 90, "oval": 15}
MIN_POINTS = 200
# x0, y0, x1, y1 in fragCoord units of the 1920x1080 frame (see the header comment; --find-rects prints them)
RECT = {"straight": (794, 94, 1209, 533), "oval": (880, 236, 1000, 700)}


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_egg.h")
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = EDITS[build]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + ([] if new is None else [lines[at - 1].replace(old, new, 1)]) + lines[at:]
    # exactly one line changed, at that number
    if new is None:
        assert len(out) == len(lines) - 1 and out[:at - 1] == lines[:at - 1] and out[at - 1:] == lines[at:]
        assert not any(l.startswith("#define BEZIER") for l in out)
    else:
        assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "app_egg_%s.h" % build
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
    target = "_ref/libsbx_ref_egg_%s.so" % build
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, REF_DEFS], check=True)
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


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    shipped = load("_ref/libsbx_ref_egg.so")
    libs = {build: build_library(build) for build in ("straight", "oval")}
    if "--find-rects" in sys.argv:
        base = render(shipped, PW, PH, P_TIME)
        for build, lib in libs.items():
            ys, xs = np.nonzero(differ(render(lib, PW, PH, P_TIME), base))
            print(build, "differs in", len(xs), "pixels; RECT", (int(xs.min()) - 8, int(ys.min()) - 8, int(xs.max()) + 9, int(ys.max()) + 9))
        sys.exit(0)
    os.makedirs(OUT_DIR, exist_ok=True)
    for build, lib in libs.items():
        frames = {"t%g" % t: render(lib, W, H, t) for t in TIMES}
        counts = [int(differ(frames["t%g" % t], render(shipped, W, H, t)).sum()) for t in TIMES]
        assert min(counts) >= MIN_PIXELS[build], (build, counts)
        assert all(not np.isnan(f).any() for f in frames.values())
        uniforms = np.array([[W, H, 0.0, 0.0, t] for t in TIMES], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        x0, y0, x1, y1 = RECT[build]
        rng = np.random.default_rng(SEED)
        pts = (rng.uniform(0, 1, size=(NPOINTS, 2)) * [x1 - x0, y1 - y0] + [x0, y0]).astype(np.float32)
        got, base = points_of(lib, pts, P_TIME), points_of(shipped, pts, P_TIME)
        n = int(differ(got, base).sum())
        assert n >= MIN_POINTS, (build, n, "choose another rectangle")
        path = os.path.join(OUT_DIR, "egg_%s.npz" % build)
        np.savez_compressed(path, uniforms=uniforms, points=pts, points_uniforms=np.array([PW, PH, 0.0, 0.0, P_TIME], dtype=np.float32),
                            points_out=got, points_shipped=base, **frames)
        print(build, os.path.getsize(path), "bytes; frames differ from the shipped build's in", counts, "pixels, the points in", n)
