#!/usr/bin/env python3
"""Generate tests/golden/clouds_builds/clouds_{height,luminance}.npz: frames and points of src/app_clouds.h rendered by the reference
header ITSELF with one of the two `#if 0` switches of its illuminate_volume on (SBX_APP_CLOUDS_HEIGHT, SBX_APP_CLOUDS_LUMINANCE;
DESIGN.md §5.13).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes two edited copies of the generated app_clouds.h next to it —
    app_clouds_height.h      the `#if 0` at :97 turned to `#if 1` (`float luminance = exp(height) / 2.;`, no light march)
    app_clouds_luminance.h   the `#if 0` at :118 turned to `#if 1` (`return luminance;`)
each edit asserted to change exactly that line — and builds them with the oracle's own pattern rule, the header and the defines given
as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_clouds_height.so REF_HDR=app_clouds_height.h REF_DEFS=-DAPP_CLOUDS
An aux set of tests/golden/reference_aux_sets.json is one more build, with the -D'SBX_REF_AUX_<name>(d)=...' defines that
oracle/aux_sets.py generates for it behind -DAPP_CLOUDS (`_ref/libsbx_ref_clouds_height@steer.so`).  oracle/_ref is git-ignored:
neither the copies nor the libraries are ever committed.  What is committed are recorded results, per build:
    t0, t1.5, t37.25        96x54 frames at the default aux block, with their `uniforms` (u_res, u_mouse, u_time per frame)
    aux_<set>               96x54 frames at u_time 1.5 under the aux sets AUX_SETS; aux_counts = pixels that differ from the
                            shipped build's frame under the same set
    points, points_uniforms, points_xor, points_shipped
                            2048 fragCoords at u_res 1920x1080 and u_time 1.5, drawn with a fixed seed from the rows above the
                            horizon cut (:212), off-centre; the edited header's sbxr_main_image answers and the shipped header's
ENCODING.  Seven float frames and the points do not fit the size that a fixture under tests/golden/ may have, so every frame and
points_out are recorded as the XOR of their rgb bit patterns with the SHIPPED build's (`x_<frame>`, `points_xor`, uint32: zero where
the builds agree — below the horizon, in clear sky — which deflates to nothing); alpha is 1 in every pixel, asserted here.  The
shipped build's frames are not stored: they are the CPU oracle's SBX_APP_CLOUDS frames, which this tool asserts equal to the
reference's shipped build bit for bit before it encodes against them.  tests/clouds_builds_model.py fixture() decodes.

Conditions, asserted here and again by tests/test_clouds_builds_cpu.py: every default-aux frame differs from the shipped build's in
>= 1500 of its 5184 pixels, no NaN anywhere, >= 500 of the points differ, the aux-set frames differ (> 0 pixels) for steer, yz and
degenerate, and `zero` (no march step runs) equals the shipped build bit for bit.

    python tools/make_golden_clouds_builds.py
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import aux_sets  # noqa: E402
from oracle.oracle import Oracle, REF_DIR, reference_root  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "clouds_builds")
W, H = 96, 54
TIMES = (0.0, 1.5, 37.25)
AUX_TIME = 1.5
AUX_SETS = ("steer", "yz", "degenerate", "zero")
PW, PH, P_TIME, NPOINTS, SEED = 1920, 1080, 1.5, 2048, 21
P_ROW0 = 648                                    # point_cam.y >= .2 there: dir.y >= .2 / sqrt(1 + (16/9)^2 + 1) = .088 > .05 (:212)
# build -> (line number, the line as it is, the line as it becomes)
EDITS = {"height": (97, "#if 0", "#if 1"), "luminance": (118, "#if 0", "#if 1")}
MIN_PIXELS, MIN_POINTS = 1500, 500


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_clouds.h")
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = EDITS[build]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + [lines[at - 1].replace(old, new, 1)] + lines[at:]
    assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "app_clouds_%s.h" % build
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(out)
    return name


def load(target):
    lib = ctypes.CDLL(os.path.join(ORACLE_DIR, target))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.sbxr_render_rows.argtypes = [fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, fp, ctypes.c_int]
    lib.sbxr_main_image.argtypes = [fp, ctypes.c_float, ctypes.c_float, fp]
    return lib


def build_library(build, aux_set=None):
    name = edited_header(build)
    defs = "-DAPP_CLOUDS"
    target = "_ref/libsbx_ref_clouds_%s.so" % build
    if aux_set is not None:
        defs += " " + aux_sets.defines("clouds", aux_sets.load()["clouds"][aux_set])
        target = "_ref/libsbx_ref_clouds_%s@%s.so" % (build, aux_set)
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, "REF_DEFS=%s" % defs], check=True)
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


def rgb_bits(a):
    assert (a[..., 3] == 1).all()
    return np.ascontiguousarray(a[..., :3]).view(np.uint32)


def shipped_frame(oracle, t, aux_set=None):
    """the shipped build's frame from the reference library, asserted equal to the oracle's (what fixture() decodes against)"""
    ref = render(load("_ref/libsbx_ref_clouds%s.so" % ("" if aux_set is None else "@" + aux_set)), W, H, t)
    aux = None if aux_set is None else aux_sets.block("clouds", aux_sets.load()["clouds"][aux_set])
    assert not differ(ref, oracle.render(1, W, H, t, aux=aux)).any(), ("the oracle's APP_CLOUDS is not the reference's", t, aux_set)
    return ref


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    shipped = load("_ref/libsbx_ref_clouds.so")
    oracle = Oracle()
    os.makedirs(OUT_DIR, exist_ok=True)
    for build in ("height", "luminance"):
        lib = build_library(build)
        frames = {"t%g" % t: render(lib, W, H, t) for t in TIMES}
        base = {"t%g" % t: shipped_frame(oracle, t) for t in TIMES}
        counts = [int(differ(frames[k], base[k]).sum()) for k in base]
        assert min(counts) >= MIN_PIXELS, (build, counts)
        aux_counts = []
        for s in AUX_SETS:
            frames["aux_" + s] = render(build_library(build, s), W, H, AUX_TIME)
            base["aux_" + s] = shipped_frame(oracle, AUX_TIME, s)
            aux_counts.append(int(differ(frames["aux_" + s], base["aux_" + s]).sum()))
        for s, c in zip(AUX_SETS, aux_counts):
            assert (c == 0) if s == "zero" else (c > 0), (build, s, c)
        assert all(not np.isnan(f).any() for f in frames.values())
        uniforms = np.array([[W, H, 0.0, 0.0, t] for t in TIMES], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        rng = np.random.default_rng(SEED)
        pts = (rng.uniform(0, 1, size=(NPOINTS, 2)) * [PW, PH - P_ROW0] + [0, P_ROW0]).astype(np.float32)
        got, pbase = points_of(lib, pts, P_TIME), points_of(shipped, pts, P_TIME)
        assert not np.isnan(got).any()
        n = int(differ(got, pbase).sum())
        assert n >= MIN_POINTS, (build, n)
        path = os.path.join(OUT_DIR, "clouds_%s.npz" % build)
        np.savez_compressed(path, uniforms=uniforms, aux_sets=np.array(AUX_SETS), aux_uniforms=np.array([W, H, 0.0, 0.0, AUX_TIME], dtype=np.float32),
                            aux_counts=np.array(aux_counts, dtype=np.int64), points=pts,
                            points_uniforms=np.array([PW, PH, 0.0, 0.0, P_TIME], dtype=np.float32), points_xor=rgb_bits(got) ^ rgb_bits(pbase),
                            points_shipped=np.ascontiguousarray(pbase[:, :3]), **{"x_" + k: rgb_bits(f) ^ rgb_bits(base[k]) for k, f in frames.items()})
        print(build, os.path.getsize(path), "bytes; default-aux frames differ from the shipped build's in", counts, "pixels, the aux-set frames",
              dict(zip(AUX_SETS, aux_counts)), ", the points in", n)
