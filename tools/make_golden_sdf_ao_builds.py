#!/usr/bin/env python3
"""Generate tests/golden/sdf_ao_builds/sdf_ao_{shadow,normals}_64x36.npz: frames of src/app_sdf_ao.h rendered by the reference
header ITSELF with one of its two `#if 0` blocks turned on (SBX_APP_SDF_AO_SHADOW, SBX_APP_SDF_AO_NORMALS).

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes two edited copies of the generated app_sdf_ao.h next to it —
    app_sdf_ao_shadow.h    the `#if 0` at :269 (the sdf_shadow call of render_impl) turned to `#if 1`
    app_sdf_ao_normals.h   the `#if 0 // debug...` at :217 (illuminate returns hit.normal) turned to `#if 1`
each edit asserted to replace exactly one line — and builds them with the oracle's own pattern rule, the header and the defines
given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_sdf_ao_shadow.so REF_HDR=app_sdf_ao_shadow.h REF_DEFS=-DAPP_SDF_AO
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are the frames they
render (sbxr_render_rows), 64x36 at three u_time values, with their uniforms — recorded results, the fixtures that pin
tests/sdf_ao_builds_model.py.  They live in a directory of their own because tests/golden/*.npz is the set of oracle-rendered
app fixtures (tests/test_golden.py), which these are not.

    python tools/make_golden_sdf_ao_builds.py
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
OUT_DIR = os.path.join(ROOT, "tests", "golden", "sdf_ao_builds")
W, H = 64, 36
# u_time turns the camera by 50 degrees per unit (app_sdf_ao.h:47) around a scene whose sun stands still at normalize(1, 2, 1):
# 18.5, 125 and 230 degrees.  The shadow falls across the ramps and the ground in all three: it changes 68 of 1654 hit pixels at
# 0.37, 310 of 1653 at 2.5 and 146 of 1653 at 4.6 (62 / 361 / 111 of them in full umbra; tests/test_sdf_ao_builds_cpu.py)
TIMES = (0.37, 2.5, 4.6)
# (build, the line to edit, its replacement)
EDITS = {"shadow": ("#if 0\n", "#if 1\n"),
         "normals": ("#if 0 // debug: output the raymarching steps\n", "#if 1 // debug: output the raymarching steps\n")}


def edited_header(build):
    src = os.path.join(REF_DIR, "src", "app_sdf_ao.h")
    lines = open(src).read().splitlines(keepends=True)
    old, new = EDITS[build]
    at = [i for i, l in enumerate(lines) if l.rstrip() == old.rstrip()]
    assert len(at) == 1, "%s: %d lines read %r, expected exactly one" % (src, len(at), old)
    assert at[0] + 1 == {"shadow": 269, "normals": 217}[build], "the block has moved: line %d" % (at[0] + 1)
    lines[at[0]] = lines[at[0]].replace("#if 0", "#if 1", 1)
    assert lines[at[0]].rstrip() == new.rstrip()
    name = "app_sdf_ao_%s.h" % build
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(lines)
    return name


def build_library(build):
    name = edited_header(build)
    target = "_ref/libsbx_ref_sdf_ao_%s.so" % build
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, "REF_DEFS=-DAPP_SDF_AO"], check=True)
    lib = ctypes.CDLL(os.path.join(ORACLE_DIR, target))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.sbxr_render_rows.argtypes = [fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, fp, ctypes.c_int]
    return lib


def render(lib, w, h, t):
    u = Oracle._uni(w, h, t, (0.0, 0.0))
    rows = np.arange(h, dtype=np.int32)
    out = np.zeros((h, w, 4), dtype=np.float32)
    lib.sbxr_render_rows(Oracle._fp(u), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), h, Oracle._fp(out), 4)
    return out


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    os.makedirs(OUT_DIR, exist_ok=True)
    for build in ("shadow", "normals"):
        lib = build_library(build)
        frames = {"t%g" % t: render(lib, W, H, t) for t in TIMES}
        uniforms = np.array([[W, H, 0.0, 0.0, t] for t in TIMES], dtype=np.float32)   # u_res, u_mouse, u_time per frame
        path = os.path.join(OUT_DIR, "sdf_ao_%s_%dx%d.npz" % (build, W, H))
        np.savez_compressed(path, uniforms=uniforms, **frames)
        print(build, os.path.getsize(path), "bytes", {k: float(np.nanmean(v[..., :3])) for k, v in frames.items()})
