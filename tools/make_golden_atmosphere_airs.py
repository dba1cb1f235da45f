#!/usr/bin/env python3
"""Generate tests/golden/atmosphere_airs/<name>_64x36.npz: the frame and 64 seeded off-centre points of every block of
tests/atmosphere_air_model.py's AIRS, rendered by the reference's own src/app_atmosphere.h with the block written into it.  That pins
the model — the definition of SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval (include/sbx.h) — against the
reference's code over other numbers than its literals and another sun than u_time makes.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per block this tool writes one edited copy next to them, app_atmosphere_air_<name>.h:
    :12                       hg_g
    :29, :30                  betaR, betaM: the vec3 of each line, floats as hex literals
    :34, :35, :37, :38, :41   hR, hM, earth_radius, atmosphere_radius, sun_power
    :47, :48                  the two sample counts
    :162                      the FROM_SPACE define: removed for view 1
    :172, :173                eye and look_at (view 1)
    :179, :180                setup_scene's two statements: removed, the sun is the block's
    :205                      the dome's ray origin (view 0)
    :230                      FOV
Every edit is asserted to start from exactly the line expected there (a preprocessor line by its text, a statement by a digest, so
that none of the reference's program text stands in this file) and to change nothing else.  The sun reaches the copy as the
statement the oracle's driver runs before every pixel (SBX_REF_RESET, oracle/ref_driver.cpp), through the make variable REF_DEFS;
the copy is built with the oracle's own pattern rule (oracle/Makefile is not edited).  oracle/_ref is git-ignored: neither the copies
nor the libraries are ever committed; the .npz files hold recorded results only.

Asserted before anything is written: the model equals the reference in every bit, frames and points; the conditions under which the
fixtures say something (atmosphere_air_model.check_conditions, of the REFERENCE's frames); the single-field property (a block that
changes one field alone changes at least one pixel, model against model); the size cap.

    python tools/make_golden_atmosphere_airs.py [--out-dir DIR]
"""
import argparse
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_raytracer_scenes import ORACLE_DIR, lit, load, points_of, render, replace_lines  # noqa: E402
from oracle.oracle import REF_DIR, Oracle, reference_root  # noqa: E402
from tests import atmosphere_air_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402


def hexf(x):
    """a binary32 value as a C literal of type float"""
    return lit(float(np.float32(x)).hex())


def vec3(v):
    return "vec3(%s, %s, %s)" % tuple(hexf(c) for c in v)


def first_vec3(new):
    """the one vec3(...) of a line replaced"""
    def edit(line):
        out, n = re.subn(r"vec3\([^()]*\)", lambda m: new, line)
        assert n == 1, line
        return out
    return edit


def number(new):
    """the one `= <decimal literal>;` of a line replaced"""
    def edit(line):
        out, n = re.subn(r"= [\d.e]+;", lambda m: "= %s;" % new, line)
        assert n == 1, line
        return out
    return edit


def header_copy(name, A):
    src = os.path.join(REF_DIR, "src", "app_atmosphere.h")
    lines = open(src).read().splitlines(keepends=True)
    edits = {12: ("#define hg_g (.76)", "#define hg_g (%s)" % hexf(A["hg_g"])),
             29: ("8d75a857d1a5bfd9", first_vec3(vec3(A["betaR"]))),
             30: ("14e67306e543cc38", first_vec3(vec3(A["betaM"]))),
             34: ("79791a5cc796948c", number(hexf(A["hR"]))),
             35: ("4f0ed5f4713899c7", number(hexf(A["hM"]))),
             37: ("ec5731d77c201e17", number(hexf(A["earth_radius"]))),
             38: ("28942dfca8f429a8", number(hexf(A["atmosphere_radius"]))),
             41: ("953b324fba2c7654", number(hexf(A["sun_power"]))),
             47: ("6fc0ff5f0333a3db", number("%d" % A["num_samples"])),
             48: ("bc3b25f32751134b", number("%d" % A["num_samples_light"])),
             179: ("1d65f3fa08cae099", ""),
             180: ("5dca6522a7c664dc", ""),
             230: ("#define FOV 1. // 45 degrees", "#define FOV %s" % hexf(A["fov"]))}
    if A["view"] == 0:
        edits[205] = ("2d3f89c20031819f", first_vec3(vec3(A["eye"])))
    else:
        edits[162] = ("#define FROM_SPACE 1", "")
        edits[172] = ("5dfb47900d513311", "\teye = %s;" % vec3(A["eye"]))
        edits[173] = ("21143c6ce002eed5", "\tlook_at = %s;" % vec3(A["look_at"]))
    out = replace_lines(lines, edits, src)
    path = "app_atmosphere_air_%s.h" % name
    with open(os.path.join(REF_DIR, "src", path), "w") as f:
        f.writelines(out)
    return path


def build_library(name, A):
    hdr = header_copy(name, A)
    target = "_ref/libsbx_ref_atmosphere_air_%s.so" % name
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated header: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    defs = "-DAPP_ATMOSPHERE '-DSBX_REF_RESET=sun_dir = %s'" % vec3(A["sun_dir"])
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=%s" % defs], check=True)
    return load(target)


def render_at(lib, w, h, u_time):
    """a reference library's frame at a u_time (make_golden_raytracer_scenes.render is this at 0)"""
    u = Oracle._uni(w, h, u_time, (0.0, 0.0))
    rows = np.arange(h, dtype=np.int32)
    out = np.zeros((h, w, 4), dtype=np.float32)
    lib.sbxr_render_rows(Oracle._fp(u), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), h, Oracle._fp(out), 8)
    return out


def check_single_fields(w, h):
    """model against model: each field alone changes a pixel (look_at in view 1)"""
    base = {v: M.frame(M.default_air(.37, v), w, h) for v in (0, 1)}
    for field, (view, A) in M.single_field_airs().items():
        changed = M.differing(M.frame(A, w, h), base[view])
        print("field %-18s (view %d) changes %4d pixels" % (field, view, int(changed.sum())))
        assert changed.any(), field


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "atmosphere_airs"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    (w, h), n = M.SIZE, M.POINTS
    frames, grounds, arrays = {}, {}, {}
    for name, A in M.AIRS.items():
        assert M.refused(A) is None, name
        lib = build_library(name, A)
        frame = render(lib, w, h)
        assert (frame[..., 3] == 1).all() and same_bits(frame, render(lib, w, h)).all(), (name, "a second render differs")
        pts = M.fixture_points(M.POINT_SEEDS[name], w, h, n)
        assert not (pts - np.floor(pts) == .5).all(axis=1).any()
        pts_out = points_of(lib, w, h, pts)
        bad = int((~same_bits(M.frame(A, w, h), frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(A, w, h, pts), pts_out)).any(axis=-1).sum())
        g = M.ground_mask(A, w, h)
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              "lit sky %.2f, ground %.2f, NaN %d, tier %s" % (((frame[..., :3] != 0).any(axis=-1) & ~g).mean(), g.mean(),
                                                             int(np.isnan(frame).any(axis=-1).sum()), M.tier_of(A)))
        assert bad == 0 and bad_pts == 0, (name, "tests/atmosphere_air_model.py is not what the reference's header computes")
        frames[name], grounds[name] = frame, g
        arrays[name] = dict(block=M.block(A), frame=frame, points=pts, points_out=pts_out)
    default_frame = render_at(load("_ref/libsbx_ref_atmosphere.so"), w, h, .37)      # the reference's build of the unedited header
    assert same_bits(default_frame, M.frame(M.default_air(.37), w, h)).all(), "the model over the default block is the reference's frame"
    M.check_conditions(frames, grounds, default_frame)
    for name, f in frames.items():
        print(name, "differs from the default block's frame in %.2f of the pixels" % M.differing(f, default_frame).mean())
    check_single_fields(w, h)
    os.makedirs(args.out_dir, exist_ok=True)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name, a in arrays.items():
        path = os.path.join(args.out_dir, "%s_%dx%d.npz" % (name, w, h))
        np.savez_compressed(path, **a)
        assert os.path.getsize(path) <= bound, (name, os.path.getsize(path), bound)
        print(path, os.path.getsize(path), "bytes (bound %d)" % bound)
