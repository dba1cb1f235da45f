#!/usr/bin/env python3
"""Generate tests/golden/egg_poses/<name>_64x36.npz: the frame and 64 seeded off-centre points of every pose of
tests/egg_pose_model.py's POSES, rendered by the reference's own src/app_egg.h with the pose written into it.  That pins the model —
the definition of SBX_APP_EGG_POSE and sbx_egg_eval (include/sbx.h) — against the reference's code: its IK.h solver,
its sdf.h primitives and its renderer as they stand, over other values than the ones u_time gives.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per pose this tool writes one edited copy next to them, app_egg_<name>.h:
    :25, :26     the eye and look_at of setup_camera: the pose's, floats as hex literals
    :40          the angle handed to rotate_around_y: the pose's turn_deg
    :74, :77     left_foot_pos and right_foot_pos: declared with the pose's values
    :80, :81     femur and tibia
    :253         FOV
Every edit is asserted to start from exactly the line expected there (a preprocessor line by its text, a statement by a digest, so
that none of the reference's program text stands in this file) and to change nothing else.  The copy is built with the oracle's own
pattern rule through make variables (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_egg_pose_<name>.so REF_HDR=app_egg_<name>.h REF_DEFS="-DAPP_EGG '-DSBX_REF_RESET=depth = -max_dist'"
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed; the .npz files hold recorded results only.

Asserted before anything is written: the model equals the reference in every bit, frames and points; the conditions under which the
fixtures say something (egg_pose_model.check_conditions); the size cap.

    python tools/make_golden_egg_poses.py [--out-dir DIR]
"""
import argparse
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
from oracle.oracle import REF_DIR, reference_root  # noqa: E402
from tests import egg_pose_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402


def hexf(x):
    """a binary32 value as a C literal of type float"""
    return lit(float(np.float32(x)).hex())


def vec3(v):
    return "vec3(%s, %s, %s)" % tuple(hexf(c) for c in v)


def innermost(new):
    """the one parenthesised group of a line that holds no other replaced by (new)"""
    def edit(line):
        out, n = re.subn(r"\([^()]*\)", "(%s)" % new, line)
        assert n == 1, line
        return out
    return edit


def number(new):
    """the one `= <decimal literal>;` of a line replaced"""
    def edit(line):
        out, n = re.subn(r"= [\d.]+;", "= %s;" % new, line)
        assert n == 1, line
        return out
    return edit


def header_copy(name, P):
    src = os.path.join(REF_DIR, "src", "app_egg.h")
    lines = open(src).read().splitlines(keepends=True)
    edits = {25: ("b60e236c39298b13", "\teye = %s;" % vec3(P["eye"])),
             26: ("d5067e8aea0d48e3", "\tlook_at = %s;" % vec3(P["look_at"])),
             40: ("ca990f5bf3492481", innermost(hexf(P["turn_deg"]))),
             74: ("95ab5c95ef55eced", "\tvec3 left_foot_pos = %s;" % vec3(P["left_foot"])),
             77: ("e2610932d95aeb7c", "\tvec3 right_foot_pos = %s;" % vec3(P["right_foot"])),
             80: ("f9b333cd7226b417", number(hexf(P["femur"]))),
             81: ("0035dd925bfdac48", number(hexf(P["tibia"]))),
             253: ("#define FOV 1. // 45 degrees", "#define FOV %s" % hexf(P["fov"]))}
    out = replace_lines(lines, edits, src)
    path = "app_egg_%s.h" % name
    with open(os.path.join(REF_DIR, "src", path), "w") as f:
        f.writelines(out)
    return path


def build_library(name, P):
    hdr = header_copy(name, P)
    target = "_ref/libsbx_ref_egg_pose_%s.so" % name
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated header: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=-DAPP_EGG '-DSBX_REF_RESET=depth = -max_dist'"], check=True)
    return load(target)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "egg_poses"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    (w, h), n = M.SIZE, M.POINTS
    frames, all_shares, arrays = {}, {}, {}
    for name, P in M.POSES.items():
        S = M.scene_of(P)
        lib = build_library(name, P)
        frame = render(lib, w, h)
        assert (frame[..., 3] == 1).all() and same_bits(frame, render(lib, w, h)).all(), (name, "a second render differs")
        pts = M.fixture_points(M.POINT_SEEDS[name], w, h, n)
        assert not (pts - np.floor(pts) == .5).all(axis=1).any()
        pts_out = points_of(lib, w, h, pts)
        sh, model = M.shares(S, w, h)
        bad = int((~same_bits(model, frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(S, w, h, pts), pts_out)).any(axis=-1).sum())
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              " ".join("%s %.2f %%" % (k, 100 * v) for k, v in sh.items()), "; NaN %d" % int(np.isnan(frame).any(axis=-1).sum()))
        assert bad == 0 and bad_pts == 0, (name, "tests/egg_pose_model.py is not what the reference's headers compute")
        frames[name], all_shares[name] = frame, sh
        arrays[name] = dict(pose=M.block(P), frame=frame, points=pts, points_out=pts_out)
    M.check_conditions(all_shares, frames)
    os.makedirs(args.out_dir, exist_ok=True)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name, a in arrays.items():
        path = os.path.join(args.out_dir, "%s_%dx%d.npz" % (name, w, h))
        np.savez_compressed(path, **a)
        assert os.path.getsize(path) <= bound, (name, os.path.getsize(path), bound)
        print(path, os.path.getsize(path), "bytes (bound %d)" % bound)
