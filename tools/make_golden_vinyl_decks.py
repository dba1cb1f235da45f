#!/usr/bin/env python3
"""Generate tests/golden/vinyl_decks/<name>_64x36.npz: the frame and 64 seeded off-centre points of every deck of
tests/vinyl_deck_model.py's DECKS, rendered by the reference's own src/app_vinyl.h with the deck written into it.  That pins the model —
the definition of SBX_APP_VINYL_DECK and sbx_vinyl_eval (include/sbx.h) — against the reference's code: its sdf.h
primitives, its shadow march, its anisotropic groove shading and its renderer as they stand, over other values than the ones u_time
and the literals give.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per deck this tool writes one edited copy next to them, app_vinyl_<name>.h:
    :45, :47, :49, :51, :53   the base colours of setup_scene: the vec3 of each line, floats as hex literals
    :61, :62                  the eye and look_at of setup_camera
    :142                      the angle handed to the tonearm's rotate_around_x: arm_tilt_deg
    :285                      sun_dir: the deck's vector as given, no normalize
    :327, :328, :329          ro_spec, a_x, a_y
    :375                      the exponent of the Phong branch
    :419, :428                `rot` and the angle of the platter's rotate_around_x: platter_deg, platter_tilt_deg
    :460                      FOV
Every edit is asserted to start from exactly the line expected there (a preprocessor line by its text, a statement by a digest, so
that none of the reference's program text stands in this file) and to change nothing else.  The copy is built with the oracle's own
pattern rule through make variables (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_vinyl_deck_<name>.so REF_HDR=app_vinyl_<name>.h REF_DEFS="-DAPP_VINYL -DSBX_ENV_REFLECT"
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed; the .npz files hold recorded results only.

Asserted before anything is written: the model equals the reference in every bit, frames and points; the conditions under which the
fixtures say something (vinyl_deck_model.check_conditions); the single-field property (a block that changes one field alone changes
at least one pixel and none whose material does not read the field, model against model); the size cap.

    python tools/make_golden_vinyl_decks.py [--out-dir DIR]
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
from tests import vinyl_deck_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402


def hexf(x):
    """a binary32 value as a C literal of type float"""
    return lit(float(np.float32(x)).hex())


def vec3(v):
    return "vec3(%s, %s, %s)" % tuple(hexf(c) for c in v)


def first_vec3(new):
    """the one vec3(...) of literals on a line replaced"""
    def edit(line):
        out, n = re.subn(r"vec3\([^()]*\)", lambda m: new, line)
        assert n == 1, line
        return out
    return edit


def number(new):
    """the one `= <decimal literal>;` of a line replaced"""
    def edit(line):
        out, n = re.subn(r"= [\d.]+;", lambda m: "= %s;" % new, line)
        assert n == 1, line
        return out
    return edit


def last_argument(new):
    """the one `, <decimal literal>)` that ends a line replaced"""
    def edit(line):
        out, n = re.subn(r", [\d.]+\)$", lambda m: ", %s)" % new, line)
        assert n == 1, line
        return out
    return edit


def header_copy(name, D):
    src = os.path.join(REF_DIR, "src", "app_vinyl.h")
    lines = open(src).read().splitlines(keepends=True)
    edits = {45: ("e134c513bbb7da79", first_vec3(vec3(D["groove_color"]))),
             47: ("1cf8db41aa452774", first_vec3(vec3(D["dead_wax_color"]))),
             49: ("d44bd0a48240243c", first_vec3(vec3(D["label_color"]))),
             51: ("d7d0854119f18e63", first_vec3(vec3(D["logo_color"]))),
             53: ("662ce247be85cab5", first_vec3(vec3(D["shiny_color"]))),
             61: ("c3bf934fb374c180", "\teye = %s;" % vec3(D["eye"])),
             62: ("b3f30f6a153f94e9", "\tlook_at = %s;" % vec3(D["look_at"])),
             142: ("976bd35935a993a6", "\t\t%s));" % hexf(D["arm_tilt_deg"])),
             285: ("0a7e8a3fa20bc913", "\t%s;" % vec3(D["sun_dir"])),
             327: ("399b3c8849502d00", number(hexf(D["ro_spec"]))),
             328: ("e73acf8435b80856", number(hexf(D["a_x"]))),
             329: ("52c18dc84f42b010", number(hexf(D["a_y"]))),
             375: ("90f01782fe847ff7", last_argument(hexf(D["shininess"]))),
             419: ("04de8f49660c338b", "\tfloat rot = %s;" % hexf(D["platter_deg"])),
             428: ("5385ae2863f29014", "\t\trotate_around_x(%s));" % hexf(D["platter_tilt_deg"])),
             460: ("#define FOV 1. // 45 degrees", "#define FOV %s" % hexf(D["fov"]))}
    out = replace_lines(lines, edits, src)
    path = "app_vinyl_%s.h" % name
    with open(os.path.join(REF_DIR, "src", path), "w") as f:
        f.writelines(out)
    return path


def build_library(name, D):
    hdr = header_copy(name, D)
    target = "_ref/libsbx_ref_vinyl_deck_%s.so" % name
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated header: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=-DAPP_VINYL -DSBX_ENV_REFLECT"], check=True)
    return load(target)


def check_single_fields(w, h):
    """model against model: each field alone changes a pixel, and none whose material does not read it"""
    base_s, base = M.shares(M.scene_of(M.default_deck(0.)), w, h)
    for field, D in M.single_field_decks().items():
        changed = M.differing(M.frame(M.scene_of(D), w, h), base)
        readers = M.READERS[field]
        stray = 0 if readers is None else int((changed & ~np.isin(base_s["mat"], readers)).sum())
        print("field %-17s changes %4d pixels, %d of them of a material that does not read it" % (field, int(changed.sum()), stray))
        assert changed.any() and stray == 0, field


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "vinyl_decks"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    (w, h), n = M.SIZE, M.POINTS
    frames, all_shares, arrays = {}, {}, {}
    for name, D in M.DECKS.items():
        S = M.scene_of(D)
        lib = build_library(name, D)
        frame = render(lib, w, h)
        assert (frame[..., 3] == 1).all() and same_bits(frame, render(lib, w, h)).all(), (name, "a second render differs")
        pts = M.fixture_points(M.POINT_SEEDS[name], w, h, n)
        assert not (pts - np.floor(pts) == .5).all(axis=1).any()
        pts_out = points_of(lib, w, h, pts)
        sh, model = M.shares(S, w, h)
        bad = int((~same_bits(model, frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(S, w, h, pts), pts_out)).any(axis=-1).sum())
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              " ".join("%s %.2f %%" % (k, 100 * sh[k]) for k in ("groove", "dead_wax", "label", "shiny")), "logo %d pixels" % sh["logo_pixels"],
              "; NaN %d" % int(np.isnan(frame).any(axis=-1).sum()))
        assert bad == 0 and bad_pts == 0, (name, "tests/vinyl_deck_model.py is not what the reference's headers compute")
        frames[name], all_shares[name] = frame, sh
        arrays[name] = dict(deck=M.block(D), frame=frame, points=pts, points_out=pts_out)
    default_shares, default_frame = M.shares(M.scene_of(M.default_deck(0.)), w, h)
    M.check_conditions(all_shares, frames, default_shares, default_frame)
    check_single_fields(w, h)
    os.makedirs(args.out_dir, exist_ok=True)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name, a in arrays.items():
        path = os.path.join(args.out_dir, "%s_%dx%d.npz" % (name, w, h))
        np.savez_compressed(path, **a)
        assert os.path.getsize(path) <= bound, (name, os.path.getsize(path), bound)
        print(path, os.path.getsize(path), "bytes (bound %d)" % bound)
