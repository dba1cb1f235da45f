#!/usr/bin/env python3
"""Generate tests/golden/planet_worlds/<name>_64x36.npz: the frame and 64 seeded off-centre points of every world of
tests/planet_world_model.py's WORLDS, rendered by the reference's own src/app_planet.h with the world written into it.  That pins the
model — the definition of SBX_APP_PLANET_WORLD (include/sbx.h) — against the reference's code over other numbers than
its literals, another camera, other angles and another sun.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per world this tool writes one edited copy next to them, app_planet_world_<name>.h:
    :20                 max_height
    :55, :56            eye, look_at
    :68                 vol_coeff_absorb
    :76                 the divisor of illuminate_volume
    :107                the vec3 of the cloud noise's offset
    :110, :111          cld_coverage, cld_fuzzy
    :114                band()'s three edges
    :127, :148          the two `steps`
    :165                TERR_STEPS
    :180, :193          the vec3 of the second terrain fBm's offset (one field, both lines)
    :224                c_L
    :258-262, :265-268  the five colours, the four limits
    :288                the sun: the normalize(vec3(...)) replaced by the block's vec3, as given
    :307, :308, :309    the three angles (the products of u_time replaced by the block's values)
    :369                FOV
Every edit is asserted to start from exactly the line expected there (a preprocessor line by its text, a statement by a digest, so
that none of the reference's program text stands in this file) and to change nothing else; floats are written as hex literals.  The
copy is built with the oracle's own pattern rule (oracle/Makefile is not edited).  oracle/_ref is git-ignored: neither the copies nor
the libraries are ever committed; the .npz files hold recorded results only.

Asserted before anything is written: the model equals the reference in every bit, frames and points; the default world's frame is the
reference's build of the unedited header; the conditions under which the fixtures say something (planet_world_model.check_conditions,
of the REFERENCE's frames); the single-field property (model against model); the size cap.

    python tools/make_golden_planet_worlds.py [--out-dir DIR]
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
from make_golden_atmosphere_airs import first_vec3, hexf, render_at, vec3  # noqa: E402
from make_golden_raytracer_scenes import ORACLE_DIR, load, points_of, render, replace_lines  # noqa: E402
from oracle.oracle import REF_DIR, reference_root  # noqa: E402
from tests import planet_world_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402


def sub_once(pattern, new):
    """the one match of `pattern` on a line replaced"""
    def edit(line):
        out, n = re.subn(pattern, lambda m: new, line)
        assert n == 1, line
        return out
    return edit


def define(name, value, spaces=" ", tail=""):
    """a `#define name literal` line inside a function (one tab) -> (its text, its replacement)"""
    return lambda old: ("\t#define %s%s%s%s" % (name, spaces, old, tail), "\t#define %s%s(%s)" % (name, spaces, value))


def header_copy(name, W):
    src = os.path.join(REF_DIR, "src", "app_planet.h")
    lines = open(src).read().splitlines(keepends=True)
    b = W["band"]
    edits = {20: ("#define max_height .4", "#define max_height (%s)" % hexf(W["max_height"])),
             55: ("20244596d5f18eee", "\teye = %s;" % vec3(W["eye"])),
             56: ("300aecef6cbbf4d9", "\tlook_at = %s;" % vec3(W["look_at"])),
             68: ("#define vol_coeff_absorb 30.034", "#define vol_coeff_absorb (%s)" % hexf(W["absorb"])),
             76: ("43ca76d092cbd2a6", sub_once(r"/ [\d.]+;", "/ (%s);" % hexf(W["cloud_light"]))),
             107: ("57fad428e466670a", first_vec3(vec3(W["cloud_offset"]))),
             110: define("cld_coverage", hexf(W["cld_coverage"]), tail=" // higher=less clouds")(".29475675"),
             111: define("cld_fuzzy", hexf(W["cld_fuzzy"]), tail=" // higher=fuzzy, lower=blockier")(".0335"),
             114: ("2973e1549029f1a9", sub_once(r"\(\S+, \S+, \S+, ", "(%s, %s, %s, " % tuple(hexf(c) for c in b))),
             127: ("8dab1e19cdf07044", sub_once(r"= \d+;", "= %d;" % W["cloud_steps"])),
             148: ("44429af782698ff3", sub_once(r"= \d+;", "= %d;" % W["shadow_steps"])),
             165: ("#define TERR_STEPS 120", "#define TERR_STEPS %d" % W["terr_steps"]),
             180: ("4c6b7114e845e8f2", first_vec3(vec3(W["terrain_offset"]))),
             193: ("0872603e0110ca57", first_vec3(vec3(W["terrain_offset"]))),
             224: ("e69689c15c935336", first_vec3(vec3(W["key_color"]))),
             258: define("c_water", vec3(W["c_water"]))("vec3(.015, .110, .455)"),
             259: define("c_grass", vec3(W["c_grass"]))("vec3(.086, .132, .018)"),
             260: define("c_beach", vec3(W["c_beach"]))("vec3(.153, .172, .121)"),
             261: define("c_rock", vec3(W["c_rock"]), spaces="  ")("vec3(.080, .050, .030)"),
             262: define("c_snow", vec3(W["c_snow"]), spaces="  ")("vec3(.600, .600, .600)"),
             265: define("l_water", hexf(W["l_water"]))(".05"),
             266: define("l_shore", hexf(W["l_shore"]))(".17"),
             267: define("l_grass", hexf(W["l_grass"]))(".211"),
             268: define("l_rock", hexf(W["l_rock"]))(".351"),
             288: ("09802867906468ed", sub_once(r"normalize\(vec3\([^()]*\)\)", vec3(W["sun_dir"]))),
             307: ("0d5cd0ceb73f93c2", sub_once(r"\([\d.]+\);", "(%s);" % hexf(W["tilt_deg"]))),
             308: ("1e706d5f1e81f71e", sub_once(r"u_time \* [-\d.]+", hexf(W["spin_deg"]))),
             309: ("af217dd1ace0855a", sub_once(r"u_time \* [-\d.]+", hexf(W["cloud_spin_deg"]))),
             369: ("#define FOV tan(radians(30.))", "#define FOV (%s)" % hexf(W["fov"]))}
    out = replace_lines(lines, edits, src)
    path = "app_planet_world_%s.h" % name
    with open(os.path.join(REF_DIR, "src", path), "w") as f:
        f.writelines(out)
    return path


def build_library(name, W):
    hdr = header_copy(name, W)
    target = "_ref/libsbx_ref_planet_world_%s.so" % name
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated header: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=-DAPP_PLANET"], check=True)
    return load(target)


def check_single_fields(w, h):
    """model against model: each field alone changes a pixel"""
    base = M.frame(M.default_world(M.T0), w, h)
    for field, W in M.single_field_worlds().items():
        changed = M.differing(M.frame(W, w, h), base)
        print("field %-16s changes %4d pixels" % (field, int(changed.sum())))
        assert changed.any(), field


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "planet_worlds"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    (w, h), n = M.SIZE, M.POINTS
    # first of all: the default world written into the header is the shipped frame, and so is the model over it
    default_frame = render_at(load("_ref/libsbx_ref_planet.so"), w, h, M.T0)
    assert same_bits(default_frame, render(build_library("default", M.default_world(M.T0)), w, h)).all(), "the default world's copy is not the shipped header"
    assert same_bits(default_frame, M.frame(M.default_world(M.T0), w, h)).all(), "the model over the default world is the reference's frame"
    frames, parts_of, arrays = {}, {}, {}
    for name, W in M.WORLDS.items():
        assert M.refused(W) is None, name
        lib = build_library(name, W)
        frame = render(lib, w, h)
        assert (frame[..., 3] == 1).all() and same_bits(frame, render(lib, w, h)).all(), (name, "a second render differs")
        pts = M.fixture_points(M.POINT_SEEDS[name], w, h, n)
        assert not (pts - np.floor(pts) == .5).all(axis=1).any()
        pts_out = points_of(lib, w, h, pts)
        parts = {}
        bad = int((~same_bits(M.frame(W, w, h, parts), frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(W, w, h, pts), pts_out)).any(axis=-1).sum())
        c = M.classes(parts, (h, w))
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              ", ".join("%s %d" % (k, int(v.sum())) for k, v in c.items()),
              "NaN %d, differs from default in %d shell pixels, tier %s" % (int(np.isnan(frame).any(axis=-1).sum()),
                                                                             int((M.differing(frame, default_frame) & c["shell"]).sum()), M.tier_of(W)))
        assert bad == 0 and bad_pts == 0, (name, "tests/planet_world_model.py is not what the reference's header computes")
        frames[name], parts_of[name] = frame, parts
        arrays[name] = dict(block=M.block(W), frame=frame, points=pts, points_out=pts_out)
    M.check_conditions(frames, parts_of, default_frame)
    check_single_fields(w, h)
    os.makedirs(args.out_dir, exist_ok=True)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name, a in arrays.items():
        path = os.path.join(args.out_dir, "%s_%dx%d.npz" % (name, w, h))
        np.savez_compressed(path, **a)
        assert os.path.getsize(path) <= bound, (name, os.path.getsize(path), bound)
        print(path, os.path.getsize(path), "bytes (bound %d)" % bound)
