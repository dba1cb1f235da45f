#!/usr/bin/env python3
"""Generate tests/golden/raytracer_scenes/<name>_64x36.npz: the frame and 64 seeded off-centre points of every scene of
tests/golden/raytracer_scenes.json, rendered by the reference's own raytracer headers with the scene written into them.  That pins
tests/raytracer_scene_model.py — the definition of SBX_APP_RAYTRACER_SCENE (include/sbx.h) — against the
reference's code for scenes other than the Cornell box.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per scene this tool writes two edited copies next to them:
    cornell_box_<name>.h    the two count defines (:8, :11) carry the scene's counts, and the body of setup_cornell_box (:41-86, between
                            the braces of :40 and :87) is replaced by generated assignments of all 8 materials, the planes, the
                            spheres, lights[0] and ambient_light, every float a hex literal
    app_raytracer_<name>.h  :7 includes that copy; :29 is `#if 0` (no animation); :96 carries the bounce count; :61 and :107 are as the
                            scene says; :40-43 assign the scene's eye and look_at; :138 defines FOV as the scene's hex literal
Every edit is asserted to start from exactly the line expected there (a preprocessor switch by its text, a statement of the reference by a
digest of the line, so that none of its program text stands in this file) and to change nothing else.  The copy is built with the
oracle's own pattern rule, header and defines given as make variables on the command line (oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_raytracer_scene_<name>.so REF_HDR=app_raytracer_<name>.h REF_DEFS=-DAPP_RAYTRACER
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed; the .npz files hold recorded results only.

The conditions under which the fixtures say something (raytracer_scene_model.check_conditions) are asserted here before anything is
written, and again of the committed files by tests/test_raytracer_scene_cpu.py; so is the model's equality with what is recorded.

    python tools/make_golden_raytracer_scenes.py [--out-dir DIR]
"""
import argparse
import ctypes
import glob
import hashlib
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle, REF_DIR, reference_root  # noqa: E402
from tests import raytracer_scene_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
SETUP_HEAD = "8276d1f4196a2ee7"                       # digest() of cornell_box.h:39, the head of setup_cornell_box


def lit(s):
    """a hex-float string of the table as a C literal of type float"""
    float.fromhex(s)
    return s + "f"


def vec3(p):
    return "vec3(%s, %s, %s)" % tuple(lit(c) for c in p)


def digest(line):
    return hashlib.sha256(line.rstrip("\n").encode()).hexdigest()[:16]


def replace_lines(lines, edits, path):
    """edits: {line number: (what is expected there, new text)}; exactly those lines change.  What is expected is stated without
    quoting the reference's statements: a one-line preprocessor switch as its text, any other line as the first 16 hex digits of its
    SHA-256 (a line that has changed in the reference stops the tool either way).  new text: a string, or a function of the old line."""
    out = list(lines)
    for at, (old, new) in edits.items():
        have = lines[at - 1].rstrip("\n")
        assert have == old or digest(have) == old, "%s:%d reads %r, which is not the line this tool was written for" % (path, at, have)
        out[at - 1] = (new(have) if callable(new) else new) + "\n"
    assert len(out) == len(lines)
    assert set(i + 1 for i in range(len(lines)) if out[i] != lines[i]) <= set(edits), "only the stated lines change"
    return out


def set_count(count):
    """the one integer literal that follows `<` on a line (the bound of a counted loop) replaced by `count`"""
    def edit(line):
        new, n = re.subn(r"< \d+;", "< %d;" % count, line)
        assert n == 1, line
        return new
    return edit


def cornell_copy(e):
    src = os.path.join(REF_DIR, "src", "cornell_box.h")
    lines = open(src).read().splitlines(keepends=True)
    lines = replace_lines(lines, {8: ("#define num_cb_planes 6", "#define num_cb_planes %d" % len(e["planes"])),
                                  11: ("#define num_cb_spheres 3", "#define num_cb_spheres %d" % len(e["spheres"]))}, src)
    # the function whose body is replaced: its head at :39, its braces at :40 and :87 (the head as a digest, like any statement)
    assert [digest(lines[38]), lines[39].rstrip(), lines[86].rstrip()] == [SETUP_HEAD, "{", "}"], src
    body = []
    for i, m in enumerate(e["materials"]):
        body.append("\tmaterials[%d].base_color = %s;" % (i, vec3(m["base_color"])))
        for key in ("metallic", "roughness", "ior", "reflectivity", "translucency"):
            body.append("\tmaterials[%d].%s = %s;" % (i, key, lit(m[key])))
    for i, p in enumerate(e["planes"]):
        body += ["\tcb_planes[%d].direction = %s;" % (i, vec3(p["direction"])), "\tcb_planes[%d].distance = %s;" % (i, lit(p["distance"])),
                 "\tcb_planes[%d].material = %d;" % (i, p["material"])]
    for i, s in enumerate(e["spheres"]):
        body += ["\tcb_spheres[%d].origin = %s;" % (i, vec3(s["origin"])), "\tcb_spheres[%d].radius = %s;" % (i, lit(s["radius"])),
                 "\tcb_spheres[%d].material = %d;" % (i, s["material"])]
    body += ["\tlights[0].type = %d;" % e["light_type"], "\tlights[0].L = %s;" % vec3(e["light_L"]),
             "\tlights[0].color = %s;" % vec3(e["light_color"]), "\tambient_light = %s;" % vec3(e["ambient"])]
    assert len(e["planes"]) >= 1 and len(e["spheres"]) >= 1, "a C array needs an element: the fixture scenes have one of each at least"
    out = lines[:40] + [b + "\n" for b in body] + lines[86:]
    assert out[:40] == lines[:40] and out[-(len(lines) - 86):] == lines[86:]
    name = "cornell_box_%s.h" % e["name"]
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(out)
    return name


def raytracer_copy(e, box):
    src = os.path.join(REF_DIR, "src", "app_raytracer.h")
    lines = open(src).read().splitlines(keepends=True)
    edits = {7: ("b22b8c678e5aaa4c", '#include "%s"' % box),                   # the include of the scene's header
             29: ("#if 1", "#if 0"),                                          # setup_scene's animation: off
             40: ("b2ba062b1604ce74", ""), 41: ("235b7338d1464728", ""),      # setup_camera's two lines about the mouse: gone
             42: ("508a64808aa642a6", "\teye = %s;" % vec3(e["eye"])),        # its assignment of the eye
             43: ("03147f68f001868d", "\tlook_at = %s;" % vec3(e["look_at"])),   # and of look_at
             61: ("#if 0", "#if %d" % e["lighting"]),                         # illuminate's lighting model
             96: ("62cd74de9a0d3774", set_count(e["bounces"])),               # render's bounce loop: its count
             107: ("#if 1 // shadow ray", "#if %d // shadow ray" % e["shadow"]),
             138: ("425b1f72f448a1a1", "#define FOV %s" % lit(e["fov"]))}
    out = replace_lines(lines, edits, src)
    assert out[41].startswith("\teye = vec3(") and out[42].startswith("\tlook_at = vec3(") and out[39] == out[40] == "\n"
    name = "app_raytracer_%s.h" % e["name"]
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(out)
    return name


def load(target):
    lib = ctypes.CDLL(os.path.join(ORACLE_DIR, target))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.sbxr_render_rows.argtypes = [fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, fp, ctypes.c_int]
    lib.sbxr_main_image.argtypes = [fp, ctypes.c_float, ctypes.c_float, fp]
    return lib


def build_library(e):
    hdr = raytracer_copy(e, cornell_copy(e))
    target = "_ref/libsbx_ref_raytracer_scene_%s.so" % e["name"]
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated headers: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=-DAPP_RAYTRACER"], check=True)
    return load(target)


def render(lib, w, h):
    u = Oracle._uni(w, h, 0.0, (0.0, 0.0))          # u_time and u_mouse are not read by the edited headers
    rows = np.arange(h, dtype=np.int32)
    out = np.zeros((h, w, 4), dtype=np.float32)
    lib.sbxr_render_rows(Oracle._fp(u), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), h, Oracle._fp(out), 8)
    return out


def points_of(lib, w, h, pts):
    u = Oracle._uni(w, h, 0.0, (0.0, 0.0))
    out = np.zeros((len(pts), 4), dtype=np.float32)
    for i, (x, y) in enumerate(pts):
        lib.sbxr_main_image(Oracle._fp(u), float(x), float(y), Oracle._fp(out[i]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "raytracer_scenes"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    table = M.scene_table()
    (w, h), n = table["size"], table["points"]
    frames, masks, arrays = {}, {}, {}
    for e in table["scenes"]:
        name, S = e["name"], M.scene_of(e)
        lib = build_library(e)
        frame = render(lib, w, h)
        assert (frame[..., 3] == 1).all() and same_bits(frame, render(lib, w, h)).all(), (name, "a second render differs")
        pts = M.fixture_points(e["points_seed"], w, h, n)
        assert not (pts - np.floor(pts) == .5).all(axis=1).any()
        pts_out = points_of(lib, w, h, pts)
        m = {}
        model = M.frame(S, w, h, m)
        bad = int((~same_bits(model, frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(S, w, h, pts), pts_out)).any(axis=-1).sum())
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              "first hits: sphere %d plane %d background %d; shadowed %d; bounces >= 2: %d, >= 3: %d; lit %d; NaN %d"
              % (int((m["first_kind"] == 2).sum()), int((m["first_kind"] == 1).sum()), int((m["first_kind"] == 0).sum()), int(m["shadowed"].sum()),
                 int((m["depth"] >= 2).sum()), int((m["depth"] >= 3).sum()), int(m["lit"].sum()), M.nan_pixels(frame)))
        assert bad == 0 and bad_pts == 0, (name, "tests/raytracer_scene_model.py is not what the reference's headers compute")
        frames[name], masks[name] = frame, m
        arrays[name] = dict(frame=frame, points=pts, points_out=pts_out)
    M.check_conditions(table, frames, masks)
    os.makedirs(args.out_dir, exist_ok=True)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name, a in arrays.items():
        path = os.path.join(args.out_dir, "%s_%dx%d.npz" % (name, w, h))
        np.savez_compressed(path, **a)
        assert os.path.getsize(path) <= bound, (name, os.path.getsize(path), bound)
        print(path, os.path.getsize(path), "bytes (bound %d)" % bound)
