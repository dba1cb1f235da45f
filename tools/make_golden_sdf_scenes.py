#!/usr/bin/env python3
"""Generate tests/golden/sdf_scenes/<name>_64x36.npz: the frame and 64 seeded off-centre points of every scene of
tests/golden/sdf_scenes.json, rendered by the reference's own src/app_sdf_ao.h with the scene written into it.  That pins
tests/sdf_scene_model.py — the definition of SBX_APP_SDF_SCENE (include/sbx.h) — against the reference's code: its
sdf.h primitives and operators called by generated statements, its renderer as it stands.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; per scene this tool writes one edited copy next to them, app_sdf_ao_<name>.h:
    :11, :209, :249, :250, :313   the background, sun_dir, the march's step count and end, FOV: the scene's values, floats as hex literals
    :15, :20                      mat_ground is the scene's checker material, mat_count is 8
    :217, :269                    the two `#if 0` blocks as the scene's view and shadow say
    :37-42, :47-49, :115-149      the bodies of setup_scene, setup_camera and sdf() (between their braces) replaced by generated
                                  statements: the 8 materials; eye and look_at; one statement per instruction of the program — a
                                  primitive `float dN = sd_*(pos - offset [rotated by mul(., rotate_around_*(deg))], ...)`, an operator
                                  `float dN = op_*(dA, dB)`, an OBJECT `acc = op_add(acc, vec2(dN, float(material)))` (the first one
                                  declares acc) — and `return acc`
Every edit is asserted to start from exactly the text expected there (a preprocessor line by its text, a statement or a body by a
digest, so that none of the reference's program text stands in this file) and to change nothing else.  The copy is built with the
oracle's own pattern rule through make variables (oracle/Makefile is not edited), the fog through the pass-throughs of its
uniform_buffer.h:
    make -C oracle _ref/libsbx_ref_sdf_scene_<name>.so REF_HDR=app_sdf_ao_<name>.h
         REF_DEFS="-DAPP_SDF_AO '-DSBX_REF_AUX_fog_density(d)=<literal>' '-DSBX_REF_AUX_fog_falloff(d)=<literal>'"
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed; the .npz files hold recorded results only.

Asserted before anything is written: the model equals the reference in every bit, frames and points; the conditions under which the
fixtures say something (sdf_scene_model.check_conditions); the size cap.

    python tools/make_golden_sdf_scenes.py [--out-dir DIR]
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
from make_golden_raytracer_scenes import ORACLE_DIR, digest, lit, load, points_of, render, replace_lines, vec3  # noqa: E402
from oracle.oracle import REF_DIR, reference_root  # noqa: E402
from tests import sdf_scene_model as M  # noqa: E402
from tests.model_common import same_bits  # noqa: E402

# (first line, last line, digest of the lines joined by "\n", digest of the function's head two lines above the first)
BODIES = {"setup_scene": (37, 42, "c0b777cff81ceeb9", "f0573b913fb53ebc"), "setup_camera": (47, 49, "a0706761c0d14d1e", "035436f05a6c1f5f"),
          "sdf": (115, 149, "9ae11bff575bd6b5", "f4fa99f2f15efbe6")}
ROT = {1: "rotate_around_x", 2: "rotate_around_y", 3: "rotate_around_z"}


def number(pattern, new):
    """the one literal matching `pattern` on a line replaced by `new`"""
    def edit(line):
        out, n = re.subn(pattern, new, line)
        assert n == 1, line
        return out
    return edit


def sdf_body(program):
    """one statement per instruction; the stack is resolved here, so the statements name their operands"""
    out, stack, first = [], [], True
    for i, I in enumerate(program):
        op, a, b, c = M.OP_VALUES[I["op"]], I["a"], I["b"], I["c"]
        if op in M.PRIMITIVES:
            q = "pos - %s" % vec3(I["offset"])
            if I["rot_axis"]:
                q = "mul(%s, %s(%s))" % (q, ROT[I["rot_axis"]], lit(I["rot_deg"]))
            call = {M.PLANE: lambda: "sd_plane(%s, %s, %s)" % (q, vec3(a[:3]), lit(a[3])),
                    M.SPHERE: lambda: "sd_sphere(%s, %s)" % (q, lit(a[0])),
                    M.BOX: lambda: "sd_box(%s, %s)" % (q, vec3(a[:3])),
                    M.TORUS: lambda: "sd_torus(%s, %s, %s)" % (q, lit(a[0]), lit(a[1])),
                    M.Y_CYLINDER: lambda: "sd_y_cylinder(%s, %s, %s)" % (q, lit(a[0]), lit(a[1])),
                    M.CYLINDER: lambda: "sd_cylinder(%s, %s, %s, %s)" % (q, vec3(a[:3]), vec3(b[:3]), lit(a[3])),
                    M.CAPSULE: lambda: "sd_capsule(%s, %s, %s, %s)" % (q, vec3(a[:3]), vec3(b[:3]), lit(a[3])),
                    M.BEZIER: lambda: "sd_bezier(%s, %s, %s, %s, %s).x" % (vec3(a[:3]), vec3(b[:3]), vec3(c[:3]), q, lit(a[3]))}[op]()
            out.append("\tfloat d%d = %s;" % (i, call))
            stack.append("d%d" % i)
        elif op in M.OPERATORS:
            d2 = stack.pop()
            d1 = stack.pop()
            fn = {M.ADD: "op_add(%s, %s)", M.SUB: "op_sub(%s, %s)", M.INTERSECT: "op_intersect(%s, %s)"}.get(op)
            out.append("\tfloat d%d = %s;" % (i, fn % (d1, d2) if fn else "op_blend(%s, %s, %s)" % (d1, d2, lit(a[0]))))
            stack.append("d%d" % i)
        else:
            v = "vec2(%s, float(%d))" % (stack.pop(), I["material"])
            out.append("\tvec2 acc = %s;" % v if first else "\tacc = op_add(acc, %s);" % v)
            first = False
    assert not stack and not first
    return out + ["\treturn acc;"]


def header_copy(e):
    src = os.path.join(REF_DIR, "src", "app_sdf_ao.h")
    lines = open(src).read().splitlines(keepends=True)
    edits = {11: ("2bfd660e042fc94a", "\treturn %s;" % vec3(e["background"])),
             15: ("#define mat_ground\t1", "#define mat_ground\t%d" % e["checker_material"]),
             20: ("#define mat_count\t6", "#define mat_count\t8"),
             209: ("220fdd163b25ff15", "_constant(vec3) sun_dir = %s;" % vec3(e["sun_dir"])),
             217: ("#if 0 // debug: output the raymarching steps", "#if %d // debug: output the raymarching steps" % e["view"]),
             249: ("3dc8653f1428aaa2", number(r"= \d+;", "= %d;" % e["march_steps"])),
             250: ("37c8b9941d9cf057", number(r"= [\d.]+;", "= %s;" % lit(e["march_end"]))),
             269: ("#if 0", "#if %d" % e["shadow"]),
             313: ("#define FOV 1. // 45 degrees", "#define FOV %s" % lit(e["fov"]))}
    out = replace_lines(lines, edits, src)
    new = {"setup_scene": ["\tmaterials[%d] = %s;" % (i, vec3(m)) for i, m in enumerate(e["materials"])],
           "setup_camera": ["\teye = %s;" % vec3(e["eye"]), "\tlook_at = %s;" % vec3(e["look_at"])],
           "sdf": sdf_body(e["program"])}
    for name in ("sdf", "setup_camera", "setup_scene"):                # from the bottom up: the line numbers above stay true
        first, last, body, head = BODIES[name]
        assert digest(lines[first - 3]) == head and lines[first - 2].rstrip() == "{" and lines[last].rstrip() == "}", (src, name)
        assert digest("".join(lines[first - 1:last]).rstrip("\n")) == body, (src, name, "the body is not the one this tool was written for")
        out[first - 1:last] = [s + "\n" for s in new[name]]
    path = "app_sdf_ao_%s.h" % e["name"]
    with open(os.path.join(REF_DIR, "src", path), "w") as f:
        f.writelines(out)
    return path


def build_library(e):
    hdr = header_copy(e)
    target = "_ref/libsbx_ref_sdf_scene_%s.so" % e["name"]
    if os.path.exists(os.path.join(ORACLE_DIR, target)):       # (the pattern rule does not know the generated header: always rebuilt)
        os.remove(os.path.join(ORACLE_DIR, target))
    defs = "-DAPP_SDF_AO '-DSBX_REF_AUX_fog_density(d)=%s' '-DSBX_REF_AUX_fog_falloff(d)=%s'" % (lit(e["fog_density"]), lit(e["fog_falloff"]))
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % hdr, "REF_DEFS=%s" % defs], check=True)
    return load(target)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden", "sdf_scenes"))
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
        model = M.frame(S, w, h)
        m = M.masks(S, w, h)
        bad = int((~same_bits(model, frame)).any(axis=-1).sum())
        bad_pts = int((~same_bits(M.points(S, w, h, pts), pts_out)).any(axis=-1).sum())
        print(name, "model vs reference: %d of %d pixels and %d of %d points differ;" % (bad, w * h, bad_pts, n),
              "hit %d, ran out %d, left %d; nearest kinds %s; shadow exits %s; NaN %d"
              % (int(m["hit"].sum()), int(m["ran_out"].sum()), int(m["left"].sum()), np.bincount(m["kind"][m["hit"]], minlength=9)[1:].tolist(),
                 np.bincount(m["shadow_exit"][m["hit"]] + 1, minlength=4).tolist(), int(np.isnan(frame).any(axis=-1).sum())))
        assert bad == 0 and bad_pts == 0, (name, "tests/sdf_scene_model.py is not what the reference's headers compute")
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
