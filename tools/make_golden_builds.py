#!/usr/bin/env python3
"""Generate tests/golden/<family>_builds/*.npz for the build families of tests/build_families.py: frames and points of a reference
shader header rendered by the reference header ITSELF with one compile-time switch the other way.  The table
says, per family and build, which line is edited, at which uniforms the frames and points are taken, how they are stored, and the
conditions under which a fixture says something; this tool records under them and tests/test_*_builds_cpu.py assert them again of the
committed files.

Runs only where the reference tree is (oracle/Makefile's REFERENCE).  `make -C oracle ref` generates oracle/_ref/src from the
reference's headers; this tool writes one edited copy of the family's header per build next to it (app_planet_unlit.h: the
`#define LIGHT` at :249 turned into a comment), each edit asserted to change exactly that line, from exactly the text expected there,
and builds it with the oracle's own pattern rule, the header and the defines given as make variables on the command line
(oracle/Makefile is not edited):
    make -C oracle _ref/libsbx_ref_planet_unlit.so REF_HDR=app_planet_unlit.h REF_DEFS=-DAPP_PLANET
oracle/_ref is git-ignored: neither the copies nor the libraries are ever committed.  What is committed are recorded results, per build:
    uniforms                u_res, u_mouse, u_time per frame
    <key per frame>         storage "raw": the float frames.  Storage "xor": the XOR of the frame's rgb bit patterns with the SHIPPED
                            build's under the same uniforms (uint32: zero where the builds agree, which deflates to nothing); alpha
                            is 1 in every pixel, asserted here.  The shipped build's frames are not stored: they are the CPU oracle's,
                            which this tool asserts equal to the reference's shipped build bit for bit before it encodes against them
    big_uniforms, <key per frame>
                            the same of the larger frame set, for the builds that have one
    points, points_uniforms, points_out | points_xor, points_shipped
                            fragCoords drawn with a fixed seed from the family's or the build's rectangle, off-centre; the edited
                            header's sbxr_main_image answers and the shipped header's
    aux_sets, aux_uniforms, aux_counts, <key per set>
                            clouds: one frame per aux set of tests/golden/reference_aux_sets.json — one more build each, with the
                            -D'SBX_REF_AUX_<name>(d)=...' defines that oracle/aux_sets.py generates (`_ref/libsbx_ref_clouds_height@steer.so`)
                            — and the pixels that differ from the shipped build's frame under the same set
tests/model_common.py builds_fixture() decodes.  NaN pixels are data: `differ` counts NaN == NaN as equal, like every comparison of
this project.

    python tools/make_golden_builds.py [FAMILY ...] [--out-dir DIR]       every family by default; DIR/<family>_builds/ instead of tests/golden/
    python tools/make_golden_builds.py egg --find-rects                   the bounding boxes egg's point rectangles were chosen from
"""
import argparse
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import aux_sets  # noqa: E402
from oracle.oracle import Oracle, REF_DIR, reference_root  # noqa: E402
from tests.build_families import FAMILIES, frame_keys  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")


def edited_header(fam, build):
    src = os.path.join(REF_DIR, "src", fam["header"])
    lines = open(src).read().splitlines(keepends=True)
    at, old, new = fam["builds"][build]["edit"]
    assert lines[at - 1].rstrip() == old, "%s:%d reads %r, expected %r" % (src, at, lines[at - 1], old)
    out = lines[:at - 1] + ([] if new is None else [lines[at - 1].replace(old, new, 1)]) + lines[at:]
    if new is None:                                 # exactly one line gone, at that number, and no other line like it left
        assert len(out) == len(lines) - 1 and out[:at - 1] == lines[:at - 1] and out[at - 1:] == lines[at:]
        assert not any(l.startswith(old) for l in out)
    else:                                           # exactly one line changed, at that number
        assert len(out) == len(lines) and [i for i in range(len(lines)) if out[i] != lines[i]] == [at - 1] and out[at - 1].rstrip() == new
    name = "%s_%s.h" % (fam["header"][:-2], build)
    with open(os.path.join(REF_DIR, "src", name), "w") as f:
        f.writelines(out)
    return name


def load(target):
    lib = ctypes.CDLL(os.path.join(ORACLE_DIR, target))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.sbxr_render_rows.argtypes = [fp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, fp, ctypes.c_int]
    lib.sbxr_main_image.argtypes = [fp, ctypes.c_float, ctypes.c_float, fp]
    return lib


def build_library(fam, build, aux_set=None):
    name, shipped = edited_header(fam, build), fam["shipped"][0]
    defs = fam["ref_defs"]
    target = "_ref/libsbx_ref_%s_%s.so" % (shipped, build)
    if aux_set is not None:
        defs += " " + aux_sets.defines(shipped, aux_sets.load()[shipped][aux_set])
        target = "_ref/libsbx_ref_%s_%s@%s.so" % (shipped, build, aux_set)
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, target, "REF_HDR=%s" % name, "REF_DEFS=%s" % defs], check=True)
    return load(target)


def render(lib, size, t, mouse=(0.0, 0.0), threads=8):
    u = Oracle._uni(size[0], size[1], t, mouse)
    rows = np.arange(size[1], dtype=np.int32)
    out = np.zeros((size[1], size[0], 4), dtype=np.float32)
    lib.sbxr_render_rows(Oracle._fp(u), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), size[1], Oracle._fp(out), threads)
    return out


def points_of(lib, size, pts, t):
    u = Oracle._uni(size[0], size[1], t, (0.0, 0.0))
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


def uniforms_array(size, uniforms):
    return np.array([[size[0], size[1], m[0], m[1], t] for t, m in uniforms], dtype=np.float32)   # u_res, u_mouse, u_time per frame


def size_bound(fam):
    """the most bytes a fixture of the family may have"""
    if fam["max_bytes"] == "largest":               # the largest .npz directly under tests/golden/
        return max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    return fam["max_bytes"]


def shipped_frame(fam, oracle, size, t, mouse=(0.0, 0.0), aux_set=None):
    """the shipped build's frame from the reference library, asserted equal to the oracle's (what builds_fixture() decodes against)"""
    name, app = fam["shipped"]
    ref = render(load("_ref/libsbx_ref_%s%s.so" % (name, "" if aux_set is None else "@" + aux_set)), size, t, mouse)
    aux = None if aux_set is None else aux_sets.block(name, aux_sets.load()[name][aux_set])
    assert not differ(ref, oracle.render(app, size[0], size[1], t, mouse=mouse, aux=aux)).any(), \
        ("the oracle's %s is not the reference's" % name, size, t, mouse, aux_set)
    return ref


def frame_set(fam, build, lib, oracle, size, uniforms, keys, min_pixels, max_nan):
    """one set of frames of a build, its conditions asserted -> (arrays to store, pixels that differ per frame, NaN pixels per frame)"""
    b = fam["builds"][build]
    threads = fam.get("render_threads", 8)
    frames = [render(lib, size, t, m, threads) for t, m in uniforms]
    base = [shipped_frame(fam, oracle, size, t, m) for t, m in uniforms]
    assert all((f[..., 3] == 1).all() for f in frames)
    if fam.get("render_twice"):
        assert all(not differ(f, render(lib, size, t, m, threads)).any() for f, (t, m) in zip(frames, uniforms)), (build, "a second render differs")
    nans = [nan_pixels(f) for f in frames]
    if max_nan is not None:
        assert max(nans) <= max_nan, (build, nans)
    counts = [int(differ(f, s).sum()) for f, s in zip(frames, base)]
    if min_pixels is not None:
        assert all(c >= m for c, m in zip(counts, np.broadcast_to(min_pixels, len(counts)))), (build, counts)
    if "equal_frames" in b and size == fam["size"]:
        first = b["equal_frames"][0]
        assert all(not differ(frames[first], frames[i]).any() for i in b["equal_frames"][1:]), (build, "frames", b["equal_frames"], "differ")
    stored = frames if fam["storage"] == "raw" else [rgb_bits(f) ^ rgb_bits(s) for f, s in zip(frames, base)]
    return dict(zip(frame_keys(keys, uniforms), stored)), counts, nans


def aux_set_frames(fam, build, oracle):
    """clouds: the build under every aux set of the family, `zero` equal to the shipped build and the others not"""
    size, t, out, counts = fam["size"], fam["aux_time"], {}, []
    for s in fam["aux_sets"]:
        frame, base = render(build_library(fam, build, s), size, t), shipped_frame(fam, oracle, size, t, aux_set=s)
        assert not np.isnan(frame).any()
        counts.append(int(differ(frame, base).sum()))
        assert (counts[-1] == 0) if s == "zero" else (counts[-1] > 0), (build, s, counts[-1])
        out["x_aux_" + s] = rgb_bits(frame) ^ rgb_bits(base)
    head = dict(aux_sets=np.array(fam["aux_sets"]), aux_uniforms=np.array([size[0], size[1], 0.0, 0.0, t], dtype=np.float32),
                aux_counts=np.array(counts, dtype=np.int64))
    return head, out, dict(zip(fam["aux_sets"], counts))


def point_set(fam, build, lib, shipped, no_nan):
    b, p = fam["builds"][build], fam["points"]
    x0, y0, x1, y1 = b.get("rect") or p["rect"] or (0, 0) + p["size"]
    rng = np.random.default_rng(p["seed"])
    pts = (rng.uniform(0, 1, size=(p["count"], 2)) * [x1 - x0, y1 - y0] + [x0, y0]).astype(np.float32)
    got, base = points_of(lib, p["size"], pts, p["time"]), points_of(shipped, p["size"], pts, p["time"])
    assert (got[:, 3] == 1).all() and (base[:, 3] == 1).all() and not (no_nan and np.isnan(got).any())
    n = int(differ(got, base).sum())
    assert n >= b.get("min_points", 0), (build, n, "choose another seed or rectangle")
    out = dict(points=pts, points_uniforms=np.array([p["size"][0], p["size"][1], 0.0, 0.0, p["time"]], dtype=np.float32))
    if fam["storage"] == "raw":
        out.update(points_out=got, points_shipped=base)
    else:
        out.update(points_xor=rgb_bits(got) ^ rgb_bits(base), points_shipped=np.ascontiguousarray(base[:, :3]))
    return out, n


def find_rects(fam, shipped):
    """egg: where the edited header's frame of the points' uniforms differs from the shipped header's"""
    p = fam["points"]
    base = render(shipped, p["size"], p["time"])
    for build in fam["builds"]:
        ys, xs = np.nonzero(differ(render(build_library(fam, build), p["size"], p["time"]), base))
        print(build, "differs in", len(xs), "pixels; RECT", (int(xs.min()) - 8, int(ys.min()) - 8, int(xs.max()) + 9, int(ys.max()) + 9))


def make(family, out_dir, oracle):
    fam = FAMILIES[family]
    shipped = load("_ref/libsbx_ref_%s.so" % fam["shipped"][0])
    os.makedirs(out_dir, exist_ok=True)
    no_nan = fam.get("no_nan", False)
    for build, b in fam["builds"].items():
        lib = build_library(fam, build)
        frames, counts, nans = frame_set(fam, build, lib, oracle, fam["size"], fam["uniforms"], fam["keys"], b.get("min_pixels"),
                                         0 if no_nan else b.get("max_nan"))
        arrays = {"uniforms": uniforms_array(fam["size"], fam["uniforms"])}    # the order of the file's members: part of its bytes
        big_counts, big_nans, aux_counts, n = [], [], {}, None
        if "aux_sets" in fam:
            head, more, aux_counts = aux_set_frames(fam, build, oracle)
            arrays.update(head)
            frames.update(more)
        if fam["points"]:
            more, n = point_set(fam, build, lib, shipped, no_nan)
            arrays.update(more)
        arrays.update(frames)
        if "min_big" in b:
            big = fam["big"]
            more, big_counts, big_nans = frame_set(fam, build, lib, oracle, big["size"], big["uniforms"], fam["big_keys"], b["min_big"],
                                                   0 if no_nan else b.get("max_nan_big"))
            arrays.update(big_uniforms=uniforms_array(big["size"], big["uniforms"]), **more)
        path = os.path.join(out_dir, fam["file"] % build)
        np.savez_compressed(path, **arrays)
        bound = size_bound(fam)
        assert bound is None or os.path.getsize(path) <= bound, (build, os.path.getsize(path), bound)
        print(family, build, os.path.getsize(path), "bytes (bound %s); %dx%d frames differ from the shipped build's in" % ((bound,) + fam["size"]),
              counts, "pixels (NaN pixels", nans, "), the big frames in", big_counts, "(NaN", big_nans, "), the aux-set frames in", aux_counts,
              ", the points in", n)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("families", nargs="*", metavar="FAMILY", help="of %s; all by default" % ", ".join(FAMILIES))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"), help="write DIR/<family>_builds/ (default: tests/golden)")
    ap.add_argument("--find-rects", action="store_true", help="egg: print the bounding boxes of the differing pixels and write nothing")
    args = ap.parse_args()
    unknown = [f for f in args.families if f not in FAMILIES]
    if unknown:
        ap.error("no such family: %s" % ", ".join(unknown))
    if not os.path.isdir(os.path.join(reference_root(), "src")):
        sys.exit("the reference tree (%s) is not on this machine: nothing to render the fixtures with" % reference_root())
    subprocess.run(["make", "-s", "-j8", "-C", ORACLE_DIR, "ref"], check=True)
    if args.find_rects:
        find_rects(FAMILIES["egg"], load("_ref/libsbx_ref_egg.so"))
        sys.exit(0)
    oracle = Oracle()
    for family in args.families or list(FAMILIES):
        make(family, os.path.join(args.out_dir, family + "_builds"), oracle)
