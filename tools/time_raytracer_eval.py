"""sbx_raytracer_eval beside SBX_APP_RAYTRACER_SCENE's frame kernel.  ONE process (the parent never opens the GPU);
the legs of a table ALTERNATE in blocks of 8 launches, every launch between its own events (tools/time_vinyl_eval.py timed); per leg the
median and min - max of N launches after a warm-up.

  functions   each of the four functions over 2^20 elements, on the Cornell block (u_time .37) and on a seeded scene of 16 planes and 16
              spheres (tests/raytracer_scene_model.tame_scene(1, (16, 16)), the scene of tools/time_raytracer_scene.py): seeded rays and
              points in the scene's box, unnormalised directions; "illuminate" and "shadow" over the hits of those rays
  frame       "render" over the 3840x2160 primary rays of the Cornell block, in frame order, beside k_raytracer_scene's frame of that block
              measured in the same run (the parent commit's figure for it: profiles/raytracer_scene_timing.txt), and the same rays in a
              fixed random permutation.  Before anything is timed the eval's colours, after the model's sRGB step, are compared with the
              frame's bits.

What the eval pays that the frame does not: 24 B in and 16 B out per ray where the frame kernel computes its ray and writes 16 B, one
64-lane wave per workgroup in launch order where the frame kernel has 8x8-pixel waves in the dispatch order, and 6 waves per SIMD (79
VGPRs) where the frame kernel fits 7.  No bar: the record states the ratio and the legs' spreads.

    python tools/time_raytracer_eval.py [--launches 40] [--warmup 16] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_vinyl_eval import BLOCK, timed  # noqa: E402

N = 1 << 20
W, H, T = 3840, 2160, .37


def elements(S, E, seed):
    """{fn: x[N, floats in]} for scene S: seeded rays in its box; the shading and shadow inputs are those rays' hits (misses: the origin)"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1, 1, size=(N, 3)) * [1.8, 1.8, 3] + [0, 2, 1.5]
    d = rng.normal(size=(N, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(.2, 2.5, size=(N, 1))
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    trace_in = np.concatenate([rays, np.full((N, 1), -1, dtype=np.float32)], axis=1)
    hits = E.evaluate("raytrace_iteration", S, trace_in)
    shade = np.concatenate([rays[:, :3], hits[:, 2:5], hits[:, 5:8], hits[:, 1:2]], axis=1).astype(np.float32)
    return {"raytrace_iteration": trace_in, "illuminate": shade, "shadow": np.ascontiguousarray(hits[:, 2:5]), "render": rays}


def child(launches, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import shaderbox_amd
    from tests import raytracer_eval_model as E
    from tests import raytracer_scene_model as M
    from tests.model_common import same_bits
    R = shaderbox_amd.Renderer(0)
    cornell = shaderbox_amd.cornell_scene(W, H, T)
    for scene, a in (("cornell", cornell), ("16+16", M.to_block(M.tame_scene(1, (16, 16))))):
        xs = {fn: torch.from_numpy(x).to(R.tdev) for fn, x in elements(M.from_block(a), E, 5).items()}
        res = timed([(fn, (lambda fn=fn: R.raytracer_eval(fn, xs[fn], a))) for fn in E.FNS], launches, warmup)
        for fn in E.FNS:
            c = R.raytracer_eval_counted(fn, xs[fn], a)[1]
            print("RESULT functions|%s|%s|%.5f|%.5f|%.5f|%d|%d" % ((scene, fn) + res[fn] + c), flush=True)
        del xs
    S = M.from_block(cornell)
    rays = E.primary_rays(S, W, H)
    ordered = torch.from_numpy(rays).to(R.tdev)
    permuted = torch.from_numpy(rays[np.random.default_rng(20).permutation(len(rays))]).to(R.tdev)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    out = R.raytracer_eval("render", ordered, cornell).cpu().numpy()
    frame = R.render("raytracer_scene", W, H, T, aux=cornell).cpu().numpy()
    same = bool(same_bits(E.finish(out[:, :3]).reshape(H, W, 4), frame).all())
    c1, c2 = R.raytracer_eval_counted("render", ordered, cornell)[1], R.raytracer_eval_counted("render", permuted, cornell)[1]
    legs = [("eval ordered", lambda: R.raytracer_eval("render", ordered, cornell)),
            ("frame", lambda: R.render("raytracer_scene", W, H, T, aux=cornell, out=buf)),
            ("eval permuted", lambda: R.raytracer_eval("render", permuted, cornell))]
    res = timed(legs, launches, warmup)
    for name, _ in legs:
        print("RESULT frame|%s|%.5f|%.5f|%.5f" % ((name,) + res[name]), flush=True)
    print("EXTRA same_bits=%d waves_ordered=%d/%d waves_permuted=%d/%d" % (same, c1[1], c1[0] + c1[1], c2[1], c2[0] + c2[1]), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.launches, args.warmup)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup), "--child"],
                       capture_output=True, text=True, timeout=1100, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("the timing process failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    rows = [ln[7:].split("|") for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    extra = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("EXTRA ")][0]
    lines = ["# tools/time_raytracer_eval.py: one process; the legs of a table alternate in blocks of %d launches; median and min - max of %d" % (BLOCK, args.launches),
             "# launches per leg after %d warm-up launches, each launch between its own events." % args.warmup, "#",
             "# 1. functions: 2^20 elements (waves: re-run / counted, from the counted twin)",
             "# %-8s %-20s %10s %10s %10s %12s   %s" % ("scene", "fn", "median ms", "min ms", "max ms", "Melements/s", "waves")]
    for _, scene, fn, med, mn, mx, wit, rerun in [x for x in rows if x[0] == "functions"]:
        lines.append("  %-8s %-20s %10.4f %10.4f %10.4f %12.1f   %d/%d"
                     % (scene, fn, float(med), float(mn), float(mx), N / float(med) / 1e3, int(rerun), int(wit) + int(rerun)))
    fr = {name: (float(med), float(mn), float(mx)) for _, name, med, mn, mx in [x for x in rows if x[0] == "frame"]}
    lines += ["#", "# 2. frame: \"render\" over the %d primary rays of the Cornell block's %dx%d frame (u_time %.2f) beside k_raytracer_scene's frame" % (W * H, W, H, T),
              "# %-20s %10s %10s %10s %12s" % ("leg", "median ms", "min ms", "max ms", "ns / ray")]
    for name in ("eval ordered", "frame", "eval permuted"):
        lines.append("  %-20s %10.4f %10.4f %10.4f %12.4f" % ((name,) + fr[name] + (fr[name][0] * 1e6 / (W * H),)))
    e, f = fr["eval ordered"], fr["frame"]
    lines += ["# " + extra + "   (waves: re-run / counted)",
              "# eval ordered / frame = %.3f (difference %.4f ms; min - max spreads %.4f and %.4f ms); the permutation costs the eval %.2fx."
              % (e[0] / f[0], e[0] - f[0], e[2] - e[1], f[2] - f[1], fr["eval permuted"][0] / e[0])]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
