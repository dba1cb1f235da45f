"""sbx_sdf_scene_eval beside SBX_APP_SDF_SCENE's frame kernel.  ONE process (the parent never opens the GPU); the legs
of a table ALTERNATE in blocks of 8 launches, every launch between its own events (tools/time_vinyl_eval.py timed); per leg the median and
min - max of N launches after a warm-up.

  functions   each of the seven functions over 2^20 elements, on the ramp block (u_time .37) and on a seeded 32-instruction scene
              (tests/sdf_scene_model.tame_scene(1, 32), the scene of tools/time_sdf_scene.py): seeded rays from a ring around the scene,
              aimed into it, half of them unnormalised; seeded points within +-3 of the origin for "sdf" and "sdf_normal"; the inputs of
              "sdf_ao", "sdf_shadow" and "illuminate" are what the device's own "render_impl", "sdf_normal", "sdf_ao" and "sdf_shadow"
              give at those rays' march exits (a miss's t is where it left), so the legs run the work a renderer would hand them
  frame       "render" over the 3840x2160 primary rays of the ramp block, in frame order, beside k_sdf_scene's frame of that block measured
              in the same run, and the same rays in a fixed random permutation.  Before anything is timed the eval's colours, after the
              model's sRGB step, are compared with the frame's bits.

What the eval pays that the frame does not: 24 B in and 16 B out per ray where the frame kernel computes its ray and writes 16 B, and one
64-lane wave per workgroup in launch order where the frame kernel has 8x8-pixel waves in the dispatch order.  No bar: the record states
the ratio and the legs' spreads, and what they allow one to read.

    python tools/time_sdf_scene_eval.py [--launches 40] [--warmup 16] [--out FILE]
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


def elements(R, a, S, seed):
    """{fn: device tensor [N, floats in]} for block a (scene dictionary S)"""
    import torch
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, size=N)
    o = np.stack([5 * np.cos(ang), rng.uniform(1, 4, size=N), 5 * np.sin(ang)], axis=1)
    aim = rng.uniform(-1, 1, size=(N, 3)) * [2.5, 1, 2.5] + [0, .8, 0] - o
    d = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    d[N // 2:] *= rng.uniform(.5, 2, size=(N - N // 2, 1))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(R.tdev)  # noqa: E731
    rays = dev(np.concatenate([o, d], axis=1))
    pts = dev(rng.uniform(-3, 3, size=(N, 3)))
    impl = R.sdf_scene_eval("render_impl", rays, a)
    p = rays[:, :3] + rays[:, 3:] * impl[:, 3:4]
    nrm = R.sdf_scene_eval("sdf_normal", p, a)
    nrm = torch.where(torch.isfinite(nrm).all(dim=1, keepdim=True), nrm, torch.tensor([0., 1., 0.], device=R.tdev))
    ao_in = torch.cat([p, nrm], dim=1)
    ao = R.sdf_scene_eval("sdf_ao", ao_in, a)
    sun = torch.tensor([float(v) for v in S["sun_dir"]], dtype=torch.float32, device=R.tdev)
    sh_in = torch.cat([p + sun * 0.05, sun.expand_as(p).contiguous()], dim=1)
    sh = R.sdf_scene_eval("sdf_shadow", sh_in, a)
    ids = torch.where(impl[:, 4:5] >= 0, impl[:, 4:5], torch.ones_like(ao))
    return {"sdf": pts, "sdf_normal": pts, "sdf_ao": ao_in, "sdf_shadow": sh_in, "illuminate": torch.cat([p, nrm, ids, ao, sh], dim=1),
            "render_impl": rays, "render": rays}


def child(launches, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import shaderbox_amd
    from tests import sdf_scene_eval_model as E
    from tests import sdf_scene_model as M
    from tests.model_common import same_bits
    R = shaderbox_amd.Renderer(0)
    ramp = shaderbox_amd.sdf_ramp_scene(W, H, T)
    for scene, a in (("ramp", ramp), ("32", M.as_aux(M.tame_scene(1, 32)))):
        xs = elements(R, a, M.from_block(bytes(a)), 5)
        res = timed([(fn, (lambda fn=fn: R.sdf_scene_eval(fn, xs[fn], a))) for fn in E.FNS], launches, warmup)
        for fn in E.FNS:
            c = R.sdf_scene_eval_counted(fn, xs[fn], a)[1]
            print("RESULT functions|%s|%s|%.5f|%.5f|%.5f|%d|%d" % ((scene, fn) + res[fn] + c), flush=True)
        del xs
    S = M.from_block(bytes(ramp))
    rays = E.primary_rays(S, W, H)
    ordered = torch.from_numpy(rays).to(R.tdev)
    permuted = torch.from_numpy(rays[np.random.default_rng(20).permutation(len(rays))]).to(R.tdev)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    out = R.sdf_scene_eval("render", ordered, ramp).cpu().numpy()
    frame = R.render("sdf_scene", W, H, T, aux=ramp).cpu().numpy()
    same = bool(same_bits(E.finish(out[:, :3]).reshape(H, W, 4), frame).all())
    c1, c2 = R.sdf_scene_eval_counted("render", ordered, ramp)[1], R.sdf_scene_eval_counted("render", permuted, ramp)[1]
    legs = [("eval ordered", lambda: R.sdf_scene_eval("render", ordered, ramp)),
            ("frame", lambda: R.render("sdf_scene", W, H, T, aux=ramp, out=buf)),
            ("eval permuted", lambda: R.sdf_scene_eval("render", permuted, ramp))]
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
    lines = ["# tools/time_sdf_scene_eval.py: one process; the legs of a table alternate in blocks of %d launches; median and min - max of %d" % (BLOCK, args.launches),
             "# launches per leg after %d warm-up launches, each launch between its own events." % args.warmup, "#",
             "# 1. functions: 2^20 elements (waves: re-run / counted, from the counted twin)",
             "# %-8s %-14s %10s %10s %10s %12s   %s" % ("scene", "fn", "median ms", "min ms", "max ms", "Melements/s", "waves")]
    for _, scene, fn, med, mn, mx, wit, rerun in [x for x in rows if x[0] == "functions"]:
        lines.append("  %-8s %-14s %10.4f %10.4f %10.4f %12.1f   %d/%d"
                     % (scene, fn, float(med), float(mn), float(mx), N / float(med) / 1e3, int(rerun), int(wit) + int(rerun)))
    fr = {name: (float(med), float(mn), float(mx)) for _, name, med, mn, mx in [x for x in rows if x[0] == "frame"]}
    lines += ["#", "# 2. frame: \"render\" over the %d primary rays of the ramp block's %dx%d frame (u_time %.2f) beside k_sdf_scene's frame" % (W * H, W, H, T),
              "# %-20s %10s %10s %10s %12s" % ("leg", "median ms", "min ms", "max ms", "ns / ray")]
    for name in ("eval ordered", "frame", "eval permuted"):
        lines.append("  %-20s %10.4f %10.4f %10.4f %12.4f" % ((name,) + fr[name] + (fr[name][0] * 1e6 / (W * H),)))
    e, f = fr["eval ordered"], fr["frame"]
    gap, room = abs(e[0] - f[0]), max(e[2] - e[1], f[2] - f[1])
    lines += ["# " + extra + "   (waves: re-run / counted)",
              "# eval ordered / frame = %.3f (difference %.4f ms; min - max spreads %.4f and %.4f ms); the permutation costs the eval %.2fx."
              % (e[0] / f[0], e[0] - f[0], e[2] - e[1], f[2] - f[1], fr["eval permuted"][0] / e[0]),
              "# Reading: the difference is %s the larger spread, so this run %s the two apart."
              % (("within", "does not tell") if gap <= room else ("beyond", "tells"))]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
