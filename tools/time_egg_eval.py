"""sbx_egg_eval and SBX_APP_EGG_POSE beside the frame kernels of APP_EGG.  Three comparisons, each in ONE process of
its own (the parent never opens the GPU) whose legs ALTERNATE in blocks of 8 launches, every launch between its own events; per leg
the median and min - max of N launches after a warm-up:

  eval   "render_scene" over the primary rays of the shipped camera's 1280x720 frame (u_time .37; computed on the host with
         tests/egg_pose_model.primary_rays) in frame order, beside the SBX_APP_EGG frame of that size and time under sbx_set_variant 1
         (k_egg<CULL = false, IEEE roots>) and under the default; the same rays in a fixed random permutation; "ik_solver" over 2^22
         seeded elements as GB/s (44 B an element) beside the plain copy tools/time_copy_kernels.py times (sbx_assemble at 3840x2160:
         16 B read + 16 B written a pixel).  The bar: the eval's median is no more than the variant-1 frame's.
  pose   SBX_APP_EGG_POSE with no block beside SBX_APP_EGG at 1920x1080: the same kernels over the same frame constants.
  egg    SBX_APP_EGG at 1920x1080 alone, run twice: the spread of two runs, against which the ratio of `pose` is read.  With
         --parent-root DIR (a checkout of the parent commit with its library built) the two runs use that tree's package.

    python tools/time_egg_eval.py [--launches 40] [--warmup 16] [--parent-root DIR] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T = 1280, 720, .37
PW, PH = 1920, 1080
BLOCK = 8


def timed(legs, launches, warmup):
    """legs: [(name, fn)] -> {name: (median, min, max)} in ms; blocks of BLOCK launches of one leg, the legs in turn"""
    import torch
    for _ in range((warmup + BLOCK - 1) // BLOCK):
        for _, fn in legs:
            for _ in range(BLOCK):
                fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for _ in range((launches + BLOCK - 1) // BLOCK):
        for name, fn in legs:
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(BLOCK)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ms[name] += [a.elapsed_time(b) for a, b in ev]
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}


def child(kind, launches, warmup, root):
    sys.path.insert(0, root)
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    extra = ""
    if kind == "eval":
        from tests import egg_pose_model as M
        P = M.default_pose(T)
        fx = (np.arange(W, dtype=np.float32) + np.float32(.5))[None, :]
        fy = (np.arange(H, dtype=np.float32) + np.float32(.5))[:, None]
        _, ro, rd = M.primary_rays(P, W, H, fx, fy)
        rays = np.stack([np.full(W * H, c, dtype=np.float32) for c in ro] + list(rd), axis=1).astype(np.float32)
        a = M.as_aux(P)
        ordered = torch.from_numpy(rays).to(R.tdev)
        permuted = torch.from_numpy(rays[np.random.default_rng(20).permutation(len(rays))]).to(R.tdev)
        # the same bits as the frame's, before anything is timed (bars and sRGB by the model)
        out = R.egg_eval("render_scene", ordered, a).cpu().numpy()
        frame = R.render("egg", W, H, T).cpu().numpy()
        pcx = M.primary_rays(P, W, H, fx, fy)[0]
        same = bool(M.same_bits(M.finish(out[:, :3], out[:, 3], pcx).reshape(H, W, 4), frame).all())
        c1, c2 = R.egg_eval_counted("render_scene", ordered, a)[1], R.egg_eval_counted("render_scene", permuted, a)[1]
        extra = "same_bits=%d waves_ordered=%d/%d waves_permuted=%d/%d" % (same, c1[1], c1[0] + c1[1], c2[1], c2[0] + c2[1])
        buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
        n_ik = 1 << 22
        ik_in = torch.from_numpy(np.random.default_rng(21).uniform(-1, 1, size=(n_ik, 8)).astype(np.float32)).to(R.tdev)
        cw, ch = 3840, 2160
        rows_max = shaderbox_amd.shard.rank_rows_max(ch, 8, 8)
        slabs = torch.rand((8, rows_max, cw, 4), dtype=torch.float32, device=R.tdev)
        cout = torch.empty((ch, cw, 4), dtype=torch.float32, device=R.tdev)

        def frame_v(v):
            R.set_variant(v)
            R.render("egg", W, H, T, out=buf)
            R.set_variant(0)
        legs = [("eval ordered", lambda: R.egg_eval("render_scene", ordered, a)), ("frame variant 1", lambda: frame_v(1)),
                ("frame default", lambda: frame_v(0)), ("eval permuted", lambda: R.egg_eval("render_scene", permuted, a)),
                ("ik_solver 2^22", lambda: R.egg_eval("ik_solver", ik_in)), ("copy 3840x2160", lambda: R.assemble(slabs, cw, ch, 8, 8, out=cout))]
    elif kind == "pose":
        buf = torch.empty((PH, PW, 4), dtype=torch.float32, device=R.tdev)
        legs = [("egg_pose no block", lambda: R.render("egg_pose", PW, PH, T, out=buf)), ("egg", lambda: R.render("egg", PW, PH, T, out=buf))]
    else:
        buf = torch.empty((PH, PW, 4), dtype=torch.float32, device=R.tdev)
        legs = [("egg", lambda: R.render("egg", PW, PH, T, out=buf))]
    res = timed(legs, launches, warmup)
    for name, _ in legs:
        print("RESULT %s|%.5f|%.5f|%.5f" % ((name,) + res[name]), flush=True)
    print("EXTRA " + extra, flush=True)
    R.close()


def run(kind, args, root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                        "--child", kind, "--root", root], capture_output=True, text=True, timeout=900, cwd=root)
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (kind, r.returncode, r.stderr[-2000:]))
    res = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            name, med, mn, mx = ln[7:].split("|")
            res[name] = (float(med), float(mn), float(mx))
    extra = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("EXTRA ")][0]
    return res, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: the two `egg` runs use it")
    ap.add_argument("--out", default=None, help="also write the tables and the readings to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.warmup, args.root)
    assert args.launches >= 24, "at least 24 timed launches per leg"
    row = lambda name, r, more="": "  %-22s %10.4f %10.4f %10.4f   %s" % (name, r[0], r[1], r[2], more)  # noqa: E731
    head = "# %-22s %10s %10s %10s" % ("leg", "median ms", "min ms", "max ms")
    lines = ["# tools/time_egg_eval.py: u_time %.2f; per comparison one process whose legs alternate in blocks of %d launches; median and" % (T, BLOCK),
             "# min - max of %d launches per leg after %d warm-up launches, each launch between its own events." % (args.launches, args.warmup), "#",
             "# 1. eval: \"render_scene\" over the %d primary rays of the shipped %dx%d frame, frame order" % (W * H, W, H), head]
    ev, extra = run("eval", args, ROOT)
    px = W * H
    for name in ("eval ordered", "frame variant 1", "frame default", "eval permuted"):
        lines.append(row(name, ev[name], "%.3f ns / ray" % (ev[name][0] * 1e6 / px)))
    ik, cp = ev["ik_solver 2^22"], ev["copy 3840x2160"]
    lines.append(row("ik_solver 2^22", ik, "%.0f GB/s (44 B an element)" % ((1 << 22) * 44 / ik[0] / 1e6)))
    lines.append(row("copy 3840x2160", cp, "%.0f GB/s (32 B a pixel)" % (3840 * 2160 * 32 / cp[0] / 1e6)))
    lines.append("# " + extra + "   (waves: re-run / counted)")
    e, f = ev["eval ordered"], ev["frame variant 1"]
    lines += ["# Bar: the eval over the ordered rays %.4f ms <= the variant-1 frame %.4f ms: %s (ratio %.3f; the default frame: %.3fx; the"
              % (e[0], f[0], "MET" if e[0] <= f[0] else "MISSED", e[0] / f[0], e[0] / ev["frame default"][0]),
              "# permutation costs the eval %.2fx)." % (ev["eval permuted"][0] / e[0]), "#",
              "# 2. pose: SBX_APP_EGG_POSE with no block beside SBX_APP_EGG at %dx%d, one process" % (PW, PH), head]
    print("\n".join(lines), flush=True)
    n0 = len(lines)
    po, _ = run("pose", args, ROOT)
    for name in ("egg_pose no block", "egg"):
        lines.append(row(name, po[name]))
    proot = args.parent_root or ROOT
    lines += ["#", "# 3. egg: SBX_APP_EGG at %dx%d alone, two runs of %s" % (PW, PH, "the parent commit's library" if args.parent_root else "this library"), head]
    runs = [run("egg", args, proot)[0]["egg"] for _ in range(2)]
    for i, r in enumerate(runs):
        lines.append(row("egg, run %d" % (i + 1), r))
    ratio = po["egg_pose no block"][0] / po["egg"][0]
    spread = max(runs[0][0], runs[1][0]) / min(runs[0][0], runs[1][0])
    lines += ["# Reading: egg_pose / egg = %.4f; the two runs differ by a factor of %.4f: the ratio lies %s that spread."
              % (ratio, spread, "WITHIN" if 1 / spread <= ratio <= spread else "OUTSIDE")]
    print("\n".join(lines[n0:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
