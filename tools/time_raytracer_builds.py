"""SBX_APP_RAYTRACER_PHONG, SBX_APP_RAYTRACER_NOSHADOW and SBX_APP_RAYTRACER_STATIC beside SBX_APP_RAYTRACER: one-launch
times at 3840x2160 of the four builds, each with the default kernel and the IEEE one (sbx_set_variant 1: IEEE roots and
normalisations, the six-plane loop).  ONE child process runs every case (the parent never opens the GPU) under one time limit, and a
failure is final: nothing is tried twice.  The cases are timed in PASSES — every case once per pass, the passes one after the other
— so that each case is measured at several moments of the run: the table gives, per case, the median over all launches, and the
lowest and highest PASS median, which is the run-to-run spread the ratios are to be read against.  Every launch is bracketed by its
own pair of events.

--baseline-lib PATH times SBX_APP_RAYTRACER of another build of libsbx.so (the parent commit's) in the same process, right after
this tree's in every pass: if the two differ by more than the spread, this tree's template parameter has leaked into the existing
kernel.

    python tools/time_raytracer_builds.py [--launches 20] [--passes 5] [--warmup 5] [--baseline-lib libsbx_parent.so]
Writes profiles/raytracer_builds_timing.txt (or --out).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, U_TIME = 3840, 2160, 1.5
APPS = ("raytracer", "raytracer_phong", "raytracer_noshadow", "raytracer_static")
# (app, kernel form, variant)
CASES = [(a, k, v) for k, v in (("default", 0), ("ieee", 1)) for a in APPS]


def with_baseline(cases, head):
    """every SBX_APP_RAYTRACER case followed by the same case of the baseline library"""
    return [c for x in cases for c in ([x, head + x[len(head):]] if x[len(head)] == "raytracer" else [x])]


def child(launches, passes, warmup, baseline):
    import torch
    import shaderbox_amd
    here = shaderbox_amd.Renderer(0)
    cases = [(here, "this tree") + c for c in CASES]
    if baseline:
        shaderbox_amd.LIB_PATH = os.path.abspath(baseline)
        base = shaderbox_amd.Renderer(0)
        cases = with_baseline(cases, (base, "baseline"))
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=here.tdev)
    for R, _, app, _, variant in cases:
        R.set_variant(variant)
        for k in range(warmup):
            R.render(app, W, H, U_TIME, out=buf)
    torch.cuda.synchronize()
    for p in range(passes):
        for i, (R, _, app, _, variant) in enumerate(cases):
            R.set_variant(variant)
            for k in range(warmup):
                R.render(app, W, H, U_TIME, out=buf)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
            for a, b in ev:
                a.record()
                R.render(app, W, H, U_TIME, out=buf)
                b.record()
            torch.cuda.synchronize()
            print("RESULT %d %d %s" % (i, p, " ".join("%.5f" % a.elapsed_time(b) for a, b in ev)), flush=True)
    for R in {id(c[0]): c[0] for c in cases}.values():
        R.close()


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raytracer_builds_timing.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.launches, args.passes, args.warmup, args.baseline_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--passes", str(args.passes),
           "--warmup", str(args.warmup)] + (["--baseline-lib", args.baseline_lib] if args.baseline_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise SystemExit("the timing process failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    names = [("this tree",) + c for c in CASES]
    if args.baseline_lib:
        names = with_baseline(names, ("baseline",))
    per = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            f = ln.split()
            per.setdefault(int(f[1]), {})[int(f[2])] = [float(x) for x in f[3:]]
    lines = ["# tools/time_raytracer_builds.py: %dx%d, float frames, u_time %g, u_mouse (0, 0); one process; %d passes over all cases, %d"
             % (W, H, U_TIME, args.passes, args.launches),
             "# back-to-back launches per case and pass after %d warm-up launches, each launch between its own events.  kernel: default ="
             % args.warmup,
             "# sbx_set_variant 0, ieee = sbx_set_variant 1.  median ms: over all launches of the case; pass lo / hi: the lowest and highest",
             "# per-pass median (the run-to-run spread); ratio: median / this tree's raytracer with the same kernel form.",
             "# %-10s %-19s %-8s %10s %10s %10s %10s %8s" % ("library", "app", "kernel", "median ms", "pass lo", "pass hi", "min ms", "ratio")]
    med = {}
    for i, (libname, app, kname, _) in enumerate(names):
        allv = [x for p in sorted(per[i]) for x in per[i][p]]
        pm = [median(v) for v in per[i].values()]
        med[(libname, app, kname)] = median(allv)
        base = med[("this tree", "raytracer", kname)]
        lines.append("  %-10s %-19s %-8s %10.4f %10.4f %10.4f %10.4f %8.3f" % (libname, app, kname, median(allv), min(pm), max(pm), min(allv),
                                                                              median(allv) / base))
    print("\n".join(lines), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
