"""SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL beside SBX_APP_EGG: one-launch times at 1920x1080 of the three builds,
each with the default kernel and the plain one (sbx_set_variant 1), on a STANDING scene (every launch at u_time 0.02: after a few
launches the dispatch-order table of the scene is in use, sbx_tile_order.h) and on an ANIMATED one (u_time advances by 1 / 600 per
launch from 0.02, the figure in view throughout: k_egg's own hot-first order, no table).  ONE child process runs every case (the parent
never opens the GPU) under one time limit, and a failure is final: nothing is tried twice.  The cases are timed in PASSES — every
case once per pass, the passes one after the other — so that each case is measured at several moments of the run: the table
gives, per case, the median over all launches, and the lowest and highest PASS median, which is the run-to-run spread the ratios
are to be read against.  Every launch is bracketed by its own pair of events.

--baseline-lib PATH times SBX_APP_EGG of another build of libsbx.so (the parent commit's) in the same process, alternating
with this tree's in every pass: if the two differ by more than the spread, this tree's template parameter has leaked into the
existing kernel.

    python tools/time_egg_builds.py [--launches 20] [--passes 5] [--warmup 5] [--baseline-lib libsbx_parent.so]
Writes profiles/egg_builds_timing.txt (or --out).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, U_TIME, DT = 1920, 1080, 0.02, 1.0 / 600.0
APPS = ("egg", "egg_straight", "egg_oval")
# (app, kernel form, variant, animated)
CASES = [(a, k, v, m) for m in (False, True) for k, v in (("default", 0), ("plain", 1)) for a in APPS]


def child(launches, passes, warmup, baseline):
    import torch
    import shaderbox_amd
    here = shaderbox_amd.Renderer(0)
    cases = [(here, "this tree") + c for c in CASES]
    if baseline:
        shaderbox_amd.LIB_PATH = os.path.abspath(baseline)
        base = shaderbox_amd.Renderer(0)
        cases = [c for x in cases for c in ([x, (base, "baseline") + x[2:]] if x[2] == "egg" else [x])]
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=here.tdev)
    for R, _, app, _, variant, moving in cases:
        R.set_variant(variant)
        for k in range(warmup):
            R.render(app, W, H, U_TIME + (k * DT if moving else 0.0), out=buf)
    torch.cuda.synchronize()
    for p in range(passes):
        for i, (R, _, app, _, variant, moving) in enumerate(cases):
            R.set_variant(variant)
            for k in range(warmup):                      # the case's own scene again: a standing one gets its table back
                R.render(app, W, H, U_TIME + (k * DT if moving else 0.0), out=buf)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
            for k, (a, b) in enumerate(ev):
                a.record()
                R.render(app, W, H, U_TIME + (k * DT if moving else 0.0), out=buf)
                b.record()
            torch.cuda.synchronize()
            print("RESULT %d %d %s" % (i, p, " ".join("%.5f" % a.elapsed_time(b) for a, b in ev)), flush=True)
    for R in {id(c[0]): c[0] for c in cases}.values():
        R.close()


def resources():
    """VGPRs, scratch and code size of every instantiation of k_egg (tools/kernel_resources.py: hipcc cross-compiles, no GPU needed)"""
    kr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "kern_egg.hip"], capture_output=True, text=True, check=True)
    return ["#", "# tools/kernel_resources.py kern_egg.hip: k_egg<CULL, WIT, BUILD>, BUILD 0 = egg, 1 = egg_straight, 2 = egg_oval"] + \
           ["# " + ln for ln in kr.stdout.splitlines()]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egg_builds_timing.txt"))
    ap.add_argument("--no-resources", action="store_true", help="leave out the kernel_resources table (it compiles kern_egg.hip)")
    ap.add_argument("--resources-only", action="store_true", help="only append that table to --out (a timing run made with --no-resources)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.resources_only:
        with open(args.out, "a") as f:
            f.write("\n".join(resources()) + "\n")
        return
    if args.child:
        return child(args.launches, args.passes, args.warmup, args.baseline_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--passes", str(args.passes),
           "--warmup", str(args.warmup)] + (["--baseline-lib", args.baseline_lib] if args.baseline_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise SystemExit("the timing process failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    names = [("this tree",) + c for c in CASES]
    if args.baseline_lib:
        names = [c for x in names for c in ([x, ("baseline",) + x[1:]] if x[1] == "egg" else [x])]
    per = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            f = ln.split()
            per.setdefault(int(f[1]), {})[int(f[2])] = [float(x) for x in f[3:]]
    lines = ["# tools/time_egg_builds.py: %dx%d, float frames; one process; %d passes over all cases, %d back-to-back launches per case and"
             % (W, H, args.passes, args.launches),
             "# pass after %d warm-up launches, each launch between its own events.  scene: standing = every launch at u_time %g,"
             % (args.warmup, U_TIME),
             "# animated = u_time %g + k / 600 at launch k.  median ms: over all launches of the case; pass lo / hi: the lowest and highest"
             % U_TIME,
             "# per-pass median (the run-to-run spread); ratio: median / this tree's egg with the same kernel form and scene.",
             "# %-10s %-13s %-8s %-9s %10s %10s %10s %10s %8s" % ("library", "app", "kernel", "scene", "median ms", "pass lo", "pass hi", "min ms", "ratio")]
    med = {}
    for i, (libname, app, kname, _, moving) in enumerate(names):
        allv = [x for p in sorted(per[i]) for x in per[i][p]]
        pm = [median(v) for v in per[i].values()]
        med[(libname, app, kname, moving)] = median(allv)
        base = med[("this tree", "egg", kname, moving)]
        lines.append("  %-10s %-13s %-8s %-9s %10.4f %10.4f %10.4f %10.4f %8.3f" % (libname, app, kname, "animated" if moving else "standing",
                                                                                    median(allv), min(pm), max(pm), min(allv), median(allv) / base))
    if not args.no_resources:
        lines += resources()
    print("\n".join(lines), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
