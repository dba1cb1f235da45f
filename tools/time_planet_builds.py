"""SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS and SBX_APP_PLANET_UNLIT beside SBX_APP_PLANET and SBX_APP_PLANET_ATMOSPHERE (DESIGN.md
§5.16): one-launch times at 7680x4320, u_time 0.37, each app with the default kernel and the plain one (sbx_set_variant 1: no exact
skips, the IEEE forms).  ONE PROCESS PER APP and pass: the parent never opens the GPU, every child runs under its own time limit, one at a time, and
a failure is final — nothing is tried twice and nothing more is started.  The apps are timed in PASSES, every app once per pass, so
that each is measured at several moments of the run by several processes: the table gives, per case, the median over all launches
and the lowest and highest PASS median, which is the run-to-run spread the ratios are to be read against.  Every launch is bracketed
by its own pair of events, after warm-up launches of the same shape.

--baseline-lib PATH times SBX_APP_PLANET and SBX_APP_PLANET_ATMOSPHERE of another build of libsbx.so (the parent commit's) by the same
processes in the same passes, right after this tree's: if the two differ by more than the baseline's own spread, this tree's template
parameter has leaked into the shipped kernels.

    python tools/time_planet_builds.py [--launches 20] [--passes 3] [--warmup 5] [--baseline-lib libsbx_parent.so]
Writes profiles/planet_builds_timing.txt (or --out).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, U_TIME = 7680, 4320, 0.37
APPS = ("planet", "planet_atmosphere", "planet_closeup", "planet_cloudless", "planet_unlit")
SHIPPED = ("planet", "planet_atmosphere")
KERNELS = (("default", 0), ("plain", 1))


def child(app, launches, warmup, lib):
    import torch
    import shaderbox_amd
    if lib:
        shaderbox_amd.LIB_PATH = os.path.abspath(lib)
    R = shaderbox_amd.Renderer(0)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    for kname, variant in KERNELS:
        R.set_variant(variant)
        for k in range(warmup):
            R.render(app, W, H, U_TIME, out=buf)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            a.record()
            R.render(app, W, H, U_TIME, out=buf)
            b.record()
        torch.cuda.synchronize()
        print("RESULT %s %s" % (kname, " ".join("%.5f" % a.elapsed_time(b) for a, b in ev)), flush=True)
    R.close()


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planet_builds_timing.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.warmup, args.lib)
    # (library, app) in the order of a pass: a shipped app of this tree, then the same of the baseline
    procs = [c for a in APPS for c in ([("this tree", a), ("baseline", a)] if args.baseline_lib and a in SHIPPED else [("this tree", a)])]
    per = {}                                        # (library, app, kernel) -> [launch times of pass 0, of pass 1, ...]
    for p in range(args.passes):
        for libname, app in procs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", app, "--launches", str(args.launches), "--warmup", str(args.warmup)]
            if libname == "baseline":
                cmd += ["--lib", args.baseline_lib]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:
                raise SystemExit("the timing process of %s (%s, pass %d) failed (%d); nothing more is started:\n%s\n%s"
                                 % (app, libname, p, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT "):
                    f = ln.split()
                    per.setdefault((libname, app, f[1]), []).append([float(x) for x in f[2:]])
            print("pass %d %-9s %-17s %s" % (p, libname, app, "  ".join("%s %.4f" % (k, median(per[(libname, app, k)][-1])) for k, _ in KERNELS)),
                  flush=True)
    lines = ["# tools/time_planet_builds.py: %dx%d, float frames, u_time %g; one process per app and pass, %d passes, the processes one after"
             % (W, H, U_TIME, args.passes),
             "# the other; per process and kernel form %d launches after %d warm-up launches, each launch between its own events.  kernel:"
             % (args.launches, args.warmup),
             "# default = sbx_set_variant 0, plain = sbx_set_variant 1.  median ms: over all launches of the case; pass lo / hi: the lowest and",
             "# highest per-pass (per-process) median, the run-to-run spread; ratio: median / this tree's planet with the same kernel form.",
             "# %-10s %-17s %-8s %10s %10s %10s %10s %8s" % ("library", "app", "kernel", "median ms", "pass lo", "pass hi", "min ms", "ratio")]
    for kname, _ in KERNELS:
        base = median([x for v in per[("this tree", "planet", kname)] for x in v])
        for libname, app in procs:
            runs = per[(libname, app, kname)]
            allv = [x for v in runs for x in v]
            pm = [median(v) for v in runs]
            lines.append("  %-10s %-17s %-8s %10.4f %10.4f %10.4f %10.4f %8.3f" % (libname, app, kname, median(allv), min(pm), max(pm), min(allv),
                                                                                  median(allv) / base))
    print("\n".join(lines), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
