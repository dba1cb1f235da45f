"""The builds of a family beside the app(s) they are builds of (tests/build_families.py `timing`): one-launch
times of every app of the family at the family's frame size and u_time, each with every kernel form (sbx_set_variant).  ONE PROCESS
PER APP and pass: the parent never opens the GPU, every child runs under its own time limit, one at a time, and a failure is final —
nothing is tried twice and nothing more is started.  The apps are timed in PASSES, every app once per pass, so that each is measured
at several moments of the run by several processes: the table gives, per case, the median over all launches and the lowest and
highest PASS median, which is the run-to-run spread the ratios are to be read against.  Every launch is bracketed by its own pair of
events, after warm-up launches of the same shape.  A family with a `dt` (egg) is timed on two scenes: standing, every launch at the
same u_time, and animated, u_time advancing by dt per launch.

--baseline-lib PATH times the shipped apps of another build of libsbx.so (the parent commit's) by the same processes in the same
passes, right after this tree's: if the two differ by more than the baseline's own spread, this tree's template parameter has leaked
into the shipped kernels.

    python tools/time_builds.py FAMILY [--launches N] [--passes N] [--warmup 5] [--baseline-lib libsbx_parent.so]
Writes profiles/<family>_builds_timing.txt (or --out).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.build_families import FAMILIES  # noqa: E402

TIMED = {f: fam["timing"] for f, fam in FAMILIES.items() if "timing" in fam}


def cases(T):
    """(label, sbx_set_variant value, u_time step per launch) of every case a child times"""
    scenes = (("standing", 0.0), ("animated", T["dt"])) if "dt" in T else (("", 0.0),)
    return [((kname + " " + scene).strip(), variant, dt) for scene, dt in scenes for kname, variant in T["kernels"]]


def child(T, app, launches, warmup, lib):
    import torch
    import shaderbox_amd
    if lib:
        shaderbox_amd.LIB_PATH = os.path.abspath(lib)
    (W, H), t0 = T["size"], T["time"]
    R = shaderbox_amd.Renderer(0)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    for label, variant, dt in cases(T):
        R.set_variant(variant)
        for k in range(warmup):
            R.render(app, W, H, t0 + k * dt, out=buf)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for k, (a, b) in enumerate(ev):
            a.record()
            R.render(app, W, H, t0 + k * dt, out=buf)
            b.record()
        torch.cuda.synchronize()
        print("RESULT %s %s" % (label.replace(" ", "/"), " ".join("%.5f" % a.elapsed_time(b) for a, b in ev)), flush=True)
    R.close()


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("family", choices=sorted(TIMED))
    ap.add_argument("--launches", type=int, default=None)
    ap.add_argument("--passes", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    T = TIMED[args.family]
    launches, passes = args.launches or T["launches"], args.passes or T["passes"]
    out = args.out or os.path.join(ROOT, "profiles", "%s_builds_timing.txt" % args.family)
    if args.child:
        return child(T, args.child, launches, args.warmup, args.lib)
    labels = [label for label, _, _ in cases(T)]
    # (library, app) in the order of a pass: a shipped app of this tree, then the same of the baseline
    procs = [c for a in T["apps"] for c in ([("this tree", a), ("baseline", a)] if args.baseline_lib and a in T["shipped"] else [("this tree", a)])]
    per = {}                                        # (library, app, case) -> [launch times of pass 0, of pass 1, ...]
    for p in range(passes):
        for libname, app in procs:
            cmd = [sys.executable, os.path.abspath(__file__), args.family, "--child", app, "--launches", str(launches), "--warmup", str(args.warmup)]
            if libname == "baseline":
                cmd += ["--lib", args.baseline_lib]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:
                raise SystemExit("the timing process of %s (%s, pass %d) failed (%d); nothing more is started:\n%s\n%s"
                                 % (app, libname, p, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT "):
                    f = ln.split()
                    per.setdefault((libname, app, f[1].replace("/", " ")), []).append([float(x) for x in f[2:]])
            print("pass %d %-9s %-17s %s" % (p, libname, app, "  ".join("%s %.4f" % (k, median(per[(libname, app, k)][-1])) for k in labels)), flush=True)
    aw, kw = max(len(a) for a in T["apps"]), max(8, max(map(len, labels)))
    lines = ["# tools/time_builds.py %s: %dx%d, float frames, u_time %g%s; one process per app and pass, %d passes, the processes one after"
             % ((args.family,) + T["size"] + (T["time"], " (animated: + k * %g at launch k)" % T["dt"] if "dt" in T else "", passes)),
             "# the other; per process and kernel form %d launches after %d warm-up launches, each launch between its own events.  kernel:"
             % (launches, args.warmup),
             "# %s.  median ms: over all launches of the case; pass lo / hi: the lowest and" % ", ".join("%s = sbx_set_variant %d" % kv for kv in T["kernels"]),
             "# highest per-pass (per-process) median, the run-to-run spread; ratio: median / this tree's %s with the same kernel form%s."
             % (T["shipped"][0], " and scene" if "dt" in T else ""),
             "# %-10s %-*s %-*s %10s %10s %10s %10s %8s" % ("library", aw, "app", kw, "kernel", "median ms", "pass lo", "pass hi", "min ms", "ratio")]
    for label in labels:
        base = median([x for v in per[("this tree", T["shipped"][0], label)] for x in v])
        for libname, app in procs:
            runs = per[(libname, app, label)]
            allv = [x for v in runs for x in v]
            pm = [median(v) for v in runs]
            lines.append("  %-10s %-*s %-*s %10.4f %10.4f %10.4f %10.4f %8.3f" % (libname, aw, app, kw, label, median(allv), min(pm), max(pm), min(allv),
                                                                                median(allv) / base))
    print("\n".join(lines), flush=True)
    if out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
