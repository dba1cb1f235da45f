"""SBX_APP_SDF_AO_SHADOW and SBX_APP_SDF_AO_NORMALS beside SBX_APP_SDF_AO: one-launch times at 3840x2160 of the
three builds, each with the default kernel and the plain one (sbx_set_variant 1).  ONE child process runs every case (the parent
never opens the GPU) under one time limit, and a failure is final: nothing is tried twice.  The cases are timed in PASSES — every
case once per pass, the passes one after the other — so that each case is measured at several moments of the run: the table
gives, per case, the median over all launches, and the lowest and highest PASS median, which is the run-to-run spread the ratios
are to be read against.  Every launch is bracketed by its own pair of events.

--baseline-lib PATH times SBX_APP_SDF_AO of another build of libsbx.so (the parent commit's) in the same process, alternating
with this tree's in every pass: if the two differ by more than the spread, this tree's template parameter has leaked into the
existing kernel.

    python tools/time_sdf_ao_builds.py [--launches 20] [--passes 5] [--warmup 5] [--baseline-lib libsbx_parent.so]
Writes profiles/sdf_ao_builds_timing.txt (or --out).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, U_TIME = 3840, 2160, 0.37
CASES = [("sdf_ao", "default", 0), ("sdf_ao", "plain", 1), ("sdf_ao_normals", "default", 0), ("sdf_ao_normals", "plain", 1),
         ("sdf_ao_shadow", "default", 0), ("sdf_ao_shadow", "plain", 1)]


def child(launches, passes, warmup, baseline):
    import torch
    import shaderbox_amd
    here = shaderbox_amd.Renderer(0)
    cases = [(here, "this tree") + c for c in CASES]
    if baseline:
        shaderbox_amd.LIB_PATH = os.path.abspath(baseline)
        cases.insert(1, (shaderbox_amd.Renderer(0), "baseline", "sdf_ao", "default", 0))
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=here.tdev)
    for R, _, app, _, variant in cases:
        R.set_variant(variant)
        for _ in range(warmup):
            R.render(app, W, H, U_TIME, out=buf)
    torch.cuda.synchronize()
    for p in range(passes):
        for i, (R, _, app, _, variant) in enumerate(cases):
            R.set_variant(variant)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_ao_builds_timing.txt"))
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
        names.insert(1, ("baseline", "sdf_ao", "default", 0))
    per = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            f = ln.split()
            per.setdefault(int(f[1]), {})[int(f[2])] = [float(x) for x in f[3:]]
    lines = ["# tools/time_sdf_ao_builds.py: %dx%d, u_time %g, float frames, default aux; one process; %d passes over all cases, %d back-to-back"
             % (W, H, U_TIME, args.passes, args.launches),
             "# launches per case and pass after %d warm-up launches, each launch between its own events.  median ms: over all launches of"
             % args.warmup,
             "# the case; pass lo / hi: the lowest and highest per-pass median (the run-to-run spread); ratio: median / this tree's sdf_ao",
             "# with the same kernel form.",
             "# %-10s %-15s %-8s %10s %10s %10s %10s %8s" % ("library", "app", "kernel", "median ms", "pass lo", "pass hi", "min ms", "ratio")]
    med = {}
    for i, (libname, app, kname, _) in enumerate(names):
        allv = [x for p in sorted(per[i]) for x in per[i][p]]
        pm = [median(v) for v in per[i].values()]
        med[(libname, app, kname)] = median(allv)
        base = med[("this tree", "sdf_ao", kname)]
        lines.append("  %-10s %-15s %-8s %10.4f %10.4f %10.4f %10.4f %8.3f" % (libname, app, kname, median(allv), min(pm), max(pm), min(allv),
                                                                              median(allv) / base))
    print("\n".join(lines), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
