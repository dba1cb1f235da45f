"""SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval beside the shipped atmosphere kernels.  Every case runs in a
process of its own (the parent never opens the GPU); per case the median and minimum of N launches after a warm-up, each between its
own events.  The sections:

  shipped   SBX_APP_ATMOSPHERE 7680x4320 and SBX_APP_ATMOSPHERE_GROUND 3840x2160, u_time .37.  With --root DIR the same two cases run
            against another checkout's package and library as well (the parent commit, built: twice, for its own run-to-run factor).
  literal   the air app with no block at 7680x4320 beside SBX_APP_ATMOSPHERE: the same kernel.
  run-time  the default block of u_time .37 with sun_power 19 alone changed, 7680x4320: the run-time kernel (variant 0) and the air
            kernel's plain form (variant 1).  Bar: the run-time kernel at or below the midpoint of SBX_APP_ATMOSPHERE and the plain form.
  eval      sbx_atmosphere_air_eval "get_incident_light" under that block over the "sky" and "envmap" ray families of
            tools/time_atmosphere_eval.py, default and plain, beside sbx_atmosphere_eval's default.  The same bar per family.
  fixtures  the four blocks of tests/atmosphere_air_model.py at 3840x2160 with the tier each took.  No bar.

Prints the table and the bars, and writes them to --out if one is given.  profiles/atmosphere_air_timing.txt is such an output with
the kernels' resources and bench.py's figures written under it by hand.

    python tools/time_atmosphere_air.py [--launches 30] [--warmup 5] [--root DIR] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = .37
BIG, MID = (7680, 4320), (3840, 2160)


def child(root, kind, what, variant, launches, warmup):
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    note = "-"
    if kind == "app":                                                  # what = app:block:WxH
        app, blk, res = what.split(":")
        w, h = map(int, res.split("x"))
        aux = None
        if blk != "none":
            from tests import atmosphere_air_model as M
            A = M.air(T, sun_power=19.) if blk == "brighter" else M.AIRS[blk]
            aux, note = M.as_aux(A), M.tier_of(A, variant)
        buf = torch.empty((h, w, 4), dtype=torch.float32, device=R.tdev)
        n = w * h

        def launch():
            R.render(app, w, h, T, out=buf, aux=aux)
        if app == "atmosphere_air":
            before = R.atmosphere_air_launches()
            launch()
            after = R.atmosphere_air_launches()
            note = "literal" if after[1] > before[1] else "plain" if after[2] > before[2] else "run-time"
    else:                                                              # what = entry:family
        import time_atmosphere_eval as TE
        from tests import atmosphere_air_model as M
        from tests import atmosphere_ground_model as GM
        entry, family = what.split(":")
        rays, n = TE.sky_rays() if family == "sky" else TE.envmap_rays()
        dev = torch.from_numpy(rays).to(R.tdev)
        if entry == "air":
            a = M.as_aux(M.air(T, sun_power=19.))
            note = "%d / %d fast waves" % (R.atmosphere_air_eval_counted("get_incident_light", dev, a)[1], (len(rays) + 63) // 64)

            def launch():
                R.atmosphere_air_eval("get_incident_light", dev, a)
        else:
            sun = tuple(float(v) for v in GM.sun_dir(T))
            note = "%d / %d fast waves" % (R.atmosphere_eval_counted("get_incident_light", dev, sun)[1], (len(rays) + 63) // 64)

            def launch():
                R.atmosphere_eval("get_incident_light", dev, sun)
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a_, b_ in ev:
        a_.record()
        launch()
        b_.record()
    torch.cuda.synchronize()
    ms = sorted(a_.elapsed_time(b_) for a_, b_ in ev)
    print("RESULT %.5f %.5f %d %s" % (ms[len(ms) // 2], ms[0], n, note.replace(" ", "_")), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=None, help="another checkout (built) whose shipped apps are measured twice beside this one's")
    ap.add_argument("--out", default=None, help="also write the table and the bars to this file")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2], int(args.child[3]), args.launches, args.warmup)
    res = lambda s: "%dx%d" % s  # noqa: E731
    sky, ground = "atmosphere:none:" + res(BIG), "atmosphere_ground:none:" + res(MID)
    cases = []
    if args.root:
        for run in (1, 2):
            cases += [("parent %d" % run, os.path.abspath(args.root), "app", sky, 0), ("parent %d" % run, os.path.abspath(args.root), "app", ground, 0)]
    cases += [("shipped", ROOT, "app", sky, 0), ("shipped", ROOT, "app", ground, 0),
              ("literal", ROOT, "app", "atmosphere_air:none:" + res(BIG), 0),
              ("run-time", ROOT, "app", "atmosphere_air:brighter:" + res(BIG), 0), ("run-time", ROOT, "app", "atmosphere_air:brighter:" + res(BIG), 1)]
    for family in ("sky", "envmap"):
        cases += [("eval", ROOT, "eval", "shipped:" + family, 0), ("eval", ROOT, "eval", "air:" + family, 0), ("eval", ROOT, "eval", "air:" + family, 1)]
    cases += [("fixtures", ROOT, "app", "atmosphere_air:%s:%s" % (name, res(MID)), 0) for name in ("sunset", "thin", "aloft", "coarse")]
    lines = ["# tools/time_atmosphere_air.py: u_time .37; one process per case; median (and minimum) of %d launches after %d warm-up launches,"
             % (args.launches, args.warmup),
             "# each between its own events.  `brighter` = the default block of u_time .37 with sun_power 19; v = sbx_set_variant.",
             "# %-9s %-42s %1s %10s %10s %10s %10s  %s" % ("section", "case", "v", "median ms", "min ms", "elements", "ns / el.", "tier / fast waves")]
    print("\n".join(lines), flush=True)
    med = {}
    for section, root, kind, what, variant in cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                            "--child", root, kind, what, str(variant)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("case %s %s %d failed (%d):\n%s" % (section, what, variant, r.returncode, r.stderr[-2000:]))
        m, mn, n, note = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
        med[(section, what, variant)] = float(m)
        line = "  %-9s %-42s %d %10.4f %10.4f %10d %10.4f  %s" % (section, what, variant, float(m), float(mn), int(n), float(m) * 1e6 / int(n),
                                                               note.replace("_", " "))
        lines.append(line)
        print(line, flush=True)
    tail = ["#"]
    if args.root:
        for what in (sky, ground):
            p1, p2, new = med[("parent 1", what, 0)], med[("parent 2", what, 0)], med[("shipped", what, 0)]
            factor = max(p1, p2) / min(p1, p2)
            ratio = new / min(p1, p2)
            tail.append("# 1. %s: parent %.4f / %.4f ms (run-to-run factor %.4f), new %.4f ms = %.4f of the parent's faster run: %s."
                        % (what, p1, p2, factor, new, ratio, "WITHIN" if ratio <= factor else "OUTSIDE"))
        factor = max(max(med[("parent 1", w, 0)], med[("parent 2", w, 0)]) / min(med[("parent 1", w, 0)], med[("parent 2", w, 0)]) for w in (sky, ground))
        lit = med[("literal", "atmosphere_air:none:" + res(BIG), 0)] / med[("shipped", sky, 0)]
        tail.append("# 2. literal tier: atmosphere_air with no block / atmosphere = %.4f against the factor %.4f: %s." % (lit, factor, "WITHIN" if lit <= factor else "OUTSIDE"))
    else:
        tail.append("# 2. literal tier: atmosphere_air with no block / atmosphere = %.4f (no --root: no factor to hold it to)."
                    % (med[("literal", "atmosphere_air:none:" + res(BIG), 0)] / med[("shipped", sky, 0)]))
    a, p, got = med[("shipped", sky, 0)], med[("run-time", "atmosphere_air:brighter:" + res(BIG), 1)], med[("run-time", "atmosphere_air:brighter:" + res(BIG), 0)]
    tail.append("# 3. run-time tier, frame: midpoint of atmosphere and the air kernel's plain form = (%.4f + %.4f) / 2 = %.4f ms; the run-time kernel %.4f ms: %s."
                % (a, p, (a + p) / 2, got, "MET" if got <= (a + p) / 2 else "MISSED"))
    for family in ("sky", "envmap"):
        a, p, got = med[("eval", "shipped:" + family, 0)], med[("eval", "air:" + family, 1)], med[("eval", "air:" + family, 0)]
        tail.append("# 3. run-time tier, %s rays: midpoint of sbx_atmosphere_eval and the air entry's plain form = (%.4f + %.4f) / 2 = %.4f ms; the air entry %.4f ms: %s."
                    % (family, a, p, (a + p) / 2, got, "MET" if got <= (a + p) / 2 else "MISSED"))
    print("\n".join(tail), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
