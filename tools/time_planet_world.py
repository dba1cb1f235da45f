"""SBX_APP_PLANET_WORLD beside SBX_APP_PLANET at 7680x4320, u_time .37.  Every case runs in a process of its own
(the parent never opens the GPU); per case the median and minimum of N launches after a warm-up, each between its own events.  The
cases are run in --passes interleaved passes (case 1 .. case n, then again), so that a drift of the machine lands on all of them; the
table shows every pass and the median of the passes' medians.  The cases:

  parent     with --root DIR (another checkout, built: the parent commit): its SBX_APP_PLANET under sbx_set_variant 0 and 1
  planet     this tree's SBX_APP_PLANET under variants 0 and 1
  orbit      the fixture world `orbit` (tests/planet_world_model.py): the literal tier, another camera, so PLANET_CLOSEUP's code
  fov-ulp    the default world of u_time .37 with fov one ulp larger: the literal tier again, the shipped frame's work through PLANET_CLOSEUP's
             code (the IEEE root for every length)
  one-bit    the default world of u_time .37 with one bit of c_snow changed: the run-time kernel over the shipped frame's work (variant 0)
             and the world kernel's plain form (variant 1)

Printed under the table: this tree's SBX_APP_PLANET against the interval of the parent's passes widened on both sides by their own
max / min ratio; the run-time tier against the parent's
variant 1 (the bar: below it) and its ratio to the parent's variant 0 (recorded, not bounded).  profiles/planet_world_timing.txt is such
an output with bench.py's figures written under it by hand.

    python tools/time_planet_world.py [--launches 10] [--warmup 3] [--passes 3] [--root DIR] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = .37
W, H = 7680, 4320


def child(root, what, variant, launches, warmup):
    sys.path.insert(0, root)
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    app, aux, note = "planet", None, "-"
    if what != "planet":
        sys.path.insert(1, ROOT)
        import numpy as np
        from tests import planet_world_model as M
        Wd = (M.WORLDS["orbit"] if what == "orbit" else M.world(T, fov=np.nextafter(M.default_world(T)["fov"], np.float32(1))) if what == "fov-ulp"
              else M.world(T, c_snow=(np.nextafter(np.float32(.6), np.float32(1)), .6, .6)))
        app, aux = "planet_world", M.as_aux(Wd)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)

    def launch():
        R.render(app, W, H, T, out=buf, aux=aux)
    if aux is not None:
        before = R.planet_world_launches()
        launch()
        after = R.planet_world_launches()
        note = ("literal", "run-time", "plain")[[y - x for x, y in zip(before, after)].index(1)]
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
    print("RESULT %.5f %.5f %s" % (ms[len(ms) // 2], ms[0], note), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--root", default=None, help="another checkout (built): the parent commit, whose SBX_APP_PLANET is measured beside this one's")
    ap.add_argument("--out", default=None, help="also write the table and the findings to this file")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]), args.launches, args.warmup)
    cases = []
    if args.root:
        cases += [("parent", os.path.abspath(args.root), "planet", 0), ("parent", os.path.abspath(args.root), "planet", 1)]
    cases += [("planet", ROOT, "planet", 0), ("planet", ROOT, "planet", 1), ("orbit", ROOT, "orbit", 0), ("fov-ulp", ROOT, "fov-ulp", 0),
              ("one-bit", ROOT, "one-bit", 0), ("one-bit", ROOT, "one-bit", 1)]
    lines = ["# tools/time_planet_world.py: %dx%d, u_time .37; one process per case and pass, %d interleaved passes; per pass the median (and" % (W, H, args.passes),
             "# minimum) of %d launches after %d warm-up launches, each between its own events.  v = sbx_set_variant." % (args.launches, args.warmup),
             "# %-8s %1s %-9s %s %12s" % ("case", "v", "tier", " ".join("%18s" % ("pass %d med (min)" % (p + 1)) for p in range(args.passes)), "median ms")]
    print("\n".join(lines), flush=True)
    got = {(c[0], c[3]): [] for c in cases}
    notes = {}
    for _ in range(args.passes):
        for section, root, what, variant in cases:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                                "--child", root, what, str(variant)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("case %s %d failed (%d):\n%s" % (section, variant, r.returncode, r.stderr[-2000:]))
            m, mn, note = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
            got[(section, variant)].append((float(m), float(mn)))
            notes[(section, variant)] = note
            print("  ... %s v%d: %s ms" % (section, variant, m), flush=True)
    med = {}
    for section, root, what, variant in cases:
        runs = got[(section, variant)]
        med[(section, variant)] = statistics.median(m for m, _ in runs)
        lines.append("  %-8s %d %-9s %s %12.4f" % (section, variant, notes[(section, variant)], " ".join("%9.4f (%6.4f)" % r for r in runs), med[(section, variant)]))
    tail = ["#"]
    rt, pl = med[("one-bit", 0)], med[("one-bit", 1)]
    if args.root:
        for v in (0, 1):
            runs = [m for m, _ in got[("parent", v)]]
            spread = max(runs) / min(runs)
            new = med[("planet", v)]
            inside = min(runs) / spread <= new <= max(runs) * spread
            tail.append("# 1. SBX_APP_PLANET, variant %d: the parent's passes %s ms (max / min %.4f); this tree %.4f ms = %.4f of the parent's median: %s."
                        % (v, " / ".join("%.4f" % m for m in runs), spread, new, new / med[("parent", v)], "WITHIN the parent's passes widened by their own max / min ratio" if inside else "OUTSIDE them"))
        p0, p1 = med[("parent", 0)], med[("parent", 1)]
    else:
        tail.append("# 1. no --root: this tree's own SBX_APP_PLANET stands in for the parent's below.")
        p0, p1 = med[("planet", 0)], med[("planet", 1)]
    tail.append("# 2. run-time tier (one-bit, variant 0) %.4f ms against SBX_APP_PLANET's variant 1 %.4f ms: %s (the bar: faster); %.4f of variant 0's %.4f ms."
                % (rt, p1, "FASTER" if rt < p1 else "NOT FASTER", rt / p0, p0))
    tail.append("# 3. the world kernel's plain form (one-bit, variant 1) %.4f ms = %.4f of SBX_APP_PLANET's variant 1." % (pl, pl / p1))
    tail.append("# 4. literal tier, another camera (orbit) %.4f ms: another frame, another amount of work; no bar." % med[("orbit", 0)])
    tail.append("# 5. literal tier, the shipped frame through PLANET_CLOSEUP's code (fov-ulp: the IEEE root, every other short form) %.4f ms = %.4f of "
                "SBX_APP_PLANET's variant 0: what the short roots alone are worth; the run-time tier is %.4f of it."
                % (med[("fov-ulp", 0)], med[("fov-ulp", 0)] / p0, rt / med[("fov-ulp", 0)]))
    print("\n".join(lines[3:] + tail), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
