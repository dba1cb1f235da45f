"""sbx_planet_eval beside the frame kernels of APP_PLANET: one-launch times of "render" over the primary rays of the
shipped camera's 1280x720 SBX_APP_PLANET frame (u_time .37; computed on the host with tests/planet_eval_model.primary_rays and laid out
in k_planet's 8x8-pixel waves, so that a wave of the entry holds the 64 rays of a wave of k_planet) and over the same rays in a fixed
random permutation, in the default form and under sbx_set_variant 1; beside them the 1280x720 frame itself under variant 1 and
variant 0 (k_planet<false> / k_planet<true>: code this entry does not change).  Every leg runs in a process of its own (the parent never
opens the GPU); per leg the median and min - max of N launches after a warm-up, each between its own events.  For the entry's legs
the waves that ran with every guarded short form on and the waves that fell back (sbx_debug_planet_eval); the default form must not
fall back for these rays in either order.  Prints the table and the bar — the default entry over the ordered rays takes no longer
than the variant-1 frame kernel's median plus the larger of the two legs' min - max spreads — and writes them to --out if one is given.
profiles/planet_eval_timing.txt is such an output with a Reading and the kernels' resources written under it by hand.

    python tools/time_planet_eval.py [--launches 30] [--warmup 5] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, T = 1280, 720, .37
LEGS = [("entry", "ordered", 0), ("entry", "permuted", 0), ("entry", "ordered", 1), ("entry", "permuted", 1), ("frame", "-", 1), ("frame", "-", 0)]
NAMES = {("entry", 0): "sbx_planet_eval render default", ("entry", 1): "sbx_planet_eval render plain",
         ("frame", 0): "SBX_APP_PLANET frame default", ("frame", 1): "SBX_APP_PLANET frame variant 1"}


def wave_order(w, h, tw=8, th=8):
    """the index of every pixel of a w x h frame (row 0 = bottom, x fastest) in tw x th tile order, lane = tw * (y % th) + x % tw"""
    ty, tx, ly, lx = np.meshgrid(np.arange(h // th), np.arange(w // tw), np.arange(th), np.arange(tw), indexing="ij")
    return ((ty * th + ly) * w + tx * tw + lx).ravel()


def rays_of(order):
    from tests import planet_eval_model as M
    rays = M.primary_rays(W, H, *M.EYES["shipped"])[wave_order(W, H)]
    if order == "permuted":
        rays = rays[np.random.default_rng(20).permutation(len(rays))]
    return np.ascontiguousarray(rays)


def child(kind, order, variant, launches, warmup):
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    counts = (-1, -1)
    if kind == "entry":
        dev = torch.from_numpy(rays_of(order)).to(R.tdev)

        def launch():
            R.planet_eval("render", dev, T)
        counts = R.planet_eval_counted("render", dev, T)[1]
    else:
        buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)

        def launch():
            R.render("planet", W, H, T, out=buf)
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print("RESULT %.5f %.5f %.5f %d %d" % (ms[len(ms) // 2], ms[0], ms[-1], counts[0], counts[1]), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table and the bar to this file")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]), args.launches, args.warmup)
    assert args.launches >= 20, "at least 20 timed launches per leg"
    lines = ["# tools/time_planet_eval.py: \"render\", u_time %.2f; one process per leg; median and min - max of %d launches after %d warm-up"
             % (T, args.launches, args.warmup),
             "# launches, each between its own events.  ordered = the %d primary rays of the shipped camera's %dx%d SBX_APP_PLANET frame,"
             % (W * H, W, H),
             "# 64 to a wave as k_planet holds them (8x8 pixels); permuted = the same rays in a fixed random permutation.",
             "# fell back = waves that took the plain form for at least one part / all waves of the launch.",
             "# %-32s %-9s %10s %10s %10s %10s %22s" % ("leg", "rays", "median ms", "min ms", "max ms", "ns / ray", "fell back")]
    print("\n".join(lines), flush=True)
    res = {}
    for kind, order, form in LEGS:                                      # form = the sbx_set_variant value of the leg
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                            "--child", kind, order, str(form)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("leg %s %s %d failed (%d):\n%s" % (kind, order, form, r.returncode, r.stderr[-2000:]))
        med, mn, mx, fast, fell = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
        med, mn, mx, fast, fell = float(med), float(mn), float(mx), int(fast), int(fell)
        res[(kind, order, form)] = (med, mn, mx, fast, fell)
        share = "-" if fast < 0 else "%d / %d" % (fell, fast + fell)
        line = "  %-32s %-9s %10.4f %10.4f %10.4f %10.4f %22s" % (NAMES[(kind, form)], order, med, mn, mx, med * 1e6 / (W * H), share)
        lines.append(line)
        print(line, flush=True)
    e, f = res[("entry", "ordered", 0)], res[("frame", "-", 1)]
    margin = max(e[2] - e[1], f[2] - f[1])
    ok = e[0] <= f[0] + margin
    none = all(res[("entry", o, 0)][4] == 0 and res[("entry", o, 0)][3] > 0 for o in ("ordered", "permuted"))
    lines += ["#", "# Bar (measured in this run): sbx_planet_eval default over the ordered rays %.4f ms <= the variant-1 frame %.4f ms"
              % (e[0], f[0]),
              "# + %.4f ms (the larger of the two legs' min - max spreads): %s.  No wave of the default form fell back, in both orders: %s."
              % (margin, "MET" if ok else "MISSED", "yes" if none else "NO"),
              "# For the reader: the default entry takes %.2fx the time of k_planet's default frame (variant 0); the permutation costs the"
              % (e[0] / res[("frame", "-", 0)][0]),
              "# default form %.2fx and the plain form %.2fx." % (res[("entry", "permuted", 0)][0] / e[0],
                                                                 res[("entry", "permuted", 1)][0] / res[("entry", "ordered", 1)][0])]
    print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
