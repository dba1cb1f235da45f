"""APP_ATMOSPHERE_GROUND beside APP_ATMOSPHERE: one-launch times of the default kernel, the plain one
(sbx_set_variant 1) and the tolerance tier (SBX_PRECISION_1E4) at 3840x2160 and 7680x4320, and k_atmosphere (exact and tier) at the
same sizes, with ms per SKY pixel: this app's rows at and above the horizon x width, the dome's pixels with z2 <= 2.  Every case
runs in a process of its own (the parent never opens the GPU); per case the median of N back-to-back launches after a warm-up,
each bracketed by its own pair of events.  Writes profiles/atmosphere_ground_timing.txt (or --out).

    python tools/time_atmosphere_ground.py [--launches 30] [--warmup 5]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("atmosphere_ground", "default", 0, "exact"), ("atmosphere_ground", "plain", 1, "exact"), ("atmosphere_ground", "tier", 0, "1e-4"),
         ("atmosphere", "default", 0, "exact"), ("atmosphere", "tier", 0, "1e-4")]
SIZES = [(3840, 2160), (7680, 4320)]
F = np.float32


def sky_pixels(app, w, h):
    """pixels that march: binary32 restatement of the kernels' own tests at pixel centres"""
    ax = F(w) / F(h)
    px = (F(2) * ((np.arange(w, dtype=F) + F(.5)) / F(w)) - F(1)) * ax
    py = F(2) * ((np.arange(h, dtype=F) + F(.5)) / F(h)) - F(1)
    if app == "atmosphere":
        z2 = px[None, :] * px[None, :] + py[:, None] * py[:, None]
        return int((z2 <= F(2)).sum())
    # the ground camera: fwd = normalize(0, .5, -1), up = cross(fwd, cross((0,1,0), fwd)); no roll, so the row decides;
    # sky <=> -dir.y < 1e-6; the sign of dir.y is that of fwd.y + up.y * py (the band 0 < denom < 1e-6 is narrower than a row)
    fy, fz = F(.5) / np.sqrt(F(1.25)), F(-1) / np.sqrt(F(1.25))
    up_y = fz * fz
    return int(((fy + up_y * py) > 0).sum()) * w


def child(app, variant, tier, launches, warmup):
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    R.set_precision(tier)
    for w, h in SIZES:
        buf = torch.empty((h, w, 4), dtype=torch.float32, device=R.tdev)
        for _ in range(warmup):
            R.render(app, w, h, 0.37, out=buf)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, b in ev:
            a.record()
            R.render(app, w, h, 0.37, out=buf)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        print("RESULT %d %d %.5f %.5f" % (w, h, ms[len(ms) // 2], ms[0]), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atmosphere_ground_timing.txt"))
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.child[2], args.launches, args.warmup)
    lines = ["# tools/time_atmosphere_ground.py: u_time .37, float frames; one process per case; median (and minimum) of %d back-to-back"
             % args.launches,
             "# launches after %d warm-up launches, each between its own events.  sky px = pixels that march (module docstring)." % args.warmup,
             "# %-18s %-8s %-10s %10s %10s %12s %14s" % ("app", "kernel", "size", "median ms", "min ms", "sky px", "ns / sky px")]
    print("\n".join(lines), flush=True)
    for app, name, variant, tier in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                            "--child", app, str(variant), tier], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("case %s %s failed (%d):\n%s" % (app, name, r.returncode, r.stderr[-2000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                w, h, med, mn = ln.split()[1:]
                w, h, med, mn = int(w), int(h), float(med), float(mn)
                sky = sky_pixels(app, w, h)
                line = "  %-18s %-8s %-10s %10.4f %10.4f %12d %14.4f" % (app, name, "%dx%d" % (w, h), med, mn, sky, med * 1e6 / sky)
                lines.append(line)
                print(line, flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
