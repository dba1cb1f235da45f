"""sbx_atmosphere_eval beside the frame kernel it shares its solver with: one-launch times of the entry (default
and sbx_set_variant 1, the plain kernel) and of the atmosphere_ground frame (default and sbx_set_variant 1) over the SAME rays:
the ground camera's sky rays at 3840x2160, u_time .37, computed on the host with tests/model_common.get_primary_ray and laid out in
the frame kernel's 8x8-tile order, so that a wave of the entry holds the 64 rays of a wave of the frame (the tile row the horizon
cuts holds sky rays only, packed).  A second family, which no camera of the library has: an equirectangular environment map of
2048x1024 directions from (0, earth_radius + 1, 0) in 8x8 tiles, half of which look below the horizon.  Every case runs in a
process of its own (the parent never opens the GPU); per case the median and minimum of N launches after a warm-up, each between
its own events.  Prints the table and the measured bar (the default entry's ns per ray at or below the midpoint of the frame
kernel's default and plain ns per sky pixel), and writes them to --out if one is given.  profiles/atmosphere_eval_timing.txt is
such an output with a Reading and the kernels' resources written under it by hand, so the tool does not write there by itself.

    python tools/time_atmosphere_eval.py [--launches 30] [--warmup 5] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, T = 3840, 2160, .37
ENV_W, ENV_H = 2048, 1024
F = np.float32
CASES = [("entry", "sky", 0), ("entry", "sky", 1), ("frame", "sky", 0), ("frame", "sky", 1), ("entry", "envmap", 0), ("entry", "envmap", 1)]
NAMES = {("entry", 0): "sbx_atmosphere_eval default", ("entry", 1): "sbx_atmosphere_eval plain",
         ("frame", 0): "atmosphere_ground default", ("frame", 1): "atmosphere_ground plain"}


def tile_order(w, h):
    """(x, y) of every pixel of a w x h grid (both multiples of 8) in 8x8-tile order: tiles row by row, lane = 8 * (y % 8) + x % 8"""
    ty, tx, ly, lx = np.meshgrid(np.arange(h // 8), np.arange(w // 8), np.arange(8), np.arange(8), indexing="ij")
    return (tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()


def sky_rays():
    from tests import atmosphere_ground_model as GM
    x, y = tile_order(W, H)
    hz = GM.horizon_row(W, H)
    keep = y >= hz
    x, y = x[keep], y[keep]
    pcx, pcy = GM.point_cam(W, H, x.astype(F) + F(.5), y.astype(F) + F(.5))
    rd = GM.get_primary_ray(pcx, pcy, GM.EYE, GM.LOOK_AT)
    assert (GM.intersect_plane_t(rd) > GM.MAX_DIST).all()
    return np.concatenate([np.tile(np.array(GM.EYE, dtype=F), (len(x), 1)), np.stack(rd, axis=-1)], axis=1), (H - hz) * W


def envmap_rays():
    x, y = tile_order(ENV_W, ENV_H)
    phi = (x + .5) / ENV_W * 2 * np.pi
    theta = (y + .5) / ENV_H * np.pi                                    # 0 = straight up
    d = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    o = np.tile([0.0, 6360e3 + 1.0, 0.0], (len(x), 1))
    return np.concatenate([o, d], axis=1).astype(F), len(x)


def child(kind, family, variant, launches, warmup):
    import torch
    import shaderbox_amd
    from tests import atmosphere_ground_model as GM
    sun = tuple(float(v) for v in GM.sun_dir(T))
    rays, marching = sky_rays() if family == "sky" else envmap_rays()
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    waves = -1
    if kind == "entry":
        dev = torch.from_numpy(rays).to(R.tdev)

        def launch():
            R.atmosphere_eval("get_incident_light", dev, sun)
        waves = R.atmosphere_eval_counted("get_incident_light", dev, sun)[1]
    else:
        assert marching == len(rays)
        buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)

        def launch():
            R.render("atmosphere_ground", W, H, T, out=buf)
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
    print("RESULT %.5f %.5f %d %d %d" % (ms[len(ms) // 2], ms[0], marching, waves, (len(rays) + 63) // 64), flush=True)
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
    lines = ["# tools/time_atmosphere_eval.py: get_incident_light, sun = the oracle's atmosphere.sun_dir(u_time .37); one process per case; median",
             "# (and minimum) of %d launches after %d warm-up launches, each between its own events.  sky = the ground camera's sky rays at"
             % (args.launches, args.warmup),
             "# %dx%d in the frame kernel's 8x8-tile order; envmap = %dx%d equirectangular directions from (0, earth_radius + 1, 0), half of them"
             % (W, H, ENV_W, ENV_H),
             "# below the horizon.  rays = rays that march; fast waves = 64-lane waves that ran the fast forms / all waves of the launch.",
             "# %-34s %-7s %10s %10s %10s %10s %19s" % ("case", "family", "median ms", "min ms", "rays", "ns / ray", "fast waves")]
    print("\n".join(lines), flush=True)
    ns = {}
    for kind, family, form in CASES:                                   # form = the sbx_set_variant value of the case
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                            "--child", kind, family, str(form)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("case %s %s %d failed (%d):\n%s" % (kind, family, form, r.returncode, r.stderr[-2000:]))
        med, mn, n, waves, all_waves = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
        med, mn, n, waves, all_waves = float(med), float(mn), int(n), int(waves), int(all_waves)
        ns[(kind, family, form)] = med * 1e6 / n
        fast = "-" if waves < 0 else "%d / %d" % (waves, all_waves)
        line = "  %-34s %-7s %10.4f %10.4f %10d %10.4f %19s" % (NAMES[(kind, form)], family, med, mn, n, med * 1e6 / n, fast)
        lines.append(line)
        print(line, flush=True)
    mid = (ns[("frame", "sky", 0)] + ns[("frame", "sky", 1)]) / 2
    got = ns[("entry", "sky", 0)]
    lines += ["#", "# Bar (measured in this run): midpoint of the frame kernel's default and plain = (%.4f + %.4f) / 2 = %.4f ns per sky pixel;"
              % (ns[("frame", "sky", 0)], ns[("frame", "sky", 1)], mid),
              "# sbx_atmosphere_eval default over the same rays = %.4f ns per ray: %s." % (got, "MET" if got <= mid else "MISSED")]
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
