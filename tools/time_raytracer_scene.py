"""SBX_APP_RAYTRACER_SCENE's kernel beside the fixed-scene kernels it generalises: one-launch times at 3840x2160,
u_time .37, of
    raytracer default / variant 1         k_raytracer as shipped (hit_walls + witnessed roots) / its plain statement: the six-plane
                                          loop with compile-time counts and the IEEE roots
    raytracer_scene default / variant 1   k_raytracer_scene over the Cornell block of the same uniforms (run-time counts, the plane loop,
                                          witnessed roots / IEEE roots): the same pixels as the two above
    raytracer_scene 16 + 16               k_raytracer_scene over a seeded scene of 16 planes and 16 spheres
                                          (tests/raytracer_scene_model.tame_scene(1, (16, 16)): 2 bounces, directional light, shadow on)
Every case runs in a process of its own, --passes times (the parent never opens the GPU); per process the median and minimum of N
launches after a warm-up, each launch between its own events.  A case's time is the median of its passes' medians and its pass spread
their largest minus their smallest.

Bar: the scene kernel's default time over the Cornell block is at or below SBX_APP_RAYTRACER's variant-1 time on the same frame, with
no margin beyond the pass spread (the larger of the two cases').  Prints the table and the bar as read in this run, and writes them to
--out if one is given; profiles/raytracer_scene_timing.txt is such an output with the kernels' resources written under it by hand.

    python tools/time_raytracer_scene.py [--launches 30] [--warmup 5] [--passes 3] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, T = 3840, 2160, .37
CASES = [("raytracer", "shipped", 0), ("raytracer", "shipped", 1), ("raytracer_scene", "cornell", 0), ("raytracer_scene", "cornell", 1),
         ("raytracer_scene", "16+16", 0)]
NAMES = {0: "default", 1: "variant 1"}


def child(app, scene, variant, launches, warmup):
    import torch
    import shaderbox_amd
    aux = None
    if scene == "cornell":
        aux = shaderbox_amd.cornell_scene(W, H, T)
    elif scene == "16+16":
        from tests import raytracer_scene_model as M
        aux = M.to_block(M.tame_scene(1, (16, 16)))
        assert (aux.n_planes, aux.n_spheres) == (16, 16)
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    before = R.raytracer_scene_launches()
    for _ in range(warmup):
        R.render(app, W, H, T, aux=aux, out=buf)
    torch.cuda.synchronize()
    assert R.raytracer_scene_launches() - before == (warmup if app == "raytracer_scene" else 0)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        R.render(app, W, H, T, aux=aux, out=buf)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print("RESULT %.5f %.5f" % (ms[len(ms) // 2], ms[0]), flush=True)
    R.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--bar-only", action="store_true", help="only the two cases the bar compares")
    ap.add_argument("--out", default=None, help="also write the table and the bar to this file")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]), args.launches, args.warmup)
    lines = ["# tools/time_raytracer_scene.py: %dx%d, u_time %.2f; one process per case and pass, %d passes; per process the median (and minimum)"
             % (W, H, T, args.passes),
             "# of %d launches after %d warm-up launches, each between its own events.  median ms = the median of the passes' medians; spread ="
             % (args.launches, args.warmup),
             "# the largest minus the smallest of them; min ms = the smallest launch of any pass.",
             "# %-18s %-8s %-10s %10s %10s %10s %12s" % ("app", "scene", "kernels", "median ms", "spread ms", "min ms", "ns / pixel")]
    print("\n".join(lines), flush=True)
    med, spread = {}, {}
    for app, scene, variant in CASES:
        if args.bar_only and (app, scene, variant) not in (("raytracer", "shipped", 1), ("raytracer_scene", "cornell", 0)):
            continue
        meds, mins = [], []
        for _ in range(args.passes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                                "--child", app, scene, str(variant)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit("case %s %s %d failed (%d):\n%s" % (app, scene, variant, r.returncode, r.stderr[-2000:]))
            a, b = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
            meds.append(float(a))
            mins.append(float(b))
        key = (app, scene, variant)
        med[key], spread[key] = sorted(meds)[len(meds) // 2], max(meds) - min(meds)
        line = "  %-18s %-8s %-10s %10.4f %10.4f %10.4f %12.4f" % (app, scene, NAMES[variant], med[key], spread[key], min(mins), med[key] * 1e6 / (W * H))
        lines.append(line)
        print(line, flush=True)
    plain, scene = ("raytracer", "shipped", 1), ("raytracer_scene", "cornell", 0)
    margin = max(spread[plain], spread[scene])
    lines += ["#", "# Bar (read in this run): raytracer_scene default over the Cornell block %.4f ms against raytracer variant 1 %.4f ms on the same frame,"
              % (med[scene], med[plain]),
              "# pass spread %.4f ms: %s." % (margin, "MET" if med[scene] <= med[plain] + margin else "MISSED")]
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
