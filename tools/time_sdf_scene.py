"""SBX_APP_SDF_SCENE's kernel beside the fixed-scene kernel whose renderer it shares: one-launch times at 3840x2160,
u_time .37, of
    sdf_scene ramp, default / variant 1   k_sdf_scene over the ramp block of the uniforms (sbx_sdf_scene_ramp: 20 instructions, 10 primitives):
                                          witnessed roots / IEEE roots
    sdf_scene 32                          k_sdf_scene over a seeded 32-instruction scene (tests/sdf_scene_model.tame_scene(1, 32))
    sdf_ao default / variant 1            k_sdf_ao as shipped (culled ramps, hardware min / max, witnessed roots) / its plain statement:
                                          all 21 primitives at every sample, the IEEE roots
Every case runs in a process of its own, --passes times (the parent never opens the GPU); per process the median and minimum of N
launches after a warm-up, each launch between its own events.  A case's time is the median of its passes' medians and its pass spread
their largest minus their smallest.

Bar: sdf_scene over the ramp block, default kernels, is at or below SBX_APP_SDF_AO's variant-1 time on the same frame size, with no margin
beyond the pass spread (the larger of the two cases').  The two frames differ — one ramp is absent, so some rays march further — so this
bounds the interpreter's overhead; it is no equality.  Prints the table and the bar as read in this run, and writes them to --out.

--lib NAME times build/ab/libsbx_NAME.so (tools/ab_build.py) instead of the product library: the operand path
(NAME:kern_sdf_scene.hip:-DSDF_SCENE_OPERANDS_LDS=0).

    python tools/time_sdf_scene.py [--launches 30] [--warmup 5] [--passes 3] [--lib NAME] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, T = 3840, 2160, .37
CASES = [("sdf_scene", "ramp", 0), ("sdf_scene", "32", 0), ("sdf_scene", "ramp", 1), ("sdf_ao", "shipped", 0), ("sdf_ao", "shipped", 1)]
NAMES = {0: "default", 1: "variant 1"}


def child(app, scene, variant, launches, warmup, lib):
    import torch
    import shaderbox_amd
    if lib:
        shaderbox_amd.LIB_PATH = os.path.join(ROOT, "build", "ab", "libsbx_%s.so" % lib)
    aux = None
    if scene == "ramp":
        aux = shaderbox_amd.sdf_ramp_scene(W, H, T)
    elif scene == "32":
        from tests import sdf_scene_model as M
        aux = M.as_aux(M.tame_scene(1, 32))
        assert aux.n_instr == 32
    R = shaderbox_amd.Renderer(0)
    R.set_variant(variant)
    buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)
    for _ in range(warmup):
        R.render(app, W, H, T, aux=aux, out=buf)
    torch.cuda.synchronize()
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
    ap.add_argument("--lib", default="", help="build/ab/libsbx_<LIB>.so instead of the product library")
    ap.add_argument("--out", default=None, help="also write the table and the bar to this file")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], int(args.child[2]), args.launches, args.warmup, args.lib)
    lines = ["# tools/time_sdf_scene.py%s: %dx%d, u_time %.2f; one process per case and pass, %d passes; per process the median (and minimum)"
             % (" --lib " + args.lib if args.lib else "", W, H, T, args.passes),
             "# of %d launches after %d warm-up launches, each between its own events.  median ms = the median of the passes' medians; spread ="
             % (args.launches, args.warmup),
             "# the largest minus the smallest of them; min ms = the smallest launch of any pass.",
             "# %-12s %-8s %-10s %10s %10s %10s %12s" % ("app", "scene", "kernels", "median ms", "spread ms", "min ms", "ns / pixel")]
    print("\n".join(lines), flush=True)
    med, spread = {}, {}
    for app, scene, variant in CASES:
        meds, mins = [], []
        for _ in range(args.passes):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                                "--lib", args.lib, "--child", app, scene, str(variant)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit("case %s %s %d failed (%d):\n%s" % (app, scene, variant, r.returncode, r.stderr[-2000:]))
            a, b = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1:]
            meds.append(float(a))
            mins.append(float(b))
        key = (app, scene, variant)
        med[key], spread[key] = sorted(meds)[len(meds) // 2], max(meds) - min(meds)
        line = "  %-12s %-8s %-10s %10.4f %10.4f %10.4f %12.4f" % (app, scene, NAMES[variant], med[key], spread[key], min(mins), med[key] * 1e6 / (W * H))
        lines.append(line)
        print(line, flush=True)
    plain, scene = ("sdf_ao", "shipped", 1), ("sdf_scene", "ramp", 0)
    margin = max(spread[plain], spread[scene])
    lines += ["#", "# Bar (read in this run): sdf_scene default over the ramp block %.4f ms against sdf_ao variant 1 %.4f ms at the same frame size,"
              % (med[scene], med[plain]),
              "# pass spread %.4f ms: %s." % (margin, "MET" if med[scene] <= med[plain] + margin else "MISSED")]
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
