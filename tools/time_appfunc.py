"""APP_FUNC against the store floor: the default kernel (hash table) and the plain one (sbx_set_variant 1, hash_w in
place) at 1920x1080 / 3840x2160 / 7680x4320, float and RGBA8 output.  Per case: the median of N back-to-back launches after a
warm-up, each bracketed by its own pair of events; the floor is a torch fill_ of the same buffer timed the same way in the same
process.  Writes profiles/appfunc_timing.txt (or the file given with --out; --append adds to it).  --lib times another build of
libsbx (an A/B build of tools/ab_build.py), in its own process.  The kernel-trace run is separate:

    rocprofv3 --kernel-trace --stats -d <dir> -o appfunc -- python tools/time_appfunc.py --launches 20 --out /dev/null
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lib", default="", help="another libsbx.so to time (default: the package's)")
    ap.add_argument("--label", default="", help="name of this build in the table (default: 'lib' or the --lib file name)")
    ap.add_argument("--plain", type=int, default=1, help="0: time the default kernel only")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appfunc_timing.txt"))
    args = ap.parse_args()
    import torch
    import shaderbox_amd
    if args.lib:
        shaderbox_amd.LIB_PATH = os.path.abspath(args.lib)
    label = args.label or (os.path.basename(args.lib) if args.lib else "libsbx")
    R = shaderbox_amd.Renderer(0)
    lines = [] if args.append else [
        "# tools/time_appfunc.py: median of %d back-to-back launches after %d warm-up launches, each between its own events;"
        % (args.launches, args.warmup),
        "# floor = torch fill_ of the same buffer, timed the same way in the same process.  ratio = kernel / floor.",
        "# %-18s %-8s %-8s %-10s %10s %10s %8s" % ("build", "kernel", "format", "size", "kernel ms", "fill ms", "ratio")]
    print("\n".join(lines), flush=True)
    kernels = [("default", 0)] + ([("plain", 1)] if args.plain else [])
    for fmt in ("rgba32f", "rgba8"):
        R.set_output_format(fmt)
        for w, h in ((1920, 1080), (3840, 2160), (7680, 4320)):
            buf = torch.empty((h, w, 4), dtype=R.pixel_dtype, device=R.tdev)
            fill = median_ms(torch, lambda: buf.fill_(0), args.launches, args.warmup)
            for name, variant in kernels:
                R.set_variant(variant)
                n = max(3, args.launches // 10) if variant == 1 else args.launches
                k = median_ms(torch, lambda: R.render("func", w, h, 0.37, out=buf), n, min(args.warmup, n))
                line = "  %-18s %-8s %-8s %-10s %10.4f %10.4f %8.2f" % (label, name, fmt, "%dx%d" % (w, h), k, fill, k / fill)
                lines.append(line)
                print(line, flush=True)
            R.set_variant(0)
    R.set_output_format("rgba32f")
    R.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
