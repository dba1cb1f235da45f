"""APP_2D / APP_2D_TEX against the store floor: every phase (u_time 2, 6, 10, 14), 1920x1080 / 3840x2160 /
7680x4320, float and RGBA8 output.  Per case: the median of N back-to-back launches after a warm-up, each bracketed by its own pair
of events; the floor is a torch fill_ of the same buffer timed the same way in the same process.  Writes profiles/app2d_timing.txt
(or the file given with --out).  The kernel-trace run is separate:

    rocprofv3 --kernel-trace --stats -d <dir> -o app2d -- python tools/time_app2d.py --launches 20 --out /dev/null
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "app2d_timing.txt"))
    args = ap.parse_args()
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    lines = ["# tools/time_app2d.py: median of %d back-to-back launches after %d warm-up launches, each between its own events;"
             % (args.launches, args.warmup),
             "# floor = torch fill_ of the same buffer, timed the same way in the same process.  ratio = kernel / floor.",
             "# %-6s %-8s %-10s %-5s %10s %10s %7s %9s" % ("app", "format", "size", "t", "kernel ms", "fill ms", "ratio", "GB/s")]
    print("\n".join(lines), flush=True)
    for fmt in ("rgba32f", "rgba8"):
        R.set_output_format(fmt)
        for w, h in ((1920, 1080), (3840, 2160), (7680, 4320)):
            buf = torch.empty((h, w, 4), dtype=R.pixel_dtype, device=R.tdev)
            fill = median_ms(torch, lambda: buf.fill_(0), args.launches, args.warmup)
            nbytes = buf.numel() * buf.element_size()
            for app in ("2d", "2d_tex"):
                for t in (2.0, 6.0, 10.0, 14.0):
                    k = median_ms(torch, lambda: R.render(app, w, h, t, out=buf), args.launches, args.warmup)
                    line = "  %-6s %-8s %-10s %-5g %10.4f %10.4f %7.3f %9.0f" % (app, fmt, "%dx%d" % (w, h), t, k, fill, k / fill,
                                                                            nbytes / k / 1e6)
                    lines.append(line)
                    print(line, flush=True)
    R.set_output_format("rgba32f")
    R.close()
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
