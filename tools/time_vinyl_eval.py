"""sbx_vinyl_eval and SBX_APP_VINYL_DECK beside the frame kernels of APP_VINYL.  Three comparisons, each in ONE process
of its own (the parent never opens the GPU) whose legs ALTERNATE in blocks of 8 launches, every launch between its own events; per leg
the median and min - max of N launches after a warm-up:

  eval   "render" over the primary rays of the shipped camera's 1280x720 frame (u_time .37; computed on the host with
         tests/vinyl_deck_model.primary_rays) in frame order, beside the SBX_APP_VINYL frame of that size and time under
         sbx_set_variant 1 (k_vinyl<CULL = false, IEEE roots>: the parent commit's kernel, its listing is unchanged) and under the
         default; the same rays in a fixed random permutation.  The bar: the eval's median is no more than the variant-1 frame's, within
         a margin of the larger of the two legs' min - max spreads.
  deck   SBX_APP_VINYL_DECK with no block beside SBX_APP_VINYL at 3840x2160: the same pixel over the same frame constants.
  vinyl  SBX_APP_VINYL at 3840x2160 alone: one run of this library, and two runs of the tree given with --parent-root (a checkout of
         the parent commit with its library built; without it, of this tree): the factor between two runs of the parent alone,
         against which both ratios are read.

    python tools/time_vinyl_eval.py [--launches 40] [--warmup 16] [--parent-root DIR] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T = 1280, 720, .37
PW, PH = 3840, 2160
BLOCK = 8


def timed(legs, launches, warmup):
    """legs: [(name, fn)] -> {name: (median, min, max)} in ms; blocks of BLOCK launches of one leg, the legs in turn"""
    import torch
    for _ in range((warmup + BLOCK - 1) // BLOCK):
        for _, fn in legs:
            for _ in range(BLOCK):
                fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for _ in range((launches + BLOCK - 1) // BLOCK):
        for name, fn in legs:
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(BLOCK)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ms[name] += [a.elapsed_time(b) for a, b in ev]
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}


def child(kind, launches, warmup, root):
    sys.path.insert(0, root)
    import torch
    import shaderbox_amd
    R = shaderbox_amd.Renderer(0)
    extra = ""
    if kind == "eval":
        from tests import vinyl_deck_model as M
        D = M.default_deck(T)
        fx, fy = M.frame_coords(W, H)
        ro, rd = M.primary_rays(D, W, H, fx, fy)
        rays = np.stack([np.full(W * H, c, dtype=np.float32) for c in ro] + list(rd), axis=1).astype(np.float32)
        a = M.as_aux(D)
        ordered = torch.from_numpy(rays).to(R.tdev)
        permuted = torch.from_numpy(rays[np.random.default_rng(20).permutation(len(rays))]).to(R.tdev)
        # the same bits as the frame's, before anything is timed (sRGB by the model)
        out = R.vinyl_eval("render", ordered, a).cpu().numpy()
        frame = R.render("vinyl", W, H, T).cpu().numpy()
        same = bool(M.same_bits(M.finish(out[:, :3]).reshape(H, W, 4), frame).all())
        c1, c2 = R.vinyl_eval_counted("render", ordered, a)[1], R.vinyl_eval_counted("render", permuted, a)[1]
        extra = "same_bits=%d waves_ordered=%d/%d waves_permuted=%d/%d" % (same, c1[1], c1[0] + c1[1], c2[1], c2[0] + c2[1])
        buf = torch.empty((H, W, 4), dtype=torch.float32, device=R.tdev)

        def frame_v(v):
            R.set_variant(v)
            R.render("vinyl", W, H, T, out=buf)
            R.set_variant(0)
        legs = [("eval ordered", lambda: R.vinyl_eval("render", ordered, a)), ("frame variant 1", lambda: frame_v(1)),
                ("frame default", lambda: frame_v(0)), ("eval permuted", lambda: R.vinyl_eval("render", permuted, a))]
    elif kind == "deck":
        buf = torch.empty((PH, PW, 4), dtype=torch.float32, device=R.tdev)
        legs = [("vinyl_deck no block", lambda: R.render("vinyl_deck", PW, PH, T, out=buf)), ("vinyl", lambda: R.render("vinyl", PW, PH, T, out=buf))]
    else:
        buf = torch.empty((PH, PW, 4), dtype=torch.float32, device=R.tdev)
        legs = [("vinyl", lambda: R.render("vinyl", PW, PH, T, out=buf))]
    res = timed(legs, launches, warmup)
    for name, _ in legs:
        print("RESULT %s|%.5f|%.5f|%.5f" % ((name,) + res[name]), flush=True)
    print("EXTRA " + extra, flush=True)
    R.close()


def run(kind, args, root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--warmup", str(args.warmup),
                        "--child", kind, "--root", root], capture_output=True, text=True, timeout=900, cwd=root)
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (kind, r.returncode, r.stderr[-2000:]))
    res = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            name, med, mn, mx = ln[7:].split("|")
            res[name] = (float(med), float(mn), float(mx))
    extra = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("EXTRA ")][0]
    return res, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: the two `vinyl` runs of the parent use it")
    ap.add_argument("--out", default=None, help="also write the tables and the readings to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.warmup, args.root)
    assert args.launches >= 24, "at least 24 timed launches per leg"
    row = lambda name, r, more="": "  %-22s %10.4f %10.4f %10.4f   %s" % (name, r[0], r[1], r[2], more)  # noqa: E731
    head = "# %-22s %10s %10s %10s" % ("leg", "median ms", "min ms", "max ms")
    lines = ["# tools/time_vinyl_eval.py: u_time %.2f; per comparison one process whose legs alternate in blocks of %d launches; median and" % (T, BLOCK),
             "# min - max of %d launches per leg after %d warm-up launches, each launch between its own events." % (args.launches, args.warmup), "#",
             "# 1. eval: \"render\" over the %d primary rays of the shipped %dx%d frame, frame order" % (W * H, W, H), head]
    ev, extra = run("eval", args, ROOT)
    px = W * H
    for name in ("eval ordered", "frame variant 1", "frame default", "eval permuted"):
        lines.append(row(name, ev[name], "%.3f ns / ray" % (ev[name][0] * 1e6 / px)))
    lines.append("# " + extra + "   (waves: re-run / counted)")
    e, f = ev["eval ordered"], ev["frame variant 1"]
    margin = max(e[2] - e[1], f[2] - f[1])
    verdict = "MET" if e[0] <= f[0] else "MET WITHIN THE MARGIN" if e[0] <= f[0] + margin else "MISSED"
    lines += ["# Bar: the eval over the ordered rays %.4f ms <= the variant-1 frame %.4f ms (margin %.4f ms, the larger min - max spread): %s"
              % (e[0], f[0], margin, verdict),
              "# (ratio %.3f; against the default frame: %.3fx; the permutation costs the eval %.2fx)."
              % (e[0] / f[0], e[0] / ev["frame default"][0], ev["eval permuted"][0] / e[0]), "#",
              "# 2. deck: SBX_APP_VINYL_DECK with no block beside SBX_APP_VINYL at %dx%d, one process" % (PW, PH), head]
    print("\n".join(lines), flush=True)
    n0 = len(lines)
    de, _ = run("deck", args, ROOT)
    for name in ("vinyl_deck no block", "vinyl"):
        lines.append(row(name, de[name]))
    proot = args.parent_root or ROOT
    lines += ["#", "# 3. vinyl: SBX_APP_VINYL at %dx%d alone: this library, then two runs of %s" % (PW, PH, "the parent commit's library" if args.parent_root else "this library again"), head]
    here = run("vinyl", args, ROOT)[0]["vinyl"]
    lines.append(row("vinyl, this library", here))
    runs = [run("vinyl", args, proot)[0]["vinyl"] for _ in range(2)]
    for i, r in enumerate(runs):
        lines.append(row("vinyl, parent run %d" % (i + 1), r))
    spread = max(runs[0][0], runs[1][0]) / min(runs[0][0], runs[1][0])
    within = lambda x: "WITHIN" if 1 / spread <= x <= spread else "OUTSIDE"  # noqa: E731
    r_deck = de["vinyl_deck no block"][0] / de["vinyl"][0]
    r_here = here[0] / (.5 * (runs[0][0] + runs[1][0]))
    lines += ["# Reading: the two runs of the parent differ by a factor of %.4f.  vinyl_deck / vinyl = %.4f: %s that factor.  vinyl here / the"
              % (spread, r_deck, within(r_deck)),
              "# parent's mean = %.4f: %s that factor." % (r_here, within(r_here))]
    print("\n".join(lines[n0:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
