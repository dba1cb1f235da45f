#!/usr/bin/env python3
"""Timing legs of the view-table change beside the headline (profiles/clouds_viewtab_timing.txt section 4), run in the tree whose
library is to be measured — its own directory is the package root, so the same file times the parent commit's tree and this one:

    python tools/time_clouds_viewtab.py <label>

3840x2160, one process, a context per leg: 10 warm-up launches, then 60 launches timed as a whole by the host clock around a final
synchronise.  `one at a time`: each launch finished before the next.  `3 in flight`: three streams, three frames — this tool's own leg,
not `value_pipelined` of `bench.py --full`.  `--legs a,b` runs only the named legs."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import shaderbox_amd  # noqa: E402
from oracle import aux_sets  # noqa: E402

W, H, N = 3840, 2160, 60
label = sys.argv[1] if len(sys.argv) > 1 else "tree"


def aux_of(fields):
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", dict(fields)).tobytes()) if fields else None


def leg(name, app="clouds", sun=None, animate=False, move=False, streams=1):
    R = shaderbox_amd.Renderer(0)
    aux = aux_of({"sun_dir": sun} if sun else None)
    st = [torch.cuda.Stream() for _ in range(streams)]
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(streams)]

    def run(n, k0):
        for k in range(k0, k0 + n):
            t = .37 + (k / 60.0 if animate or move else 0.0)
            mouse = (300.0 + (k % 200 if move else 0), 0.0)
            with torch.cuda.stream(st[k % streams]):
                R.render(app, W, H, t, mouse=mouse, aux=aux, out=outs[k % streams])
            if streams == 1:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    run(10, 0)
    t0 = time.perf_counter()
    run(N, 10)
    ms = (time.perf_counter() - t0) * 1e3 / N
    vt = R.clouds_viewtab() if hasattr(R, "clouds_viewtab") else None
    rec = R.clouds_last_selection()
    print("%-8s %-26s ms per frame %.4f | kernel (YTAB, REG, LM, SM, GT) = %s | viewtab %s"
          % (label, name, ms, (rec["ytab_used"], rec["reg"], rec["lm"], rec["sm"], rec["gt"]), vt), flush=True)
    R.close()


LEGS = {"fixed": lambda: leg("fixed, one at a time"),
        "animated": lambda: leg("animated, one at a time", animate=True),
        "moving": lambda: leg("moving camera, one at a time", move=True),
        "inflight": lambda: leg("3 in flight", streams=3),
        "yz": lambda: leg("sun 0,0.6,-0.8", sun=(0.0, 0.6, -0.8)),
        "general": lambda: leg("sun 0.3,0.2,-0.9 (general)", sun=(0.3, 0.2, -0.9)),
        "sky": lambda: leg("clouds_sky", app="clouds_sky")}
names = sys.argv[sys.argv.index("--legs") + 1].split(",") if "--legs" in sys.argv else list(LEGS)
for n in names:
    LEGS[n]()
