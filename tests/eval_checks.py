"""What the GPU test files of the eval entries (include/sbx.h sbx_<family>_eval, "a function of an app over the caller's elements")
share, written once: the bit comparison, the ragged-size / bounds / alignment check, the stream-capture check and the refusal loop.
A test file states its family's data, models and raw ctypes calls and calls in here; every assertion about one family alone (counts,
tame and untame waves, frames, n == 0 shapes) stays in its file.  A plain module (pytest does not collect it).

The raw calls are closures over the family's own middle arguments that return the entry's return code:
call(fn, in_ptr, out_ptr, n) for check_ragged, call(in_ptr, out_ptr, n) for check_capture_replay and its refused_twin."""
import ctypes

import numpy as np

from tests.model_common import F, same_bits


def differing(got, want):
    """#rows of got (a tensor or an array) with any bit other than want's, NaN == NaN; the shapes must agree"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((~same_bits(got, want).reshape(len(want), -1).all(axis=-1)).sum())


def to_dev(x):
    """a float32 host tensor of x (the Renderer methods move it to their device)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F))


def raw_call(renderer, family, lead=(), mid=(), counts=None):
    """call(fn, in_ptr, out_ptr, n) -> the return code of sbx_<family>_eval or, with `counts` (where the twin writes its counters),
    of sbx_debug_<family>_eval, straight through ctypes on the renderer's current stream: (ctx, fn, *lead, in, *mid, out, n[, counts],
    stream), `lead` and `mid` being the family's own arguments as ctypes values"""
    entry = getattr(renderer.lib, ("sbx_%s_eval" if counts is None else "sbx_debug_%s_eval") % family)
    tail = () if counts is None else (counts,)

    def call(fn, in_ptr, out_ptr, n):
        return entry(renderer.ctx, fn.encode(), *lead, ctypes.c_void_p(in_ptr), *mid, ctypes.c_void_p(out_ptr), n, *tail, renderer._stream())
    return call


def check_ragged(renderer, call, cases, n, guard=64, poison=-7.25):
    """each case (fn, (win, wout), x[n, win], want[n, wout]): out inside a poisoned buffer with `guard` words either side, in and out 4
    bytes off their allocation's 16-byte alignment; the guards stay poison, the body has the model's bits, the input is untouched"""
    import torch
    for fn, (win, wout), x, want in cases:
        x = np.ascontiguousarray(x, dtype=F)
        assert x.shape == (n, win) and want.shape == (n, wout), (fn, n, x.shape, want.shape)
        ibuf = torch.zeros(1 + win * n, dtype=torch.float32, device=renderer.tdev)
        ibuf[1:] = torch.from_numpy(x.ravel()).to(renderer.tdev)
        obuf = torch.full((1 + 2 * guard + wout * n,), poison, dtype=torch.float32, device=renderer.tdev)
        assert ibuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
        i_ptr, o_ptr = ibuf.data_ptr() + 4, obuf.data_ptr() + 4 * (1 + guard)
        assert i_ptr % 16 == 4 and o_ptr % 16 == 4
        renderer._check(call(fn, i_ptr, o_ptr, n))
        o = obuf.cpu().numpy()
        assert (o[:1 + guard] == poison).all() and (o[1 + guard + wout * n:] == poison).all(), (fn, n)
        assert differing(o[1 + guard:1 + guard + wout * n].reshape(n, wout), want) == 0, (fn, n)
        assert np.array_equal(ibuf[1:].cpu().numpy().view(np.uint32), x.ravel().view(np.uint32)), (fn, n)


def check_capture_replay(renderer, call, x, want, wout, refused_twin=None, also=()):
    """the entry is one kernel launch and nothing else: call(in_ptr, out_ptr, n) over x recorded into a graph runs nothing; replayed, it
    gives `want`; replayed over the reversed inputs in the same buffers, the reversed `want`.  refused_twin(in_ptr, out_ptr, 4): the
    counted twin, which refuses a capturing stream (-1) and leaves the capture intact.  also: further (call, x, want, wout) recorded
    into the same graph and checked the same way."""
    import torch
    jobs = []
    for c, xs, w, wo in [(call, x, want, wout)] + list(also):
        xs = np.ascontiguousarray(xs, dtype=F)
        jobs.append((c, xs, w, torch.from_numpy(xs).to(renderer.tdev), torch.zeros((len(xs), wo), dtype=torch.float32, device=renderer.tdev)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.zeros(1, device=renderer.tdev)                            # the stream exists before the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for c, xs, _, dev, out in jobs:
            renderer._check(c(dev.data_ptr(), out.data_ptr(), len(xs)))
        if refused_twin is not None:
            assert refused_twin(jobs[0][3].data_ptr(), jobs[0][4].data_ptr(), 4) == -1, "the counted twin refuses a capture"
    torch.cuda.synchronize()
    for _, _, _, _, out in jobs:
        assert bool((out == 0).all()), "a capture runs nothing"
    g.replay()
    torch.cuda.synchronize()
    for _, _, w, _, out in jobs:
        assert differing(out, w) == 0
    for _, xs, _, dev, out in jobs:
        dev.copy_(torch.from_numpy(xs[::-1].copy()))
        out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for _, _, w, _, out in jobs:
        assert differing(out, w[::-1]) == 0


def check_refusals(renderer, plain, twin, bad_args, out, sentinel=-1.0):
    """each argument tuple of bad_args is refused (-1) by the entry `plain` with an error text, and by twin(args) (the counted twin over
    the same tuple; None: the file checks none) too; `out`, filled with `sentinel` by the caller, is not written"""
    import torch
    for args in bad_args:
        assert plain(*args) == -1, args
        assert renderer.lib.sbx_last_error(renderer.ctx)
        if twin is not None:
            assert twin(args) == -1, args
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()), "a refused call writes nothing"
