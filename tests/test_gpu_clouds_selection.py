"""GPU tests of APP_CLOUDS' kernel selection (csrc/kern_clouds.hip clouds_select / launch_form): every case of
tests/clouds_selection_cases.py is launched once at 96 x 54, the record the launcher wrote (sbx_debug_clouds_last_selection) must be
the selection the case states — so each of the 19 + 19 + 8 + 3 kernels is KNOWN to have rendered a frame here — and that frame must be
the per-lane kernel's and, for the shipped build, the CPU oracle's.  Then: a ragged frame per (LM, SM, GT) of the shipped build, a frame
either side of every table-range edge, and the exp_small / regular / div3 edges, where the record must differ between the two sides.
Every frame goes into a buffer poisoned with a NaN no kernel computes; every comparison is bit for bit with NaN == NaN.  Every frame
that takes a hash-table kernel has had its lattice indices enumerated on the CPU (tests/test_clouds_hashtab_cpu.py GT_FRAMES)."""
import numpy as np
import pytest

from tests import clouds_selection_cases as C
from tests.app_checks import assert_same
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)
from tests.test_gpu_clouds_hashtab import fresh, launch, perlane, poisoned, used_table  # noqa: F401 (`fresh`: a context of its own)

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_frame(c):
    """the CPU oracle's frame of a case of the shipped build, computed once"""
    from oracle import aux_sets
    from oracle.oracle import APP_IDS
    from tests.model_common import oracle
    key = (c["app"], c["w"], c["h"], c["t"], c["mouse"], repr(sorted(c["aux"].items())))
    if key not in _ORACLE:
        aux = aux_sets.block("clouds", dict(c["aux"])) if c["aux"] else None
        _ORACLE[key] = oracle().render(APP_IDS[c["app"]], c["w"], c["h"], c["t"], mouse=c["mouse"], aux=aux, threads=8)
    return _ORACLE[key]


def expected_record(c):
    f = C.frame_of(c["app"], c["w"], c["h"], c["t"], c["mouse"], c["aux"])
    rows, kind, table = C.launch_context(c, f)
    want = C.select(f, C.BUILD_OF[c["app"]], c["variant"], rows, table)
    assert C.kernel_of(want) == c["kernel"] and kind == c["ytab"]      # (tests/test_clouds_selection_cpu.py has shown it of the hook)
    want["ytab"] = kind if want["ytab_used"] else 0
    return want


def captured(r, c, aux):
    """the case's launch recorded into a graph on a stream of its own, replayed once -> the frame"""
    import torch
    out = poisoned(r, c["w"], c["h"])
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            r.render(c["app"], c["w"], c["h"], c["t"], mouse=c["mouse"], aux=aux, out=out)
    rec = r.clouds_last_selection()                                    # the choice is made when the launch is recorded
    g.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got.view(np.uint32) == 0x7fc0beef).any(), (c["name"], "pixels left unwritten")
    return got, rec


def run_case(r, c):
    """one launch of the case on the context `r` (fresh: no table of any kind yet) -> (frame, record)"""
    import torch
    aux = C.aux_struct(c["aux"])
    kw = dict(mouse=c["mouse"], aux=aux)
    before = r.clouds_last_selection()["launches"]
    try:
        r.set_variant(c["variant"])
        if c["mode"] == "eager":
            got = launch(r, c["app"], c["w"], c["h"], c["t"], **kw)
            rec = r.clouds_last_selection()
            assert rec["launches"] == before + 1
        else:
            if c["mode"] == "captured_warm":                           # the first launch builds the table, the second sees it complete
                launch(r, c["app"], c["w"], c["h"], c["t"], **kw)
                torch.cuda.synchronize()
                launch(r, c["app"], c["w"], c["h"], c["t"], **kw)
            got, rec = captured(r, c, aux)
    finally:
        r.set_variant(0)
    assert used_table(r) == (1 if rec["gt"] else 0)
    return got, rec


def check_case(r, c, oracle_too=True):
    want = expected_record(c)
    got, rec = run_case(r, c)
    rec.pop("launches")
    assert rec == want, (c["name"], {k: (rec[k], want[k]) for k in rec if rec[k] != want[k]})
    plain = perlane(r, c["app"], c["w"], c["h"], c["t"], mouse=c["mouse"], aux=C.aux_struct(c["aux"]))
    p = r.clouds_last_selection()
    assert (p["perlane"], p["ytab_used"], p["gt"], p["build"]) == (1, 0, 0, want["build"]) and used_table(r) == 0
    assert_same(got, plain, (c["name"], "per-lane kernel"))
    if oracle_too and c["app"] in ("clouds", "clouds_sky"):
        assert_same(got, oracle_frame(c), (c["name"], "oracle"))
    return rec


# ---- 1. the table: every kernel renders a frame, and the record says which --------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in C.CASES])
def test_case_takes_its_kernel_and_renders_the_frame(fresh, name):   # noqa: F811
    check_case(fresh, C.BY_NAME[name])


def test_the_table_covers_the_launcher():
    """(the CPU suite asserts it of the hook; here of the cases this file launches)"""
    assert {(C.BUILD_OF[c["app"]], c["kernel"]) for c in C.CASES} == C.INSTANTIATIONS


# ---- 2. ragged frames: 33 x 3, one per (LM, SM, GT) of the shipped build -----------------------------------------------------------------
@pytest.mark.parametrize("name", C.RAGGED)
def test_ragged_frame(fresh, name):   # noqa: F811
    c = dict(C.BY_NAME[name], w=33, h=3, name=name + "_33x3")
    check_case(fresh, c)


def test_ragged_frames_cover_every_form_of_the_shipped_build():
    forms = {C.BY_NAME[n]["kernel"][2:] for n in C.RAGGED}
    assert forms == {k[2:] for k in C.FORMS if k[1] == 1}               # every (LM, SM, GT) that exists


# ---- 3. either side of every table-range edge ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun", ["z", "yz"])
@pytest.mark.parametrize("k", range(len(C.RANGE_EDGES)))
def test_table_range_edge(fresh, k, sun):   # noqa: F811
    e, inside, beyond = C.range_edge_cases(sun)[k]
    a = check_case(fresh, inside, oracle_too=False)
    assert (a["need_range"], a["table_range"], a["gt"]) == (e, e, C.G)
    b = check_case(fresh, beyond, oracle_too=False)
    if e < C.MAX_RANGE:
        assert (b["need_range"], b["table_range"], b["gt"]) == (2 * e, 2 * e, C.G) and fresh.clouds_hashtab()[2] == 2
    else:
        assert (b["need_range"], b["table_range"], b["gt"]) == (0, 0, 0) and fresh.clouds_hashtab()[2] == 1


# ---- 4. the predicate edges: another kernel on either side, the same frame as the oracle's on both -------------------------------------------
@pytest.mark.parametrize("edge", C.PREDICATE_EDGES, ids=lambda e: e[0])
def test_predicate_edge(fresh, edge):   # noqa: F811
    name, field, inside, outside = edge
    a = check_case(fresh, C._c(name + "_in", "clouds", C.kernel_of(C.select(C.frame_of("clouds", C.W, C.H, C.T, (0.0, 0.0), inside), 0, 0,
                                                                          C.YTAB_ROWS, C.MIN_RANGE)), 1, inside))
    b = check_case(fresh, C._c(name + "_out", "clouds", C.kernel_of(C.select(C.frame_of("clouds", C.W, C.H, C.T, (0.0, 0.0), outside), 0, 0,
                                                                           C.YTAB_ROWS, C.MIN_RANGE)), 1, outside))
    assert (a[field], b[field]) == (1, 0), name
    assert C.kernel_of(a) != C.kernel_of(b), (name, C.kernel_of(a))
