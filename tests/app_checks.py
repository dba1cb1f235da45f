"""What the GPU test files share, written once: the fixtures (`renderer`, `renderer8`, `volumes`, `variant_restored`), the comparisons
(`compare`, `assert_same`, `same_tensor`, `bits_differ`), the app lists, and the checks every app's file makes of the layers above
its kernel: rows, host rows, ranks and splits, the loopback exchanges, the 8-bit format, sbx_multi_render, the sbx_mainimage.hpp
drop-in, the app that header selects and host/sbx_render.  A test file states its app's name, sizes, times, aux block and expected frame and calls in here;
what belongs to one app stays in its file.  A plain module (pytest does not collect it): a test module imports the fixtures it
names.

`compare`, `assert_same` and model_common.same_bits count NaN == NaN as equal; `same_tensor`, `bits_differ` and torch.equal on
int32 views do not."""
import os
import subprocess

import numpy as np
import pytest

from tests.model_common import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCHANGES = [("spans", 1, (1, 1)), ("spans", 2, (1, 2)), ("direct", 1, (1, 1))]      # (exchange, groups, (root_rounds, rounds))
# the apps whose kernels write alpha = 1 and render without bound resources, as the slab tests sweep them; and the same with the
# compile-time builds of CLOUDS, VINYL and PLANET, as the point-list and 8-bit tests sweep them
UNIT_ALPHA_APPS = ["clouds", "egg", "raytracer", "atmosphere", "planet", "sdf_ao", "vinyl", "clouds_best", "clouds_ue4"]
POINT_APPS = ["planet", "clouds", "vinyl", "egg", "raytracer", "atmosphere", "sdf_ao", "clouds_best", "clouds_ue4", "clouds_sky",
              "vinyl_gpu", "planet_atmosphere"]


@pytest.fixture(scope="module")
def renderer():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def renderer8():
    """a context of its own that writes SBX_FORMAT_RGBA8 (include/sbx.h sbx_set_output_format): the module's `renderer` stays float"""
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    r.set_output_format("rgba8")
    yield r
    r.close()


@pytest.fixture(scope="module")
def volumes(renderer):
    """two different baked volumes (ddsvolgen's tiled-Worley fBm at two sizes), device + host copies; a test binds them itself"""
    v1 = renderer.worley_volume(32)
    v2 = renderer.worley_volume(16)
    return v1, v2, v1.cpu().numpy(), v2.cpu().numpy()


@pytest.fixture
def variant_restored(renderer):
    """named by a test that switches kernels (sbx_set_variant) between its renders: the module's renderer is back on the default
    kernels however the test ends"""
    yield
    renderer.set_variant(0)


def bind_small_volumes(renderer):
    """clouds_tex renders only once its noise volumes are bound: 16^3 Worley volumes, as the texture tests use"""
    vol = renderer.worley_volume(16)
    renderer.set_noise_volumes(vol, vol)


def frame_cache(fn):
    """fn(*key) computed once per key: a model frame takes seconds to minutes, and the tests of one file share it"""
    frames = {}

    def cached(*key):
        if key not in frames:
            frames[key] = fn(*key)
        return frames[key]
    return cached


def compare(gpu, ref):
    """returns (max_abs_diff over non-NaN-matching channels, #pixels with any bit difference)"""
    both_nan = np.isnan(gpu) & np.isnan(ref)
    d = np.where(both_nan, 0.0, np.abs(gpu.astype(np.float64) - ref.astype(np.float64)))
    d = np.nan_to_num(d, nan=np.inf)
    bits = (gpu.view(np.uint32) != ref.view(np.uint32)) & ~both_nan
    return float(d.max()), int(bits.any(axis=-1).sum())


def bits_differ(a, b):
    """#pixels of two tensors with any bit difference (a NaN differs from a NaN of other bits)"""
    import torch
    return int((a.view(torch.int32) != b.view(torch.int32)).any(dim=-1).sum().item())


def both_variants(r, app, w, h, t, **kw):
    """the frame of the default kernels and of the plain ones (sbx_set_variant 1), as numpy arrays"""
    try:
        r.set_variant(0)
        a = r.render(app, w, h, t, **kw).cpu().numpy()
        r.set_variant(1)
        b = r.render(app, w, h, t, **kw).cpu().numpy()
    finally:
        r.set_variant(0)
    return a, b


def oracle_points(oracle, app, w, h, t, pts, mouse=(0.0, 0.0)):
    """the oracle's mainImage at the fragCoords `pts` -> float32 [n, 4]"""
    from oracle.oracle import APP_IDS
    return np.stack([oracle.main_image(APP_IDS[app], w, h, t, float(x), float(y), mouse=mouse) for x, y in pts])


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)[:3]
        raise AssertionError("%s: %d differing channels, first %s: got %s want %s"
                             % (what, int((~ok).sum()), i.tolist(), [got[tuple(j)] for j in i], [want[tuple(j)] for j in i]))


def same_tensor(a, b, what):
    import torch
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def edge_points(w, h, seed=11):
    """fragCoords that are no pixel centres: inside the frame, around it, beyond 2^24 W (where the quotients of main.h:40 round),
    the corners, the largest finite values, inf and NaN -> float32 [767, 2]"""
    rng = np.random.default_rng(seed)
    big = float(2 ** 24) * w
    return np.concatenate([
        rng.uniform(0, 1, size=(400, 2)) * [w, h],                      # off-centre
        rng.uniform(-3, 4, size=(300, 2)) * [w, h],                     # negative and outside the frame
        rng.uniform(-1, 1, size=(50, 2)) * [big, big * 16],
        [[0, 0], [w, h], [-.5, -.5], [w - .5, h - .5], [-1, 7], [big, 3], [3, -big], [1e30, 1e30], [-3e38, 5], [3e38, -3e38]],
        [[np.inf, 5], [5, -np.inf], [np.inf, np.inf], [np.nan, 5], [5, np.nan], [np.nan, np.nan], [np.inf, np.nan]],
    ]).astype(np.float32)


def check_rows_host_rows_ranks_and_splits(renderer, app, w, h, t, want, cuts, block_rows=8, aux=None):
    """the frame `want`, whole; then the same bits from row ranges cut at `cuts`, from host rows, from every rank of 2 and 3 (gathered
    and assembled, in place with four and three channels) and from slab pieces put together by the root"""
    import torch
    from shaderbox_amd import shard
    br = block_rows
    whole = renderer.render(app, w, h, t, aux=aux)
    assert_same(whole, want, "whole")
    parts = [renderer.render(app, w, h, t, aux=aux, rows=(r0, r1)) for r0, r1 in zip([0] + list(cuts), list(cuts) + [h])]
    same_tensor(torch.cat(parts), whole, "rows")
    host = np.zeros((h, w, 4), dtype=np.float32)
    renderer.render_to_host(app, w, h, t, host, aux=aux)
    assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), "host rows"
    for n in (2, 3):
        for rr, rounds in [(1, 1), (1, 2)]:
            split = dict(aux=aux, root_rounds=rr, rounds=rounds)
            rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
            gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
            for r in range(n):
                renderer.render_rank(app, w, h, t, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], **split)
            frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
            same_tensor(frame, whole, (n, rr, rounds, "rank + assemble"))
            for ch in (4, 3):
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                if ch == 3:
                    inplace[..., 3] = 1.0
                for r in range(n):
                    renderer.render_rank_in_place(app, w, h, t, br, r, n, inplace, channels=ch, **split)
                same_tensor(inplace, whole, (n, rr, rounds, ch, "in place"))
            for ch in (4, 3):                                            # slab pieces, four channels and sbx_render_split_rgb
                slabs = torch.empty((n, rows_max, w, ch), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 0, 5, slabs[r], **split)
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 5, rows_max, slabs[r], **split)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place(app, w, h, t, br, 0, n, root, **split)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                same_tensor(root, whole, (n, rr, rounds, ch, "peers"))


def loop_frame(renderer, app, w, h, t, n, exchange, groups=1, relief=(1, 1), br=8, frames=1):
    """every rank's FramePlan of an n-rank world on this GPU, `frames` frames into the same buffers -> (the last frame, the world)"""
    import torch
    from shaderbox_amd.distributed import LoopbackWorld
    world = LoopbackWorld(n)
    plans = world.plans(renderer, w, h, block_rows=br, groups=groups, root_rounds=relief[0], rounds=relief[1], exchange=exchange)
    out = None
    for _ in range(frames):
        plans[0].frame.fill_(-7.0)                    # every pixel must be written again
        out = LoopbackWorld.render(plans, app, t)
    torch.cuda.synchronize()
    return out, world


def check_loopback_exchanges(renderer, app, n, w, h, t):
    """every rank's schedule of an n-rank world on this GPU, each of EXCHANGES: the one-launch frame"""
    full = renderer.render(app, w, h, t)
    for exchange, groups, relief in EXCHANGES:
        got, _ = loop_frame(renderer, app, w, h, t, n, exchange, groups, relief)
        same_tensor(got, full, (n, exchange, groups, relief))


def check_rgba8(renderer, app, w, h, t, aux=None):
    """SBX_FORMAT_RGBA8 frames are the float frame packed afterwards, alpha 255; returns the float frame"""
    try:
        renderer.set_output_format("rgba32f")
        f = renderer.render(app, w, h, t, aux=aux)
        packed = renderer.pack_unorm8(f, flip_y=False)
        renderer.set_output_format("rgba8")
        got = renderer.render(app, w, h, t, aux=aux)
        assert np.array_equal(got.cpu().numpy(), packed.cpu().numpy())
        assert (got.cpu().numpy()[..., 3] == 255).all()
    finally:
        renderer.set_output_format("rgba32f")
    return f


def check_multi_render(app, w, h, t, want):
    """sbx_multi_render over every visible device; want() is the expected frame, asked for only when the test runs (a model frame
    takes a while, a skip should not)"""
    import torch
    import shaderbox_amd
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("sbx_multi_render across devices needs 2 or more visible GPUs (%d visible)" % ndev)
    m = shaderbox_amd.MultiRenderer(list(range(ndev)))
    try:
        got = m.render(app, w, h, t)
        torch.cuda.synchronize()
        assert_same(got, want(), "multi")
    finally:
        m.close()


# a project that has mainImage(out vec4, in vec2) and the iResolution / iGlobalTime globals of include/sbx_mainimage.hpp
DROPIN = r'''
#include "sbx_mainimage.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
struct vec2 { float x, y; float operator[](int i) const { return i ? y : x; } };
struct vec4 { float v[4]; float& operator[](int i) { return v[i]; } };
int main(int argc, char** argv) {
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    iResolution[0] = (float)W; iResolution[1] = (float)H;
    iGlobalTime = (float)atof(argv[3]);
    std::vector<float> px((size_t)W * H * 4);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            vec4 c;
            mainImage(c, vec2{x + .5f, y + .5f});
            for (int k = 0; k < 4; ++k) px[((size_t)y * W + x) * 4 + k] = c[k];
        }
    FILE* f = fopen(argv[4], "wb");
    fwrite(px.data(), sizeof(float), px.size(), f);
    fclose(f);
    return 0;
}
'''


def check_mainimage_selects(defines, want):
    """include/sbx_mainimage.hpp, preprocessed with -D<define> for each of `defines`, renders the app `want` (its SBX_APP_* name)"""
    r = subprocess.run(["g++", "-std=c++17", "-E", "-P", "-x", "c++"] + ["-D" + d for d in defines] +
                       ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "sbx_mainimage.hpp")],
                       check=True, capture_output=True, text=True)
    assert "sbx_main_image(ctx, %s, &u" % want in r.stdout


def build_dropin(tmp_path, defines, exe_name):
    """DROPIN compiled by plain g++ with -D<define> for each of `defines`, linked with libsbx -> the executable's path"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = tmp_path / "dropin.cpp"
    src.write_text(DROPIN)
    lib = os.path.join(ROOT, "shaderbox_amd", "lib")
    exe = str(tmp_path / exe_name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__"] + ["-D" + d for d in defines] +
                   ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), "-o", exe, str(src), "-L" + lib, "-lsbx",
                    "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return exe


def run_dropin(exe, w, h, t, tmp_path):
    """the frame the drop-in program renders, float32 [h, w, 4]"""
    out = str(tmp_path / "px.f32")
    subprocess.run([exe, str(w), str(h), repr(t), out], check=True, timeout=120)
    return np.fromfile(out, dtype=np.float32).reshape(h, w, 4)


def run_sbx_render(tmp_path, app, w, h, t, flags=()):
    """the frame of host/sbx_render --f32: the file of a one-frame run is the frame's w * h * 4 floats and nothing else
    (host/sbx_render.cpp opens it "wb" and writes the frame once)"""
    exe = os.path.join(ROOT, "host", "sbx_render")
    assert os.path.exists(exe), "host/sbx_render is built by build()"
    out = str(tmp_path / "frame.f32")
    subprocess.run([exe, "--app", app, "--res", "%dx%d" % (w, h), "--time", repr(t), "--f32", out] + list(flags), check=True, timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == w * h * 4
    return raw.reshape(h, w, 4)
