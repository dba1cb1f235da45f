"""GPU tests of SBX_APP_2D / SBX_APP_2D_TEX (src/app_2d.h; include/sbx.h): every layer bit for bit, NaN == NaN, all four channels,
against the numpy restatement of tests/app2d_model.py."""
import ctypes

import numpy as np
import pytest

from tests import app2d_model as M
from tests.app_checks import assert_same, build_dropin, run_dropin
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

TIMES = [0.37, 2.0, 5.5, 9.25, 13.0, 4.0, 8.0, 12.0, 16.37, -3.1, 1000.9]


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_every_pixel(renderer, w, h):
    for t in TIMES:
        assert_same(renderer.render("2d", w, h, t), M.frame(w, h, t), ("2d", w, h, t))


@pytest.mark.parametrize("w,h", [(333, 187), (65, 3), (1, 1)])
def test_odd_and_tiny_sizes(renderer, w, h):
    for t in [0.37, 5.5, 9.25, 13.0, 8.0, -3.1]:
        want = M.frame(w, h, t)
        assert_same(renderer.render("2d", w, h, t), want, ("2d", w, h, t))
        assert_same(renderer.render("2d_tex", w, h, t), M.frame(w, h, t, M.decode_unorm8(M.checkerboard_texture())), ("2d_tex", w, h, t))
    if w % 2 and h % 2:                          # the centre pixel: r = 0 in the tunnel, NaN / Inf flow as data
        c = renderer.render("2d", w, h, 0.37).cpu().numpy()[h // 2, w // 2]
        assert not np.isfinite(c).all() or c[3] == 0, c


def test_texture(renderer):
    import torch
    default = M.decode_unorm8(M.checkerboard_texture())
    rng = np.random.default_rng(2024)
    words = rng.integers(0, 2 ** 32, size=(61, 97), dtype=np.uint64).astype(np.uint32)
    texf = rng.uniform(-2.0, 3.0, size=(23, 40, 4)).astype(np.float32)
    w, h = 640, 360
    for t in TIMES:
        assert_same(renderer.render("2d_tex", w, h, t), M.frame(w, h, t, default), ("default", t))
    dev_words = torch.from_numpy(words.view(np.int32)).to(renderer.tdev)
    renderer.set_texture2d(dev_words)
    for t in TIMES:
        assert_same(renderer.render("2d_tex", w, h, t), M.frame(w, h, t, M.decode_unorm8(words)), ("rgba8 97x61", t))
    # the same texels as a uint8 [h, w, 4] tensor (R in the low byte)
    renderer.set_texture2d(torch.from_numpy(words.view(np.uint8).reshape(61, 97, 4)).to(renderer.tdev))
    assert_same(renderer.render("2d_tex", 1920, 1080, 0.37), M.frame(1920, 1080, 0.37, M.decode_unorm8(words)), "rgba8 u8 view")
    renderer.set_texture2d(torch.from_numpy(texf).to(renderer.tdev))
    for t in TIMES:
        assert_same(renderer.render("2d_tex", w, h, t), M.frame(w, h, t, texf), ("rgba32f 40x23", t))
    # rebinding and the NULL reset take effect in stream order: three frames enqueued back to back, nothing synchronised between
    outs = [torch.empty((h, w, 4), dtype=torch.float32, device=renderer.tdev) for _ in range(3)]
    renderer.set_texture2d(dev_words)
    renderer.render("2d_tex", w, h, 2.0, out=outs[0])
    renderer.set_texture2d(torch.from_numpy(texf).to(renderer.tdev))
    renderer.render("2d_tex", w, h, 2.0, out=outs[1])
    renderer.set_texture2d(None)
    renderer.render("2d_tex", w, h, 2.0, out=outs[2])
    for o, tex, what in zip(outs, [M.decode_unorm8(words), texf, default], ["words", "float", "reset"]):
        assert_same(o, M.frame(w, h, 2.0, tex), what)
    # APP_2D itself never reads t0
    assert_same(renderer.render("2d", w, h, 2.0), M.frame(w, h, 2.0), "2d after binds")


def test_strips_and_host_rows(renderer):
    w, h = 1280, 720
    for app in ["2d", "2d_tex"]:
        for t in [0.37, 5.5, 9.25, 13.0]:
            whole = renderer.render(app, w, h, t)
            parts = [renderer.render(app, w, h, t, rows=(a, b)) for a, b in [(0, 13), (13, 14), (14, 300), (300, h)]]
            import torch
            assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32)), (app, t)
            host = np.zeros((h, w, 4), dtype=np.float32)
            renderer.render_to_host(app, w, h, t, host)
            assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), (app, t)


def test_rgba8_frames(renderer):
    import shaderbox_amd
    w, h = 800, 450
    try:
        for app in ["2d", "2d_tex"]:
            for t in [0.37, 5.5, 9.25, 13.0, 8.0]:
                renderer.set_output_format("rgba32f")
                f = renderer.render(app, w, h, t)
                packed = renderer.pack_unorm8(f, flip_y=False)
                renderer.set_output_format("rgba8")
                got = renderer.render(app, w, h, t)
                assert np.array_equal(got.cpu().numpy(), packed.cpu().numpy()), (app, t)
                if app == "2d" and t == 0.37:                      # the alpha byte is the app's, not 255
                    assert len(np.unique(got.cpu().numpy()[..., 3])) > 10
    finally:
        renderer.set_output_format("rgba32f")
    assert shaderbox_amd.SBX_FORMAT_RGBA8 == 1


def test_points_and_main_image(renderer):
    import torch
    w, h = 1920, 1080
    rng = np.random.default_rng(7)
    pts = np.concatenate([
        rng.uniform(0, 1, size=(500, 2)) * [w, h],                      # off-centre
        rng.uniform(-3, 4, size=(300, 2)) * [w, h],                     # out of frame
        [[w / 2, h / 2], [0, 0], [-1e30, 5], [1e20, -1e20], [w / 2, 1e-3], [3e38, 3e38]],
    ]).astype(np.float32)
    for app, tex in [("2d", None), ("2d_tex", M.decode_unorm8(M.checkerboard_texture()))]:
        for t in [0.37, 5.5, 9.25, 13.0, 12.0]:
            want = M.main_image(w, h, t, pts[:, 0], pts[:, 1], tex)
            got = renderer.render_points(app, w, h, t, torch.from_numpy(pts))
            assert_same(got, want, (app, t, "points"))
            batch = renderer.main_image_batch(app, w, h, t, pts[:64])
            assert_same(batch, want[:64], (app, t, "batch"))
            for i in [0, 1, 500, 801, 804]:
                c = renderer.main_image(app, w, h, t, (float(pts[i, 0]), float(pts[i, 1])))
                assert_same(np.asarray(c, dtype=np.float32), want[i], (app, t, "main_image", i))
            c = renderer.main_image(app, w, h, t, (10.5, 20.5))      # a pixel centre: served from the cached frame
            assert_same(np.asarray(c, dtype=np.float32), M.frame(w, h, t, tex, rows=[20])[0, 10], (app, t, "centre"))


def test_split_forms_and_refusals(renderer):
    import torch
    import shaderbox_amd
    from shaderbox_amd import shard
    lib, ctx = renderer.lib, renderer.ctx
    w, h, br, n = 640, 360, 8, 3
    for app in ["2d", "2d_tex"]:
        aid = shaderbox_amd.app_id(app)
        for t in [0.37, 5.5, 9.25, 13.0]:
            whole = renderer.render(app, w, h, t)
            for rr, rounds in [(1, 1), (1, 2)]:
                rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
                gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank(app, w, h, t, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], root_rounds=rr, rounds=rounds)
                frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
                assert torch.equal(frame.view(torch.int32), whole.view(torch.int32)), (app, t, rr, rounds, "rank + assemble")
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_in_place(app, w, h, t, br, r, n, inplace, root_rounds=rr, rounds=rounds)
                assert torch.equal(inplace.view(torch.int32), whole.view(torch.int32)), (app, t, rr, rounds, "in place")
                # slab pieces (sbx_render_split with a row range) and the 4-channel peer assembly
                slabs = torch.empty((n, rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 0, 5, slabs[r], root_rounds=rr, rounds=rounds)
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 5, rows_max, slabs[r], root_rounds=rr, rounds=rounds)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place(app, w, h, t, br, 0, n, root, root_rounds=rr, rounds=rounds)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                assert torch.equal(root.view(torch.int32), whole.view(torch.int32)), (app, t, rr, rounds, "peers")
        # every entry point that carries R, G, B only refuses, and writes nothing
        u = renderer.uniforms(w, h, 0.37)
        st = renderer._stream()
        sentinel = torch.full((h * w * 4 + 64,), 1234.5, dtype=torch.float32, device=renderer.tdev)
        p = ctypes.c_void_p(sentinel.data_ptr())
        calls = {
            "split_rgb": lambda: lib.sbx_render_split_rgb(ctx, aid, ctypes.byref(u), None, br, 1, n, 1, 1, 0, 1 << 20, p, st),
            "split_in_place_rgb": lambda: lib.sbx_render_split_in_place_rgb(ctx, aid, ctypes.byref(u), None, br, 1, n, 1, 1, p, st),
            "span_peer": lambda: lib.sbx_render_span_peer(ctx, aid, ctypes.byref(u), None, br, 1, n, 1, 1, 0, 1 << 20, p, st),
            "span_peer_in_place_3": lambda: lib.sbx_render_span_peer_in_place(ctx, aid, ctypes.byref(u), None, br, 1, n, 1, 1, 3, p, st),
            "span_root": lambda: lib.sbx_render_span_root(ctx, aid, ctypes.byref(u), None, br, n, 1, 1, p, st),
            "assemble_spans": lambda: lib.sbx_assemble_spans(ctx, aid, ctypes.byref(u), None, br, n, 1, 1, p, ctypes.c_int64(w * h), p, st),
        }
        for name, call in calls.items():
            assert call() == shaderbox_amd.SBX_ERR_UNSUPPORTED, (app, name)
        with pytest.raises(shaderbox_amd.SbxError) as e:
            renderer.render_rank_rows(app, w, h, 0.37, br, 1, n, 0, 8, sentinel[:8 * w * 3].view(8, w, 3))
        assert e.value.code == shaderbox_amd.SBX_ERR_UNSUPPORTED
        m = shaderbox_amd.MultiRenderer([0, 0])
        try:
            with pytest.raises(shaderbox_amd.SbxError) as e:
                m.render(app, w, h, 0.37, out=sentinel[:h * w * 4].view(h, w, 4))
            assert e.value.code == shaderbox_amd.SBX_ERR_UNSUPPORTED
        finally:
            m.close()
        torch.cuda.synchronize()
        assert bool((sentinel == 1234.5).all()), app


def test_bad_texture_arguments(renderer):
    import torch
    import shaderbox_amd
    buf = torch.zeros((64, 64, 4), dtype=torch.float32, device=renderer.tdev)
    p, st = ctypes.c_void_p(buf.data_ptr()), renderer._stream()
    for wd, ht, fmt in [(0, 4, 0), (4, 0, 1), (16385, 1, 1), (1, 16385, 0), (-3, 4, 0), (4, 4, 2), (4, 4, -1), (4, 4, 7)]:
        assert renderer.lib.sbx_set_texture2d(renderer.ctx, wd, ht, fmt, p, st) == shaderbox_amd.SBX_ERR_ARG, (wd, ht, fmt)
    assert renderer.lib.sbx_set_texture2d(None, 4, 4, 0, p, st) == shaderbox_amd.SBX_ERR_ARG
    # a refused bind leaves the default in place
    assert_same(renderer.render("2d_tex", 96, 54, 0.37), M.frame(96, 54, 0.37, M.decode_unorm8(M.checkerboard_texture())), "after refusals")


def test_cpp_dropin(tmp_path):
    for define, tex in [("APP_2D", None), ("APP_2D_TEX", M.decode_unorm8(M.checkerboard_texture()))]:
        exe = build_dropin(tmp_path, [define], define)
        for w, h, t in [(320, 180, 0.37), (97, 61, 9.25), (64, 48, 13.0)]:
            assert_same(run_dropin(exe, w, h, t, tmp_path), M.frame(w, h, t, tex), (define, w, h, t))
