"""The build families: apps that are one reference shader header with one compile-time switch the other way.
Plain data, stated once, imported by tools/make_golden_builds.py (which records the fixtures under these conditions),
tools/time_builds.py, tests/model_common.py builds_fixture() (which decodes them) and the CPU tests (which assert the same conditions
of the committed files).  A new family is one entry here, a model file and that model's own tests.  Nothing of the project is
imported.

Per family:
    header, ref_defs   the reference header and the REF_DEFS that oracle/Makefile gives it
    shipped            (app name, id in the oracle and in include/sbx.h) of the header as shipped
    builds             per build: app (lower-case name), name (the APP_* define; SBX_APP_* in sbx.h), value (the enum's), edit =
                       (line number, the line as it is, the line as it becomes or None: removed), and the caps below
    size, uniforms     the frames: (w, h) and (u_time, u_mouse) per frame
    big                the second, larger frame set, for the builds that state a `min_big`; None: the family has none
    points             size (u_res), time, count, seed, rect (x0, y0, x1, y1 in fragCoord units the points are drawn from; None: the
                       whole frame; a build's own `rect` goes first); None: the family records no points
    storage            "raw": the float frames under `keys`; "xor": the XOR of their rgb bits with the shipped build's frame under the
                       same uniforms (uint32, zero where the builds agree; alpha is 1), under `keys` / `big_keys`.  A key pattern
                       takes the frame's index (%d) or its u_time (%g)
    file               the fixture's name under tests/golden/<family>_builds/, of the build
    frames_as          what builds_fixture() hands out per frame: "array", "whtm" = (w, h, u_time, u_mouse, frame), "named" =
                       (key, u_time, aux set or None, frame)
    max_bytes          "largest": the largest .npz directly under tests/golden/; a number; None: not bounded
    timing             tools/time_builds.py: size, time, apps in the order of a pass, the shipped apps (the first is what the ratios are
                       taken to; all of them are what --baseline-lib times too), kernels = (form, sbx_set_variant value), default
                       launches and passes; dt: also time an animated scene, u_time advancing by dt per launch
Caps, the conditions that keep a fixture from saying nothing (the reference alone meets them), per build unless said otherwise:
    min_pixels         pixels of a frame that differ from the shipped build's: one number, or one per frame
    min_big            the same of a frame of the big set
    max_nan, max_nan_big   the most NaN pixels a frame may hold; family-wide `no_nan`: no NaN in any frame or point
    min_points         points that differ from the shipped build's answers
    printed_points     where no minimum was fixed beforehand: the count the fixture tool printed when it wrote the committed file, of
                       which the test asks for 80 %
"""


def _still(*times):
    return tuple((t, (0.0, 0.0)) for t in times)


FAMILIES = {
    "egg": {
        "header": "app_egg.h", "ref_defs": "-DAPP_EGG '-DSBX_REF_RESET=depth = -max_dist'", "shipped": ("egg", 3),
        "builds": {
            # x0, y0, x1, y1 of the 1920x1080 frame, chosen from the reference alone, from the pixels in which the edited header's
            # frame at u_time 0.02 differs from the shipped header's (tools/make_golden_builds.py egg --find-rects prints their
            # bounding box; 50649 pixels for straight, 7322 for oval).  straight: the box between the 5th and the 95th percentile of
            # those pixels' x and of their y: legs, knees and their shadow.  oval: the differences are a ring a pixel or two wide
            # around the egg's outline, which reaches the top of the frame, and the shadow of its taller top (rows 237-363, 4123 of
            # the pixels).  The ring's bounding box gives 114 of 4096, so the rectangle is the shadow's difference and the lower
            # left of the outline above it, up to row 700.  Measured: straight 128, 135, 100 pixels and 985 points; oval 20, 21, 20
            # and 297
            "straight": {"app": "egg_straight", "name": "APP_EGG_STRAIGHT", "value": 19, "edit": (37, "#define BEZIER", None),
                         "min_pixels": 90, "min_points": 200, "rect": (794, 94, 1209, 533)},
            "oval": {"app": "egg_oval", "name": "APP_EGG_OVAL", "value": 20, "edit": (46, "#if 1", "#if 0"),
                     "min_pixels": 15, "min_points": 200, "rect": (880, 236, 1000, 700)},
        },
        # the turntable (100 degrees per unit, :40) carries the figure out of view for |t| > 0.5.  The scene is flat-shaded, so a
        # whole frame is a weak pin of a thin member: the points carry most of the evidence
        "size": (96, 54), "uniforms": _still(0.0037, 0.02, 0.2), "big": None,
        "points": {"size": (1920, 1080), "time": 0.02, "count": 4096, "seed": 20, "rect": None},
        "storage": "raw", "keys": "t%g", "file": "egg_%s.npz", "frames_as": "array", "no_nan": True, "max_bytes": 100 * 1024,
        # standing: after a few launches the dispatch-order table of the scene is in use (sbx_tile_order.h); animated: the figure in
        # view throughout, k_egg's own hot-first order, no table
        "timing": {"size": (1920, 1080), "time": 0.02, "dt": 1.0 / 600.0, "apps": ("egg", "egg_straight", "egg_oval"), "shipped": ("egg",),
                   "kernels": (("default", 0), ("plain", 1)), "launches": 20, "passes": 5},
    },
    "sdf_ao": {
        "header": "app_sdf_ao.h", "ref_defs": "-DAPP_SDF_AO", "shipped": ("sdf_ao", 6),
        "builds": {
            "shadow": {"app": "sdf_ao_shadow", "name": "APP_SDF_AO_SHADOW", "value": 17, "edit": (269, "#if 0", "#if 1")},
            "normals": {"app": "sdf_ao_normals", "name": "APP_SDF_AO_NORMALS", "value": 18,
                        "edit": (217, "#if 0 // debug: output the raymarching steps", "#if 1 // debug: output the raymarching steps")},
        },
        # u_time turns the camera by 50 degrees per unit (app_sdf_ao.h:47) around a scene whose sun stands still at normalize(1, 2, 1):
        # 18.5, 125 and 230 degrees.  The shadow falls across the ramps and the ground in all three: it changes 68 of 1654 hit pixels
        # at 0.37, 310 of 1653 at 2.5 and 146 of 1653 at 4.6 (62 / 361 / 111 of them in full umbra; tests/test_sdf_ao_builds_cpu.py)
        "size": (64, 36), "uniforms": _still(0.37, 2.5, 4.6), "big": None, "points": None,
        "storage": "raw", "keys": "t%g", "file": "sdf_ao_%s_64x36.npz", "frames_as": "array", "max_bytes": None,
        "render_threads": 4,                        # the others' 8 would do: the value does not enter the pixels
        "timing": {"size": (3840, 2160), "time": 0.37, "apps": ("sdf_ao", "sdf_ao_normals", "sdf_ao_shadow"), "shipped": ("sdf_ao",),
                   "kernels": (("default", 0), ("plain", 1)), "launches": 20, "passes": 5},
    },
    "clouds": {
        "header": "app_clouds.h", "ref_defs": "-DAPP_CLOUDS", "shipped": ("clouds", 1),
        "builds": {
            "height": {"app": "clouds_height", "name": "APP_CLOUDS_HEIGHT", "value": 21, "edit": (97, "#if 0", "#if 1"),
                       "min_pixels": 1500, "min_points": 500},
            "luminance": {"app": "clouds_luminance", "name": "APP_CLOUDS_LUMINANCE", "value": 22, "edit": (118, "#if 0", "#if 1"),
                          "min_pixels": 1500, "min_points": 500},
        },
        "size": (96, 54), "uniforms": _still(0.0, 1.5, 37.25), "big": None,
        # one more frame per aux set of tests/golden/reference_aux_sets.json, at aux_time; `zero` (no march step runs) equals the
        # shipped build bit for bit, the others differ from it
        "aux_time": 1.5, "aux_sets": ("steer", "yz", "degenerate", "zero"),
        # the rows above the horizon cut: point_cam.y >= .2 from row 648, dir.y >= .2 / sqrt(1 + (16/9)^2 + 1) = .088 > .05 (:212)
        "points": {"size": (1920, 1080), "time": 1.5, "count": 2048, "seed": 21, "rect": (0, 648, 1920, 1080)},
        "storage": "xor", "keys": "x_t%g", "file": "clouds_%s.npz", "frames_as": "named", "no_nan": True, "max_bytes": "largest",
    },
    "raytracer": {
        "header": "app_raytracer.h", "ref_defs": "-DAPP_RAYTRACER", "shipped": ("raytracer", 4),
        "builds": {
            # measured: phong 2167, 2198, 2013, 2944 pixels and 1407 points; noshadow 533, 722, 392, 604 and 244; static 4040 each and 2030
            "phong": {"app": "raytracer_phong", "name": "APP_RAYTRACER_PHONG", "value": 23, "edit": (61, "#if 0", "#if 1"),
                      "min_pixels": 1500, "min_points": 500},
            "noshadow": {"app": "raytracer_noshadow", "name": "APP_RAYTRACER_NOSHADOW", "value": 24,
                         "edit": (107, "#if 1 // shadow ray", "#if 0 // shadow ray"), "min_pixels": 250, "min_points": 100},
            # u_time is not read: the three frames of u_mouse (0, 0) are bit-identical
            "static": {"app": "raytracer_static", "name": "APP_RAYTRACER_STATIC", "value": 25, "edit": (29, "#if 1", "#if 0"),
                       "min_pixels": 3500, "min_points": 1500, "equal_frames": (0, 1, 2)},
        },
        # u_mouse (40, 20) turns the camera by 66 degrees
        "size": (64, 64), "uniforms": _still(0.0, 0.37, 2.5) + ((1.5, (40.0, 20.0)),), "big": None,
        "points": {"size": (1920, 1080), "time": 1.5, "count": 2048, "seed": 23, "rect": None},
        "storage": "xor", "keys": "x_frame%d", "file": "raytracer_%s.npz", "frames_as": "whtm", "no_nan": True, "max_bytes": "largest",
        "timing": {"size": (3840, 2160), "time": 1.5, "apps": ("raytracer", "raytracer_phong", "raytracer_noshadow", "raytracer_static"),
                   "shipped": ("raytracer",), "kernels": (("default", 0), ("ieee", 1)), "launches": 20, "passes": 5},
    },
    "vinyl": {
        "header": "app_vinyl.h", "ref_defs": "-DAPP_VINYL -DSBX_ENV_REFLECT", "shipped": ("vinyl", 2), "also_shipped": (("vinyl_gpu", 11),),
        "builds": {
            # NaN pixels are data: sqrt of a negative dotLN * dot(V, N) in the groove shading (:339) gives 1-2 per shipped 64x36 frame
            # and some tens from the close-up camera.  Measured, 64x36 / 128x72 / points: closeup 1541, 1545, 1548, 1531 / - / 1436;
            # ridges 17, 92, 92, 89 / 355, 345 / 92; noshadow 68, 67, 65, 66 / 254, 255 / 76.  NaN pixels: closeup 76, 71, 70, 66; ridges
            # and noshadow 1, 2, 0, 0 and 11, 14 at 128x72
            "closeup": {"app": "vinyl_closeup", "name": "APP_VINYL_CLOSEUP", "value": 26, "edit": (60, "#if 1", "#if 0"),
                        "min_pixels": 1400, "min_points": 1200, "max_nan": 100},
            # the ridge's share depends strongly on the platter angle: at u_time 1.0, 1.5 and 4.0 it is 3-6 pixels, which is why the
            # times below are recorded; at 0.37 it is 17
            "ridges": {"app": "vinyl_ridges", "name": "APP_VINYL_RIDGES", "value": 27, "edit": (357, "#if 0", "#if 1"),
                       "min_pixels": (10, 60, 60, 60), "min_big": 300, "min_points": 60, "max_nan": 4, "max_nan_big": 20},
            "noshadow": {"app": "vinyl_noshadow", "name": "APP_VINYL_NOSHADOW", "value": 28, "edit": (445, "#if 1", "#if 0"),
                         "min_pixels": 50, "min_big": 200, "min_points": 50, "max_nan": 4, "max_nan_big": 20},
        },
        # u_mouse is not read.  closeup differs from the shipped build almost everywhere, so its XOR does not compress: no big set
        "size": (64, 36), "uniforms": _still(0.37, 2.5, -3.7, 7.25), "big": {"size": (128, 72), "uniforms": _still(-3.7, 7.25)},
        "points": {"size": (1920, 1080), "time": 2.5, "count": 2048, "seed": 23, "rect": None},
        "storage": "xor", "keys": "x_frame%d", "big_keys": "x_big%d", "file": "vinyl_%s.npz", "frames_as": "array", "max_bytes": "largest",
        "timing": {"size": (3840, 2160), "time": 0.37, "apps": ("vinyl", "vinyl_gpu", "vinyl_closeup", "vinyl_ridges", "vinyl_noshadow"),
                   "shipped": ("vinyl", "vinyl_gpu"), "kernels": (("default", 0), ("plain", 1)), "launches": 40, "passes": 3},
    },
    "planet": {
        "header": "app_planet.h", "ref_defs": "-DAPP_PLANET", "shipped": ("planet", 0), "also_shipped": (("planet_atmosphere", 12),),
        "mainimage_also": ("APP_PLANET_ATMOSPHERE",),
        "builds": {
            # NaN pixels are data: smoothstep(1 - .3 s, 1 - .2 s, N) with s = 0 is 0 / 0 where N == 1 (:270-273), and a zero normal of
            # the central differences normalises to NaN (:206).  The unlit build takes N = w_normal.y, which is 1 for no hit point of a
            # recorded frame: it has no NaN pixel.  Measured, 64x36 / 128x72: closeup 2304 each / -; cloudless 873, 842, 885, 865 /
            # 3468, 3451; unlit 672, 684, 649, 665 / 2583, 2662.  NaN pixels: closeup 9, 32, 88, 12; cloudless 25, 21, 50, 20 and 212,
            # 75 at 128x72; unlit none
            "closeup": {"app": "planet_closeup", "name": "APP_PLANET_CLOSEUP", "value": 29, "edit": (51, "#if 0", "#if 1"),
                        "min_pixels": 2250, "max_nan": 150, "printed_points": 2047},
            "cloudless": {"app": "planet_cloudless", "name": "APP_PLANET_CLOUDLESS", "value": 30, "edit": (63, "#define CLOUDS", "//#define CLOUDS"),
                          "min_pixels": 750, "min_big": 3000, "max_nan": 100, "max_nan_big": 300, "printed_points": 796},
            "unlit": {"app": "planet_unlit", "name": "APP_PLANET_UNLIT", "value": 31, "edit": (249, "#define LIGHT", "//#define LIGHT"),
                      "min_pixels": 580, "min_big": 2300, "max_nan": 0, "max_nan_big": 0, "printed_points": 659},
        },
        # u_mouse is not read.  closeup differs from the shipped build in every pixel, so its XOR does not compress: no big set
        "size": (64, 36), "uniforms": _still(0.37, 2.5, -3.7, 7.25), "big": {"size": (128, 72), "uniforms": _still(-3.7, 7.25)},
        "points": {"size": (1920, 1080), "time": 2.5, "count": 2048, "seed": 23, "rect": None},
        "storage": "xor", "keys": "x_frame%d", "big_keys": "x_big%d", "file": "planet_%s.npz", "frames_as": "array", "max_bytes": "largest",
        "render_twice": True,                       # the fixture tool renders every frame again and asserts the same bits
        "timing": {"size": (7680, 4320), "time": 0.37, "apps": ("planet", "planet_atmosphere", "planet_closeup", "planet_cloudless", "planet_unlit"),
                   "shipped": ("planet", "planet_atmosphere"), "kernels": (("default", 0), ("plain", 1)), "launches": 20, "passes": 3},
    },
}


def fixture_path(tests_dir, family, build):
    return "%s/golden/%s_builds/%s" % (tests_dir, family, FAMILIES[family]["file"] % build)


def frame_keys(pattern, uniforms):
    """the .npz key of every frame of a set: the pattern takes the frame's index (%d) or its u_time (%g)"""
    return [pattern % (i if "%d" in pattern else t) for i, (t, _) in enumerate(uniforms)]
