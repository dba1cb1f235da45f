// host/sbx_render.cpp — C++ host over the C ABI: renders a frame or an animation on one or several MI355X and writes
// every frame as binary PPM (sRGB 8-bit, top row first) and/or raw float32 RGBA (row 0 = bottom).
//
//   sbx_render --app clouds --res 3840x2160 [--time 0.37] [--frames N --dt S] [--mouse X,Y] [--gpus N [--exchange spans|slabs|blocks]]
//              [--ppm out_%04d.ppm] [--f32 out_%04d.f32] [--rgba8]
//     --rgba8: the kernels write the 8-bit display format themselves (SBX_FORMAT_RGBA8, include/sbx.h): 4 bytes per pixel in
//              HBM, in the multi-GPU exchange and over PCIe; the same .ppm bytes as the float frame packed afterwards; no --f32
//     APP_CLOUDS aux block (the ImGui panel of hlsltoy, util/hlsltoy/src/hlsltoy.cpp:466-483):
//              [--wind x,y,z] [--sun x,y,z] [--sun-color r,g,b] [--sun-power P] [--sky-radius R] [--sky-height Y]
//              [--sigma S] [--coverage C] [--thick T] [--steps N] [--light-steps N]
//     --clouds-panorama W H [--eye X Y Z]: instead of an app's frame, an equirectangular sky of W x H pixels seen from the eye (default
//              0 -.5 0, setup_camera's): every azimuth, elevations from the horizon (row 0) to the zenith, through sbx_clouds_eval
//              "render" (include/sbx.h) with the APP_CLOUDS aux flags and --time / --frames / --dt.  Pixel (x, y) looks along
//              (cos e sin a, sin e, -cos e cos a) with a = 2 pi (x + .5) / W and e = (pi / 2) (y + .5) / H, evaluated in binary64 and
//              rounded.  The frame holds what the entry returns: LINEAR rgb and the clouds' alpha.  One GPU, float pixels.
//     --planet-view W H EX EY EZ LX LY LZ [--fov DEG]: instead of an app's frame, APP_PLANET seen from the caller's camera: the primary
//              rays of main.h's pipeline (main.h:33-46, util.h:5-20) for a W x H frame with eye (EX, EY, EZ), look_at (LX, LY, LZ) and
//              FOV = tan(radians(DEG)) (default 30, app_planet.h:369) are computed here, in binary32 in the reference's order of
//              operations (the tangent: libm's tan of the binary32 angle, evaluated in binary64 and rounded), and go through
//              sbx_planet_eval "render" (include/sbx.h) with --time / --frames / --dt.  The frame holds what the entry returns:
//              LINEAR rgb and the cloud shell's alpha.  One GPU, float pixels.
//     --egg-view W H EX EY EZ LX LY LZ [--fov F]: instead of an app's frame, APP_EGG seen from the caller's camera: the primary rays of
//              main.h's pipeline for a W x H frame with eye (EX, EY, EZ), look_at (LX, LY, LZ) and the FOV factor F (default 1,
//              app_egg.h:253), computed here as for --planet-view, go through sbx_egg_eval "render_scene" (include/sbx.h) under the pose
//              of --time and the pose flags below; then render's bars and abs (app_egg.h:233-251) in binary32 on the host and
//              linear_to_srgb by the library's own form of it (sbx_math_eval "srgb_pow", include/sbx_test.h): the frame
//              SBX_APP_EGG_POSE renders with that camera in its block.  One GPU, float pixels.
//     --vinyl-view W H EX EY EZ LX LY LZ [--fov F]: instead of an app's frame, APP_VINYL seen from the caller's camera: the primary rays of
//              main.h's pipeline, computed here as for --egg-view (F: the FOV factor, default 1, app_vinyl.h:460), go through
//              sbx_vinyl_eval "render" (include/sbx.h) under the deck of --time and the deck flags below; then linear_to_srgb by the
//              library's own form of it (sbx_math_eval "srgb_pow"): the frame SBX_APP_VINYL_DECK renders with that camera in its block.
//              One GPU, float pixels.
//     APP_SDF_AO aux block (:484-487):  [--fog-density D] [--fog-falloff F]
//     app "sdf_ao_shadow" / "sdf_ao_normals": src/app_sdf_ao.h with its `#if 0` at :269 (soft shadows) / :217 (normals view) on; same fog flags
//     app "egg_straight" / "egg_oval": src/app_egg.h without its `#define BEZIER` (:37, cylinder legs) / with its `#if 1` at :46 off (one scaled sphere)
//     app "clouds_height" / "clouds_luminance": src/app_clouds.h with the `#if 0` of illuminate_volume at :97 (lit by height, no light march) /
//              at :118 (the light march's transmittance itself) on; every APP_CLOUDS aux flag applies
//     app "raytracer_phong" / "raytracer_noshadow" / "raytracer_static": src/app_raytracer.h with its `#if 0` at :61 on (Phong lighting) /
//              its `#if 1` at :107 off (no shadow ray) / its `#if 1` at :29 off (the scene at rest: --time does not enter)
//     app "vinyl_closeup" / "vinyl_ridges" / "vinyl_noshadow": src/app_vinyl.h with its `#if 1` at :60 off (the close-up camera) /
//              its `#if 0` at :357 on (the ridge of label and logo) / its `#if 1` at :445 off (no shadow march); 60 march steps each
//     app "planet_closeup" / "planet_cloudless" / "planet_unlit": src/app_planet.h with its `#if 0` at :51 on (the camera of :52-53) /
//              without its `#define CLOUDS` at :63 (no cloud march, no cloud shadow) / without its `#define LIGHT` at :249 (unlit terrain)
//     app "raytracer_scene": src/app_raytracer.h's render over the caller's scene (SBX_APP_RAYTRACER_SCENE, include/sbx.h):
//              --scene-bin FILE   the raw 1376 bytes of an sbx_aux_raytracer_scene (any other size is refused); without it the
//              Cornell box of --time and --mouse (sbx_raytracer_scene_cornell), SBX_APP_RAYTRACER's frame
//     app "sdf_scene": src/app_sdf_ao.h's renderer over the caller's field (SBX_APP_SDF_SCENE, include/sbx.h):
//              --scene-bin FILE   the raw 2784 bytes of an sbx_aux_sdf_scene (any other size is refused); without it the ramp block
//              of --time (sbx_sdf_scene_ramp)
//     app "egg_pose": src/app_egg.h as shipped with the rider posed by the caller (SBX_APP_EGG_POSE, include/sbx.h).  The block starts as
//              the pose of --time (sbx_egg_pose_default) and every flag replaces one field of sbx_aux_egg_pose:
//              [--pose-eye x,y,z] [--pose-look-at x,y,z] [--pose-fov F] [--turn DEG] [--left-foot x,y,z] [--right-foot x,y,z]
//              [--femur L] [--tibia L]
//     app "vinyl_deck": src/app_vinyl.h as shipped over the caller's deck (SBX_APP_VINYL_DECK, include/sbx.h).  The block starts as the deck of
//              --time (sbx_vinyl_deck_default) and every flag replaces one field of sbx_aux_vinyl_deck, so --platter-deg over a frame
//              sequence is the scratching hand:
//              [--deck-eye x,y,z] [--deck-look-at x,y,z] [--deck-fov F] [--platter-deg DEG] [--platter-tilt DEG] [--arm-tilt DEG]
//              [--deck-sun x,y,z] [--groove-color r,g,b] [--dead-wax-color r,g,b] [--label-color r,g,b] [--logo-color r,g,b]
//              [--shiny-color r,g,b] [--ro-spec V] [--a-x V] [--a-y V] [--shininess V]
//     app "atmosphere_air": src/app_atmosphere.h over the caller's air (SBX_APP_ATMOSPHERE_AIR, include/sbx.h).  The block starts as the default
//              of --time and --air-view (sbx_atmosphere_air_default) and every flag replaces one field of sbx_aux_atmosphere_air:
//              [--air-view 0|1] [--air-samples N] [--air-samples-light N] [--air-eye x,y,z] [--air-fov F] [--air-look-at x,y,z]
//              [--air-hg-g G] [--air-sun x,y,z] [--air-sun-power P] [--air-beta-r r,g,b] [--air-h-r H] [--air-beta-m r,g,b] [--air-h-m H]
//              [--air-earth-radius R] [--air-atmosphere-radius R]
//     app "planet_world": src/app_planet.h over the caller's world (SBX_APP_PLANET_WORLD, include/sbx.h).  The block starts as the default of
//              --time (sbx_planet_world_default) and every flag replaces one field of sbx_aux_planet_world, --world-<field with '-' for '_'>:
//              [--world-eye x,y,z] [--world-fov F] [--world-look-at x,y,z] [--world-tilt-deg D] [--world-sun-dir x,y,z] [--world-spin-deg D]
//              [--world-key-color r,g,b] [--world-cloud-spin-deg D] [--world-terrain-offset x,y,z] [--world-max-height V]
//              [--world-cloud-offset x,y,z] [--world-cld-coverage V] [--world-band a,b,c] [--world-cld-fuzzy V] [--world-c-water r,g,b]
//              [--world-l-water V] [--world-c-grass r,g,b] [--world-l-shore V] [--world-c-beach r,g,b] [--world-l-grass V]
//              [--world-c-rock r,g,b] [--world-l-rock V] [--world-c-snow r,g,b] [--world-absorb V] [--world-cloud-light V]
//              [--world-terr-steps N] [--world-cloud-steps N] [--world-shadow-steps N]
//     app "2d" / "2d_tex": src/app_2d.h (its alpha is not 1: the .f32 frames carry it; single GPU only), the USE_TEXTURE build
//              reading hlsltoy's default 128x128 checkerboard at t0
//     app "func": src/app_func.h, the tiled Worley fBm of its compiled 2D branch (grey, alpha 1; u_time and --mouse do not enter)
//     app "atmosphere_ground": src/app_atmosphere.h without FROM_SPACE, the camera one metre above the ground (--mouse does not enter)
//     APP_CLOUDS with USE_NOISE_TEX (app "clouds_tex"; hlsltoy's argv[2], argv[3], hlsltoy.cpp:227-238):
//              --noise-tex shape.dds,detail.dds   (DX10 RGBA32F volume .dds as util/ddsvolgen / sbx_ddsvolgen write)
//              --noise-tex bake:128,64            (bake the two volumes here with sbx_worley_volume)
//
// Plays the role of the reference's frame-granular hosts (hlsltoy.cpp:494-516: draw, advance u_time, re-upload the
// uniform blocks): frame f is rendered at u_time = time + f * dt with the aux values given on the command line, and
// every frame of --frames N is written (a printf pattern in the file name numbers the frames; without one "_%04d" is put
// before the extension when N > 1).  --gpus N shards every frame over N GPUs inside the library (sbx_multi_*).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/sbx.h"
#include "../include/sbx_test.h"      // sbx_math_eval "srgb_pow": --egg-view's linear_to_srgb

// the flags of --app planet_world: one per field of sbx_aux_planet_world, in the block's order (word = its offset in 4-byte words)
struct WorldFlag { const char* name; int word; char kind; };      // kind: 'v' three floats, 'f' one float, 'i' one int
static const WorldFlag kWorldFlags[] = {
    {"--world-eye", 0, 'v'}, {"--world-fov", 3, 'f'}, {"--world-look-at", 4, 'v'}, {"--world-tilt-deg", 7, 'f'},
    {"--world-sun-dir", 8, 'v'}, {"--world-spin-deg", 11, 'f'}, {"--world-key-color", 12, 'v'}, {"--world-cloud-spin-deg", 15, 'f'},
    {"--world-terrain-offset", 16, 'v'}, {"--world-max-height", 19, 'f'}, {"--world-cloud-offset", 20, 'v'}, {"--world-cld-coverage", 23, 'f'},
    {"--world-band", 24, 'v'}, {"--world-cld-fuzzy", 27, 'f'}, {"--world-c-water", 28, 'v'}, {"--world-l-water", 31, 'f'},
    {"--world-c-grass", 32, 'v'}, {"--world-l-shore", 35, 'f'}, {"--world-c-beach", 36, 'v'}, {"--world-l-grass", 39, 'f'},
    {"--world-c-rock", 40, 'v'}, {"--world-l-rock", 43, 'f'}, {"--world-c-snow", 44, 'v'}, {"--world-absorb", 47, 'f'},
    {"--world-cloud-light", 48, 'f'}, {"--world-terr-steps", 49, 'i'}, {"--world-cloud-steps", 50, 'i'}, {"--world-shadow-steps", 51, 'i'}};
constexpr int kWorldFlagCount = (int)(sizeof(kWorldFlags) / sizeof(kWorldFlags[0]));
static_assert(sizeof(sbx_aux_planet_world) == 56 * 4, "kWorldFlags addresses the block by words");

static int app_from_name(const std::string& s) {
    const char* names[] = {"planet", "clouds", "vinyl", "egg", "raytracer", "atmosphere", "sdf_ao", "clouds_best", "clouds_tex", "clouds_ue4",
                           "clouds_sky", "vinyl_gpu", "planet_atmosphere", "2d", "2d_tex", "func", "atmosphere_ground", "sdf_ao_shadow", "sdf_ao_normals",
                           "egg_straight", "egg_oval", "clouds_height", "clouds_luminance", "raytracer_phong", "raytracer_noshadow", "raytracer_static",
                           "vinyl_closeup", "vinyl_ridges", "vinyl_noshadow", "planet_closeup", "planet_cloudless", "planet_unlit", "raytracer_scene", "sdf_scene", "egg_pose", "vinyl_deck",
                           "atmosphere_air", "planet_world"};
    const int n = 38;
    std::string low;
    for (char c : s) low += (char)tolower(c);
    for (int i = 0; i < n; ++i)
        if (low == names[i] || low == std::string("app_") + names[i]) return i;
    return -1;
}

// A file-name pattern may hold ONE integer conversion (%d, %4d, %04d ...) and any number of "%%"; anything else (%s, %n, a
// second %d) would make the user's string an snprintf format with undefined behaviour, so it is rejected up front.
static bool pattern_ok(const std::string& p) {
    int conversions = 0;
    for (size_t i = 0; i < p.size(); ++i) {
        if (p[i] != '%') continue;
        if (i + 1 < p.size() && p[i + 1] == '%') { ++i; continue; }
        size_t j = i + 1;
        while (j < p.size() && p[j] >= '0' && p[j] <= '9') ++j;      // flag 0 and a width
        if (j >= p.size() || p[j] != 'd' || j - i > 4) return false;
        ++conversions;
        i = j;
    }
    return conversions <= 1;
}
static std::string frame_name(const std::string& pattern, int f, int frames) {
    char buf[4096];
    if (pattern.find('%') != std::string::npos) { snprintf(buf, sizeof(buf), pattern.c_str(), f); return buf; }   // checked in main
    if (frames <= 1) return pattern;
    const size_t dot = pattern.rfind('.');
    snprintf(buf, sizeof(buf), "%s_%04d%s", pattern.substr(0, dot).c_str(), f, dot == std::string::npos ? "" : pattern.substr(dot).c_str());
    return buf;
}

// a DX10 volume .dds with RGBA32F texels (what ddsvolgen writes): magic, 124-byte header, 20-byte DX10 header, texels
static bool read_dds_volume(const std::string& path, int& size, std::vector<float>& rgba) {
    FILE* fp = fopen(path.c_str(), "rb");
    if (!fp) { perror(path.c_str()); return false; }
    uint32_t head[37];                                        // 4 + 124 + 20 bytes
    bool ok = fread(head, 4, 37, fp) == 37 && head[0] == 0x20534444u && head[1] == 124 && head[21] == 0x30315844u /* DX10 */ &&
              head[32] == 2 /* R32G32B32A32_FLOAT */ && head[33] == 4 /* TEXTURE3D */;
    if (ok) {
        const uint32_t h = head[3], w = head[4], d = head[6];
        ok = h == w && w == d && w > 0 && w <= 1024;
        if (ok) {
            size = (int)w;
            rgba.resize((size_t)w * w * w * 4);
            ok = fread(rgba.data(), 16, (size_t)w * w * w, fp) == (size_t)w * w * w;
        }
    }
    fclose(fp);
    if (!ok) fprintf(stderr, "%s: not a cubic RGBA32F DX10 volume .dds\n", path.c_str());
    return ok;
}

int main(int argc, char** argv) {
    std::string app = "clouds", ppm, f32, noise_tex, scene_bin;
    int W = 1280, H = 720, frames = 1, gpus = 1, exchange = SBX_MULTI_EXCHANGE_SPANS;
    float t = 0.37f, dt = 1.f / 30.f, mx = 0, my = 0;
    sbx_aux_clouds ac;
    sbx_aux_sdf_ao as;
    sbx_aux_clouds_defaults(&ac);
    sbx_aux_sdf_ao_defaults(&as);
    bool have_ac = false, have_as = false, rgba8_out = false, panorama = false, planet_view = false;
    float eye[3] = {0.f, -.5f, 0.f};
    float pv_eye[3] = {0.f, 0.f, -2.5f}, pv_look[3] = {0.f, 0.f, 2.f}, pv_fov = 0.f;      // --fov: degrees for --planet-view (30), the factor for --egg-view (1)
    bool egg_view = false, have_fov = false;
    sbx_aux_egg_pose pose_arg{};                     // the fields the pose flags gave, and which
    bool pose_has[8] = {false, false, false, false, false, false, false, false};      // eye, fov, look_at, turn, left foot, femur, right foot, tibia
    bool vinyl_view = false;
    sbx_aux_vinyl_deck deck_arg{};                   // the fields the deck flags gave, and which (in the block's order: sbx.h)
    bool deck_has[16] = {};
    sbx_aux_atmosphere_air air_arg{};                // the fields the air flags gave, and which (air_has[0-2]: view and the counts; then the
    bool air_has[15] = {};                           // six rows of a vec3 and a scalar, then the two radii)
    sbx_aux_planet_world world_arg{};                // the fields the world flags gave, and which (kWorldFlags' order)
    bool world_has[kWorldFlagCount] = {};
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        auto vec3 = [&](float* v) { if (sscanf(next(), "%f,%f,%f", v, v + 1, v + 2) != 3) { fprintf(stderr, "%s x,y,z\n", a.c_str()); exit(2); } };
        if (a == "--app") app = next();
        else if (a == "--res") { if (sscanf(next(), "%dx%d", &W, &H) != 2) { fprintf(stderr, "--res WxH\n"); return 2; } }
        else if (a == "--time") t = (float)atof(next());
        else if (a == "--dt") dt = (float)atof(next());
        else if (a == "--frames") frames = atoi(next());
        else if (a == "--gpus") gpus = atoi(next());
        else if (a == "--exchange") {
            const std::string v = next();
            exchange = v == "slabs" ? SBX_MULTI_EXCHANGE_SLABS : v == "blocks" ? SBX_MULTI_EXCHANGE_BLOCKS : v == "spans" ? SBX_MULTI_EXCHANGE_SPANS : -1;
            if (exchange < 0) { fprintf(stderr, "--exchange slabs|blocks|spans\n"); return 2; }
        }
        else if (a == "--mouse") { if (sscanf(next(), "%f,%f", &mx, &my) != 2) { fprintf(stderr, "--mouse X,Y\n"); return 2; } }
        else if (a == "--ppm") ppm = next();
        else if (a == "--f32") f32 = next();
        else if (a == "--rgba8") rgba8_out = true;
        else if (a == "--noise-tex") noise_tex = next();
        else if (a == "--scene-bin") scene_bin = next();
        else if (a == "--clouds-panorama") { W = atoi(next()); H = atoi(next()); panorama = true; }
        else if (a == "--eye") { for (float& v : eye) v = (float)atof(next()); }
        else if (a == "--planet-view") {
            W = atoi(next()); H = atoi(next());
            for (float& v : pv_eye) v = (float)atof(next());
            for (float& v : pv_look) v = (float)atof(next());
            planet_view = true;
        }
        else if (a == "--egg-view") {
            W = atoi(next()); H = atoi(next());
            for (float& v : pv_eye) v = (float)atof(next());
            for (float& v : pv_look) v = (float)atof(next());
            egg_view = true;
        }
        else if (a == "--vinyl-view") {
            W = atoi(next()); H = atoi(next());
            for (float& v : pv_eye) v = (float)atof(next());
            for (float& v : pv_look) v = (float)atof(next());
            vinyl_view = true;
        }
        else if (a.rfind("--world-", 0) == 0) {
            int k = 0;
            while (k < kWorldFlagCount && a != kWorldFlags[k].name) ++k;
            if (k == kWorldFlagCount) { fprintf(stderr, "unknown world flag %s\n", a.c_str()); return 2; }
            float* const wf = (float*)&world_arg + kWorldFlags[k].word;
            if (kWorldFlags[k].kind == 'v') vec3(wf);
            else if (kWorldFlags[k].kind == 'f') *wf = (float)atof(next());
            else { const int v = atoi(next()); memcpy(wf, &v, sizeof(v)); }
            world_has[k] = true;
        }
        else if (a == "--air-view") { air_arg.view = atoi(next()); air_has[0] = true; }
        else if (a == "--air-samples") { air_arg.num_samples = atoi(next()); air_has[1] = true; }
        else if (a == "--air-samples-light") { air_arg.num_samples_light = atoi(next()); air_has[2] = true; }
        else if (a == "--air-eye") { vec3(air_arg.eye); air_has[3] = true; }
        else if (a == "--air-fov") { air_arg.fov = (float)atof(next()); air_has[4] = true; }
        else if (a == "--air-look-at") { vec3(air_arg.look_at); air_has[5] = true; }
        else if (a == "--air-hg-g") { air_arg.hg_g = (float)atof(next()); air_has[6] = true; }
        else if (a == "--air-sun") { vec3(air_arg.sun_dir); air_has[7] = true; }
        else if (a == "--air-sun-power") { air_arg.sun_power = (float)atof(next()); air_has[8] = true; }
        else if (a == "--air-beta-r") { vec3(air_arg.betaR); air_has[9] = true; }
        else if (a == "--air-h-r") { air_arg.hR = (float)atof(next()); air_has[10] = true; }
        else if (a == "--air-beta-m") { vec3(air_arg.betaM); air_has[11] = true; }
        else if (a == "--air-h-m") { air_arg.hM = (float)atof(next()); air_has[12] = true; }
        else if (a == "--air-earth-radius") { air_arg.earth_radius = (float)atof(next()); air_has[13] = true; }
        else if (a == "--air-atmosphere-radius") { air_arg.atmosphere_radius = (float)atof(next()); air_has[14] = true; }
        else if (a == "--deck-eye") { vec3(deck_arg.eye); deck_has[0] = true; }
        else if (a == "--deck-fov") { deck_arg.fov = (float)atof(next()); deck_has[1] = true; }
        else if (a == "--deck-look-at") { vec3(deck_arg.look_at); deck_has[2] = true; }
        else if (a == "--platter-deg") { deck_arg.platter_deg = (float)atof(next()); deck_has[3] = true; }
        else if (a == "--deck-sun") { vec3(deck_arg.sun_dir); deck_has[4] = true; }
        else if (a == "--platter-tilt") { deck_arg.platter_tilt_deg = (float)atof(next()); deck_has[5] = true; }
        else if (a == "--groove-color") { vec3(deck_arg.groove_color); deck_has[6] = true; }
        else if (a == "--arm-tilt") { deck_arg.arm_tilt_deg = (float)atof(next()); deck_has[7] = true; }
        else if (a == "--dead-wax-color") { vec3(deck_arg.dead_wax_color); deck_has[8] = true; }
        else if (a == "--ro-spec") { deck_arg.ro_spec = (float)atof(next()); deck_has[9] = true; }
        else if (a == "--label-color") { vec3(deck_arg.label_color); deck_has[10] = true; }
        else if (a == "--a-x") { deck_arg.a_x = (float)atof(next()); deck_has[11] = true; }
        else if (a == "--logo-color") { vec3(deck_arg.logo_color); deck_has[12] = true; }
        else if (a == "--a-y") { deck_arg.a_y = (float)atof(next()); deck_has[13] = true; }
        else if (a == "--shiny-color") { vec3(deck_arg.shiny_color); deck_has[14] = true; }
        else if (a == "--shininess") { deck_arg.shininess = (float)atof(next()); deck_has[15] = true; }
        else if (a == "--fov") { pv_fov = (float)atof(next()); have_fov = true; }
        else if (a == "--pose-eye") { vec3(pose_arg.eye); pose_has[0] = true; }
        else if (a == "--pose-fov") { pose_arg.fov = (float)atof(next()); pose_has[1] = true; }
        else if (a == "--pose-look-at") { vec3(pose_arg.look_at); pose_has[2] = true; }
        else if (a == "--turn") { pose_arg.turn_deg = (float)atof(next()); pose_has[3] = true; }
        else if (a == "--left-foot") { vec3(pose_arg.left_foot); pose_has[4] = true; }
        else if (a == "--femur") { pose_arg.femur = (float)atof(next()); pose_has[5] = true; }
        else if (a == "--right-foot") { vec3(pose_arg.right_foot); pose_has[6] = true; }
        else if (a == "--tibia") { pose_arg.tibia = (float)atof(next()); pose_has[7] = true; }
        else if (a == "--wind") { vec3(ac.wind_dir); have_ac = true; }
        else if (a == "--sun") { vec3(ac.sun_dir); have_ac = true; }
        else if (a == "--sun-color") { vec3(ac.sun_color); have_ac = true; }
        else if (a == "--sun-power") { ac.sun_power = (float)atof(next()); have_ac = true; }
        else if (a == "--sky-radius") { ac.atm_radius = (float)atof(next()); have_ac = true; }
        else if (a == "--sky-height") { ac.atm_ground_y = (float)atof(next()); have_ac = true; }
        else if (a == "--sigma") { ac.sigma_scattering = (float)atof(next()); have_ac = true; }
        else if (a == "--coverage") { ac.cld_coverage = (float)atof(next()); have_ac = true; }
        else if (a == "--thick") { ac.cld_thick = (float)atof(next()); have_ac = true; }
        else if (a == "--steps") { ac.cld_march_steps = atoi(next()); have_ac = true; }
        else if (a == "--light-steps") { ac.illum_march_steps = atoi(next()); have_ac = true; }
        else if (a == "--fog-density") { as.fog_density = (float)atof(next()); have_as = true; }
        else if (a == "--fog-falloff") { as.fog_falloff = (float)atof(next()); have_as = true; }
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    const int id = app_from_name(app);
    if (id < 0) { fprintf(stderr, "unknown app %s\n", app.c_str()); return 2; }
    if (frames < 1 || gpus < 1) { fprintf(stderr, "--frames and --gpus must be >= 1\n"); return 2; }
    if (rgba8_out && !f32.empty()) { fprintf(stderr, "--rgba8 renders 8-bit pixels: there is no float frame for --f32\n"); return 2; }
    if (panorama && (W < 1 || H < 1)) { fprintf(stderr, "--clouds-panorama W H\n"); return 2; }
    if (panorama && (gpus > 1 || rgba8_out)) { fprintf(stderr, "--clouds-panorama renders float pixels on one GPU\n"); return 2; }
    if (planet_view && (W < 1 || H < 1 || panorama)) { fprintf(stderr, "--planet-view W H EX EY EZ LX LY LZ (not with --clouds-panorama)\n"); return 2; }
    if (planet_view && (gpus > 1 || rgba8_out)) { fprintf(stderr, "--planet-view renders float pixels on one GPU\n"); return 2; }
    if (egg_view && (W < 1 || H < 1 || panorama || planet_view)) { fprintf(stderr, "--egg-view W H EX EY EZ LX LY LZ (not with --clouds-panorama or --planet-view)\n"); return 2; }
    if (egg_view && (gpus > 1 || rgba8_out)) { fprintf(stderr, "--egg-view renders float pixels on one GPU\n"); return 2; }
    const bool pose_flags = pose_has[0] || pose_has[1] || pose_has[2] || pose_has[3] || pose_has[4] || pose_has[5] || pose_has[6] || pose_has[7];
    if (pose_flags && id != SBX_APP_EGG_POSE && !egg_view) { fprintf(stderr, "the pose flags belong to --app egg_pose or --egg-view\n"); return 2; }
    // the pose of frame time `time`: sbx_egg_pose_default's block with the flags' fields put in
    auto pose_at = [&](float time) {
        sbx_uniforms pu{};
        pu.u_res[0] = (float)W; pu.u_res[1] = (float)H; pu.u_time = time;
        sbx_aux_egg_pose p;
        sbx_egg_pose_default(&pu, &p);
        if (pose_has[0]) memcpy(p.eye, pose_arg.eye, sizeof(p.eye));
        if (pose_has[1]) p.fov = pose_arg.fov;
        if (pose_has[2]) memcpy(p.look_at, pose_arg.look_at, sizeof(p.look_at));
        if (pose_has[3]) p.turn_deg = pose_arg.turn_deg;
        if (pose_has[4]) memcpy(p.left_foot, pose_arg.left_foot, sizeof(p.left_foot));
        if (pose_has[5]) p.femur = pose_arg.femur;
        if (pose_has[6]) memcpy(p.right_foot, pose_arg.right_foot, sizeof(p.right_foot));
        if (pose_has[7]) p.tibia = pose_arg.tibia;
        return p;
    };
    if (vinyl_view && (W < 1 || H < 1 || panorama || planet_view || egg_view)) { fprintf(stderr, "--vinyl-view W H EX EY EZ LX LY LZ (not with another view)\n"); return 2; }
    if (vinyl_view && (gpus > 1 || rgba8_out)) { fprintf(stderr, "--vinyl-view renders float pixels on one GPU\n"); return 2; }
    bool deck_flags = false;
    for (bool b : deck_has) deck_flags = deck_flags || b;
    if (deck_flags && id != SBX_APP_VINYL_DECK && !vinyl_view) { fprintf(stderr, "the deck flags belong to --app vinyl_deck or --vinyl-view\n"); return 2; }
    // the deck of frame time `time`: sbx_vinyl_deck_default's block with the flags' fields put in (a vec3 and a scalar per row of the block)
    auto deck_at = [&](float time) {
        sbx_uniforms du{};
        du.u_res[0] = (float)W; du.u_res[1] = (float)H; du.u_time = time;
        sbx_aux_vinyl_deck d;
        sbx_vinyl_deck_default(&du, &d);
        float* dst = (float*)&d;
        const float* src = (const float*)&deck_arg;
        for (int k = 0; k < 16; ++k) {
            if (!deck_has[k]) continue;
            if (k & 1) dst[(k / 2) * 4 + 3] = src[(k / 2) * 4 + 3];
            else memcpy(dst + (k / 2) * 4, src + (k / 2) * 4, 3 * sizeof(float));
        }
        return d;
    };
    bool air_flags = false;
    for (bool b : air_has) air_flags = air_flags || b;
    if (air_flags && id != SBX_APP_ATMOSPHERE_AIR) { fprintf(stderr, "the air flags belong to --app atmosphere_air\n"); return 2; }
    // the air of frame time `time`: sbx_atmosphere_air_default's block of --air-view with the flags' fields put in
    auto air_at = [&](float time) {
        sbx_uniforms du{};
        du.u_res[0] = (float)W; du.u_res[1] = (float)H; du.u_time = time;
        sbx_aux_atmosphere_air d;
        sbx_atmosphere_air_default(&du, air_has[0] ? air_arg.view : 0, &d);
        if (air_has[1]) d.num_samples = air_arg.num_samples;
        if (air_has[2]) d.num_samples_light = air_arg.num_samples_light;
        float* dst = d.eye;                          // the six rows from `eye` on
        const float* src = air_arg.eye;
        for (int k = 0; k < 10; ++k) {
            if (!air_has[3 + k]) continue;
            if (k & 1) dst[(k / 2) * 4 + 3] = src[(k / 2) * 4 + 3];
            else memcpy(dst + (k / 2) * 4, src + (k / 2) * 4, 3 * sizeof(float));
        }
        if (air_has[13]) d.earth_radius = air_arg.earth_radius;
        if (air_has[14]) d.atmosphere_radius = air_arg.atmosphere_radius;
        return d;
    };
    bool world_flags = false;
    for (bool b : world_has) world_flags = world_flags || b;
    if (world_flags && id != SBX_APP_PLANET_WORLD) { fprintf(stderr, "the world flags belong to --app planet_world\n"); return 2; }
    // the world of frame time `time`: sbx_planet_world_default's block with the flags' fields put in
    auto world_at = [&](float time) {
        sbx_uniforms du{};
        du.u_res[0] = (float)W; du.u_res[1] = (float)H; du.u_time = time;
        sbx_aux_planet_world d;
        sbx_planet_world_default(&du, &d);
        for (int k = 0; k < kWorldFlagCount; ++k)
            if (world_has[k])
                memcpy((float*)&d + kWorldFlags[k].word, (const float*)&world_arg + kWorldFlags[k].word, (kWorldFlags[k].kind == 'v' ? 3 : 1) * sizeof(float));
        return d;
    };
    for (const std::string* p : {&ppm, &f32})
        if (!pattern_ok(*p)) { fprintf(stderr, "bad file pattern %s: one %%d / %%0Nd conversion at most, a literal percent as %%%%\n", p->c_str()); return 2; }
    const void* aux = nullptr;
    if ((id == SBX_APP_CLOUDS || id == SBX_APP_CLOUDS_TEX || id == SBX_APP_CLOUDS_SKY || id == SBX_APP_CLOUDS_HEIGHT || id == SBX_APP_CLOUDS_LUMINANCE) && have_ac) aux = &ac;
    if ((id == SBX_APP_SDF_AO || id == SBX_APP_SDF_AO_SHADOW || id == SBX_APP_SDF_AO_NORMALS) && have_as) aux = &as;
    sbx_aux_raytracer_scene scene;
    sbx_aux_sdf_scene sdf_scene;
    if (!scene_bin.empty()) {
        if (id != SBX_APP_RAYTRACER_SCENE && id != SBX_APP_SDF_SCENE) { fprintf(stderr, "--scene-bin belongs to --app raytracer_scene or --app sdf_scene\n"); return 2; }
        void* dst = id == SBX_APP_SDF_SCENE ? (void*)&sdf_scene : (void*)&scene;
        const size_t bytes = id == SBX_APP_SDF_SCENE ? sizeof(sdf_scene) : sizeof(scene);
        FILE* fp = fopen(scene_bin.c_str(), "rb");
        if (!fp) { perror(scene_bin.c_str()); return 1; }
        char extra;
        const bool ok = fread(dst, 1, bytes, fp) == bytes && fread(&extra, 1, 1, fp) == 0;
        fclose(fp);
        if (!ok) { fprintf(stderr, "%s: a scene file holds the %zu bytes of an %s and nothing else\n", scene_bin.c_str(), bytes, id == SBX_APP_SDF_SCENE ? "sbx_aux_sdf_scene" : "sbx_aux_raytracer_scene"); return 2; }
        aux = dst;
    }

    sbx_ctx* ctx = nullptr;
    int rc = sbx_create(0, &ctx);
    if (rc != SBX_OK) { fprintf(stderr, "sbx_create failed (%d): a gfx950 GPU is required, there is no CPU path\n", rc); return 1; }
    sbx_multi* multi = nullptr;
    if (gpus > 1) {
        int ndev = 0;
        (void)hipGetDeviceCount(&ndev);
        std::vector<int> devs(gpus);
        for (int i = 0; i < gpus; ++i) devs[i] = ndev >= gpus ? i : i % (ndev > 0 ? ndev : 1);
        if (ndev < gpus) fprintf(stderr, "note: %d GPU(s) visible, running the %d-rank schedule with ranks sharing devices\n", ndev, gpus);
        rc = sbx_multi_create(gpus, devs.data(), &multi);
        if (rc != SBX_OK) { fprintf(stderr, "sbx_multi_create failed (%d): %s\n", rc, sbx_multi_create_error()); return 1; }
        if ((rc = sbx_multi_set_exchange(multi, exchange)) != SBX_OK) { fprintf(stderr, "exchange: %s\n", sbx_multi_last_error(multi)); return 1; }
        printf("%d ranks, transfers by %s, exchange %s\n", gpus, sbx_multi_uses_rccl(multi) ? "RCCL send/recv" : "device copies",
               exchange == SBX_MULTI_EXCHANGE_SPANS ? "spans" : exchange == SBX_MULTI_EXCHANGE_BLOCKS ? "blocks" : "slabs");
    }
    (void)hipSetDevice(0);
    if (id == SBX_APP_CLOUDS_TEX) {
        if (noise_tex.empty()) { fprintf(stderr, "app clouds_tex needs --noise-tex shape.dds,detail.dds or --noise-tex bake:S1,S2\n"); return 2; }
        int s1 = 0, s2 = 0;
        float *d1 = nullptr, *d2 = nullptr;
        if (noise_tex.rfind("bake:", 0) == 0) {
            if (sscanf(noise_tex.c_str() + 5, "%d,%d", &s1, &s2) != 2 || s1 <= 0 || s2 <= 0) { fprintf(stderr, "--noise-tex bake:S1,S2\n"); return 2; }
            if (hipMalloc((void**)&d1, (size_t)s1 * s1 * s1 * 16) != hipSuccess || hipMalloc((void**)&d2, (size_t)s2 * s2 * s2 * 16) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
            if (sbx_worley_volume(ctx, s1, d1, nullptr) != SBX_OK || sbx_worley_volume(ctx, s2, d2, nullptr) != SBX_OK) { fprintf(stderr, "sbx_worley_volume: %s\n", sbx_last_error(ctx)); return 1; }
        } else {
            const size_t comma = noise_tex.find(',');
            if (comma == std::string::npos) { fprintf(stderr, "--noise-tex shape.dds,detail.dds\n"); return 2; }
            std::vector<float> v1, v2;
            if (!read_dds_volume(noise_tex.substr(0, comma), s1, v1) || !read_dds_volume(noise_tex.substr(comma + 1), s2, v2)) return 1;
            if (hipMalloc((void**)&d1, v1.size() * 4) != hipSuccess || hipMalloc((void**)&d2, v2.size() * 4) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
            (void)hipMemcpy(d1, v1.data(), v1.size() * 4, hipMemcpyHostToDevice);
            (void)hipMemcpy(d2, v2.data(), v2.size() * 4, hipMemcpyHostToDevice);
        }
        (void)hipDeviceSynchronize();
        rc = multi ? sbx_multi_set_noise_volumes(multi, s1, d1, s2, d2) : sbx_set_noise_volumes(ctx, s1, d1, s2, d2, nullptr);
        if (rc != SBX_OK) { fprintf(stderr, "noise volumes: %s\n", multi ? sbx_multi_last_error(multi) : sbx_last_error(ctx)); return 1; }
        (void)hipDeviceSynchronize();
        (void)hipFree(d1); (void)hipFree(d2);
    }
    if (rgba8_out) {
        rc = multi ? sbx_multi_set_output_format(multi, SBX_FORMAT_RGBA8) : sbx_set_output_format(ctx, SBX_FORMAT_RGBA8);
        if (rc != SBX_OK) { fprintf(stderr, "output format: %s\n", multi ? sbx_multi_last_error(multi) : sbx_last_error(ctx)); return 1; }
    }
    // the frame, the 8-bit copy and the timing events belong to rank 0's device (the sbx_multi_* calls leave it current;
    // set again here so that nothing below depends on that)
    (void)hipSetDevice(0);
    const size_t n = (size_t)W * H * 4, npx = (size_t)W * H;
    float* dev = nullptr;
    unsigned char* dev8 = nullptr;
    if (hipMalloc((void**)&dev, (rgba8_out ? npx : n) * sizeof(float)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }   // (--rgba8: one word per pixel)
    if (!ppm.empty() && !rgba8_out && hipMalloc((void**)&dev8, npx * 4) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    std::vector<float> host(f32.empty() ? 0 : n);
    std::vector<unsigned char> rgba8(ppm.empty() ? 0 : npx * 4), rgb(ppm.empty() ? 0 : npx * 3);
    float* rays = nullptr;
    if (panorama) {
        std::vector<float> hr(npx * 6);
        const double pi = 3.14159265358979323846;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const double az = 2.0 * pi * (x + .5) / W, el = .5 * pi * (y + .5) / H;
                float* r = &hr[((size_t)y * W + x) * 6];
                r[0] = eye[0]; r[1] = eye[1]; r[2] = eye[2];
                r[3] = (float)(cos(el) * sin(az)); r[4] = (float)sin(el); r[5] = (float)(-cos(el) * cos(az));
            }
        if (hipMalloc((void**)&rays, hr.size() * sizeof(float)) != hipSuccess ||
            hipMemcpy(rays, hr.data(), hr.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    }
    std::vector<float> view_pcx;                     // --egg-view: point_cam.x of every pixel, for the bars
    float *lin = nullptr, *srgb = nullptr;          // --egg-view: the linear colours (3 floats a pixel) and their sRGB form, on the device
    float* vout = nullptr;                          // --vinyl-view: what "render" returns, 5 floats a pixel
    if (planet_view || egg_view || vinyl_view) {
        // main.h:33-46 and util.h:5-20 in binary32, operation by operation (dot = (x x + y y) + z z, normalize = three divisions by the root)
        struct V { float x, y, z; };
        auto dot3 = [](V a, V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };
        auto norm3 = [&](V v) { const float l = sqrtf(dot3(v, v)); return V{v.x / l, v.y / l, v.z / l}; };
        auto cross3 = [](V a, V b) { return V{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; };
        const float fov = (egg_view || vinyl_view) ? (have_fov ? pv_fov : 1.f) : (float)tan((double)((have_fov ? pv_fov : 30.f) * 0.017453292519943295f));
        if (egg_view) {
            view_pcx.resize(npx);
            if (hipMalloc((void**)&lin, npx * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&srgb, npx * 3 * sizeof(float)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
        }
        if (vinyl_view && (hipMalloc((void**)&lin, npx * 3 * sizeof(float)) != hipSuccess || hipMalloc((void**)&srgb, npx * 3 * sizeof(float)) != hipSuccess ||
                           hipMalloc((void**)&vout, npx * 5 * sizeof(float)) != hipSuccess)) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
        const float fw = (float)W, fh = (float)H, aspect = fw / fh;
        const V fwd = norm3(V{pv_look[0] - pv_eye[0], pv_look[1] - pv_eye[1], pv_look[2] - pv_eye[2]});
        const V right = cross3(V{0.f, 1.f, 0.f}, fwd), up = cross3(fwd, right);
        std::vector<float> hr(npx * 6);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float fx = (float)x + .5f, fy = (float)y + .5f;
                const float pcx = ((2.f * (fx / fw) - 1.f) * aspect) * fov, pcy = ((2.f * (fy / fh) - 1.f) * 1.f) * fov;
                const V d = norm3(V{(fwd.x + up.x * pcy) + right.x * pcx, (fwd.y + up.y * pcy) + right.y * pcx, (fwd.z + up.z * pcy) + right.z * pcx});
                float* r = &hr[((size_t)y * W + x) * 6];
                r[0] = pv_eye[0]; r[1] = pv_eye[1]; r[2] = pv_eye[2];
                r[3] = d.x; r[4] = d.y; r[5] = d.z;
                if (egg_view) view_pcx[(size_t)y * W + x] = pcx;
            }
        if (hipMalloc((void**)&rays, hr.size() * sizeof(float)) != hipSuccess ||
            hipMemcpy(rays, hr.data(), hr.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int f = 0; f < frames; ++f) {
        sbx_uniforms u{};
        u.u_res[0] = (float)W; u.u_res[1] = (float)H; u.u_mouse[0] = mx; u.u_mouse[1] = my; u.u_time = t + f * dt;   // hlsltoy.cpp:502-504
        sbx_aux_egg_pose frame_pose;
        if (id == SBX_APP_EGG_POSE) { frame_pose = pose_at(u.u_time); aux = &frame_pose; }
        sbx_aux_vinyl_deck frame_deck;
        if (id == SBX_APP_VINYL_DECK) { frame_deck = deck_at(u.u_time); aux = &frame_deck; }
        sbx_aux_atmosphere_air frame_air;
        if (id == SBX_APP_ATMOSPHERE_AIR) { frame_air = air_at(u.u_time); aux = &frame_air; }
        sbx_aux_planet_world frame_world;
        if (id == SBX_APP_PLANET_WORLD) { frame_world = world_at(u.u_time); aux = &frame_world; }
        (void)hipEventRecord(e0, nullptr);
        if (panorama) rc = sbx_clouds_eval(ctx, "render", have_ac ? &ac : nullptr, u.u_time, rays, dev, npx, nullptr);
        else if (planet_view) rc = sbx_planet_eval(ctx, "render", u.u_time, rays, dev, npx, nullptr);
        else if (egg_view) {
            const sbx_aux_egg_pose pose = pose_at(u.u_time);
            rc = sbx_egg_eval(ctx, "render_scene", &pose, rays, dev, npx, nullptr);
            // render's bars and abs (app_egg.h:233-251) on what render_scene returned (rgb, depth), in binary32 in the reference's order of
            // operations (smoothstep: t = clamp((x - e0) / (e1 - e0), 0, 1), t t (3 - 2 t); mix: x (1 - a) + y a; step: x < edge ? 0 : 1)
            std::vector<float> px(n), l3(npx * 3);
            if (rc == SBX_OK && hipMemcpy(px.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            for (size_t i = 0; rc == SBX_OK && i < npx; ++i) {
                const float x = fabsf(fabsf(view_pcx[i]) - 0.6f) - 0.05f;
                float ts = (x - 0.0f) / (0.01f - 0.0f);
                ts = ts < 0.f ? 0.f : ts;                    // m_max(ts, 0) then m_min(., 1): compare-and-select, a NaN stays
                ts = 1.f < ts ? 1.f : ts;
                const float bar_factor = 1.0f - (ts * ts) * (3.0f - 2.f * ts);
                const float depth_factor = 1.f - (px[i * 4 + 3] < 1.f ? 0.f : 1.f);
                const float a = bar_factor * depth_factor;
                for (int k = 0; k < 3; ++k) l3[i * 3 + k] = fabsf(px[i * 4 + k] * (1.f - a) + .6f * a);
            }
            if (rc == SBX_OK && hipMemcpy(lin, l3.data(), l3.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            if (rc == SBX_OK) rc = sbx_math_eval(ctx, "srgb_pow", lin, nullptr, srgb, npx * 3, nullptr);
            if (rc == SBX_OK && hipMemcpy(l3.data(), srgb, l3.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            for (size_t i = 0; i < npx; ++i) { px[i * 4] = l3[i * 3]; px[i * 4 + 1] = l3[i * 3 + 1]; px[i * 4 + 2] = l3[i * 3 + 2]; px[i * 4 + 3] = 1.f; }      // main.h:52
            if (rc == SBX_OK && hipMemcpy(dev, px.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        }
        else if (vinyl_view) {
            const sbx_aux_vinyl_deck deck = deck_at(u.u_time);
            rc = sbx_vinyl_eval(ctx, "render", &deck, rays, vout, npx, nullptr);
            // main.h's linear_to_srgb and alpha 1 on the linear rgb "render" returned (t and the material id are not part of a frame)
            std::vector<float> v5(npx * 5), l3(npx * 3), px(n);
            if (rc == SBX_OK && hipMemcpy(v5.data(), vout, v5.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            for (size_t i = 0; i < npx; ++i) for (int k = 0; k < 3; ++k) l3[i * 3 + k] = v5[i * 5 + k];
            if (rc == SBX_OK && hipMemcpy(lin, l3.data(), l3.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            if (rc == SBX_OK) rc = sbx_math_eval(ctx, "srgb_pow", lin, nullptr, srgb, npx * 3, nullptr);
            if (rc == SBX_OK && hipMemcpy(l3.data(), srgb, l3.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            for (size_t i = 0; i < npx; ++i) { px[i * 4] = l3[i * 3]; px[i * 4 + 1] = l3[i * 3 + 1]; px[i * 4 + 2] = l3[i * 3 + 2]; px[i * 4 + 3] = 1.f; }      // main.h:52
            if (rc == SBX_OK && hipMemcpy(dev, px.data(), n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        }
        else rc = multi ? sbx_multi_render(multi, id, &u, aux, dev, nullptr) : sbx_render_rows(ctx, id, &u, aux, 0, H, dev, nullptr);
        if (rc != SBX_OK) { fprintf(stderr, "render: %s\n", multi ? sbx_multi_last_error(multi) : sbx_last_error(ctx)); return 1; }
        (void)hipEventRecord(e1, nullptr);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        printf("frame %d  u_time %.4f  %s %dx%d  %.3f ms  %.1f Mpix/s\n", f, u.u_time, panorama ? "clouds panorama" : planet_view ? "planet view" : egg_view ? "egg view" : vinyl_view ? "vinyl view" : app.c_str(), W, H, ms, W * (double)H / ms / 1e3);
        if (!f32.empty()) {
            if (hipMemcpy(host.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            FILE* fp = fopen(frame_name(f32, f, frames).c_str(), "wb");
            if (!fp) { perror("fopen"); return 1; }
            fwrite(host.data(), sizeof(float), n, fp);
            fclose(fp);
        }
        if (!ppm.empty()) {
            // the back-buffer write of hlsltoy (R8G8B8A8_UNORM, top row first) on the device, then 4 B/pixel over PCIe
            if (rgba8_out) {
                // the kernels wrote this format already (row 0 = bottom): 4 B/pixel over PCIe, the rows turned here
                if (hipMemcpy(rgba8.data(), dev, npx * 4, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
                for (int y = 0; y < H; ++y) {
                    const unsigned char* src = &rgba8[(size_t)(H - 1 - y) * W * 4];
                    unsigned char* dst = &rgb[(size_t)y * W * 3];
                    for (int x = 0; x < W; ++x) { dst[x * 3] = src[x * 4]; dst[x * 3 + 1] = src[x * 4 + 1]; dst[x * 3 + 2] = src[x * 4 + 2]; }
                }
            } else {
            rc = sbx_pack_unorm8(ctx, W, H, dev, dev8, /*flip_y=*/1, nullptr);
            if (rc != SBX_OK) { fprintf(stderr, "sbx_pack_unorm8: %s\n", sbx_last_error(ctx)); return 1; }
            if (hipMemcpy(rgba8.data(), dev8, npx * 4, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); return 1; }
            for (size_t i = 0; i < npx; ++i) { rgb[i * 3] = rgba8[i * 4]; rgb[i * 3 + 1] = rgba8[i * 4 + 1]; rgb[i * 3 + 2] = rgba8[i * 4 + 2]; }
            }
            FILE* fp = fopen(frame_name(ppm, f, frames).c_str(), "wb");
            if (!fp) { perror("fopen"); return 1; }
            fprintf(fp, "P6\n%d %d\n255\n", W, H);
            fwrite(rgb.data(), 1, rgb.size(), fp);
            fclose(fp);
        }
    }
    if (rays) (void)hipFree(rays);
    if (vout) (void)hipFree(vout);
    if (lin) (void)hipFree(lin);
    if (srgb) (void)hipFree(srgb);
    if (dev8) (void)hipFree(dev8);
    (void)hipFree(dev);
    if (multi) sbx_multi_destroy(multi);
    sbx_destroy(ctx);
    return 0;
}
