/* include/sbx.h — C ABI of libsbx: the MI355X drop-in for shaderbox's mainImage() hot path.
 *
 * What this boundary replaces.  In the reference a *host* evaluates
 *     void mainImage(out vec4 fragColor, in vec2 fragCoord)        (src/main.h:6-53)
 * once per pixel for the app chosen by one global APP_* define (README.md:11-22,
 * src/Makefile:9): the external VML/SDL harness on the C++ path (src/Makefile:21), or the
 * D3D11 host util/hlsltoy (its per-frame Draw, util/hlsltoy/src/hlsltoy.cpp:494-495, with
 * the uniforms of src/uniform_buffer.h uploaded as cbuffers b0/b1, hlsltoy.cpp:402-426,
 * 502-516).  A per-pixel FFI into a GPU is meaningless, so the boundary is frame-granular:
 * one call renders rows of one frame of one app into a caller-owned RGBA32F framebuffer in
 * device memory (sbx_render_rows); sbx_main_image keeps the per-pixel signature on top of it
 * for hosts that want their loop unchanged.  Everything a host needs is plain C: pointers,
 * sizes, POD structs.
 *
 * Conventions (all from the reference):
 *   - framebuffer: row-major float4 RGBA, 16 B/pixel, row 0 = BOTTOM row (main.h:40-43: the
 *     y flip is HLSL-only), alpha = 1 (main.h:52);
 *   - fragCoord of pixel (x, y) is (x + .5, y + .5);
 *   - `_mutable` globals have GLSL per-invocation meaning (def.h:18): every pixel starts from
 *     the initialisers;
 *   - errors: the reference has none (void everywhere, NaN flows to the framebuffer).  Here every
 *     entry point returns 0 on success or a negative sbx_status; NaNs stay data; nothing aborts.
 *   - threading: one caller per sbx_ctx at a time; calls are asynchronous on the given HIP
 *     stream (hipStream_t passed as void*; NULL = the default stream).
 */
#ifndef SBX_H
#define SBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point, enum value or struct layout of this header changes (2 = round 5: the store exchange
 * sbx_shared_*, sbx_stats, sbx_abi_version itself; the test hooks moved to sbx_test.h).  Not bumped for SBX_APP_2D / SBX_APP_2D_TEX,
 * sbx_set_texture2d, sbx_checkerboard_texture, SBX_APP_FUNC, SBX_APP_ATMOSPHERE_GROUND, SBX_APP_SDF_AO_SHADOW, SBX_APP_SDF_AO_NORMALS, SBX_APP_EGG_STRAIGHT, SBX_APP_EGG_OVAL, SBX_APP_CLOUDS_HEIGHT, SBX_APP_CLOUDS_LUMINANCE, SBX_APP_RAYTRACER_PHONG, SBX_APP_RAYTRACER_NOSHADOW, SBX_APP_RAYTRACER_STATIC, SBX_APP_VINYL_CLOSEUP, SBX_APP_VINYL_RIDGES, SBX_APP_VINYL_NOSHADOW, SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS, SBX_APP_PLANET_UNLIT, sbx_noise_eval's "worley_fbm", sbx_atmosphere_eval, SBX_APP_RAYTRACER_SCENE with sbx_aux_raytracer_scene and sbx_raytracer_scene_cornell, SBX_APP_SDF_SCENE with sbx_aux_sdf_scene, sbx_sdf_scene_ramp and sbx_sdf_eval, sbx_clouds_eval, sbx_planet_eval, SBX_APP_EGG_POSE with sbx_aux_egg_pose and sbx_egg_pose_default, sbx_egg_eval, SBX_APP_VINYL_DECK with sbx_aux_vinyl_deck and sbx_vinyl_deck_default, sbx_vinyl_eval, SBX_APP_ATMOSPHERE_AIR with sbx_aux_atmosphere_air and sbx_atmosphere_air_default, sbx_atmosphere_air_eval, sbx_raytracer_eval: new enum values after the old ones,
 * new entry points and names only, no value renumbered and no layout changed, so a host built against version 2 without them works unchanged.  A host checks
 * sbx_abi_version() == SBX_ABI_VERSION after loading the library: include/sbx_mainimage.hpp and shaderbox_amd.load_library do. */
#define SBX_ABI_VERSION 2
int sbx_abi_version(void);

/* App selector = the reference's APP_* project defines, in README.md:15-22 order, plus
 * APP_SDF_AO (src/uniform_buffer.h:56, util/hlsltoy/src/hlsltoy.cpp:488). */
typedef enum sbx_app {
    SBX_APP_PLANET = 0,      /* src/app_planet.h as shipped: CLOUDS (:63) and LIGHT (:249) defined, the `#if 0` of setup_camera (:51) off.  The
                                 builds with one of the three the other way are SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS and
                                 SBX_APP_PLANET_UNLIT */
    SBX_APP_CLOUDS = 1,      /* src/app_clouds.h as shipped: both `#if 0` of illuminate_volume (:97, :118) off.  The builds with one of them
                                on are SBX_APP_CLOUDS_HEIGHT and SBX_APP_CLOUDS_LUMINANCE */
    SBX_APP_VINYL = 2,      /* C++-build semantics: 60 march steps (src/app_vinyl.h:411-416).  src/app_vinyl.h as shipped: the `#if 1` of
                                setup_camera (:60) and of the shadow ray (:445) on, the `#if 0` of illuminate's ridge (:357) off.  The builds
                                with one of the three the other way are SBX_APP_VINYL_CLOSEUP, SBX_APP_VINYL_RIDGES and
                                SBX_APP_VINYL_NOSHADOW */
    SBX_APP_EGG = 3,         /* src/app_egg.h as shipped: BEZIER defined (:37) and the `#if 1` egg (:46-52).  The builds with one of the two
                                switches the other way are SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL */
    SBX_APP_RAYTRACER = 4,   /* src/app_raytracer.h as shipped: the `#if 1` of setup_scene (:29) and of the shadow ray (:107) on, the `#if 0` of
                                illuminate (:61) off.  The builds with one of the three the other way are SBX_APP_RAYTRACER_PHONG,
                                SBX_APP_RAYTRACER_NOSHADOW and SBX_APP_RAYTRACER_STATIC */
    SBX_APP_ATMOSPHERE = 5,  /* src/app_atmosphere.h as shipped, FROM_SPACE defined (:162): the sky dome (:190-209).  The build without
                                the define is SBX_APP_ATMOSPHERE_GROUND */
    SBX_APP_SDF_AO = 6,      /* src/app_sdf_ao.h as shipped: both `#if 0` blocks off (:217-219, :269-274).  The builds with one of them on are
                                SBX_APP_SDF_AO_SHADOW and SBX_APP_SDF_AO_NORMALS */
    /* not an APP_* define of the reference: the stand-alone shader src/app_clouds_best.h (own mainImage :669-696),
       numbered after the reference's apps */
    SBX_APP_CLOUDS_BEST = 7,
    /* APP_CLOUDS compiled with USE_NOISE_TEX (src/app_clouds.h:9,51-56,69-81): density from two 3-D noise textures
       (sbx_set_noise_volumes) instead of the procedural fBm; same aux block as APP_CLOUDS */
    SBX_APP_CLOUDS_TEX = 8,
    /* the UE4 cloud variant, ue4/volumetric_clouds/Shaders/app_clouds.usf (ue4_render_clouds :234-265): a library for an
       Unreal material, not a mainImage shader.  Host mapping of this build: cam_dir = the primary-ray direction of
       APP_CLOUDS' camera, time = u_time, parameters = the TWEAK defaults (:4-17) or an sbx_aux_clouds_ue4 block, result
       through main.h's sRGB epilogue.  No reference-held answers: parity unpinned. */
    SBX_APP_CLOUDS_UE4 = 9,
    /* APP_CLOUDS compiled with SKY_SPHERE (src/app_clouds.h:8,14-19,154-162; intersect_sphere_from_inside src/intersect.h:35-53):
       the march starts where the view ray meets the sphere ((0, atm_ground_y, 0), atm_radius) — which makes those two fields
       of the aux block live — runs along the view ray itself, the layer turns with rotate_around_x(u_time) and
       cld_noise_factor is 10 / atm_radius.  Same aux block as APP_CLOUDS (wind_dir is not read).  Parity unpinned (no
       reference-held answers; bit-identical to the oracle's restatement). */
    SBX_APP_CLOUDS_SKY = 10,
    /* APP_VINYL with the march length of its GLSL / HLSL builds: 180 steps instead of the C++ build's 60
       (src/app_vinyl.h:411-416).  Everything else as SBX_APP_VINYL. */
    SBX_APP_VINYL_GPU = 11,
    /* BASELINE config 5 read literally — "APP_ATMOSPHERE Rayleigh/Mie over APP_PLANET terrain".  The reference has no shader that
       composites the two (SURVEY.md 8a note); this labelled extension is APP_PLANET (src/app_planet.h:303-367) with its
       background() (:23-41, shown where the view ray misses the atmosphere shell :316-318 and behind the clouds :364-366)
       replaced by APP_ATMOSPHERE's get_incident_light (src/app_atmosphere.h:78-160) for the ray from (0, earth_radius + 1, 0)
       (:204-207) along the VIEW direction, lit by APP_ATMOSPHERE's sun (setup_scene :177-181, a function of u_time).
       No reference-held answers: PARITY UNPINNED (bit-identical to the oracle's restatement of the same definition). */
    SBX_APP_PLANET_ATMOSPHERE = 12,
    /* not APP_* defines of the reference: the author's tunnel / road UV demo src/app_2d.h with its own mainImage (:70-111).
       t = mod(u_time, 16) picks one of four phases with the reference's strict inequalities (:80-103): tunnel; tunnel(1) mixed
       into road(1) with weight (t - 4) / 4; road; road(1) mixed into tunnel(1) with weight (t - 12) / 4; then
       color *= 1 - tent_filter(2 uv.y - 1) (:106).  sample() is checkboard_pattern(uv, 2.) as (cb, cb, cb, 1) (src/util.h:95-101).
       ALPHA IS NOT 1: the shader writes `color` straight to fragColor (:108), its alpha scaled by the tunnel's r and by the tent.
       So the entry points that carry only R, G, B — sbx_render_split_rgb, sbx_render_split_in_place_rgb, sbx_render_span_peer,
       sbx_render_span_peer_in_place with 3 channels, and the span exchange around them (sbx_render_span_root, sbx_assemble_spans)
       — return SBX_ERR_UNSUPPORTED for these apps and write nothing, as does sbx_multi_render.  Four-channel forms work: rows,
       strips, points, sbx_main_image*, ranks, splits (in place too) and their assemblies; SBX_FORMAT_RGBA8 stores unorm8(alpha).
       THE PORT'S CHOICE, parity unpinned: at t exactly 4, 8 or 12, and for non-finite u_time, no branch runs and the reference's
       `color` is uninitialised; the port writes (0, 0, 0, 0) times the tent.  NaN / Inf (the r = 0 pixel of an odd frame size,
       points far outside the frame) flow through as data.  Math: DESIGN.md §3 (atan is the binary64 atan2 of the spec). */
    SBX_APP_2D = 13,
    /* SBX_APP_2D built with USE_TEXTURE (src/app_2d.h:3-30): sample() is u_tex0.Sample(u_sampler0, uv), the t0 texture of
       sbx_set_texture2d (default: hlsltoy's 128x128 checkerboard, util/hlsltoy/src/hlsltoy.cpp:66-87, 217-223, bound with a
       LINEAR / WRAP sampler :242-249, 434-437) filtered by the sbx texture-filter spec reduced to two axes and four channels. */
    SBX_APP_2D_TEX = 14,
    /* not an APP_* define of the reference: src/app_func.h, the function plotter with its own mainImage (:63-111), in the branch
       it compiles (`#if 1 // 2D`, :79-85): t = (fragCoord + .5) / u_res (:72), n = worley_fbm((t, 0)) — the tiled Worley fBm of
       :17-47, nine noise_w (src/noise_worley.h:20-51) over the periods 4, 8, 16, 24, 32, 64 — and fragColor = (n, n, n, 1) (:110),
       no sRGB.  u_time and u_mouse do not enter.  Alpha is 1, so every output form holds it (rgb, span, split, SBX_FORMAT_RGBA8,
       sbx_multi_render).  The reference does not compile as shipped (its ashima-noise submodule is absent); the port is what the
       compiled branch computes under the math spec of DESIGN.md §3, which is also the shader's GLSL meaning.  hlsltoy's HLSL build
       would flip t.y and hash cell -1 for L - 1 at the left and bottom edges (its fmod): parity with it is not pinned.
       The `#else // 1D` plot branch (ashima's cnoise / snoise) is not ported. */
    SBX_APP_FUNC = 15,
    /* APP_ATMOSPHERE compiled WITHOUT FROM_SPACE (src/app_atmosphere.h:162, 168-174, 210-225): mainImage of src/main.h:6-53 with
       FOV 1 (:230), eye = (0, earth_radius + 1, 0), look_at = (0, earth_radius + 1.5, -1) (:172-173; both y values are exact in
       binary32) — a perspective camera one metre above the ground, looking at the horizon.  setup_scene (:177-181) is unchanged: the
       sun of SBX_APP_ATMOSPHERE for the same u_time.  render (:211-224): terrain = plane((0, -1, 0), earth_radius), hit = no_hit,
       intersect_plane(eye, terrain, hit) (src/intersect.h:61-77, with its P0 = (d, d, d) and its `denom < 1e-6` and
       `t < 0 || t > hit.t` tests as written); hit.t > max_dist -> get_incident_light (:78-160) along the PRIMARY RAY, else
       (.33, .33, .33); then linear_to_srgb, alpha 1.  u_mouse does not enter.  The camera has no roll, so the row decides sky or
       ground (the bottom 22 % of a 16:9 frame is ground); sky channels exceed 1 near the sun and are stored unclamped in float
       frames.  A NaN DIRECTION IS A GROUND HIT (a non-finite fragCoord given to sbx_render_points): `denom < 1e-6` is false, t is
       NaN, `t < 0 || t > hit.t` is false, the hit is recorded and the pixel is grey — not black as in the dome build.  Alpha is 1, so
       every output form holds it (rgb, span, split, SBX_FORMAT_RGBA8, sbx_multi_render).  sbx_set_variant(1) selects the plain
       kernel (no wave-level exits, none of the kernel-internal math forms); SBX_PRECISION_1E4 applies (below).  No reference-held
       answers: parity unpinned — bit-identical to the model over the oracle's get_incident_light (tests/atmosphere_ground_model.py). */
    SBX_APP_ATMOSPHERE_GROUND = 16,
    /* APP_SDF_AO compiled with the `#if 0` at src/app_sdf_ao.h:269 turned on (:269-274): at a hit, sh = sdf_shadow({p + sun_dir * 0.05,
       sun_dir}) — the 20-step soft-shadow march of :183-207 towards sun_dir = normalize(1, 2, 1) (:209): sdf(p) first, `t > 20` leaves
       with the umbra so far, `d.x < .005` returns .05, then t += d.x and umbra = min(umbra, 32 * d.x / t) — and sh multiplies the key
       light (:225).  Everything else as SBX_APP_SDF_AO: same camera, same sbx_aux_sdf_ao block (fog density and falloff; the defaults
       when aux is NULL), same fog, abs (:310) and sRGB epilogue; pixels that miss the scene are unchanged.  sbx_set_variant(1) selects
       the plain kernel as for SBX_APP_SDF_AO; SBX_PRECISION_1E4 is ignored.  Definition: tests/sdf_ao_builds_model.py, pinned against
       frames of the edited reference header (tests/golden/sdf_ao_builds/). */
    SBX_APP_SDF_AO_SHADOW = 17,
    /* APP_SDF_AO compiled with the `#if 0` at src/app_sdf_ao.h:217 turned on (:217-219; the shadow block off as shipped): illuminate
       returns hit.normal — sdf_normal's six-tap gradient, normalized (:152-163) — as the colour.  That value still goes through
       render's fog mix and abs (:305-310) and main.h's linear_to_srgb, so a frame shows |mix(n, 1, fog)|^(1/2.2); a zero gradient's
       normalize(0) = NaN is the pixel's data.  Pixels that miss the scene are unchanged (background under fog).  Aux block, variants
       and precision as SBX_APP_SDF_AO_SHADOW. */
    SBX_APP_SDF_AO_NORMALS = 18,
    /* APP_EGG compiled without the `#define BEZIER` of src/app_egg.h:37: the legs are four sd_cylinder segments (src/sdf.h:95-109)
       instead of the two sd_bezier tubes of :111-116 — left_leg_a = sd_cylinder(p + pelvis, 0, knee_l - side, thick) and left_leg_b =
       sd_cylinder(p + knee_l, 0, left_foot_pos - knee_l, thick) (:86-93), right_leg_a = sd_cylinder(p + pelvis, 0, knee_r + side, thick)
       with pelvis = -side and right_leg_b = sd_cylinder(p + knee_r, 0, right_foot_pos - knee_r, thick) (:97-104); thick = .05, the knees
       are the IK solver's (:85, :96).  THE TWO LEGS ARE NOT JOINED ALIKE (:106-109): legs = op_add(vec2(op_blend(left_leg_a.x,
       left_leg_b.x, .01), material), op_add(right_leg_a, right_leg_b)) — the left knee is a smooth minimum with k = .01 (src/sdf.h:38-47),
       the right knee a plain union.  Everything else as SBX_APP_EGG: the `#if 1` egg of three blended spheres, feet, wheel, ground and
       the order of their unions (:140-143), camera (:23-27, FOV 1), the 80-step trace and the 20-step shadowmarch of ground hits
       (:161-231), the flat colours, `depth` fresh per invocation (:188), the bars (:239-248), abs, linear_to_srgb, alpha 1, no aux
       block.  u_mouse does not enter.  Alpha is 1, so every output form holds it (rgb, span, split, SBX_FORMAT_RGBA8,
       sbx_multi_render).  sbx_set_variant 0-3 mean what they mean for SBX_APP_EGG (1 = every member evaluated everywhere, 2 / 3 = the
       recorded-domain roots with the re-run forced / the IEEE roots only); SBX_PRECISION_1E4 is ignored.  Definition:
       tests/egg_builds_model.py, pinned against frames and points of the edited reference header (tests/golden/egg_builds/). */
    SBX_APP_EGG_STRAIGHT = 19,
    /* APP_EGG compiled with the `#if 1` at src/app_egg.h:46 turned to `#if 0` (BEZIER defined as shipped): the egg is the `#else` of
       :53-66 — ONE sphere, sd_sphere(iscale * (scale * (p - vec3(0, egg_y, 0))), 0.475) with egg_y = .65, s = 1.55, scale =
       diag(s, 1, 1) and iscale = diag(1. / s, 1. / s, 1.) — instead of the three spheres and two op_blend of :47-52.  OPERATION ORDER:
       the inner product first, scale * q, then iscale * (that); each mat3 * vec3 is (col0 * v.x + col1 * v.y) + col2 * v.z, zero
       terms included (0 * inf is a NaN and (-0) + 0 is +0, as in the reference's C++ build), and 1. / s is the binary32 quotient.
       So x is scaled up by s and down again (two roundings, not the identity), y is divided by s, z is unchanged: a spheroid
       stretched to .475 * 1.55 along y — its top stands above the blended egg's — whose field is not a distance (it under-estimates
       along y by the factor 1.55).  Everything else, the variants and the precision tier as SBX_APP_EGG_STRAIGHT says; the legs are
       the Bezier tubes. */
    SBX_APP_EGG_OVAL = 20,
    /* APP_CLOUDS compiled with the `#if 0` of src/app_clouds.h:97 turned to `#if 1` (:118 as shipped): the height-lit build.
       illuminate_volume's light march (:100-115) is gone; `float luminance = exp(height) / 2.;` stands in its place, with height the
       main march's cloud.height = float(i) / float(cld_march_steps) of the step (:183).  So per lit main step i (density >= .005,
       :132) illuminate_volume returns (luminance * sun_power) * henyey_greenstein_phase_func(clamp(dot(sun_dir, eye.direction), 0, 1))
       with luminance = exp(float(i) / float(cld_march_steps)) / 2., exp the math spec's binary32 exp, the division by 2 exact.
       illum_march_steps is not read; sun_dir enters only the sky colour and the phase.  Everything else as SBX_APP_CLOUDS: camera,
       render_sky_color, the `< 0.05` horizon exit (:212: the same span table), density_func, integrate_volume, the alpha > .999
       exit, the cutoff smoothstep, abs, linear_to_srgb, alpha 1.  Aux block: sbx_aux_clouds (NULL = its defaults).  The procedural
       build only: the combinations with SKY_SPHERE / USE_NOISE_TEX and the build with BOTH switches on are not offered.  Alpha is 1,
       so every output form holds it (rows, points, sbx_main_image*, ranks, splits, rgb, span, the store exchange, SBX_FORMAT_RGBA8,
       sbx_multi_render).  sbx_set_variant(ctx, 1) = the plain per-lane kernel, as for SBX_APP_CLOUDS.  Definition:
       tests/clouds_builds_model.py, pinned against frames and points of the edited reference header (tests/golden/clouds_builds/). */
    SBX_APP_CLOUDS_HEIGHT = 21,
    /* APP_CLOUDS compiled with the `#if 0` of src/app_clouds.h:118 turned to `#if 1` (:97 as shipped): the raw-luminance build.  The
       light march of :100-115 runs exactly as in SBX_APP_CLOUDS and illuminate_volume returns its vol.transmittance unscaled
       (`return luminance;`): sun_power is not read and the phase function is not evaluated (sun_dir still enters the sky colour and
       the light march's direction).  Everything else, the aux block, the output forms, the variant and what is not offered as
       SBX_APP_CLOUDS_HEIGHT says. */
    SBX_APP_CLOUDS_LUMINANCE = 22,
    /* APP_RAYTRACER compiled with the `#if 0` of src/app_raytracer.h:61 turned to `#if 1` (:29 and :107 as shipped): the Phong build.
       illuminate calls illum_blinn_phong (src/light.h:44-62) instead of illum_cook_torrance; that function is compiled in the `#else`
       branch of its own `#if 0 // Blinn specular` (:53), the Phong specular, so per lit hit
           diffuse = max(0., dot(L, N)) * base_color;  R = reflect(-L, N);  specular = pow(max(0., dot(R, V)), 50.) * vec3(1, 1, 1)
       with reflect(I, N) = I - 2. * dot(N, I) * N (src/util_optics.h:17-22), pow the math spec's binary32 pow, and
       ambient + diffuse + specular returned.  The material's roughness and ior are not read; the mat_debug early return of :51-53
       stands before it.  (The Blinn branch of :53 does not compile in the C++ form and is not offered.)  Everything else as
       SBX_APP_RAYTRACER: camera (u_mouse turns it), the animated scene, the shadow ray, the reflection bounce, alpha 1.  No aux
       block.  Every output form holds it (rows, host rows, points, sbx_main_image*, ranks, splits, rgb, the exchanges with whole
       rows, SBX_FORMAT_RGBA8, sbx_multi_render).  sbx_set_variant as for SBX_APP_RAYTRACER (include/sbx_test.h).  Two switches at
       once are not offered.  Definition: tests/raytracer_builds_model.py, pinned against frames and points of the edited reference
       header (tests/golden/raytracer_builds/). */
    SBX_APP_RAYTRACER_PHONG = 23,
    /* APP_RAYTRACER compiled with the `#if 1 // shadow ray` of src/app_raytracer.h:107 turned to `#if 0` (:29 and :61 as shipped):
       the unshadowed build.  :108-121 are gone: no second raytrace_iteration from the first hit towards the light and no
       `color *= 0.1`.  Everything else, the output forms, the variants and what is not offered as SBX_APP_RAYTRACER_PHONG says; the
       lighting is Cook-Torrance as shipped. */
    SBX_APP_RAYTRACER_NOSHADOW = 24,
    /* APP_RAYTRACER compiled with the `#if 1` of src/app_raytracer.h:29 turned to `#if 0` (:61 and :107 as shipped): the Cornell box
       at rest.  setup_scene ends after setup_cornell_box: the left sphere stays at (0.75, 1, -0.75), the right one at
       (-0.75, 0.75, 0.75) (src/cornell_box.h:77-82) and the light at (0, 3.8, 0) (:85; z is 0, not 1.5).  u_time is not read: every
       value of it, inf and NaN included, gives the same frame; u_mouse turns the camera as shipped.  The shipped kernels over
       another frame block.  Everything else as SBX_APP_RAYTRACER_PHONG says; the lighting is Cook-Torrance as shipped. */
    SBX_APP_RAYTRACER_STATIC = 25 /* (the separating comma stands behind this comment) */,
    /* APP_VINYL compiled with the `#if 1` of setup_camera at src/app_vinyl.h:60 turned to `#if 0` (:357 and :445 as shipped): the
       close-up camera of :64-65, eye (-2, 1.5, 5.5) looking at (-1.5, 0, 0), over the label, the spindle and the headshell.  Scene,
       march (the C++ build's 60 steps), shadow, shading and epilogue are SBX_APP_VINYL's: the shipped kernels over another frame block.
       No aux block, u_mouse unused, alpha 1.  Every output form holds it (rows, host rows, points, sbx_main_image*, ranks, splits,
       rgb, the exchanges with whole rows, SBX_FORMAT_RGBA8, sbx_multi_render).  sbx_set_variant 0-3 as for SBX_APP_VINYL
       (include/sbx_test.h).  NaN pixels are data: sqrt of a negative dotLN * dot(V, N) in the groove shading (:339) gives some in
       every build, more from this camera.  Not offered: the 180-step forms of the three builds, two switches at once, the SHADERTOY
       branches, and the `#if 0` at :291 (hit.normal is still render's (0, 1, 0) there: the frame would be (0, sh, 0), a shadow mask).
       Definition: tests/vinyl_builds_model.py, pinned against frames and points of the edited reference header
       (tests/golden/vinyl_builds/). */
    SBX_APP_VINYL_CLOSEUP = 26,
    /* APP_VINYL compiled with the `#if 0` of illuminate at src/app_vinyl.h:357 turned to `#if 1` (:60 and :445 as shipped): the ridged
       label.  After sdf_normal, hits of mat_label and mat_logo get :359-362 on the unrotated hit.origin:
           r = length(hit.origin);  B = hit.origin / r;  s = saw(r * .9);  hit.normal = normalize(hit.normal + B * float(s > .975))
       with saw(x) = x - floor(x).  Everything else, the output forms, the variants and what is not offered as SBX_APP_VINYL_CLOSEUP
       says; the camera is the shipped one. */
    SBX_APP_VINYL_RIDGES = 27,
    /* APP_VINYL compiled with the `#if 1` of render at src/app_vinyl.h:445 turned to `#if 0` (:60 and :357 as shipped): the unshadowed
       build.  :446-449 are gone: no 20-step sdf_shadow march from the hit, sh stays 1. and the colour is illuminate's.  Everything
       else, the output forms, the variants and what is not offered as SBX_APP_VINYL_CLOSEUP says; the camera is the shipped one. */
    SBX_APP_VINYL_NOSHADOW = 28 /* (the separating comma stands behind this comment) */,
    /* APP_PLANET compiled with the `#if 0` of setup_camera at src/app_planet.h:51 turned to `#if 1` (:63 and :249 as shipped): the
       camera of :52-53, eye (0, 0, -1.93) looking at (-.1, .9, 2) — the limb seen from close by.  Terrain, clouds, lighting, shadow
       and epilogue are SBX_APP_PLANET's.  No aux block, u_mouse unused, alpha 1.  Every output form holds it (rows, host rows,
       points, sbx_main_image*, ranks, splits, rgb, spans with the atmosphere-shell test from this camera, the exchanges,
       SBX_FORMAT_RGBA8, sbx_multi_render).  sbx_set_variant as for SBX_APP_PLANET: 1 = the plain kernel without its exact skips
       (include/sbx_test.h).  NaN pixels are data: smoothstep(1 - .3 s, 1 - .2 s, N) with s = 0 is 0 / 0 where N == 1 (:270-273);
       some tens per 64x36 frame in this build and the shipped one.  Not offered: two of the three switches at once, the flat
       background() of :26, any of the three builds combined with SBX_APP_PLANET_ATMOSPHERE, the HLSL branch.
       Definition: tests/planet_builds_model.py, pinned against frames and points of the edited reference header
       (tests/golden/planet_builds/). */
    SBX_APP_PLANET_CLOSEUP = 29,
    /* APP_PLANET compiled without the `#define CLOUDS` of src/app_planet.h:63 (:51 and :249 as shipped): :344-347 and :355-361 are
       gone — no 75-step clouds_march, no 5-step clouds_shadow_march.  `cloud` is the static object that nothing writes: cloud.radiance
       and cloud.alpha are its zeros, shadow stays 1., and the two mix of :363 / :365 run on those zeros.  Everything else, the output
       forms, the variant and what is not offered as SBX_APP_PLANET_CLOSEUP says; the camera is the shipped one. */
    SBX_APP_PLANET_CLOUDLESS = 30,
    /* APP_PLANET compiled without the `#define LIGHT` of src/app_planet.h:249 (:51 and :63 as shipped): N = w_normal.y (:254) and
       ocean = water (:292); shoreline is not lit, sdf_terrain_normal with its six 7+7-octave detail maps and setup_lights are never
       evaluated.  Clouds and their ground shadow as shipped.  No NaN pixel in any recorded frame (N == 1 needs a hit on the planet's
       y axis).  Everything else, the output forms, the variant and what is not offered as SBX_APP_PLANET_CLOSEUP says; the camera is
       the shipped one. */
    SBX_APP_PLANET_UNLIT = 31,
    /* The raytracer over the CALLER'S scene: what the reference's README lists as its "minimal raytracer framework" and "minimal
       Cook-Torrance lighting and material setup".  mainImage of src/main.h:6-53 over render of src/app_raytracer.h:88-136, with the
       scene, the camera and the FOV taken from the aux block sbx_aux_raytracer_scene (below) instead of setup_scene / setup_camera /
       :138.  u_res is read; u_time and u_mouse are not.  aux == NULL means sbx_raytracer_scene_cornell(uni, 0, .): SBX_APP_RAYTRACER's
       frame.  Alpha is 1, so every output form holds it (rows, host rows, points, sbx_main_image*, ranks, splits, rgb, the exchanges
       with whole rows: sbx_span_table has no model for it; SBX_FORMAT_RGBA8, sbx_multi_render).
       SEMANTICS, all as the reference's code has them (tests/raytracer_scene_model.py is the definition):
         - planes and spheres are taken in array order, as raytrace_iteration does (:75-83); a later primitive replaces an earlier one
           at equal t.  Planes are never skipped.  In the shadow trace spheres whose material is 0 are skipped (mat_to_ignore =
           mat_debug, :116): a material-0 sphere is the reference's light bulb, drawn flat with materials[0].base_color (:51-53), and
           it casts no shadow.  A sphere whose material is -1 (mat_invalid, the mat_to_ignore of :97) is never intersected;
         - a material id outside 0..7 gives the zero material (get_material's loop finds nothing, material.h:19-36);
         - metallic, translucency and light_color are carried but not read;
         - normals and light_L are never normalised: intersect_plane (src/intersect.h:61-77) uses `direction` as given, with its
           P0 = (distance, distance, distance), its `denom < 1e-6` and its `t < 0 || t > hit.t`;
         - with LIGHT_DIR, illuminate takes L = light_L as given (light.h:22-23); the shadow ray still uses light_L - hit.origin (:109,
           the reference's TODO);
         - the background is black (:13-16);
         - the shadow ray is cast on bounce 0 only; illuminate takes the PRIMARY origin on every bounce (:105); reflect's swapped
           arguments are kept (:127);
         - every float bit pattern is data: NaN, inf, denormals, a zero radius or normal flow through as the reference's operations
           make them.
       SBX_ERR_ARG, before anything is enqueued, for n_planes or n_spheres outside 0..16, bounces outside 1..8, or a light_type /
       lighting / shadow outside the values listed at the block.
       sbx_set_variant as for SBX_APP_RAYTRACER: 1 and 3 select the IEEE roots and normalisations, 2 forces the witness re-run.
       NOT OFFERED: more than one light (the reference reads lights[0]), refraction, other primitives, more than 16 + 16 primitives,
       an acceleration structure, and the drop-in header sbx_mainimage.hpp, which has no way to state a scene. */
    SBX_APP_RAYTRACER_SCENE = 32,
    /* The sphere tracer of src/app_sdf_ao.h over the CALLER'S field: what the reference's README lists as its "signed distance field
       functions and operators" (src/sdf.h).  mainImage of src/main.h:6-53 over render / render_impl / sdf_normal / sdf_ao / sdf_shadow /
       illuminate of src/app_sdf_ao.h exactly as written, with sdf(pos) a small postfix PROGRAM of the aux block sbx_aux_sdf_scene
       (below) and the block's values in place of the literals its comments name.  u_res is read; u_time and u_mouse are not.
       aux == NULL means sbx_sdf_scene_ramp(uni, .).  Alpha is 1, so every output form holds it (rows, host rows, points,
       sbx_main_image*, ranks, splits, rgb, the exchanges with whole rows: sbx_span_table has no model for it; SBX_FORMAT_RGBA8,
       sbx_multi_render).
       SEMANTICS (tests/sdf_scene_model.py is the definition).  The program's instructions run in array order over a stack of floats:
         - a PRIMITIVE computes q = pos - offset, then, if rot_axis != 0, q = mul(q, rotate_around_{x,y,z}(rot_deg)) — the matrices of
           util.h:44-69, the row-vector product with every zero term kept, sin / cos of radians(rot_deg) evaluated by the math spec on
           the host once per frame — and pushes the float the reference's function returns: sd_plane(q, a.xyz, a.w), sd_sphere(q, a.x),
           sd_box(q, a.xyz), sd_torus(q, a.x, a.y), sd_y_cylinder(q, a.x, a.y), sd_cylinder(q, a.xyz, b.xyz, a.w),
           sd_capsule(q, a.xyz, b.xyz, a.w), sd_bezier(a.xyz, b.xyz, c.xyz, q, a.w).x (sdf.h:49-171);
         - an OPERATOR pops d2 (the top), then d1, and pushes op_add(d1, d2), op_sub(d1, d2), op_intersect(d1, d2) or
           op_blend(d1, d2, a.x) (the float forms, sdf.h:13-47);
         - OBJECT pops d and folds vec2(d, float(material)) into the scene's result with the vec2 op_add (sdf.h:5-11):
           acc = first ? v : op_add(acc, v), that is acc.x < v.x ? acc : v — at equal distance, or with a NaN, the LATER object wins.
           This is how the reference's apps build scenes: float CSG per object, a material per object, a union of objects;
         - sdf(pos) is acc after the last instruction; the hit's material is int(acc.y).
       The hit threshold .005, sdf_shadow's 20 steps / end 20 / .05 offset / factor 32 / darkest .05, the AO's five taps, the three
       light colours, the checker scale .5, the abs, the fog formula, linear_to_srgb and alpha 1 stay the reference's.  sun_dir is used
       as given, never normalised.  Every float bit pattern is data: NaN, inf, denormals, a zero k, a zero-length cylinder, a collinear
       Bezier flow through as the reference's operations make them; every loop has a validated bound.
       SBX_ERR_ARG, before anything is enqueued and with nothing written, for: n_instr outside 1..32, an unknown op, rot_axis outside
       0..3, material outside 0..7 on an OBJECT (get_material leaves its result uninitialised outside the table), checker_material
       outside -1..7, march_steps outside 1..512, shadow or view outside {0, 1}, a stack that underflows, that exceeds
       SBX_SDF_MAX_STACK, that is not empty at an OBJECT after its pop or at the end, and a last instruction that is not OBJECT.
       sbx_set_variant as for SBX_APP_SDF_AO: 1 and 3 select the IEEE roots, 2 forces the witness re-run.
       NOT OFFERED: nested frames (a host composes its offsets itself), scaling, per-object light or AO settings, more than 32
       instructions, and the drop-in header sbx_mainimage.hpp, which has no way to state a scene. */
    SBX_APP_SDF_SCENE = 33,
    /* src/app_egg.h as shipped (BEZIER defined, the `#if 1` egg) with the rider POSED BY THE CALLER: what the reference's README lists
       as its "2D two bone IK solver" (src/IK.h) at work.  The aux block sbx_aux_egg_pose (below) states the camera, the turntable's
       angle, both feet and both bone lengths — the values app_egg.h derives from u_time or states as literals at :25, :26, :40, :74,
       :77, :80, :81 and :253; aux == NULL means sbx_egg_pose_default(uni, .), and the frame is then SBX_APP_EGG's in every bit.
       u_res is read; u_time and u_mouse are not.  Alpha is 1: the output forms are the ones SBX_APP_RAYTRACER_SCENE lists.
       SEMANTICS (tests/egg_pose_model.py is the definition), all as app_egg.h and IK.h have them:
         - everything not in the block stays the reference's literal: `side`, both pelvis points, `thick`, the egg, the wheel, the
           ground, the (0, .5, 3.5) offset, the order of the unions, the 80-step trace, the 20-step shadow march of ground hits, the
           flat colours, `depth` fresh per pixel, the bars, abs, linear_to_srgb;
         - the knees are ik_solver(pelvis, foot, femur, tibia) exactly as IK.h:18-41 states it: a foot whose z differs from its
           pelvis' gives a 3-D `goal` rotated about z, as the arithmetic says;
         - a goal beyond femur + tibia gives a NaN knee; by op_add's `d1.x < d2.x ? d1 : d2` that leg and that foot then drop out of
           the union, and the frame holds no NaN;
         - every float bit pattern is data: nothing is refused beyond what any app refuses.
       sbx_set_variant 0-3 mean what they mean for SBX_APP_EGG, except that a block from which a non-finite frame constant follows
       (a NaN knee, toe or bounding sphere, a non-finite angle) always takes the reference form (variant 1's kernel): same bits.
       SBX_PRECISION_1E4 is ignored.
       NOT OFFERED: the STRAIGHT / OVAL builds under a pose, other bone counts or a per-leg pelvis, a pose for the wheel or the egg,
       and the drop-in header sbx_mainimage.hpp, which has no way to state a block. */
    SBX_APP_EGG_POSE = 34,
    /* src/app_vinyl.h as shipped (SHADERTOY undefined, the C++ build's 60 march steps) over the CALLER'S DECK: the turntable whose
       platter angle, tilts, sun, colours and groove BRDF the caller states — among them what the header's "scratching support" branch
       (:420-425, SHADERTOY only) lets the user's hand do: set the platter's angle.  The aux block sbx_aux_vinyl_deck (below) states the
       camera, the three angles, the sun, the five base colours, the Ward constants of illuminate and the shininess of its Phong
       branch; aux == NULL means sbx_vinyl_deck_default(uni, .), and the frame is then SBX_APP_VINYL's in every bit.  u_res is read;
       u_time and u_mouse are not.  Alpha is 1: the output forms are the ones SBX_APP_VINYL has.
       SEMANTICS (tests/vinyl_deck_model.py is the definition), all as app_vinyl.h has them:
         - everything not in the block stays the reference's literal: the geometry of platter, logo, spindle, defects and tonearm,
           ro_diff, the groove pitch 24, the noise scale and amplitude, the 60 march steps, the 20 shadow steps, mat_debug, the white
           background, linear_to_srgb;
         - sun_dir is used as given, never normalised: a sun of another length scales the shadow ray's steps and the dot products;
         - every float bit pattern is data — a sun below the disc, a zero or NaN sun, a_x = 0, a negative colour, eye == look_at — and
           the result is what the reference's arithmetic gives, NaN pixels included: nothing is refused beyond what any app refuses.
       sbx_set_variant 0-3 mean what they mean for SBX_APP_VINYL, except that a block outside the domain of k_vinyl's culls and hardware
       min / max (a value beyond 1e4, 1e10 for an angle; a non-finite frame constant: csrc/sbx_vinyl.h) always takes the reference
       form (variant 1's kernel): same bits.  The colours, Ward constants and shininess do not enter that domain.
       NOT OFFERED: the RIDGES and NOSHADOW builds or the 180 steps of SBX_APP_VINYL_GPU under a deck, a deck for the geometry,
       u_mouse.z (the caller states platter_deg instead), and the drop-in header sbx_mainimage.hpp, which has no way to state a block. */
    SBX_APP_VINYL_DECK = 35,
    /* src/app_atmosphere.h as shipped over the CALLER'S AIR: the Rayleigh/Mie study with every number the header states taken from
       the aux block sbx_aux_atmosphere_air (below) — scattering coefficients, scale heights, both radii, the sun and its power, the
       Henyey-Greenstein g, the two sample counts, the observer and FOV — and with either of the header's two builds chosen by
       `view`: 0 = the FROM_SPACE build's sky dome (:190-209), 1 = the build without it (:210-225: get_primary_ray, the terrain plane
       ((0, -1, 0), earth_radius), the grey .33).  aux == NULL means sbx_atmosphere_air_default(uni, 0, .), and the frame is then
       SBX_APP_ATMOSPHERE's in every bit; the default block of view 1 gives SBX_APP_ATMOSPHERE_GROUND's.  u_res is read; u_time
       and u_mouse are not when a block is passed.  Alpha is 1.
       SEMANTICS (tests/atmosphere_air_model.py is the definition), all as app_atmosphere.h has them:
         - what is not in the block stays the reference's: the 1.1 of :146, rayleigh_phase_func, the Henyey-Greenstein choice of the
           `#if 1`, the atmosphere sphere centred at 0, linear_to_srgb;
         - sun_dir is used as given: setup_scene's rotation (:179-180) does not run and nothing is normalised;
         - earth_radius is the height reference of both marches and, in view 1, the distance of the terrain plane; -height / hR and
           t1 / float(num_samples) are binary32 divisions by the block's values;
         - every float bit pattern is data — NaN, inf, a zero or non-unit sun, atmosphere_radius < earth_radius, hR = 0, hg_g = 1,
           eye == look_at — and the result is what the plain statement of the header computes, NaN pixels included.
       REFUSED (SBX_ERR_ARG, nothing written): view not 0 or 1, num_samples outside 1 ... 64, num_samples_light outside 1 ... 32, a
       non-zero reserved word.
       SBX_PRECISION_1E4 is ignored: the app stays exact.  sbx_set_variant 1 takes the plain statement for every wave (same bits).
       NOT OFFERED: a caller's value for the 1.1, Schlick's phase function, more suns, ozone or other layers, the tolerance tier,
       SBX_APP_PLANET_ATMOSPHERE under a block, and the drop-in header sbx_mainimage.hpp, which has no way to state a block. */
    SBX_APP_ATMOSPHERE_AIR = 36,
    /* src/app_planet.h as shipped (CLOUDS and LIGHT defined) over the CALLER'S WORLD: every number the header states as a one-line
       literal taken from the aux block sbx_aux_planet_world (below) — camera and FOV, the tilt and the two spins, the sun and the key
       light's colour, max_height, both noise offsets (the terrain "seed"), cloud coverage, fuzziness, band and absorption, the five
       colours and four limits, the cloud's light divisor and the three step counts.  aux == NULL means
       sbx_planet_world_default(uni, .), and the frame is then SBX_APP_PLANET's in every bit.  u_res is read; u_time and u_mouse are
       not when a block is passed.  Alpha is 1.
       SEMANTICS (tests/planet_world_model.py is the definition), all as app_planet.h has them:
         - what is not in the block stays the reference's: the planet {0, 1}, the fBm scales, lacunarities, gains and octave counts,
           the terrain smoothstep edges .35 / .6 / 1, TERR_EPS, the .4567, the .001 of the normal, the two fill lights, background(),
           the .7 / .33 of the ground shadow, rot = rotate_around_x(spin) * rotate_around_y(tilt), linear_to_srgb;
         - everything derived is binary32 arithmetic on the block's values in the header's order: max_ray_dist = max_height * 4, the
           atmosphere's radius 1 + max_height, t_step = max_ray_dist / float(cloud_steps) and max_height / float(shadow_steps),
           c_water / 2, cld_coverage + cld_fuzzy;
         - sun_dir is used as given, never normalised;
         - every float bit pattern is data — NaN, inf, a zero sun, max_height <= 0, cld_fuzzy = 0, unordered band edges,
           eye == look_at, an eye inside the planet — and the result is what the plain statement of the header computes, NaN pixels
           included.
       REFUSED (SBX_ERR_ARG, nothing written): terr_steps outside 1 ... 512, cloud_steps outside 1 ... 256, shadow_steps outside
       1 ... 32, a non-zero reserved word.
       sbx_set_variant 1 takes the plain statement over the block's numbers for every block (same bits); so does, whatever the variant, a
       block outside the stated domain of the short forms (csrc/kern_planet_world.hip, csrc/sbx_frames.hip planet_world_tame).  A block that differs
       from the default in camera, angles and sun only runs SBX_APP_PLANET's own kernels over its frame block.
       sbx_planet_world_eval (below) evaluates the header's functions over the caller's rays and points under the same block.
       NOT OFFERED: the CLOSEUP / CLOUDLESS / UNLIT builds or SBX_APP_PLANET_ATMOSPHERE under a world, a world for the literals
       listed above, a span model for the multi-GPU split (every block's span is the whole row), and the drop-in header
       sbx_mainimage.hpp, which has no way to state a block. */
    SBX_APP_PLANET_WORLD = 37
} sbx_app;

typedef enum sbx_status {
    SBX_OK = 0,
    SBX_ERR_ARG = -1,          /* NULL pointer, bad row range, bad resolution ... */
    SBX_ERR_UNSUPPORTED = -2,  /* app not on the accelerated path */
    SBX_ERR_HIP = -3,          /* a HIP runtime call failed; see sbx_last_error() */
    SBX_ERR_NO_DEVICE = -4,    /* no gfx950 device visible: the library never falls back to a CPU */
    SBX_ERR_FAULT = -5         /* a kernel reported an internal invariant violation on this device (sticky; sbx_fault_status) */
} sbx_status;

/* cbuffer b0 (src/uniform_buffer.h:25-30): u_res@c0.xy, u_mouse@c0.zw, u_time@c1.x.
 * On the C++/Shadertoy path these are iResolution / iMouse / iGlobalTime (:32-36). */
typedef struct sbx_uniforms {
    float u_res[2];
    float u_mouse[2];
    float u_time;
    float _pad[3];
} sbx_uniforms;

/* cbuffer b1 for APP_CLOUDS (src/uniform_buffer.h:39-55), same packoffsets and defaults.
 * Pass NULL as `aux` to get the defaults (what the C++/GLSL builds compile in, :13). */
typedef struct sbx_aux_clouds {
    float wind_dir[3];   float _pad0;   /* c0   default (0, 0, .2)     */
    float sun_dir[3];    float _pad1;   /* c1   default (0, 0, -1)     */
    float sun_color[3];  float _pad2;   /* c2   default (1, .7, .55)   */
    float sun_power;                    /* c3.x default 8              */
    int32_t cld_march_steps;            /* c3.y default 100            */
    int32_t illum_march_steps;          /* c3.z default 6              */
    float sigma_scattering;             /* c3.w default .15            */
    float cld_coverage;                 /* c4.x default .535           */
    float cld_thick;                    /* c4.y default 125            */
    float atm_radius;                   /* c4.z default 5000 (SKY_SPHERE only, unused) */
    float atm_ground_y;                 /* c4.w default 4750 (SKY_SPHERE only, unused) */
} sbx_aux_clouds;

/* cbuffer b1 for APP_SDF_AO (src/uniform_buffer.h:56-60) */
typedef struct sbx_aux_sdf_ao {
    float fog_density;   /* c0.x default .1 */
    float fog_falloff;   /* c0.y default .5 */
    float _pad[2];
} sbx_aux_sdf_ao;

/* the material parameters of ue4_render_clouds (app_clouds.usf:234-243) for SBX_APP_CLOUDS_UE4; NULL = the TWEAK block's
 * defaults (:4-7) with the SUN_DIR / WIND_DIR macros (:13-14, functions of u_time) */
typedef struct sbx_aux_clouds_ue4 {
    float coverage, thickness, absorbtion, fuzziness;   /* c0   defaults .50, 15, 1.030725, .035 */
    float sun_dir[3];    float _pad1;                   /* c1   used when use_dirs != 0 */
    float wind_dir[3];   int32_t use_dirs;              /* c2   use_dirs = 0: SUN_DIR / WIND_DIR of the shader */
} sbx_aux_clouds_ue4;
void sbx_aux_clouds_ue4_defaults(sbx_aux_clouds_ue4* aux);

/* the scene of SBX_APP_RAYTRACER_SCENE: plain data, 1376 bytes, in 16-byte registers like the other blocks */
#define SBX_RT_MAX_PLANES 16
#define SBX_RT_MAX_SPHERES 16
typedef struct sbx_rt_material { float base_color[3]; float metallic, roughness, ior, reflectivity, translucency; } sbx_rt_material; /* material.h:5-12; 32 B */
typedef struct sbx_rt_plane  { float direction[3]; float distance; int32_t material; int32_t _pad[3]; } sbx_rt_plane;   /* 32 B */
typedef struct sbx_rt_sphere { float origin[3];    float radius;   int32_t material; int32_t _pad[3]; } sbx_rt_sphere;  /* 32 B */
typedef struct sbx_aux_raytracer_scene {
    float eye[3];         float fov;            /* c0  fov = the FOV factor of main.h:45, used as given */
    float look_at[3];     int32_t bounces;      /* c1  the `2` of app_raytracer.h:96; 1..8 */
    float light_L[3];     int32_t light_type;   /* c2  lights[0]: 1 = LIGHT_POINT, 2 = LIGHT_DIR (light.h:5-12) */
    float light_color[3]; int32_t lighting;     /* c3  0 = illum_cook_torrance, 1 = illum_blinn_phong's Phong branch (:61) */
    float ambient[3];     int32_t shadow;       /* c4  ambient_light (light.h:16); shadow 1 = the `#if 1` of :107, 0 = off */
    int32_t n_planes, n_spheres, _pad[2];       /* c5  0..16 each */
    sbx_rt_material materials[8];               /* num_materials slots; id 0 is mat_debug */
    sbx_rt_plane planes[SBX_RT_MAX_PLANES];     /* taken in array order, as raytrace_iteration does */
    sbx_rt_sphere spheres[SBX_RT_MAX_SPHERES];
} sbx_aux_raytracer_scene;
/* Host only, no context: what setup_scene + setup_camera + :138 of src/app_raytracer.h make of these uniforms — the u_mouse rotation
 * of the eye, the u_time animation of the left sphere, the right sphere and the light (unless at_rest: the `#if 0` of :29, u_time not
 * read), fov = tan(radians(30.)) of the math spec, bounces 2, point light, Cook-Torrance, shadow on, ambient .01, 6 planes, 3 spheres.
 * The block SBX_APP_RAYTRACER_SCENE renders when aux is NULL is this one with at_rest = 0. */
void sbx_raytracer_scene_cornell(const sbx_uniforms* uni, int at_rest, sbx_aux_raytracer_scene* out);

/* the field and the renderer settings of SBX_APP_SDF_SCENE: plain data, 2784 bytes.  (app_sdf_ao.h:N names the line of
 * src/app_sdf_ao.h whose literal the value replaces.) */
#define SBX_SDF_MAX_INSTR 32
#define SBX_SDF_MAX_STACK 4
enum { SBX_SDF_PLANE = 1, SBX_SDF_SPHERE, SBX_SDF_BOX, SBX_SDF_TORUS, SBX_SDF_Y_CYLINDER, SBX_SDF_CYLINDER, SBX_SDF_CAPSULE, SBX_SDF_BEZIER,
       SBX_SDF_ADD = 16, SBX_SDF_SUB, SBX_SDF_INTERSECT, SBX_SDF_BLEND,
       SBX_SDF_OBJECT = 32 };
typedef struct sbx_sdf_instr {            /* 80 B */
    int32_t op, rot_axis;                 /* rot_axis 0 none, 1 x, 2 y, 3 z */
    float rot_deg; int32_t material;      /* material: SBX_SDF_OBJECT only, 0..7 */
    float offset[3]; float _pad;
    float a[4], b[4], c[4];
} sbx_sdf_instr;
typedef struct sbx_aux_sdf_scene {        /* 2784 B */
    float eye[3];        float fov;               /* main.h's FOV factor, as given (app_sdf_ao.h:313 has 1.) */
    float look_at[3];    int32_t march_steps;     /* :249, 1..512 (70) */
    float sun_dir[3];    float march_end;         /* :209 USED AS GIVEN, never normalised; :250 (20.) */
    float background[3]; int32_t shadow;          /* :11; the `#if 0` of :269: 0 | 1 */
    float fog_density, fog_falloff; int32_t view, checker_material;   /* view 0 shaded, 1 = the `#if 0` of :217 (normals); checker: the id that gets :237-240, -1 none */
    int32_t n_instr, _pad[3];
    float materials[8][4];                        /* rgb, pad */
    sbx_sdf_instr program[SBX_SDF_MAX_INSTR];
} sbx_aux_sdf_scene;
/* Host only, no context: the block SBX_APP_SDF_SCENE renders when aux is NULL.  app_sdf_ao.h's camera for u_time (setup_camera :45-50),
 * FOV 1, sun = normalize(1, 2, 1) of the math spec, the six shipped materials (slots 6 and 7 zero), background (.1, .1, .7), fog
 * .1 / .5, 70 steps, end 20, shadow 0, view 0, checker material 1, and as the program ONE ramp of sdf_pipe (:54-113) in sdf_pipe's own
 * coordinates plus the ground plane, 20 instructions:
 *     box (0,1,0) size; y-cylinder rotated x -90 at (0 + .7, 1 + .5, 0 + 0); SUB; OBJECT 2          the ramp
 *     y-cylinder rotated x -90 at (0 + (-1.3 + .525), 1 + 1, 0 + 0); OBJECT 5                       the coping bar
 *     rail box, bars 1 2 ADD 3 ADD 4 5 ADD ADD, ADD; OBJECT 4                                        the deck railing (stack depth 4)
 *     plane (0, 1, 0), 0; OBJECT 1                                                                   the ground
 * Each offset is the binary32 value (o1 - o2) of the reference's two successive offsets `p = pos - o1; p + o2` or (o1 + o2) of
 * `p = pos - o1; p -= o2`, component by component — ONE subtraction per primitive where the reference makes two, so the frame is
 * a new one, not SBX_APP_SDF_AO's; that frame's nested rotate_around_y(180) (:134) and its tree of vec2 unions (:108-110, :137,
 * :147-149) are not expressible in this block either. */
void sbx_sdf_scene_ramp(const sbx_uniforms* uni, sbx_aux_sdf_scene* out);

/* the pose of SBX_APP_EGG_POSE and sbx_egg_eval: plain data, 64 bytes.  (:N names the line of src/app_egg.h whose value the field
 * replaces.) */
typedef struct sbx_aux_egg_pose {          /* 64 B */
    float eye[3];        float fov;        /* :25; :253 (main.h's FOV factor, as given) */
    float look_at[3];    float turn_deg;   /* :26; the angle handed to rotate_around_y at :40 (the reference: u_time * -100.0) */
    float left_foot[3];  float femur;      /* left_foot_pos of :74 as a value; :80 */
    float right_foot[3]; float tibia;      /* right_foot_pos of :77; :81 */
} sbx_aux_egg_pose;
/* Host only, no context: what setup_camera and sdf() of app_egg.h make of uni->u_time, the block SBX_APP_EGG_POSE renders when aux is
 * NULL.  The feet are wheel_pos + mul(rotate_around_z(-u_time * 400.), (0, +-.3, +-.2)) by the math spec, turn_deg is the binary32
 * product u_time * -100.0f, femur .8, tibia .75, eye (0, .25, 5.25), look_at (0, .25, 0), fov 1. */
void sbx_egg_pose_default(const sbx_uniforms* uni, sbx_aux_egg_pose* out);

/* the deck of SBX_APP_VINYL_DECK and sbx_vinyl_eval: plain data, 128 bytes.  (:N names the line of src/app_vinyl.h whose value the field
 * replaces.) */
typedef struct sbx_aux_vinyl_deck {        /* 128 B */
    float eye[3];            float fov;               /* :61;  :460 (main.h's FOV factor, as given) */
    float look_at[3];        float platter_deg;       /* :62;  `rot` as handed to rotate_around_y at :427 (the reference: u_time * 200.; the
                                                         SHADERTOY build's scratching hand of :422-424 puts u_mouse.y here) */
    float sun_dir[3];        float platter_tilt_deg;  /* :284-285, used as given, never normalised;  the angle handed to rotate_around_x at :428 */
    float groove_color[3];   float arm_tilt_deg;      /* :45;  the angle handed to rotate_around_x at :141-142 */
    float dead_wax_color[3]; float ro_spec;           /* :47;  :327 */
    float label_color[3];    float a_x;               /* :49;  :328 */
    float logo_color[3];     float a_y;               /* :51;  :329 */
    float shiny_color[3];    float shininess;         /* :53;  the 50. of :375 */
} sbx_aux_vinyl_deck;
/* Host only, no context: what app_vinyl.h makes of uni->u_time by the math spec, the block SBX_APP_VINYL_DECK renders when aux is NULL.
 * platter_deg is the binary32 product u_time * 200.f, platter_tilt_deg sin(u_time) * .1f, arm_tilt_deg sin(u_time * 3.6758f) * .1f,
 * sun_dir the spec's normalize(-1, 4, -3), the colours the literals of :40-54, ro_spec .0725, a_x .025, a_y .5, shininess 50, fov 1,
 * eye (0, 5.75, 6.75), look_at (0, -2.5, 0). */
void sbx_vinyl_deck_default(const sbx_uniforms* uni, sbx_aux_vinyl_deck* out);

/* the air of SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval: plain data, 128 bytes.  (:N names the line of src/app_atmosphere.h
 * whose value the field replaces.) */
typedef struct sbx_aux_atmosphere_air {    /* 128 B */
    int view;                                         /* 0: the FROM_SPACE build's render (:190-209); 1: the build without it (:210-225) */
    int num_samples, num_samples_light;               /* :47-48; 1 ... 64 and 1 ... 32 */
    int reserved0;                                    /* must be 0 */
    float eye[3];            float fov;               /* the ray origin of :205 (view 0), the eye of :172 (view 1);  FOV (:230) */
    float look_at[3];        float hg_g;              /* :173, read by view 1 only;  :12, as henyey_greenstein_phase_func reads it */
    float sun_dir[3];        float sun_power;         /* the sun as given (setup_scene's rotation does not run), never normalised;  :41 */
    float betaR[3];          float hR;                /* :29;  :34 */
    float betaM[3];          float hM;                /* :30;  :35 */
    float earth_radius, atmosphere_radius;            /* :37-38: the height reference and (view 1) the terrain plane;  the `atmosphere` sphere */
    float reserved[6];                                /* must be 0 (as bit patterns) */
} sbx_aux_atmosphere_air;
/* Host only, no context: the reference's numbers, with the sun that setup_scene (:177-181) makes of uni->u_time by the math spec — the
 * block SBX_APP_ATMOSPHERE_AIR renders when aux is NULL (view 0).  eye (0, earth_radius + 1, 0) and look_at (0, earth_radius + 1.5, -1)
 * in both views, fov 1, counts 16 / 8.  A view other than 0 or 1 is written as given (and refused by the app). */
void sbx_atmosphere_air_default(const sbx_uniforms* uni, int view, sbx_aux_atmosphere_air* out);

/* the world of SBX_APP_PLANET_WORLD: plain data, 224 bytes.  (:N names the line of src/app_planet.h whose literal the field
 * replaces.) */
typedef struct sbx_aux_planet_world {      /* 224 B */
    float eye[3];            float fov;             /* :55;  :369 (main.h's FOV factor, as given) */
    float look_at[3];        float tilt_deg;        /* :56;  the angle handed to rotate_around_y at :307 (27) */
    float sun_dir[3];        float spin_deg;        /* the vector :288 multiplies by local_xform, as given, never normalised;  the angle
                                                       handed to rotate_around_x at :308 (the reference: u_time * -12.) */
    float key_color[3];      float cloud_spin_deg;  /* c_L of :224;  the angle of :309 (the reference: u_time * 8.) */
    float terrain_offset[3]; float max_height;      /* the vec3 of :180 and :193 (one field, both lines);  :20 */
    float cloud_offset[3];   float cld_coverage;    /* the vec3 of :107;  :110 */
    float band[3];           float cld_fuzzy;       /* the .2, .35, .65 of :114;  :111 */
    float c_water[3];        float l_water;         /* :258;  :265 */
    float c_grass[3];        float l_shore;         /* :259;  :266 */
    float c_beach[3];        float l_grass;         /* :260;  :267 */
    float c_rock[3];         float l_rock;          /* :261;  :268 */
    float c_snow[3];         float absorb;          /* :262;  vol_coeff_absorb :68 */
    float cloud_light;                              /* the .055 of :76 */
    int terr_steps, cloud_steps, shadow_steps;      /* TERR_STEPS :165 (1 ... 512);  the `steps` of :127 (1 ... 256) and of :148 (1 ... 32) */
    unsigned reserved[4];                           /* must be 0 */
} sbx_aux_planet_world;
/* Host only, no context: the header's numbers — eye (0, 0, -2.5), look_at (0, 0, 2), fov the spec's tan(radians(30)), tilt 27, the sun
 * the spec's normalize(1, 1, 0), key (7, 5, 3), counts 120 / 75 / 5 — with spin_deg and cloud_spin_deg the binary32 products
 * u_time * -12.f and u_time * 8.f: the block SBX_APP_PLANET_WORLD renders when aux is NULL. */
void sbx_planet_world_default(const sbx_uniforms* uni, sbx_aux_planet_world* out);

typedef struct sbx_ctx sbx_ctx;

/* Fill the aux blocks with the reference's defaults. */
void sbx_aux_clouds_defaults(sbx_aux_clouds* aux);
void sbx_aux_sdf_ao_defaults(sbx_aux_sdf_ao* aux);

/* Create / destroy a context bound to HIP device `device`.  Owns only small device scratch
 * (APP_CLOUDS' per-frame y tables, timing events, the cached frame of sbx_main_image); the
 * framebuffer of the render calls always belongs to the caller.
 * APP_CLOUDS (and its HEIGHT / LUMINANCE builds) also allocates, on the first eager launch that can use it, a table of the lattice
 * hashes its frames index: 2 MB for frames whose noise lattice indices stay below 2^18 (the default frame: 6.4e4), a larger one —
 * the next power of two — when a frame's bound outgrows it, at most 32 MB (indices below 2^22; frames beyond that keep the kernels
 * that hash per wave).  Tables are never rebuilt; all of them together stay below 64 MB and are freed by sbx_destroy.  Nothing is
 * allocated inside a stream capture.
 * THE VIEW TABLE.  The same apps also keep, per camera, what a pixel computes outside its march — sky colour, phase value, horizon
 * weight — for every pixel of the full frame: 20 bytes per frame pixel per key, two keys per context (166 MB for one 3840 x 2160
 * camera, 332 MB if a second camera of that size alternates with it).  The key is the camera, the sun (sun_dir, sun_color) and u_res;
 * u_time, the wind and the cloud parameters are no part of it.  A table is built on the stream of the third consecutive eager launch
 * of a key (counted over the launches that may read one), so a camera that moves every frame never builds one; a slot is given to another key only after the launches that read it
 * have completed; only one-rank frame and row-range launches under a sun on the z axis (sun_dir.x = sun_dir.y = 0, the default; the
 * HEIGHT build under any sun) read one — never a point list, a span or a multi-rank strip, nor SBX_APP_CLOUDS_SKY.  A frame whose table would exceed SBX_CLOUDS_VIEWTAB_DEFAULT_BYTES (7680 x 4320: 664 MB) gets none and
 * renders with the kernels that compute these values per pixel: the pixels are the same bits either way.  The environment variable
 * SBX_CLOUDS_VIEWTAB=0 (read once per process) switches the tables off.  Freed by sbx_destroy. */
#define SBX_CLOUDS_VIEWTAB_DEFAULT_BYTES ((size_t)256 << 20)
int sbx_create(int device, sbx_ctx** out);
void sbx_destroy(sbx_ctx* ctx);

/* Render rows [y0, y1) of the frame described by `uni` (u_res = full frame size) for `app`.
 * `rgba` points at device memory for row y0: pixel (x, y) lands at rgba[((y - y0) * W + x) * 4].
 * This is the replacement of "for every pixel: mainImage(fragColor, fragCoord)". */
int sbx_render_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux,
                    int y0, int y1, float* rgba, void* stream);
/* The same rows for a host that owns a HOST framebuffer (SURVEY.md 8b "Entry signature": rgba_device_or_host; the reference's
 * harness loops mainImage over a host surface, src/main.h:6-53): `rgba_host` is host memory for row y0, 4-byte aligned, in the
 * context's output format (16 or 4 bytes per pixel).  The rows are rendered into a staging buffer of the context, behind whatever
 * `stream` holds, and copied out; returns when all pixels are in `rgba_host`.  Pinned memory (hipHostMalloc / hipHostRegister): up to
 * sixteen strips, each copied at the link's rate while the next ones render (CLOUDS 4K 3.55 ms for a 2.7 ms kernel at these clocks
 * + 2.3 ms of copy; an 8K frame 10 ms for 9.3 ms of copy).
 * Pageable memory: one strip, one synchronous copy.  Not capturable; one caller per context.
 * (sbx_render_rows itself accepts any DEVICE-ACCESSIBLE pointer: handed pinned host memory, the kernel's own stores cross PCIe —
 * no staging, one launch; profiles/r05_host_boundary.txt has both.) */
int sbx_render_rows_host(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux,
                         int y0, int y1, void* rgba_host, void* stream);

/* The reference's own per-pixel entry, for hosts that keep their pixel loop:
 *     void mainImage(out vec4 fragColor, in vec2 fragCoord)            src/main.h:6-9
 * (what the absent VML/SDL harness calls per pixel, src/Makefile:21).  mainImage is a function of fragCoord — it divides it
 * by u_res (main.h:40) and never snaps or clamps it — and so is this call:
 *   - fragCoord = the centre (x + .5, y + .5) of a pixel of the frame (y = 0 at the bottom row) and u_res whole numbers: the
 *     first call for a given (app, uniforms, aux) renders the whole frame on the GPU with one launch and brings it to pinned
 *     host memory — the kernel's own stores cross PCIe, no copy follows it; later calls read their pixel from it;
 *   - ANY other fragCoord (off-centre: a supersampling host; outside the frame; a fractional u_res): evaluated exactly at that
 *     coordinate by a one-point launch (sbx_main_image_batch with n = 1) — never another pixel's sample.
 * Safe to call from several host threads on one context (serialised inside); hosts with many samples per frame should use
 * sbx_main_image_batch or sbx_render_points. */
int sbx_main_image(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux,
                   const float fragCoord[2], float fragColor[4]);
/* mainImage at n arbitrary fragCoords in ONE launch: the per-pixel entry in the shape a GPU can serve (n samples of a
 * supersampling / jittering / foveated host).  Nothing is cached and nothing is assumed about the coordinates; u_res may be any
 * positive finite numbers.  sbx_main_image_batch: host arrays (fragCoords n x 2 floats in, fragColors n x 4 floats out),
 * staged through pinned memory, returns when the colours are there.  sbx_render_points: device arrays (frag n x 2, rgba n x 4,
 * 16-byte aligned), asynchronous on `stream`. */
int sbx_main_image_batch(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, size_t n,
                         const float* fragCoords, float* fragColors);
int sbx_render_points(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, size_t n,
                      const float* frag, float* rgba, void* stream);

/* Render the cyclic row-blocks owned by one rank of an N-way split: blocks of
 * `block_rows` rows, rank r owns blocks r, r+N, r+2N, ...  The rank's rows are written densely,
 * in increasing y, into `rgba` (capacity sbx_rank_rows() rows).  Each pixel is computed from its
 * GLOBAL (x, y), so the assembled frame is bit-identical to a 1-GPU render. */
int sbx_render_rank(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux,
                    int block_rows, int rank, int nranks, float* rgba, void* stream);
/* Same, restricted to slab rows [r0, r1) of the rank (r1 is clipped to sbx_rank_rows()); `rgba` points at
 * slab row r0.  Lets a host pipeline the slab in groups: render group g, start its transfer, render g+1. */
int sbx_render_rank_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux,
                         int block_rows, int rank, int nranks, int r0, int r1, float* rgba, void* stream);
/* Number of rows rank `rank` owns (<= sbx_rank_rows_max). */
int sbx_rank_rows(int height, int block_rows, int rank, int nranks);
/* Rows every rank's buffer must hold so that an equal-count gather works: max over ranks. */
int sbx_rank_rows_max(int height, int block_rows, int nranks);
/* Root-side frame assembly after the gather: `gathered` holds nranks slabs of
 * sbx_rank_rows_max() rows each (rank-major); scatter them to their global rows of `frame`. */
int sbx_assemble(sbx_ctx* ctx, int width, int height, int block_rows, int nranks,
                 const float* gathered, float* frame, void* stream);

/* The same split with ROOT RELIEF.  Rank 0, the gather's root, also receives nranks - 1 slabs and assembles the frame;
 * so that it does not become the slowest rank it can be dealt fewer row-blocks: blocks go out in cycles of `rounds`
 * rounds, a round gives one block to every rank, and rank 0 is left out of the rounds >= root_rounds
 * (0 <= root_rounds <= rounds; root_rounds = rounds = 1 is the plain cyclic split of the calls above).
 * sbx_render_split renders slab rows [r0, r1) of `rank` (r1 is clipped to the rank's row count), sbx_split_rows_max
 * is the slab height every rank allocates, sbx_assemble_split the root-side scatter. */
int sbx_split_rank_rows(int height, int block_rows, int rank, int nranks, int root_rounds, int rounds);
int sbx_split_rows_max(int height, int block_rows, int nranks, int root_rounds, int rounds);
int sbx_render_split(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                     int nranks, int root_rounds, int rounds, int r0, int r1, float* rgba, void* stream);
int sbx_assemble_split(sbx_ctx* ctx, int width, int height, int block_rows, int nranks, int root_rounds, int rounds,
                       const float* gathered, float* frame, void* stream);
/* The rows of `rank` written IN PLACE: `frame` is a full-size frame (height * width pixels) and every row of the rank
 * lands at its global position; the other ranks' rows are not touched.  What the owner of the frame uses for its own share
 * (no slab, no assembly pass). */
int sbx_render_split_in_place(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                              int nranks, int root_rounds, int rounds, float* frame, void* stream);
/* The direct exchange of a one-process-per-GPU host (the reference has no multi-device path; SURVEY.md 8e "Collective": the
 * peers' row-blocks go to the root by point-to-point sends, the root's own rows never move).  The alpha of every pixel is the
 * constant 1 that mainImage's caller writes (src/main.h:52), so a peer's slab crosses xGMI as 3 floats per pixel:
 * sbx_render_split_rgb = sbx_render_split with a slab of rows x width x 3 floats (12 bytes per pixel, 25 % fewer bytes on
 * the link and in the root's HBM).  sbx_assemble_peers scatters the slabs of ranks 1 .. nranks-1 (`peers`: rank-major,
 * sbx_split_rows_max() rows each, `channels` = 3 or 4 floats per pixel) to their global rows of the RGBA `frame`, writing
 * alpha = 1 for 3-channel slabs, and leaves the rows of rank 0 — rendered with sbx_render_split_in_place — untouched. */
int sbx_render_split_rgb(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                         int nranks, int root_rounds, int rounds, int r0, int r1, float* rgb, void* stream);
int sbx_assemble_peers(sbx_ctx* ctx, int width, int height, int block_rows, int nranks, int root_rounds, int rounds,
                       int channels, const float* peers, float* frame, void* stream);

/* ---- The span exchange: only the EXPENSIVE part of a row-block is sharded -----------------------------------------------
 * (The reference has no multi-device path; this is the build's answer to SURVEY.md 8e at the sizes where the one exchange step
 * is link-bound: at 7680x4320 a peer's 3-channel slab is 49.8 MB, 0.65 ms on one xGMI link at its 76.8 GB/s peak, against 0.47 ms
 * of APP_ATMOSPHERE rendering per rank.)  Several apps leave mainImage through an early exit over a large part of the frame:
 * APP_CLOUDS below the horizon (src/app_clouds.h:212), APP_ATMOSPHERE outside the dome and where the view ray dives under the
 * ground (src/app_atmosphere.h:196-207, 65-67), APP_PLANET where the ray misses the atmosphere shell (src/app_planet.h:315-321).
 * sbx_span_table gives, for every row-block g of the split, the interval [x0, x1) of columns (multiples of 64) OUTSIDE of which
 * the host expects only such cheap pixels — a hint computed with the kernels' own tests at tile corners, widened by a tile:
 *   - a peer renders and sends only the spans of its blocks, packed block after block, 3 floats per pixel (sbx_render_span_peer);
 *   - the frame's owner renders its own blocks AND everything outside the other blocks' spans, in place, with ONE launch over the
 *     frame (sbx_render_span_root), receives the packed slabs (still exactly one exchange step) and scatters them, writing alpha
 *     (sbx_assemble_spans).
 * Whoever renders a pixel runs the app's full kernel on its global coordinates: the table moves work and bytes, never a bit of
 * the image.  Apps without a model get whole rows (the exchange then equals the direct one).
 *
 * sbx_span_table (host only; no context, no GPU): table = 4 int32 per row-block {x0, x1, offset of the block's span in its
 * owner's packed slab (pixels), owner rank} or NULL; rank_pixels = nranks int64 (pixels of every rank's packed slab; rank 0's
 * counts its own spans, which never travel) or NULL; max_width = the widest span among the peers' blocks or NULL.  Returns the
 * number of row-blocks or a negative sbx_status.  The table depends on (app, u_res, u_mouse, split) only.
 * sbx_render_span_peer: slab rows [r0, r1) (whole blocks; r1 clipped) of peer `rank` (1 .. nranks-1); `rgb` is the START of the
 * rank's packed slab (3 * rank_pixels[rank] floats): the table's offsets are absolute in it, so a host can render and send the
 * slab in pieces.  sbx_assemble_spans: `peers` holds the slab of rank r at (r - 1) * stride_pixels * 3 floats.
 * The context keeps the device copies of the last few tables; a frame whose table is not on the device yet cannot be recorded
 * into a stream capture (render it once before). */
int sbx_span_table(int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks, int root_rounds, int rounds,
                   int32_t* table, int64_t* rank_pixels, int32_t* max_width);
int sbx_render_span_peer(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank, int nranks,
                         int root_rounds, int rounds, int r0, int r1, float* rgb, void* stream);
int sbx_render_span_root(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks,
                         int root_rounds, int rounds, float* frame, void* stream);
int sbx_assemble_spans(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks,
                       int root_rounds, int rounds, const float* peers, int64_t stride_pixels, float* frame, void* stream);

/* ---- The store exchange: the peers render IN PLACE into the owner's frame ------------------------------------------------
 * (The reference has no multi-device path; this is the form of the ONE exchange step in which the frame's owner
 * does nothing for the others: no landing area, no receive kernels, no scatter pass.)  The owner allocates the frame through the
 * library and exports it; every peer — another PROCESS on another (or the same) GPU: hipIpcGetMemHandle / hipIpcOpenMemHandle; or
 * another rank of the same process: the pointer itself — maps it and renders its row-blocks of the split straight into it with
 * sbx_render_split_in_place[_rgb]: the exchange is the render kernels' own pixel stores over xGMI, 16 bytes per pixel (float4),
 * 12 (sbx_render_split_in_place_rgb: three dwords; the alpha of every pixel is the constant 1 of src/main.h:52, written once when the
 * frame is created) or 4 (SBX_FORMAT_RGBA8).  Two small flag kernels per frame and rank order it, through a page of fine-grained
 * memory next to the frame:
 *     owner:  sbx_shared_frame_begin (stream-ordered behind whatever read the previous frame: tells the peers the frame may be
 *             overwritten) .. its own sbx_render_split_in_place .. sbx_shared_frame_end (the stream continues when every peer's
 *             rows of THIS frame are in place);
 *     peer r: sbx_shared_frame_begin (waits for the owner's go) .. sbx_render_split_in_place .. sbx_shared_frame_end (signals).
 * Every rank calls begin / end once per frame, in order; frames of one sbx_shared are sequential, a host keeps several frames in
 * flight with several sbx_shared (one per stream).  A wait that sees no signal for ~10 s raises the device's fault word
 * (sbx_fault_status) instead of hanging.  Pixels are written by the app's full kernel from their global coordinates, so the frame
 * is bit-identical to a one-GPU render.
 * sbx_shared_create: `frame_bytes` = height * width * (16 or 4); nranks >= 1.  sbx_shared_export fills an opaque handle that may
 * be sent to the other processes by any means (it holds no pointers valid elsewhere); sbx_shared_open maps it on `ctx`'s device.
 * sbx_shared_frame = the frame's address in THIS process.  Closing the owner's object frees the frame: close the peers' first. */
typedef struct sbx_shared sbx_shared;
typedef struct sbx_shared_handle { unsigned char opaque[192]; } sbx_shared_handle;
int sbx_shared_create(sbx_ctx* ctx, size_t frame_bytes, int nranks, sbx_shared** out);
int sbx_shared_export(sbx_shared* s, sbx_shared_handle* handle);
int sbx_shared_open(sbx_ctx* ctx, const sbx_shared_handle* handle, sbx_shared** out);
void sbx_shared_close(sbx_shared* s);
float* sbx_shared_frame(sbx_shared* s);
size_t sbx_shared_bytes(sbx_shared* s);            /* bytes of the frame (as given to sbx_shared_create), on either side */
int sbx_shared_frame_begin(sbx_shared* s, int rank, void* stream);
int sbx_shared_frame_end(sbx_shared* s, int rank, void* stream);
/* The store exchange with SPANS (the two ideas together, for frames whose pixel stores would bind a link: 7680x4320 in float
 * pixels): a peer renders only the spans of its row-blocks (sbx_span_table) — in place, into the owner's mapped frame, `channels` = 3
 * or 4 dwords per float pixel — and the owner renders its own blocks and everything outside the spans with sbx_render_span_root.
 * No slab, no landing area, no scatter; the links carry the expensive pixels only (29.7 instead of 49.8 MB per peer at 7680x4320). */
int sbx_render_span_peer_in_place(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                                  int nranks, int root_rounds, int rounds, int channels, float* frame, void* stream);
/* sbx_render_split_in_place writing only R, G, B of every float4 pixel (three dwords at a 16-byte stride); under
 * SBX_FORMAT_RGBA8 it is sbx_render_split_in_place. */
int sbx_render_split_in_place_rgb(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                                  int nranks, int root_rounds, int rounds, float* frame, void* stream);

/* The write into hlsltoy's DXGI_FORMAT_R8G8B8A8_UNORM back buffer (util/hlsltoy/src/hlsltoy.cpp:79,192): float RGBA
 * rows -> 8-bit RGBA by the Direct3D float -> UNORM rule (NaN -> 0, clamp to [0, 1], * 255 + .5, truncate).
 * `rgba` and `out` are device pointers (width * rows pixels each); flip_y != 0 writes the top row first
 * (D3D / image-file order; the float frame has row 0 at the bottom). */
int sbx_pack_unorm8(sbx_ctx* ctx, int width, int rows, const float* rgba, unsigned char* out, int flip_y,
                    void* stream);

/* OUTPUT FORMAT of the frame-granular entry points (default SBX_FORMAT_RGBA32F).  With SBX_FORMAT_RGBA8 every pixel a render
 * call writes — whole frames, strips, a rank's slabs (4- or "3-channel"), span slabs, in-place renders — is ONE 32-bit word
 * R | G << 8 | B << 16 | 255 << 24 by the Direct3D float -> UNORM rule of sbx_pack_unorm8 (the display format of the
 * reference's hosts: hlsltoy's R8G8B8A8_UNORM back buffer), written by the render kernel itself instead of its float pixel: the
 * `float*` buffers of those calls then hold width * rows words (4-byte aligned), and the assembly calls (sbx_assemble*,
 * sbx_assemble_peers with any `channels`, sbx_assemble_spans) move such words.  A frame rendered this way equals
 * sbx_pack_unorm8(flip_y = 0) of the float frame, bit for bit.  What it is for: a multi-GPU exchange that carries 4 instead of
 * 12 bytes per pixel (a 7680x4320 frame at 8 GPUs is bound by the 7 xGMI links into the root in float pixels), and a frame
 * that is written once in the format it is shown in.  sbx_render_points, sbx_main_image and sbx_main_image_batch always
 * return float colours. */
enum { SBX_FORMAT_RGBA32F = 0, SBX_FORMAT_RGBA8 = 1 };
int sbx_set_output_format(sbx_ctx* ctx, int format);

/* PRECISION TIER of the frame-granular and per-pixel entry points (default SBX_PRECISION_EXACT: every pixel bit-identical to the
 * CPU oracle of this repository).  SBX_PRECISION_1E4 is a labelled, opt-in tolerance tier for SBX_APP_ATMOSPHERE and
 * SBX_APP_ATMOSPHERE_GROUND only (every other app ignores it and stays exact): BASELINE.json's bar is 1e-4 per float channel against
 * the C++ reference, not bit-equality, and get_incident_light (src/app_atmosphere.h:50-160: 336 exp per sky pixel, no threshold that
 * amplifies a rounding difference) meets it with the hardware's binary32 exp2 in place of the math spec's binary64 table form — about
 * half the frame time.  SBX_APP_ATMOSPHERE: max |diff| against the oracle over every pixel of the 7680x4320 frame and over a sweep of
 * sun positions is asserted in the tests (measured 2.4e-7).  SBX_APP_ATMOSPHERE_GROUND: max |tier - exact| over every pixel of the
 * 3840x2160 frame at u_time 0, .37, 2, 3.1 and 100.25 is asserted <= 1e-4; measured 4.8e-7 (at u_time 2 and 3.1, where channels
 * reach 2.96 and 1.79 near the sun); ground pixels are exact, and sbx_set_variant(1) (sbx_test.h) renders the exact frame under it.
 * Not offered for APP_CLOUDS / APP_PLANET: their coverage and density edges turn a 1-ulp difference into 1e-3 pixels. */
enum { SBX_PRECISION_EXACT = 0, SBX_PRECISION_1E4 = 1 };
int sbx_set_precision(sbx_ctx* ctx, int precision);

/* Counters of a context since its creation (or the last sbx_reset_stats): what a host or a test reads to see what its calls
 * turned into.  render_launches = render-kernel launches enqueued by any entry point; main_image_hits = sbx_main_image calls
 * served from the cached frame; main_image_frames = whole frames sbx_main_image rendered; main_image_points = one-point launches. */
typedef struct sbx_stats {
    uint64_t render_launches;
    uint64_t main_image_hits;
    uint64_t main_image_frames;
    uint64_t main_image_points;
    uint64_t _reserved[4];
} sbx_stats;
int sbx_get_stats(sbx_ctx* ctx, sbx_stats* out);
int sbx_reset_stats(sbx_ctx* ctx);

/* Per-launch timing: when enabled, every render call brackets its kernel with HIP events on the
 * launch stream; sbx_last_kernel_ms() synchronises on the last pair and returns the duration. */
int sbx_set_timing(sbx_ctx* ctx, int enabled);
int sbx_last_kernel_ms(sbx_ctx* ctx, float* ms);

/* The noise library as standalone functions over n points (xyz interleaved, device arrays), 3 floats out
 * per point: "noise_iq" (src/noise_iq.h:11-29, out[0]); "hash_w" (src/noise_worley.h:5-17);
 * "noise_w" (:20-51; params[0] = domain_repeat; out = sqrt F1, sqrt F2, |cell id|);
 * "fbm_worley_tile" (src/fbm.h:8 as instantiated at util/ddsvolgen/src/ddsvolgen.cpp:52;
 * params = lacunarity, init_gain, gain; out[0]); "worley_fbm" (src/app_func.h:41-47 over :17-39: the nine noise_w of
 * SBX_APP_FUNC at the point, out[0]; params unused).
 * (include/sbx_test.h documents three more names that exist for the parity tests of the recorded-domain forms.) */
int sbx_noise_eval(sbx_ctx* ctx, const char* fn, const float* xyz, const float* params, float* out,
                   size_t n, void* stream);
/* The Rayleigh/Mie scattering solver (src/app_atmosphere.h:50-160) as standalone functions over n rays of the caller's and a sun
 * of the caller's: what the reference reaches only through its cameras and u_time.  `rays`: device memory, n x 6 floats (origin
 * xyz, direction xyz; metres, planet centre at 0, earth_radius 6360e3, atmosphere_radius 6420e3); `out`: device memory, n x 3 floats,
 * not overlapping `rays`; both need only 4-byte alignment.  `sun_dir`: HOST memory, 3 floats, read during the call and used as
 * given — never normalised, as the reference never normalises its rotated (0, 1, 0).
 *   "get_incident_light" (:78-160): out = the linear RGB along the ray (no camera, no sRGB, no alpha); (0, 0, 0) where isect_sphere
 *       is false (:85-88).
 *   "get_sun_light" (:50-76): out = {overground ? 1 : 0, optical_depthR, optical_depthM} along the ray itself, both depths starting
 *       at 0; where the march returns early (:66-67) the depths are the partial sums the reference leaves in its _inout
 *       arguments.  sun_dir is not read and may be NULL.
 * Exact for every bit pattern of input: NaN and inf are data.  Asynchronous on `stream` and capturable (no allocation, no wait); not
 * counted in sbx_stats.render_launches; sbx_set_precision does not enter.  n == 0 returns SBX_OK and touches nothing;
 * SBX_ERR_ARG for a NULL ctx / fn / rays / out, a NULL sun_dir with "get_incident_light", an unknown name, n > 2^31. */
int sbx_atmosphere_eval(sbx_ctx* ctx, const char* fn, const float* rays, const float* sun_dir, float* out,
                        size_t n, void* stream);
/* sbx_atmosphere_eval under the caller's air: the same two names, element layouts and contract, with every number of the solver —
 * betaR, betaM, hR, hM, both radii, sun_power, hg_g, the sample counts and the sun — read from `air` (HOST memory, read during the
 * call).  view, eye, look_at and fov are not read; the counts and the reserved words are checked as SBX_APP_ATMOSPHERE_AIR checks
 * them.  With the reference's solver numbers (sbx_atmosphere_air_default) the result is sbx_atmosphere_eval's with that sun in every
 * bit.  Exact for every bit pattern of block and rays.  Asynchronous on `stream` and capturable (no allocation, no wait); not counted
 * in sbx_stats.render_launches; sbx_set_variant 1 selects the plain statement for every wave (same bits).  n == 0 returns SBX_OK
 * and touches nothing; SBX_ERR_ARG, with nothing written, for a NULL ctx / fn / air / rays / out, an unknown name, n > 2^31, a count
 * out of range or a non-zero reserved word. */
int sbx_atmosphere_air_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_atmosphere_air* air, const float* rays, float* out,
                            size_t n, void* stream);
/* The SDF library on its own (src/sdf.h): sdf(pos) of SBX_APP_SDF_SCENE's program over the caller's points — the field's value
 * without a renderer: collision queries, a mesher's samples, another renderer's march.  `scene`: HOST memory, read during the call;
 * ONLY n_instr and program are read, and they are validated as SBX_APP_SDF_SCENE validates them (SBX_ERR_ARG, nothing written).
 * `xyz`: device memory, n x 3 floats; `out`: device memory, n x 2 floats — the distance, then the nearest object's material id as a
 * float — not overlapping `xyz`; both need only 4-byte alignment.  Exact for every bit pattern of input: NaN and inf are data.
 * Asynchronous on `stream` and capturable (no allocation, no wait); not counted in sbx_stats.render_launches; sbx_set_variant 1 / 3
 * select the IEEE roots as for the app.  n == 0 returns SBX_OK and touches nothing; SBX_ERR_ARG also for a NULL ctx / scene / xyz /
 * out and n > 2^31. */
int sbx_sdf_eval(sbx_ctx* ctx, const sbx_aux_sdf_scene* scene, const float* xyz, float* out, size_t n, void* stream);
/* SBX_APP_SDF_SCENE's renderer (src/app_sdf_ao.h, with sdf(pos) the block's program) as standalone functions over n elements of the
 * caller's, under the caller's block: what the app reaches only through its pinhole camera and into sRGB pixels — normals for a
 * mesher's vertices, an AO or soft-shadow bake at surface samples, hit points and materials for picking rays, the trace for another
 * lens, a probe grid or a reflection ray of a host's own integrator.  `scene`: HOST memory, read during the call, required and
 * validated as SBX_APP_SDF_SCENE validates it (the app's texts) whatever n is; its eye, look_at and fov are not read.  `in`, `out`:
 * device memory, not overlapping, 4-byte alignment suffices.  Per element:
 *   "sdf"                       in 3: pos.  out 2: the distance, then the material id as a float: the same bits as sbx_sdf_eval.
 *   "sdf_normal" (:152-163)     in 3: p.  out 3.
 *   "sdf_ao" (:165-181)         in 6: hit.origin xyz, hit.normal xyz.  out 1: the `c` of :179.
 *   "sdf_shadow" (:183-207)     in 6: ray origin xyz, direction xyz — the element's own direction, not the block's sun_dir: the
 *                               function takes any ray.  out 1.  It runs whatever the block's `shadow` says (the switch is
 *                               "render_impl"'s).
 *   "illuminate" (:211-243)     in 9: hit.origin xyz, hit.normal xyz, the material id as a float, ao, sh.  out 3.  int() of the id is
 *                               taken as for sbx_vinyl_eval — toward zero, saturating at the ends of int, 0 for a NaN.  An id outside
 *                               0..7 gives the zero colour: the port's choice, the reference's get_material leaves its result unset
 *                               there.  The checker test is int(id) == checker_material, as written.  Under view == 1 the result is
 *                               hit.normal (:217-219 compiled in).  The reference's `eye` argument enters only V (:220), which nothing
 *                               reads: it has no slot.
 *   "render_impl" (:245-285)    in 6: ray origin xyz, direction xyz.  out 5: rgb and t of the vec4 it returns, then the hit's material
 *                               id as a float, or -1 where :284 returned the background.  It runs under the block's march_steps,
 *                               march_end, shadow, view, background and materials.
 *   "render" (:287-311)         in 6: as above.  out 4: the LINEAR rgb after the fog and the `abs` (no sRGB, no alpha), then orig.w.
 *                               The fog's ray.origin.y and ray.direction.y are the element's.
 * Directions and normals are used as given, never normalised; sun_dir is used as given.  Every bit pattern is data, NaN results
 * included.  Asynchronous on `stream` and capturable (one kernel launch and nothing else); not counted in sbx_stats.render_launches;
 * sbx_set_variant 1 / 3 select the IEEE roots as for the app (same bits).  n == 0 returns SBX_OK with `in` and `out` not looked at;
 * SBX_ERR_ARG, with nothing written, for a NULL ctx / fn / scene / in / out, a block the app refuses (at n == 0 too), an unknown
 * name, n > 2^31.  tests/sdf_scene_eval_model.py is the definition. */
int sbx_sdf_scene_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_sdf_scene* scene, const float* in, float* out, size_t n, void* stream);
/* The volumetric clouds and their sky (src/app_clouds.h, the procedural build as shipped: SKY_SPHERE and USE_NOISE_TEX undefined, both
 * `#if 0` of illuminate_volume off) as standalone functions over n elements of the caller's: what the reference reaches only through
 * pixels of the one camera setup_camera fixes at (0, -.5, 0) — sky panoramas and cube faces, the sky a reflective surface of another
 * scene sees, the density field for the caller's own volume bake.  `aux`: HOST memory, read during the call, NULL = the reference's
 * defaults; validated as SBX_APP_CLOUDS validates its block (negative march steps: SBX_ERR_ARG, nothing written).  `in`, `out`: device
 * memory, not overlapping, 4-byte alignment suffices.  Per element:
 *   "render" (:204-218)            in 6: ray origin xyz, direction xyz.  out 4: the linear RGB render returns (no sRGB), then the alpha
 *                                  render_clouds returned for this ray — 0 where :212 returned the sky.
 *   "render_clouds" (:153-202)     in 6: as above.  out 4: the vec4 of :201.
 *   "render_sky_color" (:36-46)    in 3: eye_dir.  out 3.
 *   "density_func" (:62-86)        in 3: pos_in (this build does not read `height`).  out 1.
 *   "illuminate_volume" (:91-123)  in 6: origin xyz, V xyz; L is aux->sun_dir.  out 1.
 * The ray origin stands where the reference's eye.origin does (:166); u_time enters only through the wind offset (:167); there is no
 * camera, no u_res and no u_mouse.  Directions are used as given, never normalised; a ray with dir.y <= 0, a zero, NaN or inf component
 * is data: the result is whatever the reference's arithmetic gives.  Exact for every bit pattern of input.
 * Asynchronous on `stream` and capturable (inside a capture it allocates nothing, queries nothing and waits for nothing); not counted
 * in sbx_stats.render_launches; sbx_set_precision does not enter; sbx_set_variant 1 selects the plain statement (same bits).  n == 0
 * returns SBX_OK and touches nothing; SBX_ERR_ARG for a NULL ctx / fn / in / out, an unknown name, n > 2^31. */
int sbx_clouds_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_clouds* aux, float u_time, const float* in, float* out, size_t n,
                    void* stream);
/* The planet's terrain, cloud shell and shading (src/app_planet.h as shipped: CLOUDS and LIGHT defined) as standalone functions over n
 * elements of the caller's: what the reference reaches only through pixels of setup_camera's two views — an orbiting or landing
 * camera, a cube map of the planet, an equirectangular albedo / height bake, a collision query against the terrain.  There is no
 * camera, no u_res and no u_mouse.  `in`, `out`: device memory, not overlapping, 4-byte alignment suffices.  Per element:
 *   "render" (:303-367)                 in 6: ray origin xyz, direction xyz, in the space of `eye` (planet at 0, radius 1).  out 4: the
 *                                       linear RGB render returns (no sRGB), then cloud.alpha as read at :352 / :365 — 0 where :320
 *                                       returned the background.
 *   "terrain_march" (:311-342)          in 6: as above.  out 4: hit.t after intersect_sphere (no_hit's t where it missed), then t,
 *                                       df.x, df.y as they stand at :344 — the initialisers of :323-324 where :320 returned.
 *   "sdf_terrain_map" (:175-186)        in 3: pos (planet-local, i.e. after `rot`).  out 2.
 *   "sdf_terrain_map_detail" (:188-199) in 3: pos.  out 2.
 *   "sdf_terrain_normal" (:201-212)     in 3: p.  out 3.
 *   "clouds_density" (:106-114)         in 4: cloud.pos xyz, cloud.height.  out 1: `dens` as handed to integrate_volume.
 *   "illuminate" (:238-298)             in 4: pos xyz, df.y.  out 3.  local_xform is `rot` of u_time; `eye` is not read.
 *   "background" (:23-41)               in 3: eye.direction.  out 3.
 * u_time is read by "render", "terrain_march" and "illuminate" only, through rot / rot_cloud (:307-309).  Directions are used as given,
 * never normalised.  Every bit pattern is data — a zero, NaN or inf component, an origin inside the shell or inside the planet, the
 * exact centre where normalize(pos) is 0/0: the result is whatever the reference's arithmetic gives, NaN results included.
 * Asynchronous on `stream` and capturable (inside a capture it allocates nothing, queries nothing and waits for nothing); not counted
 * in sbx_stats.render_launches; sbx_set_precision does not enter; sbx_set_variant 1 selects the plain statement (same bits).  n == 0
 * returns SBX_OK and touches nothing; SBX_ERR_ARG, with nothing written, for a NULL ctx / fn / in / out, an unknown name, n > 2^31. */
int sbx_planet_eval(sbx_ctx* ctx, const char* fn, float u_time, const float* in, float* out, size_t n, void* stream);
/* sbx_planet_eval under the caller's world: the same eight names, element layouts and contract, with the numbers and the three angles
 * read from `world` (host memory, read during the call) instead of u_time and the header's literals.  eye, look_at and fov are not
 * read; the counts and the reserved words are checked as SBX_APP_PLANET_WORLD checks them (SBX_ERR_ARG, nothing written).  Under
 * sbx_planet_world_default(uni, .) the result is sbx_planet_eval's at uni->u_time in every bit.  "clouds_density" takes
 * t_step = max_height * 4 / float(cloud_steps).  tests/planet_world_model.py is the definition. */
int sbx_planet_world_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_planet_world* world, const float* in, float* out, size_t n, void* stream);
/* The two bone IK solver (src/IK.h) and the egg's field, shadow and trace (src/app_egg.h as shipped) as standalone functions over n
 * elements of the caller's, under the caller's pose: what the reference reaches only through pixels of its one fixed camera — the
 * solver for a host's own rig, the field for collision queries, the trace for another camera or a reflection.  `pose`: HOST memory,
 * read during the call; only turn_deg, the feet and the bones are read, the camera is not.  `in`, `out`: device memory, not
 * overlapping, 4-byte alignment suffices.  Per element:
 *   "ik_solver" (IK.h:44-52)       in 8: start xyz, goal xyz, L1, L2.  out 3.  `pose` is not read and may be NULL.
 *   "sdf" (:38-144)                in 3: P (world).  out 2: the distance, the material id as a float.
 *   "sdf_normal" (:146-157)        in 3: p.  out 3.
 *   "shadowmarch" (:161-186)       in 6: origin xyz, direction xyz.  out 1.
 *   "render_scene" (:190-231)      in 6: origin xyz, direction xyz.  out 4: the rgb it returns, then `depth` as it stands after the
 *                                  call, starting from -max_dist (:188) for every element.
 * Directions are used as given, never normalised; the ground's shadow ray keeps sh_dir = (0, 1, 1).  Exact for every bit pattern,
 * NaN results included.  Asynchronous on `stream` and capturable (inside a capture it allocates nothing, queries nothing and waits
 * for nothing); not counted in sbx_stats.render_launches; sbx_set_variant 1 selects the plain statement (same bits).  n == 0 returns
 * SBX_OK and touches nothing; SBX_ERR_ARG, with nothing written, for a NULL ctx / fn / in / out, a NULL pose for any name but
 * "ik_solver", an unknown name, n > 2^31. */
int sbx_egg_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_egg_pose* pose, const float* in, float* out, size_t n, void* stream);
/* The turntable's field, normal, soft shadow, shading and trace (src/app_vinyl.h as shipped) as standalone functions over n elements of
 * the caller's, under the caller's deck: what the reference reaches only through pixels of two fixed cameras — the field for collision
 * queries, the anisotropic groove BRDF of illuminate for a host's own surfaces, the trace for another camera or a reflection.  `deck`:
 * HOST memory, read during the call; the camera fields (eye, fov, look_at) are not read.  `in`, `out`: device memory, not overlapping,
 * 4-byte alignment suffices.  Per element:
 *   "sdf" (:251-259)          in 3: pos (world).  out 2: the distance, the material id as a float.
 *   "sdf_normal" (:261-272)   in 3: p.  out 3.
 *   "sdf_shadow" (:381-405)   in 6: origin xyz, direction xyz.  out 1.
 *   "illuminate" (:287-379)   in 7: eye xyz, hit.origin xyz, the material id as a float.  out 3.  int() of the id is taken as :439
 *                             does — toward zero, saturating at the ends of int, 0 for a NaN; an id outside 1-5 takes the `else`
 *                             branch, with the white of mat_debug for 0 and the zero colour of an unset slot for any other.
 *   "render" (:407-458)       in 6: origin xyz, direction xyz.  out 5: the LINEAR rgb it returns (no sRGB), `t` as it stands where
 *                             render returns, then the hit's material id as a float, or 0 where :457 returned the background.
 * Directions are used as given, never normalised; the shadow ray of "render" is the block's sun_dir.  Exact for every bit pattern,
 * NaN results included.  Asynchronous on `stream` and capturable (inside a capture it allocates nothing, queries nothing and waits
 * for nothing); not counted in sbx_stats.render_launches; sbx_set_variant 1 selects the plain statement (same bits).  n == 0 returns
 * SBX_OK and touches nothing; SBX_ERR_ARG, with nothing written, for a NULL ctx / fn / deck / in / out, an unknown name, n > 2^31. */
int sbx_vinyl_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_vinyl_deck* deck, const float* in, float* out, size_t n, void* stream);
/* The raytracer's trace, shading, shadow test and render (src/app_raytracer.h over src/intersect.h, src/light.h, src/util_optics.h) as
 * standalone functions over n elements of the caller's, under the caller's scene: what SBX_APP_RAYTRACER_SCENE reaches only through
 * its pinhole camera and into sRGB pixels — for rays of another lens, a probe grid, the secondary rays of a host's own integrator, a
 * picking ray.  `scene`: HOST memory, read during the call, required and range-checked as the app checks it (counts 0..16, bounces 1..8,
 * light_type 1 | 2, lighting 0 | 1, shadow 0 | 1) whatever n is; its eye, look_at and fov are not read.  `in`, `out`: device memory, not
 * overlapping, 4-byte alignment suffices.  Per element:
 *   "raytrace_iteration" (:70-86)  in 7: origin xyz, direction xyz, mat_to_ignore as a float (-1: none).  out 8: hit.t, the hit's
 *                                  material id as a float, hit.origin xyz, hit.normal xyz; a miss is no_hit of def.h: t =
 *                                  (float)(1e8 + 1e1), material -1, zeros.  Planes are taken in array order and never skipped; a
 *                                  sphere whose material equals mat_to_ignore is.
 *   "illuminate" (:46-68)          in 10: eye xyz, hit.origin xyz, hit.normal xyz, the material id as a float.  out 3: the colour
 *                                  under the block's lighting model, light type and ambient colour; material 0 gives the flat
 *                                  mat_debug colour, an id outside 0..7 the zero material.
 *   "shadow" (:109-116)            in 3: hit.origin.  out 2: shadow_hit.t of the ray from hit.origin + shadow_dir * BIAS with
 *                                  mat_debug ignored, then length(shadow_line); shadow_line = lights[0].L - hit.origin also under
 *                                  LIGHT_DIR, as in the reference.  It runs whatever the block's `shadow` says (the switch is
 *                                  "render"'s); render darkens the pixel where out[0] < out[1].
 *   "render" (:88-136)             in 6: origin xyz, direction xyz.  out 4: the LINEAR rgb (no sRGB) over the block's bounce count,
 *                                  shadow switch and lighting, the ray's own origin being the primary origin of :105; then the
 *                                  depth, the number of bounce-loop traces that found a hit, as a float (0: the background).
 * intersect_plane and intersect_sphere on their own are "raytrace_iteration" over a block with one primitive: they have no entry.
 * int() of a material id or mat_to_ignore is taken as for sbx_vinyl_eval — toward zero, saturating at the ends of int, 0 for a NaN.
 * Directions are used as given, never normalised.  Exact for every bit pattern, NaN results included.  Asynchronous on `stream` and
 * capturable (one kernel launch and nothing else); not counted in sbx_stats.render_launches; sbx_set_variant 1 selects the IEEE roots
 * (same bits).  n == 0 returns SBX_OK with `in` and `out` not looked at; SBX_ERR_ARG, with nothing written, for a NULL ctx / fn /
 * scene / in / out, a scene outside the ranges above (the app's texts), an unknown name, n > 2^31. */
int sbx_raytracer_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_raytracer_scene* scene, const float* in, float* out, size_t n, void* stream);
/* The size^3 RGBA32F noise volume util/ddsvolgen bakes (ddsvolgen.cpp:101-117): R =
 * fbm_worley_tile((xyz + .5)/size, 2, 1, .5), G = B = A = 0, x fastest.  `rgba`: size^3 * 4 floats. */
int sbx_worley_volume(sbx_ctx* ctx, int size, float* rgba, void* stream);

/* Bind the two 3-D noise textures of APP_CLOUDS' USE_NOISE_TEX build: u_tex_noise (t1, the cloud shape) and
 * u_tex_noise_2 (t2, the Worley detail), src/app_clouds.h:52-55 — what hlsltoy loads from the .dds files named on its
 * command line and binds with a MIN_MAG_MIP_LINEAR / WRAP sampler (util/hlsltoy/src/hlsltoy.cpp:227-249, 437).
 * Each is a size^3 RGBA32F volume in device memory, x fastest (the layout util/ddsvolgen writes, ddsvolgen.cpp:101-117;
 * sbx_worley_volume produces one).  The shader reads only .r: the call copies that channel into the context (R32F,
 * a quarter of the footprint) on `stream` and scans the copies for the range of the texel values (k_clouds_tex derives a bound on
 * the density from it and uses a cheaper, equal form of exp inside that bound); the call returns when both have finished, and the
 * caller's buffers are not referenced afterwards.  Inside a stream capture there is no scan and no wait.
 * SampleLevel is evaluated by the sbx texture-filter spec: texel centres at (i + .5) / size, WRAP,
 * trilinear blend with binary32 weights in x, y, z order.  Renders of SBX_APP_CLOUDS_TEX must be ordered after this
 * call (same stream, or an event). */
int sbx_set_noise_volumes(sbx_ctx* ctx, int shape_size, const float* shape_rgba, int detail_size,
                          const float* detail_rgba, void* stream);
/* The t0 texture of SBX_APP_2D_TEX (src/app_2d.h:3-30; what hlsltoy binds at t0, util/hlsltoy/src/hlsltoy.cpp:434).  `texels`:
 * device memory, width x height texels, row-major, row 0 at v = 0; `format` SBX_FORMAT_RGBA8 (R8G8B8A8_UNORM words, R in the low
 * byte, decoded to c / 255 correctly rounded) or SBX_FORMAT_RGBA32F (float4).  1 <= width, height <= 16384.  The call copies the
 * texture into the context (as RGBA32F) on `stream` and returns when the copy is done; the caller's buffer is not referenced
 * afterwards (inside a stream capture it does not wait).  texels = NULL restores the default, hlsltoy's 128x128 checkerboard.  Renders
 * of SBX_APP_2D_TEX enqueued after the call read the new texture (same stream, or an event); earlier ones keep the old.
 * Sampling (DESIGN.md §3 "SampleLevel", two axes): per axis u = c * size - .5, i = floor(u), f = u - i, WRAP by
 * i - size * floor(i / size) folded into [0, size) (NaN -> texel 0), mix in x, then in y, binary32 weights.  Any coordinate reads
 * only texels inside the texture.  SBX_ERR_ARG for a bad size or format. */
int sbx_set_texture2d(sbx_ctx* ctx, int width, int height, int format, const void* texels, void* stream);
/* hlsltoy's CreateTextureCheckboard (util/hlsltoy/src/hlsltoy.cpp:66-87) for a size x size texture, host only:
 * out[y * size + x] = ((x & freq) == (y & freq)) ? 0xff000000 : 0xffffffff.  The default t0 is (128, 16). */
void sbx_checkerboard_texture(int size, int freq, uint32_t* out);

/* ---- Multi-GPU frames inside the library (SURVEY.md §8b "Ownership", §8e "Collective") -----------------------------
 * One process drives `nranks` ranks; devices[i] is the HIP device of rank i, rank 0 owns the frame.  With all devices
 * distinct the library creates its communicator with ncclCommInitAll (rccl.h:236; librccl is dlopen'ed here, not linked)
 * and every peer's slab travels by ONE ncclSend / ncclRecv pair (rccl.h:700,722; all pairs of a frame in one group, N-1 distinct
 * xGMI links) into a landing area on rank 0, from where one small kernel scatters the rows into the frame; rank 0 renders its
 * own blocks in place.  Devices may repeat (several ranks on one GPU — how the N-rank schedule runs on fewer GPUs than
 * ranks): those transfers are device copies.  The split is the cyclic row-block split of sbx_render_split (default 8-row
 * blocks, no root relief).  Every sbx_multi_* call leaves rank 0's device current (hipSetDevice). */
typedef struct sbx_multi sbx_multi;
int sbx_multi_create(int nranks, const int* devices, sbx_multi** out);
/* Why the last sbx_multi_create of this process failed (e.g. the dlopen / dlsym text for librccl); "" after a success. */
const char* sbx_multi_create_error(void);
/* How the peers' rows reach rank 0: SLABS (default) = one send / receive per peer of its whole 3-channel slab + one scatter
 * kernel; BLOCKS = one send / receive pair per row-block straight into the final rows (no landing area, no scatter kernel,
 * but (N-1) x blocks point-to-point operations per frame in one group). */
enum { SBX_MULTI_EXCHANGE_SLABS = 0, SBX_MULTI_EXCHANGE_BLOCKS = 1,
       SBX_MULTI_EXCHANGE_SPANS = 2 /* the span exchange above: packed spans only, rank 0 renders the rest (sbx_render_span_*) */,
       SBX_MULTI_EXCHANGE_PEER_STORES = 3 /* no RCCL, no slabs: every rank renders its row-blocks in place into rank 0's frame through
                                             peer access — the exchange is the render kernels' own float4 stores over xGMI (16 B per
                                             pixel), rank 0 lands and scatters nothing.  UNMEASURED on more than one device: across distinct
                                             devices it returns SBX_ERR_UNSUPPORTED unless the environment has SBX_ENABLE_PEER_STORES=1
                                             (also without peer access).  The validated form of the same idea, with explicit ordering
                                             flags and across processes, is the store exchange sbx_shared_* above */ };
int sbx_multi_set_exchange(sbx_multi* m, int mode);
void sbx_multi_destroy(sbx_multi* m);
int sbx_multi_ranks(const sbx_multi* m);
int sbx_multi_uses_rccl(const sbx_multi* m);             /* 1: RCCL send/recv, 0: device / peer copies */
int sbx_multi_set_split(sbx_multi* m, int block_rows, int root_rounds, int rounds);
/* sbx_set_output_format on every rank: with SBX_FORMAT_RGBA8 `frame` of sbx_multi_render holds width * height 32-bit words and
 * every exchange form moves 4 bytes per pixel. */
int sbx_multi_set_output_format(sbx_multi* m, int format);
/* The two noise volumes of SBX_APP_CLOUDS_TEX (device memory on rank 0's device), handed to every rank; synchronous. */
int sbx_multi_set_noise_volumes(sbx_multi* m, int shape_size, const float* shape_rgba, int detail_size,
                                const float* detail_rgba);
/* One frame over all ranks into `frame` (height * width RGBA32F pixels in rank 0's device memory).  Asynchronous: the
 * work starts after what is already enqueued on `stream` (a stream of rank 0's device; NULL = its default stream) and
 * `stream` continues when the whole frame is in place.  Up to two frames may be in flight (alternate two streams and two
 * frames); the pixels are bit-identical to a one-GPU render. */
int sbx_multi_render(sbx_multi* m, int app, const sbx_uniforms* uni, const void* aux, float* frame, void* stream);
const char* sbx_multi_last_error(sbx_multi* m);
/* Self-test of the RCCL calls the multi-GPU path is made of, on ONE device: dlopen librccl, ncclCommInitAll({device}), one
 * grouped ncclSend / ncclRecv pair from the rank to itself on two streams, compare.  0 = ok; *step (may be NULL) names the
 * failing step: 1 load, 2 communicator, 3 buffers, 4 group call, 5 data. */
int sbx_multi_rccl_selftest(int device, int* step);

/* Internal-invariant faults.  The cooperative hash cache of APP_CLOUDS / APP_PLANET serves lattice-cell misses in a loop that
 * needs at most 64 rounds and is bounded at 4096; reaching the bound would mean wrong pixels.  Instead of passing silently the
 * wave sets a sticky word in pinned host memory (one per device): from then on every render call on a context of that device
 * returns SBX_ERR_FAULT — checked on entry, without synchronising — and sbx_last_error says why, until sbx_clear_fault (which
 * waits for the device first).  sbx_fault_status = the check on its own (e.g. after synchronising a frame).  The waits of the
 * store exchange (sbx_shared_frame_begin / _end) report a signal that never arrived the same way. */
int sbx_fault_status(sbx_ctx* ctx);
int sbx_clear_fault(sbx_ctx* ctx);

const char* sbx_last_error(sbx_ctx* ctx);
const char* sbx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SBX_H */
