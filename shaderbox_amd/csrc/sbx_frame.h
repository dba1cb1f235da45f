// shaderbox_amd/csrc/sbx_frame.h — per-frame constant blocks and the row map.
//
// The reference recomputes frame constants per pixel (mainImage calls setup_camera() and
// setup_scene() for every fragment, /root/reference/src/main.h:35-38; APP_EGG even rebuilds its
// rotations and IK inside every sdf() call, src/app_egg.h:40-128).  They depend only on the
// uniforms, so the host evaluates them ONCE per frame with the same math spec (sbx_math.h is
// bit-identical on host and device) and passes them as kernel arguments: on gfx950 kernel
// arguments are wave-uniform and live in SGPRs, which is the "per-tile camera/uniform
// constants" staging the design calls for without spending LDS or VGPRs on them.
#pragma once
#include <hip/hip_runtime.h>
#include "sbx_vec.h"

namespace sbx {

// local row r of a launch -> global row y of the frame.
//   contiguous strip:  block_rows = nrows, nranks = 1, rank = 0      -> y = y0 + r
//   cyclic row-blocks: rank owns blocks rank, rank+nranks, ...        
//   cyclic with root relief: the blocks are dealt in cycles of `rounds` rounds; a round deals one block to every
//     rank, except that rank 0 (the gather's root, which also receives and assembles the frame) is left out of the
//     rounds >= root_rounds.  root_rounds = rounds = 1 is the plain cyclic split.
struct RowMap {
    int width, height;
    int y0, block_rows, nranks, rank;
    int nrows;   // local rows in this launch
    int r0;      // first local row of this launch within the rank's slab (sub-range launches)
    int root_rounds, rounds;
    int in_place;   // 0: rows are written densely (slab row r); 1: at their global row y of a full-size frame
    int rgb;        // 1: the output holds 3 floats per pixel (a peer's slab on its way to the root: alpha is the constant 1 of
                    //    main.h:52 and need not cross xGMI); 0: float4 pixels; 2: one R8G8B8A8_UNORM word per pixel
                    //    (sbx_set_output_format: the display format of the reference's hosts, 4 bytes per pixel everywhere);
                    //    3: float4 pixels of which only R, G, B are written (sbx_render_split_in_place_rgb)
    // POINT LIST (sbx_render_points / sbx_main_image): frag != NULL makes the launch evaluate mainImage at `npoints` arbitrary
    // fragCoords read from device memory (x, y interleaved) instead of at the pixel centres of a row range: the launch is laid
    // out as a pseudo-frame of `width` columns whose "pixel" (x, r) is point r * width + x; results are written densely, 4
    // (or 3) floats per point.  u_res stays the real frame's: fragCoord / u_res is what mainImage computes (main.h:40).
    const float* frag;
    int npoints;
    // SPANS (sbx_render_span_peer / sbx_render_span_root; the multi-GPU exchange that ships only the expensive part of a
    // row-block): span[g] = {x0, x1, off, owner} for every GLOBAL row-block g of the frame — pixels x0 <= x < x1 of the block
    // are the part that is sharded ("heavy": the host expects real work there), the rest leaves mainImage through an early
    // exit and is rendered by the frame's owner itself; `off` = where the block's span starts in its owner's packed slab
    // (in pixels), `owner` = the rank the split deals the block to.
    //   span_mode 1 (a peer): the launch covers the rank's local rows x the widest span; a pixel is rendered iff it lies in
    //                 its block's span and lands at slab pixel off + row_in_block * (x1 - x0) + (x - x0);
    //   span_mode 2 (the owner of the frame, in place over the WHOLE frame): a pixel is rendered iff its block is rank 0's
    //                 or it lies OUTSIDE its block's span.
    //   span_mode 3 (a peer of the store exchange, sbx_render_span_peer_in_place): the launch covers the rank's rows at the frame's
    //                 full width; a pixel is rendered iff it lies in its block's span and lands at its GLOBAL position of the owner's
    //                 full-size frame (waves outside the span exit at once).
    // Either way every pixel is computed by the same kernel from its global coordinates: the spans decide who renders a
    // pixel, never what it looks like.
    const int4* span;
    int span_mode;
    // DISPATCH ORDER (round 6; a hint about cost, never about pixels): order != NULL makes workgroup i of the launch render tile
    // order[i] = bx | by << 16 instead of tile i — a permutation of the launch's tiles, built from the previous frame's per-tile
    // cost, longest first (sbx_tile_order.h, kern_util.hip k_order_count / _scan / _place); cost != NULL: lane 0 of every wave's first tile
    // column writes its wave's duration (100 MHz ticks) to cost[tile].
    const unsigned* order = nullptr;
    unsigned* cost = nullptr;
};
// blocks in one cycle, and the position of (round, rank) in it
SBX_HD int split_cycle_blocks(int nranks, int root_rounds, int rounds) {
    return root_rounds * nranks + (rounds - root_rounds) * (nranks - 1);
}
SBX_HD int row_to_y(const RowMap& m, int r) {
    const int rr = r + m.r0;
    const int blk = rr / m.block_rows;                       // local block index in the rank's slab
    const int cnt = (m.rank == 0) ? m.root_rounds : m.rounds;    // blocks this rank gets per cycle
    const int cycle = blk / cnt, round = blk - cycle * cnt;
    const int v = (round < m.root_rounds) ? round * m.nranks + m.rank
                                          : m.root_rounds * m.nranks + (round - m.root_rounds) * (m.nranks - 1) + (m.rank - 1);
    const int gblk = cycle * split_cycle_blocks(m.nranks, m.root_rounds, m.rounds) + v;
    return m.y0 + gblk * m.block_rows + (rr - blk * m.block_rows);
}

// Camera part of mainImage (src/main.h:33-48) + get_primary_ray (src/util.h:5-20)
struct Camera {
    float res_x, res_y;
    float aspect_x;   // u_res.x / u_res.y
    float fov;
    v3 eye, fwd, up, right;
    double rres_x, rres_y;   // recip64(u_res): fragCoord / u_res as an exact multiply (sbx_math.h div_by)
};
SBX_HD Camera make_camera(float res_x, float res_y, float fov, v3 eye, v3 look_at) {
    Camera c;
    c.res_x = res_x; c.res_y = res_y;
    c.aspect_x = res_x / res_y;            // main.h:33
    c.fov = fov;
    c.rres_x = recip64(res_x); c.rres_y = recip64(res_y);
    c.eye = eye;
    c.fwd = normalize(look_at - eye);      // util.h:10
    v3 up = V3(0, 1, 0);
    c.right = cross(up, c.fwd);            // util.h:12
    c.up = cross(c.fwd, c.right);          // util.h:13
    return c;
}
// point_cam.xy for fragCoord (main.h:40,44-46); point_cam.z = -1
SBX_HD v2 point_cam(const Camera& c, float fx, float fy) {
    float nx = div_by(fx, c.rres_x), ny = div_by(fy, c.rres_y);   // main.h:40
    return V2(((2.0f * nx - 1.0f) * c.aspect_x) * c.fov, ((2.0f * ny - 1.0f) * 1.0f) * c.fov);
}
SBX_HD v3 primary_dir(const Camera& c, v2 pc) {
    return normalize(c.fwd + c.up * pc.y + c.right * pc.x);   // util.h:17
}
// linear_to_srgb (src/util.h:72-77): p = 1/2.2 in binary32
#ifndef SBX_SRGB_FAST
#define SBX_SRGB_FAST 1     // device: srgb_pow_ of sbx_math.h (pow_'s operations in ~45 instead of ~100 instructions; equal on all 2^32 arguments)
#endif
SBX_HD v3 to_srgb(v3 c) {
#if SBX_SRGB_FAST
    return V3(srgb_pow_(c.x), srgb_pow_(c.y), srgb_pow_(c.z));
#else
    const float p = 1.f / 2.2f;
    return V3(pow_(c.x, p), pow_(c.y, p), pow_(c.z, p));
#endif
}

// ---- APP_CLOUDS (src/app_clouds.h, src/uniform_buffer.h:39-55) ----------------------------
struct FrameClouds {
    Camera cam;
    v3 sun_dir, sun_color;
    v3 wind_off;          // wind_dir * u_time * (1/cld_noise_factor)   app_clouds.h:167
    float sun_power, sigma;
    int steps, lsteps;
    float dt;             // cld_thick / float(cld_march_steps)         app_clouds.h:98,180
    float cov, cov_hi;    // 1 - cld_coverage, cov + .0135              app_clouds.h:83-84
    double cov_rd;        // recip64(cov_hi - cov): the smoothstep division becomes an exact multiply
    float cov_d, cov_r;   // cov_hi - cov and RN(1 / that): the same division through div3_ (sbx_math.h) in k_clouds' SM kernels
    float thr1, thr2;     // cov - .1876, cov - .06255: the staged main sample's two cut-offs (launch_clouds)
    int lip_ok;           // 1: the march positions are small enough for k_clouds' Lipschitz sample skip (set per launch by
                          //    launch_clouds / clouds_lip_domain; 0 disables the skip, nothing else)
    int exp_small;        // 1: every exp argument of the REG kernels lies in [-0.205, -0] (sigma, dt >= 0, .94 sigma dt <= .205): they
                          //    use exp_small_ of sbx_math.h instead of exp_reg64_ (set per launch by launch_clouds; same bits)
    // SKY_SPHERE build (app_clouds.h:8,14-19,154-162; SBX_APP_CLOUDS_SKY): the march starts where the view ray meets a sphere
    // around the viewer (intersect_sphere_from_inside) and runs along the view ray itself; the table-less kernels only
    int sky;              // 1: SKY_SPHERE
    float nf;             // cld_noise_factor: .001, or (1 / atm_radius) * 10 for SKY_SPHERE            app_clouds.h:18,20
    float atm_y, atm_r;   // atmosphere = sphere((0, atm_ground_y, 0), atm_radius)                     app_clouds.h:15-17
    m3 sky_rot;           // rotate_around_x(u_time)                                                   app_clouds.h:160
};
// The builds of illuminate_volume's two `#if 0` switches (app_clouds.h:97, :118; include/sbx.h): SBX_APP_CLOUDS, _CLOUDS_HEIGHT,
// _CLOUDS_LUMINANCE.  The frame constants are the same in all three, so the build is no field of FrameClouds — the shipped kernels
// take the arguments they always took — but an argument of launch_clouds; the HEIGHT build's per-step luminances lie behind the
// frame's y rows in the y table (kern_clouds.hip lum_of), so they need no pointer of their own either.
enum { CLOUDS_DEFAULT = 0, CLOUDS_HEIGHT = 1, CLOUDS_LUMINANCE = 2 };

// ---- APP_EGG (src/app_egg.h) ----------------------------------------------------------------
struct BezierFrame {      // the P-independent part of sd_bezier (src/sdf.h:147-153)
    v3 b, u, v, w;
    v2 a2, c2;
    v3 bc; float br;      // a sphere around the control triangle (hence around the curve), radius rounded up: sbx_sdf.h bezier_far
};
struct CylFrame {         // the P-independent part of sd_cylinder with P0 = 0 (src/sdf.h:104,106-107)
    v3 dir;
    float len1, len0;
};
struct FrameEgg {
    Camera cam;
    m3 rot_y;             // rotate_around_y(u_time * -100)            app_egg.h:40
    v3 left_foot, right_foot;   //                                      app_egg.h:73-77
    BezierFrame leg_l, leg_r;   //                                      app_egg.h:111-116
    CylFrame foot_l, foot_r;    //                                      app_egg.h:120-128
    v3 foot_ml, foot_mr;        // midpoints of the toe cylinders in p space: -foot - toe/16 (kern_egg.hip)
    v3 oc; float orad;          // sphere around everything but the ground plane, in sdf()'s p space (kern_egg.hip egg_far)
    v3 ocw;                     // the same centre in WORLD space, rot_y^T (oc + (0, .5, 3.5)): the cull test needs no rotation
};
// The build without `#define BEZIER` (app_egg.h:37; SBX_APP_EGG_STRAIGHT): FrameEgg and the four sd_cylinder legs of :86-93, :97-104,
// in the order left a (pelvis -> knee), left b (knee -> foot), right a, right b.  A type of its own, so that the kernels of the
// other builds take the arguments they always took (k_egg's shipped build compiles to the same instructions as before it had builds).
struct FrameEggStraight : FrameEgg {
    CylFrame leg[4];            // axes knee_l - side, left_foot - knee_l, knee_r + side, right_foot - knee_r (all with P0 = 0)
    v3 leg_o[4];                // what sdf() adds to p before the call: side, knee_l, -side, knee_r
    v3 leg_m[4];                // midpoints of the cylinders in p space: -leg_o - dir * len1 / 2 (kern_egg.hip)
    float leg_k[4];             // len1 / 2 + thick + .0025 + 1e-3: half length, radius, what op_blend(.., .01) can take off, slack
};
enum { EGG_DEFAULT = 0, EGG_STRAIGHT = 1, EGG_OVAL = 2 };   // the builds of app_egg.h (include/sbx.h): SBX_APP_EGG, _EGG_STRAIGHT, _EGG_OVAL

// ---- APP_RAYTRACER (src/app_raytracer.h, cornell_box.h) -------------------------------------
struct RtPlane { v3 n; float d; int mat; };
struct RtSphere { v3 o; float r; int mat; double rr; };   // rr = recip64(r): the normal's three divisions by r (intersect.h:32)
struct RtMaterial { v3 base_color; float roughness, ior, reflectivity;
                    float r0; };   // fresnel_factor(1, ior, .)'s R0 = ((1 - ior) / (1 + ior))^2, util_optics.h:10-11
struct FrameRaytracer {
    Camera cam;
    RtPlane planes[6];
    RtSphere spheres[3];
    RtMaterial mats[8];
    v3 light;             // lights[0].L
};
// The builds of app_raytracer.h's three compile-time switches (include/sbx.h): SBX_APP_RAYTRACER, _RAYTRACER_PHONG (illuminate's
// `#if 0` at :61 on), _RAYTRACER_NOSHADOW (render's `#if 1` at :107 off), _RAYTRACER_STATIC (setup_scene's `#if 1` at :29 off).
// The first two are kernel template parameters (kern_raytracer.hip); the third is another frame block for the shipped kernels
// (build_raytracer).  FrameRaytracer is the same type in all four.
enum { RT_DEFAULT = 0, RT_PHONG = 1, RT_NOSHADOW = 2, RT_STATIC = 3 };
// SBX_APP_RAYTRACER_SCENE (include/sbx.h sbx_aux_raytracer_scene): the caller's scene.  A type of its own, so that k_raytracer takes the
// arguments it always took.  What the file's compile-time switches are for the Cornell box are run-time values here; the counts are
// validated on the host (0..16 each, bounces 1..8) before a launch, so every array index of the kernel is in range.
constexpr int RT_MAX_PLANES = 16, RT_MAX_SPHERES = 16;
struct FrameRtScene {
    Camera cam;
    int n_planes, n_spheres;
    int bounces;          // the `2` of app_raytracer.h:96
    int lighting;         // 0 illum_cook_torrance, 1 illum_blinn_phong (:61)
    int shadow;           // the `#if 1` of :107
    int light_type;       // 1 LIGHT_POINT, 2 LIGHT_DIR (light.h:5-6)
    v3 light;             // lights[0].L
    v3 ambient;           // ambient_light light.h:16
    RtMaterial mats[8];
    RtPlane planes[RT_MAX_PLANES];
    RtSphere spheres[RT_MAX_SPHERES];
};

// ---- APP_ATMOSPHERE (src/app_atmosphere.h) --------------------------------------------------
struct FrameAtmosphere {
    Camera cam;
    v3 sun_dir;           // (0,1,0) * rotate_around_x(-|sin(t/2)|*90)  app_atmosphere.h:177-181
};
// SBX_APP_ATMOSPHERE_AIR / sbx_atmosphere_air_eval: the solver's numbers from the caller's block (include/sbx.h sbx_aux_atmosphere_air),
// the second argument of k_atmosphere_air and k_atmosphere_air_eval.  The sun and (for the app) the eye travel in FrameAtmosphere.
struct AtmAir {
    v3 betaR, betaM;                  // :29-30
    float hR, rhR, hM, rhM;           // :34-35 and RN(1 / h): div3_'s pair (read by the fast forms only)
    float earth_r, atmos_r;           // :37-38
    float sun_power, g;               // :41, :12
    int ns, nl;                       // :47-48
    int dead_ok;                      // the dead-ray exit may run: all six betas are positive numbers (sbx_atmosphere.h "CALLER'S AIR")
};

// ---- APP_SDF_AO (src/app_sdf_ao.h) ----------------------------------------------------------
struct FrameSdfAo {
    Camera cam;
    m3 rx_m90;            // rotate_around_x(-90)   app_sdf_ao.h:63,77
    m3 ry_180;            // rotate_around_y(180)   app_sdf_ao.h:134
    v3 sun_dir;           // normalize(1,2,1)       app_sdf_ao.h:209
    float fog_density, fog_falloff;
};

// SBX_APP_SDF_SCENE (include/sbx.h sbx_aux_sdf_scene): app_sdf_ao.h's renderer over the caller's field, a postfix program.  One
// instruction as the kernel reads it: the point-independent part of its primitive evaluated on the host, each host operation the same
// binary32 operation the reference performs per call (the rotation's sin / cos; sd_cylinder's dir, length(P1), length(P0) sdf.h:104-107;
// sd_capsule's ab and dot(ab, ab) :168-169; sd_bezier's w, u, v, a2, c2 :147-153 — normalisations with IEEE quotients, sbx_frames.hip).
//   p[]:  PLANE n d | SPHERE r | BOX b | TORUS R r | Y_CYLINDER r h | CYLINDER dir len1 len0 P0 R | CAPSULE a ab dot(ab,ab) r |
//         BEZIER b u v w a2 c2 thickness | BLEND k | OBJECT float(material)
// 32 x 92 B: the frame, RowMap and the output pointer are 3288 B of the 4 KB a kernel may take by value — no buffer, no allocation.
constexpr int SDF_MAX_INSTR = 32;
// SBX_SDF_* as a bit number: primitives 1..8 -> 0..7, operators 16..19 -> 8..11, OBJECT 32 -> 12.  One bit per op, so that the
// interpreter tests bits one after the other and the compiler cannot fold the tests back into a switch tree
constexpr int sdf_op_bit(int op) { return op < 16 ? op - 1 : op < 32 ? op - 8 : 12; }
struct SdfOp {
    int ctl;              // what steers the interpreter, one scalar load per instruction: 1 << sdf_op_bit(op) | rot_axis << 16
    float s, c;           // sin / cos of radians(rot_deg)
    v3 off;
    float p[17];
};
struct FrameSdfScene {
    Camera cam;
    int n_instr;          // 1..32, validated with the program's stack discipline before a launch (sbx_frames.hip sdf_scene_check)
    int steps;            // app_sdf_ao.h:249, 1..512
    int shadow, view;     // the `#if 0` of :269 and of :217
    int checker;          // the material id that gets :237-240
    float end;            // :250
    float fog_density, fog_falloff;
    v3 sun_dir;           // :209, as given
    v3 background;        // :11
    v3 mats[8];
    SdfOp prog[SDF_MAX_INSTR];
};

// ---- APP_PLANET (src/app_planet.h) ----------------------------------------------------------
struct FramePlanet {
    Camera cam;
    m3 rot, rot_cloud, rot_t;   // app_planet.h:307-309, transpose(rot) :356
    v3 L;                       // rot * normalize(1,1,0)   app_planet.h:289
    int atm_sky;                // 1: SBX_APP_PLANET_ATMOSPHERE — background() is APP_ATMOSPHERE's get_incident_light (kern_planet.hip)
    v3 atm_sun;                 // its sun: (0,1,0) * rotate_around_x(-|sin(t/2)|*90)   app_atmosphere.h:177-181
};
// The builds of app_planet.h's compile-time switches (include/sbx.h): SBX_APP_PLANET, _PLANET_CLOUDLESS (`#define CLOUDS` at :63 gone),
// _PLANET_UNLIT (`#define LIGHT` at :249 gone), _PLANET_CLOSEUP (setup_camera's `#if 0` at :51 on).  All three are kernel template
// parameters (kern_planet.hip); CLOSEUP is also another camera in the frame block (build_planet).  FramePlanet is the same type in
// all four; none of the three is combined with atm_sky.
enum { PLANET_DEFAULT = 0, PLANET_CLOUDLESS = 1, PLANET_UNLIT = 2, PLANET_CLOSEUP = 3 };
// SBX_APP_PLANET_WORLD's run-time tier (kern_planet_world.hip k_planet_world): FramePlanet's fields built from the caller's block
// (include/sbx.h sbx_aux_planet_world) plus the numbers k_planet has as literals, and what the host derives from them in the header's
// binary32 order (sbx_frames.hip build_planet_world).  The (d, r) pairs are a divisor and RN(1 / d) for div3_ of sbx_math.h.
// what only the shading of a ground hit reads: the kernel fetches it from its argument block there, not at its start, so that these 37
// words hold no SGPRs across the marches (kern_planet_world.hip pw_late)
struct PlanetWorldShade {
    m3 rot_t;                               // transpose(rot) :356
    v3 L;                                   // rot * sun_dir, the sun as given
    v3 key_color;
    v3 c_water, c_water_half, c_grass, c_beach, c_rock, c_snow;    // c_water_half: c_water / 2. (:284)
    float l_water, l_shore, l_grass, l_rock;
};
// what the terrain march and the detail maps read, and what the two cloud marches read: fetched where each begins, as `shade` is
struct PlanetWorldTerrain {
    m3 rot;                                 // :308
    v3 terrain_offset;
    float max_height, max_height_r;         // :20 and RN(1 / it)
    float max_ray_dist;                     // max_height * 4 (:21)
    int terr_steps;
};
struct PlanetWorldCloud {
    m3 rot_cloud;                           // :309
    v3 cloud_offset;
    float max_height, max_height_r;
    float band0, band1, band2;              // :114
    float band_d01, band_r01, band_d12, band_r12;   // band1 - band0, band2 - band1
    float cov, cov_hi, cov_d, cov_r;        // cld_coverage, cld_coverage + cld_fuzzy (:112), their difference
    float neg_absorb;                       // -vol_coeff_absorb (:87)
    float cloud_light, cloud_light_r;       // :76
    float t_step_cloud, t_step_shadow;      // max_ray_dist / float(cloud_steps) (:128); max_height / float(shadow_steps) (:149)
    float shell_lo2, shell_hi2;             // a cloud-march sample with |o|^2 below / above lies outside the band's shell (0 / inf: no such claim)
    int cloud_steps, shadow_steps;
};
struct FramePlanetWorld {
    Camera cam;
    float atm_radius;                       // 1 + max_height (:311-312)
    float hit2_max;                         // (atm_radius + 1)^2: the wave-wide test on |hit_o|^2
    int tame;                               // planet_world_tame: the block lies in the domain of the short forms (kern_planet_world.hip)
    PlanetWorldTerrain terr;
    PlanetWorldCloud cloud;
    PlanetWorldShade shade;
};

// ---- "clouds_best" (src/app_clouds_best.h, the stand-alone cloud shader) ------
// The march runs along projection = dir / dir.y, whose y component is exactly 1, from origin.y = eye.y + 100:
// sample height, `cloud.height`, illuminate_volume() = exp(height)/1.95 and the y coordinate of the five
// noise octaves are the same for every pixel.  One row per march step, built on the host with the math spec.
constexpr int CB_STEPS = 50;                                   // cld_march_steps :410
struct CBRow { float qy[5]; float illum; };
struct FrameCloudsBest {
    Camera cam;
    v3 sun_dir;               // normalize(0, 0, -1)                                          :415
    float wind_z;             // -u_time * .2                                                 :414
    float march_step;         // cld_thick / float(steps)                                     :603
    float cov;                // cld_coverage                                                 :411
    double cov_rd;            // recip64((cov + .035) - cov)                                  :583
    CBRow row[CB_STEPS];
};

// ---- the UE4 cloud variant (ue4/volumetric_clouds/Shaders/app_clouds.usf) ----------------
constexpr int UE4_STEPS = 25;                                  // STEPS :16
struct FrameCloudsUe4 {
    Camera cam;               // host mapping: APP_CLOUDS' camera (src/app_clouds.h:23-30), FOV 1
    v3 sun_dir, wind_dir;     // SUN_DIR / WIND_DIR :13-14 or the aux block's
    float march_step;         // thickness / float(steps)                                     :199
    float absorbtion;
    float cov;                // 1 - coverage                                                 :256
    double cov_rd;            // recip64((cov + fuzziness) - cov)                             :175
    float cov_d, cov_r;       // (cov + fuzziness) - cov and RN(1 / that): the same division through div3_ (sbx_math.h)
    float eh[UE4_STEPS];      // exp(h) / 1.75 with h = float(i) / float(steps)               :213,221
};

// ---- APP_VINYL (src/app_vinyl.h; C++ build) -------------------------------------------------
struct Capsule { v3 a, ab; double rd; };   // sd_capsule(p, a, b, r): ab = b - a, rd = recip64(dot(ab, ab))
struct FrameVinyl {
    Camera cam;
    m3 platter_rot;            // rotate_around_y(200 t) * rotate_around_x(sin(t) * .1)      app_vinyl.h:424-426
    v3 sun_dir;                // normalize(-1, 4, -3)                                        :285-286
    m3 ry30, rym30;            // logo                                                        :74,77
    m3 wobble;                 // rotate_around_x(sin(3.6758 t) * .1)                         :141-142
    Capsule arm1, arm2, arm3;  //                                                             :151-153
    BezierFrame armb;          // sd_bezier(a11, a2, a33, ., R)                               :154
    v3 a3;                     //                                                             :150
    m3 arm_xform, fl_rot, fl_rot2, ctg_rot, cut_rx10, cut_rym5, cut2_rz10;   // :163-232
    v3 fl_sub1, fl_sub2;       // arm_right * clr_r, arm_up * clr_r                           :191-193
    CylFrame collar;           // sd_cylinder(., 0, arm_fwd * .05, .)                         :173-176
    int steps;                 // march steps: 60 (the C++ build) or 180 (the GLSL / HLSL builds, SBX_APP_VINYL_GPU)   :411-416
};
// The builds of app_vinyl.h's compile-time switches (include/sbx.h): SBX_APP_VINYL, _VINYL_RIDGES (illuminate's `#if 0` at :357 on),
// _VINYL_NOSHADOW (render's `#if 1` at :445 off), _VINYL_CLOSEUP (setup_camera's `#if 1` at :60 off).  RIDGES and NOSHADOW are kernel
// template parameters (kern_vinyl.hip); CLOSEUP is another camera in the frame block for the shipped kernels (build_vinyl).
// FrameVinyl is the same type in all four.
enum { VINYL_DEFAULT = 0, VINYL_RIDGES = 1, VINYL_NOSHADOW = 2, VINYL_CLOSEUP = 3, VINYL_DECK = 4 };
// VINYL_DECK (SBX_APP_VINYL_DECK, sbx_vinyl_eval): the shipped hit block with illuminate's literals read from the caller's block.  The
// choice: an argument of its OWN beside an unchanged FrameVinyl, not new members of FrameVinyl — the frame block is the first kernel
// argument of all five shipped apps and is copied word by word into LDS (sbx_ldsframe.h), so any member added to it changes their
// argument list, their LDS size and their device code; these 19 words are read once per hit pixel, after the march, and sit in SGPRs.
struct VinylShade {
    v3 color[5];               // materials[mat_groove .. mat_shiny].base_color                app_vinyl.h:45-53
    float ro_spec, a_x, a_y;   //                                                             :327-329
    float shininess;           // the exponent of :375
};

// ---- APP_2D / APP_2D_TEX (src/app_2d.h:70-111; not APP_* defines of the reference) -----------------
// Everything mainImage decides from the uniforms alone: the phase of t = mod(u_time, 16) (:80-103; 4 = none of the four branches
// runs, color stays (0, 0, 0, 0)), the time the phase hands perturb_tunnel / perturb_road and its mix weight.
struct Frame2d {
    double rres_x, rres_y;    // recip64(u_res): fragCoord / u_res as an exact multiply (sbx_math.h div_by)      :72
    double rpi;               // recip64(PI): a / PI as an exact multiply                                         :60
    float time;               // u_time (phases 0, 2) or 1 (phases 1, 3)                                         :83,88-89,95,99-100
    float w, omw;             // mix weight (t - 4) / 4 or (t - 12) / 4, and 1 - w (GLSL mix)                      :90,101
    int phase;                // 0: tunnel, 1: tunnel -> road, 2: road, 3: road -> tunnel, 4: none (t = 4, 8, 12 or NaN)
    // APP_2D_TEX: the context's copy of t0 (sbx_set_texture2d), RGBA32F texels, row 0 at v = 0
    const float4* tex;
    int tw, th;
    float ftw, fth;
    double rtw, rth;          // recip64(tw), recip64(th): the wrap's quotient
};

// ---- APP_FUNC (src/app_func.h:63-111, the `#if 1 // 2D` branch; not an APP_* define of the reference) ----------------------
// The shader reads only u_res: t = (fragCoord + .5) / u_res (:72).  The hash table holds hash_w of every cell the six periods can
// reach from pos.z = 0 (kern_func.hip, built once per context at sbx_create).
struct FrameFunc {
    float res_x, res_y;       // u_res, the divisors of :72 (IEEE quotients)
    const float4* tab;        // FUNC_TABLE_CELLS hashes (kern_func.hip); unused by the plain kernel
};

}  // namespace sbx
