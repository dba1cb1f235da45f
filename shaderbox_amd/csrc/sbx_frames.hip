// shaderbox_amd/csrc/sbx_frames.hip — the per-frame constant block of every app, and the defaults of the aux blocks.
//
// What the reference's hosts and the frame-constant prologue of each mainImage() compute from the uniforms alone, evaluated once per
// frame on the host with the shared math spec (sbx_math.h) and handed to the kernels as arguments.  Pure host math over the spec: it
// is compiled with the library's flags, -ffp-contract=off among them, because they are part of that spec.
#include "sbx_ctx.h"
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace sbx;

namespace sbx {

FrameClouds build_clouds(const sbx_uniforms& U, const sbx_aux_clouds& A, bool sky_sphere) {
    FrameClouds F;
    // setup_camera app_clouds.h:23-30
    const v3 eye = V3(0, -.5f, 0);
    const float angle = U.u_mouse[0] * .5f;
    const v3 look_at = mul(rotate_around_y(angle), V3(0, 0, -1));
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, eye, look_at);   // FOV 1. :219
    F.sun_dir = V3(A.sun_dir[0], A.sun_dir[1], A.sun_dir[2]);
    F.sun_color = V3(A.sun_color[0], A.sun_color[1], A.sun_color[2]);
    const v3 wind = V3(A.wind_dir[0], A.wind_dir[1], A.wind_dir[2]);
    F.wind_off = wind * U.u_time * (1.f / .001f);                      // :167
    F.sun_power = A.sun_power;
    F.sigma = A.sigma_scattering;
    F.steps = A.cld_march_steps;
    F.lsteps = A.illum_march_steps;
    F.dt = A.cld_thick / (float)A.cld_march_steps;                     // :98,180
    F.cov = 1.f - A.cld_coverage;                                      // :83
    F.cov_hi = F.cov + .0135f;                                         // :84
    F.cov_rd = recip64(F.cov_hi - F.cov);
    F.cov_d = F.cov_hi - F.cov;
    F.cov_r = 1.0f / F.cov_d;
    F.lip_ok = 0;                                                      // decided per launch (launch_clouds)
    F.exp_small = 0;
    F.thr1 = F.thr2 = 0.f;                                             // set per launch (launch_clouds)
    // SKY_SPHERE (:8,14-19,154-162)
    F.sky = sky_sphere ? 1 : 0;
    F.atm_y = A.atm_ground_y;
    F.atm_r = A.atm_radius;
    F.nf = sky_sphere ? ((1.f / A.atm_radius) * 10.f) : .001f;        // cld_noise_factor :18 / :20
    F.sky_rot = rotate_around_x(U.u_time);                            // :160
    return F;
}

static BezierFrame bezier_frame(v3 a, v3 b, v3 c) {                    // sdf.h:147-153
    BezierFrame B;
    B.b = b;
    B.w = normalize(cross(c - b, a - b));
    B.u = normalize(c - b);
    B.v = normalize(cross(B.w, B.u));
    B.a2 = V2(dot(a - b, B.u), dot(a - b, B.v));
    B.c2 = V2(dot(c - b, B.u), dot(c - b, B.v));
    B.bc = (a + b + c) * (1.f / 3.f);              // any point works; the radius below is measured from it
    B.br = fmax_(fmax_(length(a - B.bc), length(b - B.bc)), length(c - B.bc)) * 1.001f + 1e-4f;
    return B;
}
static CylFrame cyl_frame(v3 P0, v3 P1) {                              // sdf.h:104,106-107
    CylFrame C;
    C.dir = normalize(P1 - P0);
    C.len1 = length(P1);
    C.len0 = length(P0);
    return C;
}
static v3 ik_solver(v3 start, v3 goal_abs, float L1, float L2) {       // IK.h:5-52
    const v3 goal = goal_abs - start;
    const float G = length(goal);
    const float cos_theta = (L1 * L1 + G * G - L2 * L2) / (2.f * L1 * G);
    const float sin_theta = sqrt_(1.f - cos_theta * cos_theta);
    const m3 rot = M3(cos_theta, -sin_theta, 0, sin_theta, cos_theta, 0, 0, 0, 1.f);
    return start + mul(rot, normalize(goal) * L1);
}
// What setup_camera (:23-27) and sdf() (:40, :68-81) of app_egg.h make of u_time, as the block of SBX_APP_EGG_POSE (include/sbx.h): the
// ONE statement of the shipped pose — build_egg and sbx_egg_pose_default both read it
static void egg_default_pose(const sbx_uniforms& U, sbx_aux_egg_pose& A) {
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    put(A.eye, V3(.0f, .25f, 5.25f));                                  // :25
    put(A.look_at, V3(.0f, .25f, .0f));                                // :26
    A.fov = 1.f;                                                       // :253
    const float t = U.u_time;
    A.turn_deg = t * -100.0f;                                          // :40
    const v3 wheel_pos = V3(0, 1.2f, 0);
    const float pedal_radius = 0.3f, pedal_speed = 400.f, pedal_off = 0.2f;
    const m3 rot_z = rotate_around_z(-t * pedal_speed);                // :73,76
    put(A.left_foot, wheel_pos + mul(rot_z, V3(0.f, pedal_radius, pedal_off)));
    put(A.right_foot, wheel_pos + mul(rot_z, V3(0.f, -pedal_radius, -pedal_off)));
    A.femur = 0.8f; A.tibia = 0.75f;                                   // :80-81
}
// build: EGG_DEFAULT (app_egg.h as shipped), EGG_STRAIGHT (without `#define BEZIER`, :37) or EGG_OVAL (`#if 1` at :46 -> `#if 0`)
FrameEggStraight build_egg(const sbx_uniforms& U, int build) {
    sbx_aux_egg_pose A;
    egg_default_pose(U, A);
    return build_egg_pose(U, A, build);
}
// The frame of a pose: everything sdf() computes before it reads its point, from the block's values where app_egg.h has u_time or a
// literal (include/sbx.h sbx_aux_egg_pose).  Every bound below (the toe midpoints, the Bezier spheres, the bounding sphere) is
// computed FROM the pose, none is a constant of the shipped one: they hold for any pose whose frame is finite (egg_pose_tame).
FrameEggStraight build_egg_pose(const sbx_uniforms& U, const sbx_aux_egg_pose& A, int build) {
    FrameEggStraight F;
    F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, V3(A.eye[0], A.eye[1], A.eye[2]), V3(A.look_at[0], A.look_at[1], A.look_at[2]));   // app_egg.h:23-27,253
    F.rot_y = rotate_around_y(A.turn_deg);                             // :40
    const v3 wheel_pos = V3(0, 1.2f, 0);
    const float pedal_off = 0.2f;
    F.left_foot = V3(A.left_foot[0], A.left_foot[1], A.left_foot[2]);  // :73-77
    F.right_foot = V3(A.right_foot[0], A.right_foot[1], A.right_foot[2]);
    const v3 side = V3(0, 0, pedal_off);
    const float femur = A.femur, tibia = A.tibia, thick = .05f;           // :80-82
    const v3 zero = V3(0.f, 0.f, 0.f);
    const v3 knee_l = ik_solver(zero + side, F.left_foot, femur, tibia);   // :84-85
    const v3 knee_r = ik_solver(zero - side, F.right_foot, femur, tibia);  // :95-96
    F.leg_l = bezier_frame(-(zero + side), -knee_l, -F.left_foot);         // :111-113
    F.leg_r = bezier_frame(-(zero - side), -knee_r, -F.right_foot);        // :114-116
    // the straight legs (:86-93, :97-104): sd_cylinder(p + o, 0, axis, thick) fills, in p space, the segment from -o to -o - axis
    const v3 leg_o[4] = {zero + side, knee_l, zero - side, knee_r};
    const v3 leg_axis[4] = {knee_l - side, F.left_foot - knee_l, knee_r + side, F.right_foot - knee_r};
    for (int i = 0; i < 4; ++i) {
        F.leg[i] = cyl_frame(zero, leg_axis[i]);
        F.leg_o[i] = leg_o[i];
        F.leg_m[i] = -leg_o[i] + F.leg[i].dir * (F.leg[i].len1 * -.5f);
        F.leg_k[i] = F.leg[i].len1 * .5f + (thick + .0025f + 1e-3f);
    }
    const v3 left_toe = normalize(V3(F.left_foot.y - knee_l.y, knee_l.x - F.left_foot.x, 0));     // :120
    const v3 right_toe = normalize(V3(F.right_foot.y - knee_r.y, knee_r.x - F.right_foot.x, 0));  // :125
    F.foot_l = cyl_frame(zero, left_toe / 8.f);
    F.foot_r = cyl_frame(zero, right_toe / 8.f);
    // Bounding sphere of the egg, legs, feet and wheel (everything but the ground), see kern_egg.hip egg_far: each
    // member m has a centre c and a radius rho such that its sdf value is >= .7 * (|p - c| - rho) wherever that is
    // positive: egg spheres r + .36 (two smooth-mins of k = .5 lower the union by <= .25), tubes br + .061 (the .85
    // factor and the thickness), toe cylinders .161 around their midpoint (max(axis, slabs) >= |.|/sqrt2 - 1/16),
    // wheel 1.03.
    // The other builds have other members, so the sphere is the build's own (it also drives k_egg's hot rectangle):
    //   straight legs: max(line, plane, plane) - R >= |p - M| / sqrt2 - len / 2 - R around the midpoint M, and op_blend(a, b, .01)
    //                  lies at most .01 / 4 below min(a, b): rho = sqrt2 (len / 2 + R + .0025), which is 1.4143 leg_k
    //   oval egg:      |iscale scale q| >= |q| / 1.55, so the value is >= (|q| - 1.55 * .475) / 1.55: rho = .74, at the slope
    //                  1 / 1.55 < .7 that egg_far<EGG_OVAL> allows for (every other member's .7 holds a fortiori)
    F.foot_ml = -F.left_foot + left_toe * (-1.f / 16.f);
    F.foot_mr = -F.right_foot + right_toe * (-1.f / 16.f);
    const float egg_y = 0.65f;
    if (build == EGG_DEFAULT) {
        const v3 cs[8] = {V3(0, egg_y, 0), V3(0, egg_y - 0.45f, 0), V3(0, egg_y + 0.45f, 0), F.leg_l.bc, F.leg_r.bc,
                          -F.left_foot + left_toe * (-1.f / 16.f), -F.right_foot + right_toe * (-1.f / 16.f), -wheel_pos};
        const float rs[8] = {.475f + .36f, .25f + .36f, .25f + .36f, F.leg_l.br + .061f, F.leg_r.br + .061f, .161f, .161f, 1.03f};
        v3 c = V3(0, 0, 0);
        for (int i = 0; i < 8; ++i) c = c + cs[i] * .125f;
        float R = 0.f;
        for (int i = 0; i < 8; ++i) R = fmax_(R, length(cs[i] - c) + rs[i]);
        F.oc = c;
        F.orad = R * 1.001f + 1e-3f;
    } else {
        v3 cs[10];
        float rs[10];
        int n = 0;
        auto member = [&](v3 c, float rho) { cs[n] = c; rs[n] = rho; ++n; };
        if (build == EGG_OVAL) member(V3(0, egg_y, 0), .74f);
        else { member(V3(0, egg_y, 0), .475f + .36f); member(V3(0, egg_y - 0.45f, 0), .25f + .36f); member(V3(0, egg_y + 0.45f, 0), .25f + .36f); }
        if (build == EGG_STRAIGHT) for (int i = 0; i < 4; ++i) member(F.leg_m[i], F.leg_k[i] * 1.4143f);
        else { member(F.leg_l.bc, F.leg_l.br + .061f); member(F.leg_r.bc, F.leg_r.br + .061f); }
        member(F.foot_ml, .161f); member(F.foot_mr, .161f); member(-wheel_pos, 1.03f);
        v3 c = V3(0, 0, 0);
        for (int i = 0; i < n; ++i) c = c + cs[i] * (1.f / (float)n);
        float R = 0.f;
        for (int i = 0; i < n; ++i) R = fmax_(R, length(cs[i] - c) + rs[i]);
        F.oc = c;
        F.orad = R * 1.001f + 1e-3f;
    }
    F.ocw = mul(transpose(F.rot_y), F.oc + V3(0, 0.5f, 3.5f));     // p = rot_y P - (0, .5, 3.5)  <=>  P = rot_y^T (p + (0, .5, 3.5))
    return F;
}

// Do k_egg's culls and witnessed roots stand for this pose?  Their proofs (kern_egg.hip, sbx_sdf.h) take finite frame constants and
// sample points of the scene's own scale: a NaN knee (a goal beyond femur + tibia), a NaN toe or Bezier frame (collinear or coincident
// points), a non-finite angle or camera leave comparisons against NaN, and a coordinate near 2^64 overflows the squared lengths the
// culls compare.  So: every value of the block finite and within 1e4 in magnitude (a ray then stays within 15 + twice that of the
// origin, the trace's own end), and every derived constant of the frame finite.  Anything else renders with the reference form
// (CULL = false, IEEE roots: sbx_set_variant 1's kernel), which is the same operations as the reference on whatever the values are.
bool egg_pose_tame(const sbx_aux_egg_pose& A, const FrameEgg& F) {
    static_assert(sizeof(sbx_aux_egg_pose) == 16 * sizeof(float), "sbx_aux_egg_pose is 16 floats (include/sbx.h)");
    float a[16];                                                       // eye, fov, look_at, turn_deg, left_foot, femur, right_foot, tibia
    std::memcpy(a, &A, sizeof(a));
    // (turn_deg is an angle: its bound is the one sbx_capi.hip's tame_time puts on u_time * -100, inside which the spec's sin / cos
    // return a rotation)
    for (int i = 0; i < 16; ++i) if (!(std::fabs(a[i]) <= (i == 7 ? 1e10f : 1e4f))) return false;
    auto fin = [](float x) { return std::fabs(x) <= 3.4028234e38f; };  // NaN compares false
    auto fin3 = [&](v3 v) { return fin(v.x) && fin(v.y) && fin(v.z); };
    auto finb = [&](const BezierFrame& B) { return fin3(B.b) && fin3(B.u) && fin3(B.v) && fin3(B.w) && fin(B.a2.x) && fin(B.a2.y) && fin(B.c2.x) && fin(B.c2.y) && fin3(B.bc) && fin(B.br); };
    auto finc = [&](const CylFrame& C) { return fin3(C.dir) && fin(C.len1) && fin(C.len0); };
    return fin3(F.cam.eye) && fin3(F.cam.fwd) && fin3(F.cam.right) && fin3(F.cam.up) && fin(F.cam.fov) && fin(F.cam.aspect_x) &&
           fin3(F.rot_y.c0) && fin3(F.rot_y.c1) && fin3(F.rot_y.c2) && finb(F.leg_l) && finb(F.leg_r) && finc(F.foot_l) && finc(F.foot_r) &&
           fin3(F.foot_ml) && fin3(F.foot_mr) && fin3(F.oc) && fin(F.orad) && fin3(F.ocw);
}

// The Cornell box of app_raytracer.h as a scene block (include/sbx.h sbx_aux_raytracer_scene): setup_scene :18-36 over setup_cornell_box
// cornell_box.h:39-87, setup_camera :38-44 and the FOV of :138.  The ONE statement of that scene: build_raytracer (the four builds of
// SBX_APP_RAYTRACER) and sbx_raytracer_scene_cornell (SBX_APP_RAYTRACER_SCENE's default block) both read it.
static void cornell_block(const sbx_uniforms& U, bool at_rest, sbx_aux_raytracer_scene& A) {
    std::memset(&A, 0, sizeof(A));
    const float cb = 2.f;                                              // cb_plane_dist cornell_box.h:62
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    // setup_camera app_raytracer.h:38-44
    v2 mouse = V2(0, 0);
    if (!(U.u_mouse[0] < 1e-4f)) mouse = V2(2.f * (U.u_res[0] / U.u_mouse[0]) - 1.f, 2.f * (U.u_res[1] / U.u_mouse[1]) - 1.f);
    const m3 rot_y = rotate_around_y(mouse.x * 30.f);
    put(A.eye, mul(rot_y, V3(0, cb, 2.333f * cb)));
    put(A.look_at, V3(0, cb, 0));
    A.fov = tan_(radians_(30.f));                                      // FOV :138
    A.bounces = 2;                                                     // :96
    A.light_type = 1;                                                  // LIGHT_POINT cornell_box.h:83
    A.lighting = 0;                                                    // illum_cook_torrance :64
    A.shadow = 1;                                                      // :107
    put(A.light_color, V3(1.f, 1.f, 1.f));                             // cornell_box.h:85
    put(A.ambient, V3(.01f, .01f, .01f));                              // light.h:16
    // materials: zero-initialised slots (App. B5), mat_debug :20-25, cornell box cornell_box.h:47-55
    auto material = [&](int i, v3 c, float metallic, float roughness, float ior, float reflectivity) {
        put(A.materials[i].base_color, c);
        A.materials[i].metallic = metallic; A.materials[i].roughness = roughness; A.materials[i].ior = ior;
        A.materials[i].reflectivity = reflectivity; A.materials[i].translucency = 0.f;
    };
    material(0, V3(1.f, 1.f, 1.f), 0.f, 0.f, 1.f, 0.f);
    material(1, V3(0.7913f, 0.7913f, 0.7913f), .0f, .5f, 1.f, 0.f);
    material(2, V3(0.6795f, 0.0612f, 0.0529f), 0.f, .5f, 1.f, 0.f);
    material(3, V3(0.1878f, 0.1274f, 0.4287f), 0.f, .5f, 1.f, 0.f);
    material(4, V3(0.95f, 0.64f, 0.54f), 1.f, .1f, 1.f, 1.f);
    material(5, V3(1.f, 0.77f, 0.345f), 1.f, .05f, 1.333f, 1.f);
    // planes, in array-index order ground, behind, front, ceiling, left, right  cornell_box.h:57-69
    auto plane = [&](int i, v3 n, float d, int mat) { put(A.planes[i].direction, n); A.planes[i].distance = d; A.planes[i].material = mat; };
    A.n_planes = 6;
    plane(0, V3(0, -1, 0), 0.f, 1);
    plane(1, V3(0, 0, -1), -cb, 1);
    plane(2, V3(0, 0, 1), cb, 1);
    plane(3, V3(0, 1, 0), 2.f * cb, 1);
    plane(4, V3(1, 0, 0), cb, 2);
    plane(5, V3(-1, 0, 0), -cb, 3);
    // spheres and light as cornell_box.h:71-85 puts them: the whole scene at rest (the `#if 1` at app_raytracer.h:29 off), which
    // reads no u_time
    auto sphere = [&](int i, v3 o, float r, int mat) { put(A.spheres[i].origin, o); A.spheres[i].radius = r; A.spheres[i].material = mat; };
    A.n_spheres = 3;
    sphere(0, V3(0, 2.5f * cb + 0.4f, 0), 1.5f, 0);
    v3 left = V3(0.75f, 1, -0.75f), right = V3(-0.75f, 0.75f, 0.75f), light = V3(0, 2.f * cb - 0.2f, 0);
    if (!at_rest) {                                                    // the animation app_raytracer.h:29-35
        const float s = sin_(U.u_time), c = cos_(U.u_time);
        left = left + V3(0, abs_(s), c + 1.f);
        right.z = 0.f;
        light.z = 1.5f;
    }
    sphere(1, left, 0.75f, 4);
    sphere(2, right, 0.75f, 5);
    put(A.light_L, light);
}
static v3 v3_of(const float* p) { return V3(p[0], p[1], p[2]); }
static RtMaterial rt_material(const sbx_rt_material& m) {
    const float Rn = (1.f - m.ior) / (1.f + m.ior);                    // util_optics.h:10-11 with n1 = 1, per material
    return RtMaterial{v3_of(m.base_color), m.roughness, m.ior, m.reflectivity, Rn * Rn};
}
static RtPlane rt_plane(const sbx_rt_plane& p) { return RtPlane{v3_of(p.direction), p.distance, p.material}; }
static RtSphere rt_sphere(const sbx_rt_sphere& s) { return RtSphere{v3_of(s.origin), s.radius, s.material, recip64(s.radius)}; }

FrameRaytracer build_raytracer(const sbx_uniforms& U, int build) {
    sbx_aux_raytracer_scene A;
    cornell_block(U, build == RT_STATIC, A);
    FrameRaytracer F;
    F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, v3_of(A.eye), v3_of(A.look_at));
    for (int i = 0; i < 8; ++i) F.mats[i] = rt_material(A.materials[i]);
    for (int i = 0; i < 6; ++i) F.planes[i] = rt_plane(A.planes[i]);
    for (int i = 0; i < 3; ++i) F.spheres[i] = rt_sphere(A.spheres[i]);
    F.light = v3_of(A.light_L);
    return F;
}

// the range checks of a caller's scene, the app's and sbx_raytracer_eval's: the counts are within the arrays, the switches are switches
const char* raytracer_scene_check(const sbx_aux_raytracer_scene& A) {
    if (A.n_planes < 0 || A.n_planes > SBX_RT_MAX_PLANES || A.n_spheres < 0 || A.n_spheres > SBX_RT_MAX_SPHERES)
        return "raytracer scene: n_planes and n_spheres must lie in 0..16";
    if (A.bounces < 1 || A.bounces > 8) return "raytracer scene: bounces must lie in 1..8";
    if (A.light_type != 1 && A.light_type != 2) return "raytracer scene: light_type must be 1 (LIGHT_POINT) or 2 (LIGHT_DIR)";
    if (A.lighting != 0 && A.lighting != 1) return "raytracer scene: lighting must be 0 (Cook-Torrance) or 1 (Phong)";
    if (A.shadow != 0 && A.shadow != 1) return "raytracer scene: shadow must be 0 or 1";
    return nullptr;
}

// SBX_APP_RAYTRACER_SCENE / sbx_raytracer_eval: the caller's block (one that passed raytracer_scene_check) as the kernels read it.
// The slots past the counts are copied as they are; the kernels never read them.
FrameRtScene build_raytracer_scene(const sbx_uniforms& U, const sbx_aux_raytracer_scene& A) {
    FrameRtScene F;
    F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, v3_of(A.eye), v3_of(A.look_at));
    F.n_planes = A.n_planes; F.n_spheres = A.n_spheres;
    F.bounces = A.bounces; F.lighting = A.lighting; F.shadow = A.shadow; F.light_type = A.light_type;
    F.light = v3_of(A.light_L);
    F.ambient = v3_of(A.ambient);
    for (int i = 0; i < 8; ++i) F.mats[i] = rt_material(A.materials[i]);
    for (int i = 0; i < RT_MAX_PLANES; ++i) F.planes[i] = rt_plane(A.planes[i]);
    for (int i = 0; i < RT_MAX_SPHERES; ++i) F.spheres[i] = rt_sphere(A.spheres[i]);
    return F;
}

FrameAtmosphere build_atmosphere(const sbx_uniforms& U) {
    FrameAtmosphere F;
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, V3(0, 0, 0), V3(0, 1, 0));   // app_atmosphere.h:164-175,230
    const m3 rot = rotate_around_x(-abs_(sin_(U.u_time / 2.f)) * 90.f);             // :179
    F.sun_dir = mul(V3(0, 1, 0), rot);                                              // :180 (v * M)
    return F;
}

// app_atmosphere.h without FROM_SPACE: the camera of :172-173 (both y values exact in binary32), the same sun
FrameAtmosphere build_atmosphere_ground(const sbx_uniforms& U) {
    FrameAtmosphere F = build_atmosphere(U);
    const float earth_radius = 6360e3f;                                             // :37
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, V3(0, earth_radius + 1.f, 0), V3(0, earth_radius + 1.5f, -1));   // :172-173,230
    return F;
}

// ---- SBX_APP_ATMOSPHERE_AIR (include/sbx.h sbx_aux_atmosphere_air; the tiers: sbx_atmosphere.h "CALLER'S AIR") ----------------------
// the reference's numbers (app_atmosphere.h:12,29-41,47-48,172-173,230; the literals of sbx_atmosphere.h) with the sun of build_atmosphere
static void atmosphere_default_air(const sbx_uniforms& U, int view, sbx_aux_atmosphere_air& A) {
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    std::memset(&A, 0, sizeof(A));
    const float earth_radius = 6360e3f;
    A.view = view;
    A.num_samples = 16; A.num_samples_light = 8;
    put(A.eye, V3(0, earth_radius + 1.f, 0)); A.fov = 1.f;
    put(A.look_at, V3(0, earth_radius + 1.5f, -1)); A.hg_g = .76f;
    put(A.sun_dir, build_atmosphere(U).sun_dir); A.sun_power = 20.0f;
    put(A.betaR, V3(5.5e-6f, 13.0e-6f, 22.4e-6f)); A.hR = 7994.0f;
    put(A.betaM, V3(21e-6f, 21e-6f, 21e-6f)); A.hM = 1200.0f;
    A.earth_radius = earth_radius; A.atmosphere_radius = 6420e3f;
}
const char* atmosphere_air_check(const sbx_aux_atmosphere_air& A, bool app) {
    static_assert(sizeof(sbx_aux_atmosphere_air) == 128, "sbx_aux_atmosphere_air is 128 bytes (include/sbx.h)");
    if (app && A.view != 0 && A.view != 1) return "atmosphere air: view must be 0 (the sky dome) or 1 (the ground camera)";
    if (A.num_samples < 1 || A.num_samples > 64) return "atmosphere air: num_samples must lie in 1..64";
    if (A.num_samples_light < 1 || A.num_samples_light > 32) return "atmosphere air: num_samples_light must lie in 1..32";
    uint32_t r[6];
    std::memcpy(r, A.reserved, sizeof(r));
    if (A.reserved0 != 0 || (r[0] | r[1] | r[2] | r[3] | r[4] | r[5]) != 0u) return "atmosphere air: the reserved words must be 0";
    return nullptr;
}
// view 0: main.h's camera of the FROM_SPACE build (:169-170; only point_cam reads it) with the block's FOV, and the block's eye as the
// dome's ray origin (:205); view 1: the camera of :172-173 from the block
FrameAtmosphere build_atmosphere_air(const sbx_uniforms& U, const sbx_aux_atmosphere_air& A) {
    FrameAtmosphere F;
    const v3 eye = V3(A.eye[0], A.eye[1], A.eye[2]);
    if (A.view == 0) {
        F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, V3(0, 0, 0), V3(0, 1, 0));
        F.cam.eye = eye;
    } else {
        F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, eye, V3(A.look_at[0], A.look_at[1], A.look_at[2]));
    }
    F.sun_dir = V3(A.sun_dir[0], A.sun_dir[1], A.sun_dir[2]);
    return F;
}
static bool positive_number(float v) { return v > 0.f && std::isfinite(v); }
AtmAir atmosphere_air_numbers(const sbx_aux_atmosphere_air& A) {
    AtmAir K;
    K.betaR = V3(A.betaR[0], A.betaR[1], A.betaR[2]);
    K.betaM = V3(A.betaM[0], A.betaM[1], A.betaM[2]);
    K.hR = A.hR; K.rhR = 1.0f / A.hR;
    K.hM = A.hM; K.rhM = 1.0f / A.hM;
    K.earth_r = A.earth_radius; K.atmos_r = A.atmosphere_radius;
    K.sun_power = A.sun_power; K.g = A.hg_g;
    K.ns = A.num_samples; K.nl = A.num_samples_light;
    K.dead_ok = 1;
    for (int k = 0; k < 3; ++k) if (!positive_number(A.betaR[k]) || !positive_number(A.betaM[k])) K.dead_ok = 0;
    return K;
}
// the host's part of the class (kern_atmosphere.hip atm_eval_sun_ok): a sun that is finite and a unit vector to 1e-4
static bool air_sun_ok(const float* s) {
    const float ss = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
    return std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]) && std::fabs(ss - 1.0f) <= 1e-4f;
}
static bool same_floats(const float* a, const float* b, int n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }
// radii, scale heights and counts are the reference's bit for bit: the domain in which sbx_atmosphere.h's proofs are written
static bool air_default_geometry(const sbx_aux_atmosphere_air& A, const sbx_aux_atmosphere_air& D) {
    return same_floats(&A.earth_radius, &D.earth_radius, 1) && same_floats(&A.atmosphere_radius, &D.atmosphere_radius, 1) &&
           same_floats(&A.hR, &D.hR, 1) && same_floats(&A.hM, &D.hM, 1) && A.num_samples == 16 && A.num_samples_light == 8;
}
bool atmosphere_air_tame(const sbx_aux_atmosphere_air& A) {
    sbx_aux_atmosphere_air D;
    atmosphere_default_air(sbx_uniforms{}, 0, D);
    return air_default_geometry(A, D) && air_sun_ok(A.sun_dir);
}
int atmosphere_air_tier(const sbx_aux_atmosphere_air& A, int variant, bool app) {
    if (variant == 1) return ATM_AIR_PLAIN;
    sbx_aux_atmosphere_air D;
    atmosphere_default_air(sbx_uniforms{}, 0, D);
    const bool solver = air_default_geometry(A, D) && same_floats(A.betaR, D.betaR, 3) && same_floats(A.betaM, D.betaM, 3) &&
                        same_floats(&A.sun_power, &D.sun_power, 1) && same_floats(&A.hg_g, &D.hg_g, 1);
    if (app && solver && same_floats(A.eye, D.eye, 3) && (A.view == 1 || same_floats(&A.fov, &D.fov, 1))) return ATM_AIR_LITERAL;
    return atmosphere_air_tame(A) ? ATM_AIR_RUNTIME : ATM_AIR_PLAIN;
}
bool atmosphere_air_literal_fin(const sbx_aux_atmosphere_air& A, const FrameAtmosphere& F) {
    if (!air_sun_ok(A.sun_dir)) return false;
    if (A.view == 0) return true;
    const float ff = (F.cam.fwd.x * F.cam.fwd.x + F.cam.fwd.y * F.cam.fwd.y) + F.cam.fwd.z * F.cam.fwd.z;
    return std::fabs(ff - 1.0f) <= 1e-4f;                          // (a NaN compares false)
}

FrameSdfAo build_sdf_ao(const sbx_uniforms& U, const sbx_aux_sdf_ao& A) {
    FrameSdfAo F;
    const m3 rot = rotate_around_y(U.u_time * 50.f);                   // app_sdf_ao.h:45-50
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, mul(rot, V3(0, 3, 5)), V3(0, 0, 0));
    F.rx_m90 = rotate_around_x(-90.f);
    F.ry_180 = rotate_around_y(180.f);
    F.sun_dir = normalize(V3(1, 2, 1));
    F.fog_density = A.fog_density;
    F.fog_falloff = A.fog_falloff;
    return F;
}

// ---- SBX_APP_SDF_SCENE (include/sbx.h sbx_aux_sdf_scene) -------------------------------------------------------------------------
// The checks of include/sbx.h, in its order: the renderer's settings (unless program_only), then the program walked once with its
// stack depth.  After it every loop of k_sdf_scene has a bound and every stack slot is written before it is read.
const char* sdf_scene_check(const sbx_aux_sdf_scene& A, bool program_only) {
    if (A.n_instr < 1 || A.n_instr > SBX_SDF_MAX_INSTR) return "sdf scene: n_instr must lie in 1..32";
    if (!program_only) {
        if (A.checker_material < -1 || A.checker_material > 7) return "sdf scene: checker_material must lie in -1..7";
        if (A.march_steps < 1 || A.march_steps > 512) return "sdf scene: march_steps must lie in 1..512";
        if (A.shadow != 0 && A.shadow != 1) return "sdf scene: shadow must be 0 or 1";
        if (A.view != 0 && A.view != 1) return "sdf scene: view must be 0 or 1";
    }
    int depth = 0;
    for (int i = 0; i < A.n_instr; ++i) {
        const sbx_sdf_instr& I = A.program[i];
        if (I.op >= SBX_SDF_PLANE && I.op <= SBX_SDF_BEZIER) {
            if (I.rot_axis < 0 || I.rot_axis > 3) return "sdf scene: rot_axis must lie in 0..3";
            if (++depth > SBX_SDF_MAX_STACK) return "sdf scene: the stack exceeds SBX_SDF_MAX_STACK";
        } else if (I.op >= SBX_SDF_ADD && I.op <= SBX_SDF_BLEND) {
            if (I.rot_axis < 0 || I.rot_axis > 3) return "sdf scene: rot_axis must lie in 0..3";
            if (depth < 2) return "sdf scene: the stack underflows at an operator";
            --depth;
        } else if (I.op == SBX_SDF_OBJECT) {
            if (I.rot_axis < 0 || I.rot_axis > 3) return "sdf scene: rot_axis must lie in 0..3";
            if (I.material < 0 || I.material > 7) return "sdf scene: an OBJECT's material must lie in 0..7";
            if (depth < 1) return "sdf scene: the stack underflows at an OBJECT";
            if (--depth != 0) return "sdf scene: the stack is not empty at an OBJECT after its pop";
        } else {
            return "sdf scene: unknown op";
        }
    }
    if (A.program[A.n_instr - 1].op != SBX_SDF_OBJECT) return "sdf scene: the last instruction must be an OBJECT";
    return nullptr;                                                    // (depth is 0 here: the last OBJECT left it so)
}

// normalize(v) with three IEEE quotients: sbx_vec.h's form divides through a binary64 reciprocal, which is not the IEEE quotient where
// the quotient is subnormal (sbx_math.h) — the caller's numbers can be anything
static v3 normalize_ieee(v3 v) {
    const float l = length(v);
    return V3(v.x / l, v.y / l, v.z / l);
}
static v3 v3_at(const float* p) { return V3(p[0], p[1], p[2]); }

FrameSdfScene build_sdf_scene(const sbx_uniforms& U, const sbx_aux_sdf_scene& A) {
    FrameSdfScene F;
    std::memset(&F, 0, sizeof(F));
    {                                                                  // make_camera (sbx_frame.h), util.h:10-13, IEEE quotients
        const v3 eye = v3_at(A.eye), look_at = v3_at(A.look_at);
        Camera& c = F.cam;
        c.res_x = U.u_res[0]; c.res_y = U.u_res[1];
        c.aspect_x = U.u_res[0] / U.u_res[1];
        c.fov = A.fov;
        c.rres_x = recip64(U.u_res[0]); c.rres_y = recip64(U.u_res[1]);
        c.eye = eye;
        c.fwd = normalize_ieee(look_at - eye);
        c.right = cross(V3(0, 1, 0), c.fwd);
        c.up = cross(c.fwd, c.right);
    }
    F.n_instr = A.n_instr; F.steps = A.march_steps; F.shadow = A.shadow; F.view = A.view; F.checker = A.checker_material;
    F.end = A.march_end; F.fog_density = A.fog_density; F.fog_falloff = A.fog_falloff;
    F.sun_dir = v3_at(A.sun_dir); F.background = v3_at(A.background);
    for (int i = 0; i < 8; ++i) F.mats[i] = v3_at(A.materials[i]);
    for (int i = 0; i < A.n_instr; ++i) {                              // (the slots past n_instr stay zero; the kernel never reads them)
        const sbx_sdf_instr& I = A.program[i];
        SdfOp& O = F.prog[i];
        O.ctl = (int)(1u << sdf_op_bit(I.op) | (unsigned)I.rot_axis << 16);
        const float ang = radians_(I.rot_deg);                         // util.h:44-69
        O.s = sin_(ang); O.c = cos_(ang);
        O.off = v3_at(I.offset);
        auto put = [&O](int k, v3 v) { O.p[k] = v.x; O.p[k + 1] = v.y; O.p[k + 2] = v.z; };
        switch (I.op) {
        case SBX_SDF_PLANE: case SBX_SDF_BOX: for (int k = 0; k < 4; ++k) O.p[k] = I.a[k]; break;
        case SBX_SDF_SPHERE: O.p[0] = I.a[0]; break;
        case SBX_SDF_TORUS: case SBX_SDF_Y_CYLINDER: O.p[0] = I.a[0]; O.p[1] = I.a[1]; break;
        case SBX_SDF_CYLINDER: {                                       // sdf.h:104,106-107
            const v3 P0 = v3_at(I.a), P1 = v3_at(I.b);
            put(0, normalize_ieee(P1 - P0));
            O.p[3] = length(P1); O.p[4] = length(P0);
            put(5, P0);
            O.p[8] = I.a[3];
            break;
        }
        case SBX_SDF_CAPSULE: {                                        // sdf.h:168-169
            const v3 a = v3_at(I.a), ab = v3_at(I.b) - a;
            put(0, a); put(3, ab);
            O.p[6] = dot(ab, ab);
            O.p[7] = I.a[3];
            break;
        }
        case SBX_SDF_BEZIER: {                                         // sdf.h:147-153
            const v3 a = v3_at(I.a), b = v3_at(I.b), c = v3_at(I.c);
            const v3 w = normalize_ieee(cross(c - b, a - b));
            const v3 u = normalize_ieee(c - b);
            const v3 v = normalize_ieee(cross(w, u));
            put(0, b); put(3, u); put(6, v); put(9, w);
            O.p[12] = dot(a - b, u); O.p[13] = dot(a - b, v);
            O.p[14] = dot(c - b, u); O.p[15] = dot(c - b, v);
            O.p[16] = I.a[3];
            break;
        }
        case SBX_SDF_BLEND: O.p[0] = I.a[0]; break;
        case SBX_SDF_OBJECT: O.p[0] = (float)I.material; break;
        default: break;
        }
    }
    return F;
}

// The default block of SBX_APP_SDF_SCENE (include/sbx.h sbx_sdf_scene_ramp): one ramp of sdf_pipe (app_sdf_ao.h:54-113) and the ground
static void sdf_ramp_block(const sbx_uniforms& U, sbx_aux_sdf_scene& A) {
    std::memset(&A, 0, sizeof(A));
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    const m3 rot = rotate_around_y(U.u_time * 50.f);                   // setup_camera :45-50
    put(A.eye, mul(rot, V3(0, 3, 5)));
    put(A.look_at, V3(0, 0, 0));
    A.fov = 1.f;                                                       // :313
    A.march_steps = 70; A.march_end = 20.f;                            // :249-250
    put(A.sun_dir, normalize(V3(1, 2, 1)));                            // :209
    put(A.background, V3(.1f, .1f, .7f));                              // :11
    A.shadow = 0; A.view = 0; A.checker_material = 1;
    A.fog_density = .1f; A.fog_falloff = .5f;                          // uniform_buffer.h:56-60
    const v3 mats[6] = {V3(1, 1, 1), V3(0, .2f, 0), V3(.1f, .1f, .1f), V3(.1f, .1f, .1f), V3(.1f, .1f, .1f), V3(.4f, .4f, .4f)};   // :35-43
    for (int i = 0; i < 6; ++i) put(A.materials[i], mats[i]);
    int n = 0;
    auto prim = [&](int op, v3 off, float a0, float a1, float a2, float a3, int axis = 0, float deg = 0.f) {
        sbx_sdf_instr& I = A.program[n++];
        I.op = op; I.rot_axis = axis; I.rot_deg = deg;
        put(I.offset, off);
        I.a[0] = a0; I.a[1] = a1; I.a[2] = a2; I.a[3] = a3;
    };
    auto oper = [&](int op) { A.program[n++].op = op; };
    auto object = [&](int material) { sbx_sdf_instr& I = A.program[n++]; I.op = SBX_SDF_OBJECT; I.material = material; };
    const v3 size = V3(1.3f, 1.f, 1.25f);                              // :52
    const v3 o1 = V3(0, size.y, 0);                                    // :58, :74
    prim(SBX_SDF_BOX, o1, size.x, size.y, size.z, 0.f);                // :60
    prim(SBX_SDF_Y_CYLINDER, o1 + V3(.7f, .5f, 0), size.y + .55f, 2.f * size.z + .1f, 0.f, 0.f, 1, -90.f);   // :62-66
    oper(SBX_SDF_SUB);                                                 // :69
    object(2);                                                         // mat_pipe
    prim(SBX_SDF_Y_CYLINDER, o1 + V3(-size.x + .525f, size.y, 0), .025f, 2.f * size.z, 0.f, 0.f, 1, -90.f);   // :76-81
    object(5);                                                         // mat_coping
    const v3 o2 = V3(0, size.y * 2.f, 0);                              // :86
    prim(SBX_SDF_BOX, o2 - V3(size.x, -.25f, 0), .025f, .05f, size.z, 0.f);   // rail :88-90
    const float H = -.125f;
    const float bz[5] = {0.f, size.z / 2.f, size.z, -size.z / 2.f, -size.z};   // :94-98
    auto bar = [&](int k) { prim(SBX_SDF_BOX, o2 - V3(size.x, H, bz[k]), .025f, .125f, .025f, 0.f); };
    bar(0); bar(1); oper(SBX_SDF_ADD);                                 // b_a :99
    bar(2); oper(SBX_SDF_ADD);                                         // b_b :100
    bar(3); bar(4); oper(SBX_SDF_ADD);                                 // b_c :101
    oper(SBX_SDF_ADD);                                                 // b_d :102
    oper(SBX_SDF_ADD);                                                 // op_add(rail, bars) :106
    object(4);                                                         // mat_deck
    prim(SBX_SDF_PLANE, V3(0, 0, 0), 0.f, 1.f, 0.f, 0.f);              // ground :143-145
    object(1);                                                         // mat_ground
    A.n_instr = n;
}

static Capsule capsule(v3 a, v3 b) {                                   // sdf.h:168-169
    Capsule c;
    c.a = a;
    c.ab = b - a;
    c.rd = recip64(dot(c.ab, c.ab));
    return c;
}
// What setup_scene (:40-54), setup_camera (:56-67), render (:419-428), sdf_tonearm (:141-142), illuminate (:327-329, :375) and :284-285 of
// app_vinyl.h make of u_time or state as literals, as the block of SBX_APP_VINYL_DECK (include/sbx.h): the ONE statement of the shipped
// deck — build_vinyl and sbx_vinyl_deck_default both read it
static void vinyl_default_deck(const sbx_uniforms& U, sbx_aux_vinyl_deck& A) {
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    put(A.eye, V3(0, 5.75f, 6.75f));                                   // :61
    put(A.look_at, V3(0, -2.5f, 0));                                   // :62
    A.fov = 1.f;                                                       // :460
    const float t = U.u_time;
    A.platter_deg = t * 200.f;                                         // :419
    A.platter_tilt_deg = sin_(t) * .1f;                                // :428
    A.arm_tilt_deg = sin_(t * 3.6758f) * .1f;                          // :141-142
    put(A.sun_dir, normalize(V3(-1, 4, -3)));                          // :284-285
    put(A.groove_color, V3(.01f, .01f, .01f));                         // :45
    put(A.dead_wax_color, V3(.05f, .05f, .05f));                       // :47
    put(A.label_color, V3(.5f, .5f, .0f));                             // :49
    put(A.logo_color, V3(0, 0, .7f));                                  // :51
    put(A.shiny_color, V3(.7f, .7f, .7f));                             // :53
    A.ro_spec = .0725f; A.a_x = .025f; A.a_y = .5f;                    // :327-329
    A.shininess = 50.f;                                                // :375
}
FrameVinyl build_vinyl(const sbx_uniforms& U, int steps, int build) {
    sbx_aux_vinyl_deck A;
    vinyl_default_deck(U, A);
    if (build == VINYL_CLOSEUP) {                                      // setup_camera's `#else` :64-65
        A.eye[0] = -2; A.eye[1] = 1.5f; A.eye[2] = 5.5f;
        A.look_at[0] = -1.5f; A.look_at[1] = 0; A.look_at[2] = 0;
    }
    return build_vinyl_deck(U, A, steps);
}
VinylShade vinyl_shade_of(const sbx_aux_vinyl_deck& A) {
    auto get = [](const float* d) { return V3(d[0], d[1], d[2]); };
    VinylShade D;
    D.color[0] = get(A.groove_color); D.color[1] = get(A.dead_wax_color); D.color[2] = get(A.label_color);
    D.color[3] = get(A.logo_color); D.color[4] = get(A.shiny_color);
    D.ro_spec = A.ro_spec; D.a_x = A.a_x; D.a_y = A.a_y; D.shininess = A.shininess;
    return D;
}
// Do k_vinyl's culls and hardware min / max stand for this deck?  The domain is argued at the top of sbx_vinyl.h: every value of the
// block's first sixteen (camera, angles, sun) finite and within 1e4 in magnitude — the three angles within 1e10, the bound
// sbx_capi.hip's tame_time puts on u_time * 200 — and every derived constant of the frame finite.  The colours and shading constants
// are not part of it.  Anything else renders with the reference form (CULL = false, IEEE roots: sbx_set_variant 1's kernel).
bool vinyl_deck_tame(const sbx_aux_vinyl_deck& A, const FrameVinyl& F) {
    static_assert(sizeof(sbx_aux_vinyl_deck) == 32 * sizeof(float), "sbx_aux_vinyl_deck is 32 floats (include/sbx.h)");
    float a[16];                                                       // eye, fov, look_at, platter_deg, sun_dir, platter_tilt_deg, groove_color, arm_tilt_deg
    std::memcpy(a, &A, sizeof(a));
    for (int i = 0; i < 12; ++i) if (!(std::fabs(a[i]) <= ((i & 3) == 3 && i != 3 ? 1e10f : 1e4f))) return false;
    if (!(std::fabs(a[15]) <= 1e10f)) return false;
    auto fin = [](float x) { return std::fabs(x) <= 3.4028234e38f; };  // NaN compares false
    auto fin3 = [&](v3 v) { return fin(v.x) && fin(v.y) && fin(v.z); };
    auto finm = [&](const m3& m) { return fin3(m.c0) && fin3(m.c1) && fin3(m.c2); };
    return fin3(F.cam.eye) && fin3(F.cam.fwd) && fin3(F.cam.right) && fin3(F.cam.up) && fin(F.cam.fov) && fin(F.cam.aspect_x) &&
           finm(F.platter_rot) && finm(F.wobble) && fin3(F.sun_dir);
}
// The frame of a deck: everything render and sdf_tonearm compute before they read a point, from the block's values where app_vinyl.h
// has u_time or a literal (include/sbx.h sbx_aux_vinyl_deck).  The tonearm's frames depend on nothing.
FrameVinyl build_vinyl_deck(const sbx_uniforms& U, const sbx_aux_vinyl_deck& A, int steps) {
    FrameVinyl F;
    F.steps = steps;                                                   // :411-416
    F.cam = make_camera(U.u_res[0], U.u_res[1], A.fov, V3(A.eye[0], A.eye[1], A.eye[2]), V3(A.look_at[0], A.look_at[1], A.look_at[2]));   // app_vinyl.h:56-67,460
    F.platter_rot = mul(rotate_around_y(A.platter_deg), rotate_around_x(A.platter_tilt_deg));          // :419,426-428
    F.sun_dir = V3(A.sun_dir[0], A.sun_dir[1], A.sun_dir[2]);          // :284-285, as given
    F.ry30 = rotate_around_y(30.f);
    F.rym30 = rotate_around_y(-30.f);
    F.wobble = rotate_around_x(A.arm_tilt_deg);                        // :141-142
    const float R = .1f, H = .8f;
    const v3 base_p = V3(-7, 0, -5);
    const v3 a1 = V3(-6, H, -3), a11 = V3(-4.25f, H, 2), a2 = V3(-4.1f, H, 2.45f), a33 = V3(-3.5f, H, 3), a3 = V3(-2, H, 4);
    F.arm1 = capsule(base_p + V3(-1, H, -2), a1);
    F.arm2 = capsule(a1, a11);
    F.arm3 = capsule(a33, a3);
    F.armb = bezier_frame(a11, a2, a33);
    F.a3 = a3;
    const v3 arm_fwd = normalize(a3 - a33);
    const v3 arm_up = V3(0, 1, 0);
    const v3 arm_right = cross(arm_fwd, arm_up);
    F.arm_xform = m3{arm_fwd, arm_up, arm_right};
    const float clr_r = R * 1.5f;
    F.collar = cyl_frame(V3(0, 0, 0), V3(0, 0, 0) + arm_fwd * .05f);
    F.fl_rot = mul(F.arm_xform, rotate_around_x(45.f));
    F.fl_sub1 = arm_right * clr_r;
    F.fl_sub2 = arm_up * clr_r;
    F.fl_rot2 = rotate_around_x(-45.f);
    F.ctg_rot = rotate_around_z(44.f);
    F.cut_rx10 = rotate_around_x(10.f);
    F.cut_rym5 = rotate_around_y(-5.f);
    F.cut2_rz10 = rotate_around_z(10.f);
    (void)R;
    return F;
}

FramePlanet build_planet(const sbx_uniforms& U, bool atm_sky, int build) {
    FramePlanet F;
    F.atm_sky = atm_sky ? 1 : 0;
    F.atm_sun = build_atmosphere(U).sun_dir;
    if (build == PLANET_CLOSEUP) F.cam = make_camera(U.u_res[0], U.u_res[1], tan_(radians_(30.f)), V3(.0f, 0, -1.93f), V3(-.1f, .9f, 2));   // setup_camera's `#if` branch :52-53
    else F.cam = make_camera(U.u_res[0], U.u_res[1], tan_(radians_(30.f)), V3(0, 0, -2.5f), V3(0, 0, 2));   // app_planet.h:47-58,368
    const m3 rot_y = rotate_around_y(27.f);                            // :307
    F.rot = mul(rotate_around_x(U.u_time * -12.f), rot_y);             // :308
    F.rot_cloud = mul(rotate_around_x(U.u_time * 8.f), rot_y);         // :309
    F.rot_t = transpose(F.rot);                                        // :356
    F.L = mul(F.rot, normalize(V3(1, 1, 0)));                          // :289
    return F;
}

// ---- SBX_APP_PLANET_WORLD (include/sbx.h sbx_aux_planet_world; the tiers and their domains: kern_planet_world.hip) ----------------
// the header's numbers (app_planet.h:20,55-56,68,76,107-114,127,148,165,180,224,258-268,288,307-309,369) with the two spins of u_time
static void planet_default_world(const sbx_uniforms& U, sbx_aux_planet_world& W) {
    auto put = [](float* d, v3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    std::memset(&W, 0, sizeof(W));
    put(W.eye, V3(0, 0, -2.5f)); W.fov = tan_(radians_(30.f));
    put(W.look_at, V3(0, 0, 2)); W.tilt_deg = 27.f;
    put(W.sun_dir, normalize(V3(1, 1, 0))); W.spin_deg = U.u_time * -12.f;
    put(W.key_color, V3(7, 5, 3)); W.cloud_spin_deg = U.u_time * 8.f;
    put(W.terrain_offset, V3(1.9489f, 2.435f, .5483f)); W.max_height = .4f;
    put(W.cloud_offset, V3(.35f, 13.35f, 2.67f)); W.cld_coverage = .29475675f;
    put(W.band, V3(.2f, .35f, .65f)); W.cld_fuzzy = .0335f;
    put(W.c_water, V3(.015f, .110f, .455f)); W.l_water = .05f;
    put(W.c_grass, V3(.086f, .132f, .018f)); W.l_shore = .17f;
    put(W.c_beach, V3(.153f, .172f, .121f)); W.l_grass = .211f;
    put(W.c_rock, V3(.080f, .050f, .030f)); W.l_rock = .351f;
    put(W.c_snow, V3(.600f, .600f, .600f)); W.absorb = 30.034f;
    W.cloud_light = .055f;
    W.terr_steps = 120; W.cloud_steps = 75; W.shadow_steps = 5;
}
const char* planet_world_check(const sbx_aux_planet_world& W) {
    static_assert(sizeof(sbx_aux_planet_world) == 224, "sbx_aux_planet_world is 224 bytes (include/sbx.h)");
    if (W.terr_steps < 1 || W.terr_steps > 512) return "planet world: terr_steps must lie in 1..512";
    if (W.cloud_steps < 1 || W.cloud_steps > 256) return "planet world: cloud_steps must lie in 1..256";
    if (W.shadow_steps < 1 || W.shadow_steps > 32) return "planet world: shadow_steps must lie in 1..32";
    if ((W.reserved[0] | W.reserved[1] | W.reserved[2] | W.reserved[3]) != 0u) return "planet world: the reserved words must be 0";
    return nullptr;
}
// FramePlanet from the block: what build_planet makes of the header's literals, made of the caller's (the literal tier's frame)
FramePlanet build_planet_world_literal(const sbx_uniforms& U, const sbx_aux_planet_world& W) {
    FramePlanet F;
    F.atm_sky = 0;
    F.atm_sun = V3(0, 0, 0);                                           // (read with atm_sky only)
    F.cam = make_camera(U.u_res[0], U.u_res[1], W.fov, V3(W.eye[0], W.eye[1], W.eye[2]), V3(W.look_at[0], W.look_at[1], W.look_at[2]));
    const m3 rot_y = rotate_around_y(W.tilt_deg);                      // :307
    F.rot = mul(rotate_around_x(W.spin_deg), rot_y);                   // :308
    F.rot_cloud = mul(rotate_around_x(W.cloud_spin_deg), rot_y);       // :309
    F.rot_t = transpose(F.rot);                                        // :356
    F.L = mul(F.rot, V3(W.sun_dir[0], W.sun_dir[1], W.sun_dir[2]));    // :288, the sun as given
    return F;
}
static bool pw_in(float v, float lo, float hi) { return v >= lo && v <= hi; }                    // (a NaN is in no interval)
static bool pw_zero_or_mag(float v, float lo, float hi) { return v == 0.f || pw_in(std::fabs(v), lo, hi); }
// columns of length 1 and at right angles to 1e-5 (a NaN or inf entry fails)
static bool pw_orthonormal(const m3& m) {
    const v3 c[3] = {m.c0, m.c1, m.c2};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double d = (double)c[i].x * c[j].x + (double)c[i].y * c[j].y + (double)c[i].z * c[j].z;
            if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-5)) return false;
        }
    return true;
}
// the angles and matrices of a frame: what tame_time (sbx_capi.hip) proves of u_time for SBX_APP_PLANET — the spec's sin / cos reduce
// their argument accurately below 2^30 rad; 1e9 degrees are 1.75e7 rad — and, checked rather than argued, the products orthonormal
static bool pw_rotations_tame(const sbx_aux_planet_world& W, const FramePlanet& F) {
    return pw_in(std::fabs(W.tilt_deg), 0.f, 1e9f) && pw_in(std::fabs(W.spin_deg), 0.f, 1e9f) && pw_in(std::fabs(W.cloud_spin_deg), 0.f, 1e9f) &&
           pw_orthonormal(F.rot) && pw_orthonormal(F.rot_cloud);
}
// The literal tier's SKIP kernel (k_planet<true, false, PLANET_CLOSEUP>, or the shipped instantiation for the shipped camera): its
// short forms want every march position finite and small (sbx_planet.h PL_MED3, PL_EXP4K; kern_planet_eval.hip's 256 / 4 / 18.6
// chain).  eye and look_at within 256 per coordinate, |fov| <= 16 and a camera whose fwd, up, right came out finite with |fwd| = 1 to
// 1e-5 (eye == look_at gives NaN and fails): rd = normalize(fwd + up y + right x) is then a unit vector for every finite point_cam,
// fwd being at right angles to both; hit_o = eye + rd t0 lies on the atmosphere sphere of radius 1.4 up to the cancellation in
// d2 = |rc|^2 - tca^2 (|rc|^2 <= 2e5, half an ulp .008: thc off by at most sqrt(.02), hit_o within .2 of the sphere or of the closest
// approach) — within 4 per coordinate, rd within 1, which is the chain's premise: |p| <= 18.6 at every sample.
bool planet_world_camera_tame(const sbx_aux_planet_world& W, const FramePlanet& F) {
    for (int k = 0; k < 3; ++k) if (!pw_in(std::fabs(W.eye[k]), 0.f, 256.f) || !pw_in(std::fabs(W.look_at[k]), 0.f, 256.f)) return false;
    if (!pw_in(std::fabs(W.fov), 0.f, 16.f)) return false;
    const v3 v[3] = {F.cam.fwd, F.cam.up, F.cam.right};
    for (int k = 0; k < 3; ++k) if (!std::isfinite(v[k].x) || !std::isfinite(v[k].y) || !std::isfinite(v[k].z)) return false;
    const double ff = (double)v[0].x * v[0].x + (double)v[0].y * v[0].y + (double)v[0].z * v[0].z;
    return std::fabs(ff - 1.0) <= 1e-5 && pw_rotations_tame(W, F);
}
FramePlanetWorld build_planet_world(const sbx_uniforms& U, const sbx_aux_planet_world& W) {
    auto get = [](const float* s) { return V3(s[0], s[1], s[2]); };
    const FramePlanet P = build_planet_world_literal(U, W);
    FramePlanetWorld F;
    F.cam = P.cam;
    PlanetWorldTerrain& T = F.terr;
    PlanetWorldCloud& C = F.cloud;
    PlanetWorldShade& S = F.shade;
    T.rot = P.rot; C.rot_cloud = P.rot_cloud; S.rot_t = P.rot_t; S.L = P.L;
    S.key_color = get(W.key_color);
    T.terrain_offset = get(W.terrain_offset); C.cloud_offset = get(W.cloud_offset);
    S.c_water = get(W.c_water); S.c_grass = get(W.c_grass); S.c_beach = get(W.c_beach); S.c_rock = get(W.c_rock); S.c_snow = get(W.c_snow);
    S.c_water_half = S.c_water / 2.f;                                  // :284
    S.l_water = W.l_water; S.l_shore = W.l_shore; S.l_grass = W.l_grass; S.l_rock = W.l_rock;
    T.max_height = C.max_height = W.max_height; T.max_height_r = C.max_height_r = 1.0f / W.max_height;
    T.max_ray_dist = W.max_height * 4.f;                               // :21
    F.atm_radius = 1.f + W.max_height;                                 // :311-312
    C.band0 = W.band[0]; C.band1 = W.band[1]; C.band2 = W.band[2];
    C.band_d01 = C.band1 - C.band0; C.band_r01 = 1.0f / C.band_d01;
    C.band_d12 = C.band2 - C.band1; C.band_r12 = 1.0f / C.band_d12;
    C.cov = W.cld_coverage; C.cov_hi = W.cld_coverage + W.cld_fuzzy;   // :112
    C.cov_d = C.cov_hi - C.cov; C.cov_r = 1.0f / C.cov_d;
    C.neg_absorb = -W.absorb;                                          // :87
    C.cloud_light = W.cloud_light; C.cloud_light_r = 1.0f / W.cloud_light;
    C.t_step_cloud = T.max_ray_dist / float(W.cloud_steps);            // :128
    C.t_step_shadow = W.max_height / float(W.shadow_steps);            // :149
    T.terr_steps = W.terr_steps; C.cloud_steps = W.cloud_steps; C.shadow_steps = W.shadow_steps;
    // the shell of band(): 1 + band0 mh < |p| < 1 + band2 mh, squared and moved out by 1e-3 (the argument: kern_planet_world.hip);
    // no claim for unordered or non-finite edges, for mh <= 0 or for an edge radius below .05
    C.shell_lo2 = 0.f; C.shell_hi2 = INFINITY;
    if (W.band[0] < W.band[1] && W.band[1] < W.band[2] && std::isfinite(W.band[0]) && std::isfinite(W.band[2]) && W.max_height > 0.f &&
        std::isfinite(W.max_height)) {
        const double lo = 1.0 + (double)W.band[0] * (double)W.max_height, hi = 1.0 + (double)W.band[2] * (double)W.max_height;
        if (lo >= .05) C.shell_lo2 = std::nextafter((float)(lo * lo * (1.0 - 1e-3)), 0.f);
        if (hi >= .05 && hi * hi * (1.0 + 1e-3) < 1e30) C.shell_hi2 = std::nextafter((float)(hi * hi * (1.0 + 1e-3)), INFINITY);
    }
    const double rmax = (double)F.atm_radius + 1.0;
    F.hit2_max = (float)(rmax * rmax);
    F.tame = planet_world_tame(W) ? 1 : 0;
    return F;
}
// the domain of k_planet_world<true>'s guarded forms, bound by bound as kern_planet_world.hip states and uses them
bool planet_world_tame(const sbx_aux_planet_world& W) {
    const float e20 = 0x1p-20f;
    if (!pw_in(W.max_height, .02f, 2.f)) return false;
    for (int k = 0; k < 3; ++k) {
        if (!pw_in(std::fabs(W.terrain_offset[k]), 0.f, 64.f) || !pw_in(std::fabs(W.cloud_offset[k]), 0.f, 64.f)) return false;
        if (!pw_zero_or_mag(W.band[k], e20, 4.f)) return false;
    }
    if (!pw_in(W.band[1] - W.band[0], e20, 8.f) || !pw_in(W.band[2] - W.band[1], e20, 8.f)) return false;
    if (!pw_zero_or_mag(W.cld_coverage, e20, 4.f)) return false;
    const float hi = W.cld_coverage + W.cld_fuzzy;
    if (!pw_in(hi - W.cld_coverage, 0x1p-30f, 8.f)) return false;
    const float mrd = W.max_height * 4.f;
    const float ts = std::fmax(mrd / float(W.cloud_steps), W.max_height / float(W.shadow_steps));
    if (!pw_in(std::fabs(W.absorb) * ts, 0.f, 80.f)) return false;
    if (!pw_in(std::fabs(W.cloud_light), e20, 0x1p20f)) return false;
    sbx_uniforms u{};
    u.u_res[0] = 64.f; u.u_res[1] = 36.f;                              // (the rotations do not read them)
    return pw_rotations_tame(W, build_planet_world_literal(u, W));
}
// sbx_set_variant 1: k_planet_world<false> for EVERY block, a literal-tier one included.  Otherwise PLANET_WORLD_LITERAL where every
// field but the camera, the three angles and the sun is the default's bit for bit — SBX_APP_PLANET's own kernels over
// build_planet_world_literal's block (sbx_capi.hip picks the instantiation) — and else the run-time kernel, fast for a tame block.
int planet_world_tier(const sbx_aux_planet_world& W, int variant) {
    if (variant == 1) return PLANET_WORLD_PLAIN;
    sbx_aux_planet_world D;
    planet_default_world(sbx_uniforms{}, D);
    const size_t mid = offsetof(sbx_aux_planet_world, cloud_spin_deg);
    const bool numbers = std::memcmp(W.key_color, D.key_color, sizeof(W.key_color)) == 0 &&
                         std::memcmp((const char*)&W + mid + sizeof(float), (const char*)&D + mid + sizeof(float), sizeof(W) - mid - sizeof(float)) == 0;
    if (numbers) return PLANET_WORLD_LITERAL;
    return planet_world_tame(W) ? PLANET_WORLD_RUNTIME : PLANET_WORLD_PLAIN;
}

FrameCloudsBest build_clouds_best(const sbx_uniforms& U) {
    FrameCloudsBest F;
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, V3(0, 1.f, 0), V3(0, 1.6f, -1));   // app_clouds_best.h:635-641,663
    F.sun_dir = normalize(V3(0, 0, -1));                               // :415
    F.wind_z = -U.u_time * .2f;                                        // :414
    const float cld_thick = 90.f;                                      // :412
    F.march_step = cld_thick / float(CB_STEPS);                        // :603
    F.cov = .3125f;                                                    // :411
    F.cov_rd = recip64((F.cov + .035f) - F.cov);                       // smoothstep(cov, cov + .035, dens) :583
    // y of the march: projection.y = dir.y / dir.y = 1, so origin.y = eye.y + 1 * 100 and iter.y = 1 * march_step
    const float origin_y = F.cam.eye.y + 1.0f * 100.f;                 // :611
    const float iter_y = 1.0f * F.march_step;                          // :606
    float pos_y = origin_y;
    for (int i = 0; i < CB_STEPS; ++i) {
        const float height = (pos_y - origin_y) / cld_thick;           // :619-620
        F.row[i].illum = exp_(height) / 1.95f;                         // illuminate_volume :591-597
        float q = (pos_y * .001f + 0.f) * 2.032f;                      // density_func :581-582 (wind.y = 0)
        for (int k = 0; k < 5; ++k) { F.row[i].qy[k] = q; q = q * 2.6434f; }   // fbm: p *= lacunarity
        pos_y = pos_y + iter_y;                                        // :628
    }
    return F;
}

FrameCloudsUe4 build_clouds_ue4(const sbx_uniforms& U, const sbx_aux_clouds_ue4& A) {
    FrameCloudsUe4 F;
    const v3 eye = V3(0, -.5f, 0);                                      // host mapping: src/app_clouds.h:23-30
    const v3 look_at = mul(rotate_around_y(U.u_mouse[0] * .5f), V3(0, 0, -1));
    F.cam = make_camera(U.u_res[0], U.u_res[1], 1.f, eye, look_at);
    if (A.use_dirs) {
        F.sun_dir = V3(A.sun_dir[0], A.sun_dir[1], A.sun_dir[2]);
        F.wind_dir = V3(A.wind_dir[0], A.wind_dir[1], A.wind_dir[2]);
    } else {
        F.sun_dir = normalize(V3(0, abs_(sin_(U.u_time * .3f)), -1));    // SUN_DIR app_clouds.usf:14
        F.wind_dir = V3(0, 0, -U.u_time * .2f);                          // WIND_DIR :13
    }
    F.march_step = A.thickness / float(UE4_STEPS);                      // :199
    F.absorbtion = A.absorbtion;
    F.cov = 1.f - A.coverage;                                           // :256
    F.cov_rd = recip64((F.cov + A.fuzziness) - F.cov);                  // :175
    F.cov_d = (F.cov + A.fuzziness) - F.cov;
    F.cov_r = 1.0f / F.cov_d;
    for (int i = 0; i < UE4_STEPS; ++i) F.eh[i] = exp_(float(i) / float(UE4_STEPS)) / 1.75f;   // :213,221
    return F;
}

// APP_2D / APP_2D_TEX (src/app_2d.h:70-111): what mainImage decides from the uniforms alone
Frame2d build_2d(const sbx_uniforms& U) {
    Frame2d F{};
    F.rres_x = recip64(U.u_res[0]); F.rres_y = recip64(U.u_res[1]);
    F.rpi = recip64(3.14159265359f);                                   // PI, src/def.h:51
    const float t = mod_(U.u_time, 16.f);                              // :80
    F.w = 0.f; F.time = 1.f;
    if (t < 4.f) { F.phase = 0; F.time = U.u_time; }                   // :82
    else if (t > 4.f && t < 8.f) { F.phase = 1; F.w = (t - 4.f) / 4.f; }     // :88
    else if (t > 8.f && t < 12.f) { F.phase = 2; F.time = U.u_time; }        // :94
    else if (t > 12.f) { F.phase = 3; F.w = (t - 12.f) / 4.f; }              // :99
    else F.phase = 4;                                                  // t = 4, 8, 12 or NaN: no branch runs
    F.omw = 1.f - F.w;
    return F;
}

}  // namespace sbx

extern "C" {

void sbx_checkerboard_texture(int size, int freq, uint32_t* out) {    // hlsltoy.cpp:66-87 (square: its buffer[y*h + x])
    if (!out || size <= 0) return;
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x)
            out[(size_t)y * size + x] = ((x & freq) == (y & freq)) ? 0xff000000u : 0xffffffffu;
}

void sbx_raytracer_scene_cornell(const sbx_uniforms* uni, int at_rest, sbx_aux_raytracer_scene* out) {
    if (!uni || !out) return;
    cornell_block(*uni, at_rest != 0, *out);
}

void sbx_atmosphere_air_default(const sbx_uniforms* uni, int view, sbx_aux_atmosphere_air* out) {
    if (!uni || !out) return;
    atmosphere_default_air(*uni, view, *out);
}

void sbx_planet_world_default(const sbx_uniforms* uni, sbx_aux_planet_world* out) {
    if (!uni || !out) return;
    planet_default_world(*uni, *out);
}

void sbx_vinyl_deck_default(const sbx_uniforms* uni, sbx_aux_vinyl_deck* out) {
    if (!uni || !out) return;
    vinyl_default_deck(*uni, *out);
}

void sbx_egg_pose_default(const sbx_uniforms* uni, sbx_aux_egg_pose* out) {
    if (!uni || !out) return;
    egg_default_pose(*uni, *out);
}

void sbx_sdf_scene_ramp(const sbx_uniforms* uni, sbx_aux_sdf_scene* out) {
    if (!uni || !out) return;
    sdf_ramp_block(*uni, *out);
}

void sbx_aux_clouds_ue4_defaults(sbx_aux_clouds_ue4* a) {              // app_clouds.usf:4-7
    if (!a) return;
    std::memset(a, 0, sizeof(*a));
    a->coverage = .50f; a->thickness = 15.f; a->absorbtion = 1.030725f; a->fuzziness = 0.035f;
    a->sun_dir[2] = -1.f; a->use_dirs = 0;
}

void sbx_aux_clouds_defaults(sbx_aux_clouds* a) {                      // uniform_buffer.h:39-55
    if (!a) return;
    std::memset(a, 0, sizeof(*a));
    a->wind_dir[2] = .2f;
    a->sun_dir[2] = -1.f;
    a->sun_color[0] = 1.f; a->sun_color[1] = .7f; a->sun_color[2] = .55f;
    a->sun_power = 8.f;
    a->cld_march_steps = 100;
    a->illum_march_steps = 6;
    a->sigma_scattering = .15f;
    a->cld_coverage = .535f;
    a->cld_thick = 125.f;
    a->atm_radius = 5000.f;
    a->atm_ground_y = 4750.f;
}
void sbx_aux_sdf_ao_defaults(sbx_aux_sdf_ao* a) {                      // uniform_buffer.h:56-60
    if (!a) return;
    std::memset(a, 0, sizeof(*a));
    a->fog_density = .1f;
    a->fog_falloff = .5f;
}

}  // extern "C"
