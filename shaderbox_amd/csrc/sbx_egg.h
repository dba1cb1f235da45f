// shaderbox_amd/csrc/sbx_egg.h — APP_EGG's device functions (src/app_egg.h as kern_egg.hip's header describes it): the cull sphere, sdf()
// with its per-member culls, the shadow march and the trace's 80 steps, over a FrameEgg and a witness of the square roots (sbx_sdf.h).
// Shared by k_egg (kern_egg.hip: SBX_APP_EGG, its two builds and SBX_APP_EGG_POSE) and k_egg_eval (kern_egg_eval.hip: sbx_egg_eval).
//
// Every cull bound below is derived from the FRAME (FrameEgg.oc / orad / ocw, foot_ml / foot_mr, BezierFrame.bc / br, built from the pose in
// sbx_frames.hip build_egg_pose), none from the shipped pose: the bounds hold for any pose whose frame constants are finite and for sample
// points of the scene's scale (sbx_frames.hip egg_pose_tame; anything else is given CULL = false and the IEEE roots).
#pragma once
#include "sbx_device.h"
#include "sbx_sdf.h"

namespace sbx {

// Is everything but the ground plane farther away than the ground?  Every other member of the union is
// >= .7 * (|p - oc| - orad) (FrameEgg, built in sbx_frames.hip), so with K = 1.43 (ground + 1e-3) + orad (1.43 > 1/.7),
// |p - oc| > K puts all of them strictly above the ground's distance: sdf() is the ground plane, exactly.
// The test runs on the WORLD point P against the centre carried to world space (FrameEgg.ocw): |P - ocw| is |p - oc| up to the 1e-6
// by which a rounded rotation matrix changes a length, far inside the 0.1 % by which 1.43 exceeds 1 / .7 — so a point that is far
// never pays for the turntable rotation (round 4: the culled call is ~28 instead of ~45 instructions; sky and ground waves are
// mostly such calls).  Any valid cull returns the same bits: it only ever claims what the full union would have returned.
// EGG_OVAL: its egg only gives >= (|q| - .74) / 1.55 (below), a slope under .7, so its constant is 1.56 > 1.55 (1 + 1e-3) — with the
// same 0.1 % for the rotation — and .7 > 1 / 1.56 keeps every other member's bound.
template <int BUILD>
__device__ __forceinline__ bool egg_far(const FrameEgg& F, v3 P, float ground_d) {
    const v3 q = P - F.ocw;
    const float K = (ground_d + 1e-3f) * (BUILD == EGG_OVAL ? 1.56f : 1.43f) + F.orad;
    return ground_d >= 0.f && dot(q, q) > K * K;
}

// CULL = false (sbx_set_variant 1) evaluates every member everywhere: the reference form, kept for the parity sweeps
// W: the square roots' witness (sbx_sdf.h): Wit<true> takes the five-instruction roots and records arguments outside their domain
template <bool CULL, int BUILD, class W>
__device__ __forceinline__ D2 egg_sdf(const FrameEgg& F, v3 P, W& w) {
    const float mat_egg = 1.f, mat_bike = 2.f, mat_ground = 3.f;              // :17-20
    {
        const D2 ground = {dot(V3(0.f, 1.f, 0.f), P) + (1.2f + 0.5f), mat_ground};       // sd_plane :136-138
        if (CULL && egg_far<BUILD>(F, P, ground.d)) return ground;
    }
    const v3 p = mul(F.rot_y, P) - V3(0, 0.5f, 3.5f);                         // :40-41
    // Members are evaluated cheapest first with a running minimum `dmin`; a member whose lower bound exceeds it
    // cannot be the union's result and enters as +inf (op_add2 is a strict `<`, so the winner and its material
    // are unchanged).  Lower bounds (all with >= 1e-3 of slack over the rounding of the evaluation itself):
    //   wheel  : distance to the unit circle - .03             >= |pw| - 1.03
    //   foot   : max(axis, |u + 1/16| - 1/16) - .05            >= |P - M| / sqrt2 - 1/16 - .05   (M = midpoint)
    //   egg    : two smooth-mins (k = .5) of three spheres     >= |p - (0, .65, 0)| - .7 - .25
    //   leg    : bezier_far (sbx_sdf.h)
    // EGG_OVAL's egg: w = iscale (scale q) with q = p - (0, .65, 0) is (q.x up to two roundings, q.y / 1.55, q.z): every component
    //   is at least the 1 / 1.55 (1 - 2^-22) of q's in magnitude, so the sphere gives |w| - .475 >= |q| / 1.5501 - .475, and
    //   |q| > 1.552 (dmin + .475 + 2e-3) puts it above dmin + 1e-3
    // EGG_STRAIGHT's legs: sd_cylinder0 is max(dist, -plane_1, -plane_2) - R.  With u = dot(dir, P) the axial coordinate and r = dist
    //   the radial one, the planes are -u - len and u, whose maximum is |u + len / 2| - len / 2: the field is
    //   max(r, |a| - h) - R for a = u + h the axial coordinate from the MIDPOINT M and h = len / 2, and max(r, |a| - h) >=
    //   max(r, |a|) - h >= |P - M| / sqrt2 - h (along a diagonal the maximum grows only at 1 / sqrt2 of the distance; the feet's
    //   bound).  So a leg is > dmin + 1e-3 where |p - M| > 1.4143 (dmin + h + R + 1e-3).  op_blend(a, b, k) = mix(b, a, h) - k h (1 - h)
    //   lies between min(a, b) - k / 4 and min(a, b), so the left pair (k = .01) is above dmin + 1e-3 where BOTH members are above
    //   dmin + .0025 + 1e-3: FrameEgg.leg_k = h + R + .0025 + 1e-3 for all four, and the left pair is skipped or evaluated as one
    //   (op_blend of a +inf is NaN, not the other member).  1e-3 more outside the product covers the rounding of M and of dot.
    const float inf = u2f(0x7f800000u);
    const D2 ground = {dot(V3(0.f, 1.f, 0.f), P) + (1.2f + 0.5f), mat_ground};           // sd_plane :136-138
    float dmin = ground.d;
    const bool pos_d = CULL && dmin >= 0.f;          // the bounds below assume a non-negative running minimum

    const v3 wheel_pos = V3(0, 1.2f, 0);
    const v3 pw = p + wheel_pos;
    D2 bike = {inf, mat_bike};
    {
        const float K = dmin * 1.001f + (1.03f + 2e-3f);
        if (!(pos_d && dot(pw, pw) > K * K))
            bike.d = w.length(V2(w.length(V2(pw.x, pw.y)) - 1.f, pw.z)) - .03f;              // sd_torus sdf.h:75-83
    }
    dmin = fmin_(dmin, bike.d);

    const float thick = .05f;
    D2 left_foot = {inf, mat_egg}, right_foot = {inf, mat_egg};
    {
        const float K = (dmin + (.0625f + .05f + 1e-3f)) * 1.4143f + 1e-3f;
        const v3 ql = p - F.foot_ml, qr = p - F.foot_mr;
        if (!(pos_d && dot(ql, ql) > K * K)) left_foot.d = sd_cylinder0<false>(F.foot_l, p + F.left_foot, thick, w);     // :120-123
        if (!(pos_d && dot(qr, qr) > K * K)) right_foot.d = sd_cylinder0<false>(F.foot_r, p + F.right_foot, thick, w);   // :125-128
    }
    const D2 feet = op_add2(left_foot, right_foot);
    dmin = fmin_(dmin, feet.d);

    const float egg_y = 0.65f;
    D2 egg = {inf, mat_egg};
    {
        const v3 qe = p - V3(0, egg_y, 0);
        const float K = BUILD == EGG_OVAL ? (dmin + (.475f + 2e-3f)) * 1.552f : dmin * 1.001f + (.95f + 3e-3f);
        if (BUILD == EGG_OVAL) {                                                         // :53-66
            if (!(pos_d && dot(qe, qe) > K * K)) {
                // mat3 * vec3 is (c0 v.x + c1 v.y) + c2 v.z, scale first, then iscale, zero terms included: 0 * inf is a NaN, and
                // (-0) + 0 is +0.  1. / s is the binary32 quotient (the reference's -fsingle-precision-constant).
                const float s = 1.55f;
                const m3 scale = M3(s, 0, 0, 0, 1, 0, 0, 0, 1);
                const m3 iscale = M3(1.f / s, 0, 0, 0, 1.f / s, 0, 0, 0, 1.f);
                egg.d = w.length(mul(iscale, mul(scale, qe))) - 0.475f;
            }
        } else if (!(pos_d && dot(qe, qe) > K * K)) {
            const float egg_m = w.length(p - V3(0, egg_y, 0)) - 0.475f;                  // :47-49
            const float egg_b = w.length(p - V3(0, egg_y - 0.45f, 0)) - 0.25f;
            const float egg_t = w.length(p - V3(0, egg_y + 0.45f, 0)) - 0.25f;
            const float egg_1 = op_blend(egg_m, egg_b, .5f);
            egg.d = op_blend(egg_1, egg_t, .5f);
        }
    }
    dmin = fmin_(dmin, egg.d);

    const D2 _1 = op_add2(feet, bike);
    const D2 _2 = op_add2(egg, _1);
    D2 legs;
    if constexpr (BUILD == EGG_STRAIGHT) {                                               // :86-93, :97-109
        const FrameEggStraight& L = static_cast<const FrameEggStraight&>(F);             // (what k_egg<., ., EGG_STRAIGHT> is given)
        auto far = [&](int i) {
            const v3 q = p - L.leg_m[i];
            const float K = (dmin + L.leg_k[i]) * 1.4143f + 1e-3f;
            return pos_d && dot(q, q) > K * K;
        };
        auto leg = [&](int i) { return sd_cylinder0<false>(L.leg[i], p + L.leg_o[i], thick, w); };
        // the right pair first: a plain union, each member on its own; then the left pair, as one
        D2 right_a = {inf, mat_egg}, right_b = {inf, mat_egg};
        if (!far(2)) right_a.d = leg(2);
        dmin = fmin_(dmin, right_a.d);
        if (!far(3)) right_b.d = leg(3);
        dmin = fmin_(dmin, right_b.d);
        D2 left = {inf, mat_egg};
        if (!(far(0) && far(1))) left.d = op_blend(leg(0), leg(1), .01f);
        legs = op_add2(left, op_add2(right_a, right_b));
    } else {
        const float leg_l = (CULL && bezier_far(F.leg_l, p, thick, dmin)) ? inf : sd_bezier_x(F.leg_l, p, thick, w);     // :102-118
        const float leg_r = (CULL && bezier_far(F.leg_r, p, thick, dmin)) ? inf : sd_bezier_x(F.leg_r, p, thick, w);
        legs = op_add2(D2{leg_l, mat_egg}, D2{leg_r, mat_egg});
    }
    const D2 _3 = op_add2(legs, _2);
    return op_add2(ground, _3);
}

template <bool CULL, int BUILD, class W>
__device__ __forceinline__ float egg_shadowmarch(const FrameEgg& F, v3 ro, v3 rd, W& w) {   // :161-186
    float t = 0.f, umbra = 1.f;
    for (int i = 0; i < 20; ++i) {
        const v3 p = ro + rd * t;
        const D2 d = egg_sdf<CULL, BUILD>(F, p, w);
        if (t > 10.f) break;
        if (d.d < 0.001f) return 0.1f;
        t += d.d;
        umbra = fmin_(umbra, 15.f * d.d / t);
    }
    return umbra;
}

// One ray of render_scene's trace loop (:190-231).  The trace only FINDS the hit; what the reference does inside the loop at the hit
// (`:205-228`: depth, the 20-step shadow march of ground pixels, the flat colours, `break`) runs after the loop, once per wave with all
// of its hit lanes, instead of once per distinct hit iteration of the wave with the few lanes that hit in that iteration.  Per lane the
// same operations on the same values in the same order.  1920x1080: 0.54 -> 0.27 ms.  (Trace and shadow march as ONE loop around one
// copy of the sdf — lanes with a ground hit start their shadow march while neighbours still trace — is slower: 0.283 vs 0.273 ms, 4K
// 0.68 vs 0.64; the per-lane phase logic costs more than the shorter waves save.)
// (`done` has no reader; without it hipcc allocates k_egg's registers differently, so it stays until a change that re-times k_egg.)
struct EggRay { float t; bool done, hit; int mat; v3 hp; int steps; };

// the trace's 80 steps, up to the hit or the far plane
template <bool CULL, int BUILD, class W>
__device__ __forceinline__ void egg_trace_steps(const FrameEgg& F, v3 ro, v3 rd, EggRay& r, W& w) {
    for (int i = 0; i < 80; ++i) {                          // render_scene :190-231
        const v3 p = ro + rd * r.t;
        const D2 d = egg_sdf<CULL, BUILD>(F, p, w);
        if (r.t > 15.f) { r.done = true; break; }
        if (d.d < 0.001f) { r.hit = true; r.mat = (int)d.m; r.hp = p; r.done = true; break; }
        r.t += d.d;
#ifdef SBX_EGG_STATS
        ++r.steps;
#endif
    }
}

}  // namespace sbx
