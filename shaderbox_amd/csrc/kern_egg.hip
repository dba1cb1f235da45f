// shaderbox_amd/csrc/kern_egg.hip — APP_EGG: sphere-traced SDF scene ("Vectorpark egg").
//
// Follows /root/reference/src/app_egg.h: sdf :38-144, shadowmarch :161-186, render_scene
// :190-231, render (bars overlay) :233-251, with the SDF library of src/sdf.h and the IK solver of
// src/IK.h.  Everything in sdf() that does not depend on the sample point (the turntable and
// pedal rotations, both feet, both IK knees, the Bezier frames of the legs, the toe cylinders'
// axes) is a frame constant evaluated once on the host (FrameEgg); only the point-dependent part
// runs per march step.  `depth` (a _mutable global, :188) is a per-thread register that starts
// at -max_dist for every pixel = GLSL per-invocation semantics.
//
// BUILD (sbx_frame.h EGG_*; include/sbx.h) is the header's build, the two one-line switches of its sdf():
//   EGG_DEFAULT    as shipped (SBX_APP_EGG)
//   EGG_STRAIGHT   without `#define BEZIER` (:37; SBX_APP_EGG_STRAIGHT): the legs are the four sd_cylinder segments of :86-93, :97-104,
//                  the left pair joined by op_blend(.., .01), the right pair by op_add (:106-109)
//   EGG_OVAL       the `#if 1` at :46 turned to `#if 0` (SBX_APP_EGG_OVAL): the egg is the one sphere of :53-66, evaluated at
//                  iscale * (scale * (p - (0, egg_y, 0))) with s = 1.55
// A template parameter: every `BUILD ==` below is decided at compile time, and k_egg<., ., EGG_DEFAULT> is the kernel it was.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "sbx_device.h"
#include "sbx_sdf.h"

#ifndef EGG_TW
#define EGG_TW 16          // wave tile EGG_TW x 64/EGG_TW pixels (profiles/r01_tile_shapes.txt)
#endif
#ifndef EGG_TX
#define EGG_TX 1           // waves per workgroup: 1 (4: the same single launch, 7 % slower with frames in flight at 1080p, 3 % at 4K;
#endif                     // census round 6: 4500 instead of 5900 waves resident — a workgroup's slots come back all at once)

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

// HOT-FIRST DISPATCH.  Workgroups start in increasing (blockIdx.y, blockIdx.x).  The census of a 1920x1080 launch
// (tools/egg_census.py, profiles/r04_egg_census.txt) shows the chip full for the first 95 us and then 125 us of tail with fewer than
// 500 of 7168 wave slots in use: the ~350 waves on the SILHOUETTE of the egg and its legs, whose grazing rays run all 80 trace steps
// next to the surface (no member of the union can be culled there), take 100-175 us each and start around t = 50 us because the
// rows are dealt bottom to top.  With `hot` = the tiles under the projected bounding sphere of everything but the ground
// (launch_egg), the first hot.w * hot.h workgroups take those tiles and the others take the rest of the frame in row order: the
// long waves start at t = 0 and the cheap ones fill in behind them.  Which tile a workgroup renders changes nothing about a pixel.
#ifndef EGG_HOT_FIRST
#define EGG_HOT_FIRST 1
#endif
#ifndef EGG_LDS_PAD
#define EGG_LDS_PAD 0      // bytes of dynamic LDS per (single-wave) workgroup, allocated only to CAP the waves per SIMD (see launch_egg)
#endif
struct HotRect { int x0, y0, w, h; };       // in workgroup tiles; w = 0: plain order
__device__ __forceinline__ void hot_first_tile(const HotRect& R, int gx, int& bx, int& by) {
    const int b = by * gx + bx, nr = R.w * R.h;
    if (b < nr) { by = R.y0 + b / R.w; bx = R.x0 + (b - (b / R.w) * R.w); return; }
    int c = b - nr;
    const int below = R.y0 * gx;
    if (c < below) { by = c / gx; bx = c - by * gx; return; }
    c -= below;
    const int side = gx - R.w, mid = R.h * side;
    if (c < mid) {
        const int q = c / side, k = c - q * side;
        by = R.y0 + q;
        bx = k < R.x0 ? k : k + R.w;
        return;
    }
    c -= mid;
    by = R.y0 + R.h + c / gx;
    bx = c - (c / gx) * gx;
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

#ifndef EGG_WITNESS
#define EGG_WITNESS 1      // five-instruction square roots with a recorded domain (sbx_sdf.h Wit): 0 = the IEEE roots only
#endif

// One pixel up to (colour, depth) — render_scene :190-231 — with the roots of witness `w`
template <bool CULL, int BUILD, class W>
__device__ __forceinline__ void egg_pixel(const FrameEgg& F, v2 pc, W& w, v3& color, float& depth, int& st_trace, int& st_shadow) {
    const v3 ro = F.cam.eye, rd = primary_dir(F.cam, pc, w);
    depth = -1e8f;                                          // :188, fresh per pixel
    color = V3(.1f, .1f, .7f);                              // background :9-12
    EggRay r;
    r.t = 0.f; r.done = false; r.hit = false; r.mat = 0; r.hp = V3(0, 0, 0); r.steps = 0;
    egg_trace_steps<CULL, BUILD>(F, ro, rd, r, w);
#ifdef SBX_EGG_STATS
    st_trace = r.steps;
    st_shadow = (r.hit && r.mat == 3) ? 1 : 0;
#endif
    if (r.hit) {
        if (r.mat == 1 || r.mat == 2) depth = fmax_(depth, r.hp.z);
        float s = 1.f;
        if (r.mat == 3) {
            const v3 sh_dir = V3(0, 1, 1);
            s = egg_shadowmarch<CULL, BUILD>(F, r.hp + sh_dir * 0.05f, sh_dir, w);
        }
        v3 base = V3(1, 1, 1);                              // illuminate :29-35
        if (r.mat == 3) base = V3(13.f / 255.f, 104.f / 255.f, 0.f / 255.f);
        else if (r.mat == 1) base = V3(0.9f, 0.95f, 0.95f);
        else if (r.mat == 2) base = V3(.2f, .2f, .2f);
        color = base * s;
    }
}

// bars overlay :233-251
__device__ __forceinline__ v3 egg_bars(v3 color, float pcx, float depth) {
    const float bar_factor = 1.0f - smoothstep_(0.0f, 0.01f, abs_((abs_(pcx) - 0.6f)) - 0.05f);
    const float depth_factor = 1.f - step_(1.f, depth);
    return abs3(mix3(color, V3(.6f, .6f, .6f), bar_factor * depth_factor));
}

// WIT: 0 = IEEE roots; 1 = witnessed roots (the shipped form); 2 = the same with the witness's lower edge at 1.0, so that waves
// near any primitive's axis DO record and re-run (sbx_set_variant 2: the test of the re-run path — same frame required)
template <int BUILD> struct EggFrame { using type = FrameEgg; };
template <> struct EggFrame<EGG_STRAIGHT> { using type = FrameEggStraight; };      // FrameEgg and the four cylinders (sbx_frame.h)
template <bool CULL, int WIT, int BUILD = EGG_DEFAULT>
__global__ void __launch_bounds__(64 * EGG_TX) k_egg(typename EggFrame<BUILD>::type F, RowMap M, float* __restrict__ out, HotRect hot) {
#ifdef SBX_EGG_STATS
    const unsigned long long st_t0 = __builtin_amdgcn_s_memrealtime();      // census build (tools/egg_census.py): 100 MHz counter
#endif
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
    int st_trace = 0, st_shadow = 0;
#ifndef EGG_VCONST
#define EGG_VCONST 1       // the constants every sdf() call starts with — the turntable rotation and the cull sphere — in VGPRs: a VALU
#endif                     // instruction with an SGPR source issues at half rate on gfx950 (profiles/r02_ubench_issue.txt)
    if (EGG_VCONST) {
        asm volatile("" : "+v"(F.rot_y.c0.x), "+v"(F.rot_y.c0.y), "+v"(F.rot_y.c0.z), "+v"(F.rot_y.c1.x), "+v"(F.rot_y.c1.y),
                          "+v"(F.rot_y.c1.z), "+v"(F.rot_y.c2.x), "+v"(F.rot_y.c2.y), "+v"(F.rot_y.c2.z));
        asm volatile("" : "+v"(F.ocw.x), "+v"(F.ocw.y), "+v"(F.ocw.z), "+v"(F.orad));
#if EGG_VCONST > 1
        asm volatile("" : "+v"(F.foot_ml.x), "+v"(F.foot_ml.y), "+v"(F.foot_ml.z), "+v"(F.foot_mr.x), "+v"(F.foot_mr.y), "+v"(F.foot_mr.z));
#endif
    }
    int bx = (int)blockIdx.x, by = (int)blockIdx.y;
    if (EGG_HOT_FIRST && hot.w > 0 && !M.order) hot_first_tile(hot, (int)gridDim.x, bx, by);          // wave-uniform (a dispatch-order table, once there is one, knows better)
    const Pixel px = pixel_of<EGG_TW, EGG_TX>(M, (int)threadIdx.x, bx, by, (int)gridDim.y);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    float depth;
    v3 color;
    if (WIT != 0) {
        Wit<true> w;
        if (WIT == 2) w.lo = 0x3F800000u;
        egg_pixel<CULL, BUILD>(F, pc, w, color, depth, st_trace, st_shadow);
        if (__builtin_amdgcn_ballot_w64(w.bad) != 0ull) {      // some lane took a root outside the proved interval: the IEEE forms
            Wit<false> w0;
            egg_pixel<CULL, BUILD>(F, pc, w0, color, depth, st_trace, st_shadow);
        }
    } else {
        Wit<false> w0;
        egg_pixel<CULL, BUILD>(F, pc, w0, color, depth, st_trace, st_shadow);
    }
    tile_cost_store_at(M, tl_t0, bx, by);                  // (bx, by: after the hot-first mapping)
    color = egg_bars(color, pc.x, depth);
#ifdef SBX_EGG_STATS
    {   // lane 0 of the wave: start / end time, the wave's longest trace, lanes that ran a shadow march, the wave's place
        int mx = st_trace;
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
        const int nsh = __popcll(__builtin_amdgcn_ballot_w64(st_shadow != 0));
        const unsigned long long st_t1 = __builtin_amdgcn_s_memrealtime();
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        float4 o4;
        o4.x = __uint_as_float((unsigned)(st_t0 & 0xffffffffu));
        o4.y = __uint_as_float((unsigned)(st_t1 - st_t0));
        o4.z = __uint_as_float((unsigned)mx | ((unsigned)nsh << 8) | ((xcc & 0xfu) << 16) | ((hwid & 0xffffu) << 20));
        o4.w = __uint_as_float((unsigned)st_trace | ((unsigned)st_shadow << 8));     // per LANE: trace steps, shadow march
        reinterpret_cast<float4*>(out)[px.idx] = o4;
        return;
    }
#endif
    store_rgba(M, out, px.idx, to_srgb(color));
}

// The projection of the sphere (F.oc, F.orad) around everything but the ground (sdf()'s p space: P = rot_y^T (p + (0, .5, 3.5))) in
// point_cam units: x = X / Z and y = Y / Z over the sphere.  false: the camera is inside or beside the sphere.
static bool egg_extents(const FrameEgg& F, float& pxa, float& pxb, float& pya, float& pyb) {
    const v3 c = mul(transpose(F.rot_y), F.oc + V3(0, 0.5f, 3.5f));
    const v3 v = c - F.cam.eye;
    const float depth = dot(v, F.cam.fwd), r = F.orad;
    if (!(depth > r * 1.05f)) return false;
    // the planes through the eye that contain the camera's up axis and touch the sphere — in the (right, fwd) plane the sphere is a
    // circle of radius r at (vx, depth), the tangents from the origin are at phi +- asin(r / d)
    const float vx = dot(v, F.cam.right), vy = dot(v, F.cam.up);
    auto extent = [&](float side, float& lo, float& hi) {
        const float d = sqrt_(side * side + depth * depth);
        const float phi = std::atan2(side, depth), al = std::asin(std::min(1.f, r / d));
        const float a = std::max(phi - al, -1.5f), b = std::min(phi + al, 1.5f);
        lo = std::tan(a); hi = std::tan(b);
    };
    extent(vx, pxa, pxb);
    extent(vy, pya, pyb);
    return pxa == pxa && pxb == pxb && pya == pya && pyb == pyb;
}

// The tiles under that projection, for a launch that covers whole rows of the frame from row M.y0 (a contiguous strip; other maps:
// plain order).  A hint about cost: off by any amount it only changes the order in which the same workgroups run.
static HotRect egg_hot_rect(const FrameEgg& F, const RowMap& M, dim3 grid) {
    HotRect none{0, 0, 0, 0};
    if (!EGG_HOT_FIRST || M.nranks != 1 || M.frag || M.span_mode || M.r0 != 0) return none;
    float pxa, pxb, pya, pyb;
    if (!egg_extents(F, pxa, pxb, pya, pyb)) return none;
    // point_cam = ((2 ndc - 1) * aspect * fov, (2 ndc - 1) * fov)  ->  pixel = ndc * res
    const float sx = F.cam.aspect_x * F.cam.fov, sy = F.cam.fov;
    auto pix = [](float pc, float scale, float res) { return (pc / scale + 1.f) * .5f * res; };
    const float xa = pix(pxa, sx, F.cam.res_x), xb = pix(pxb, sx, F.cam.res_x);
    const float ya = pix(pya, sy, F.cam.res_y) - (float)M.y0, yb = pix(pyb, sy, F.cam.res_y) - (float)M.y0;
    if (!(xa == xa && xb == xb && ya == ya && yb == yb)) return none;
    constexpr int TWP = EGG_TW * EGG_TX, THP = 64 / EGG_TW;
    const int gx = (int)grid.x, gy = (int)grid.y;
    const int x0 = std::max(0, std::min(gx, (int)std::floor(xa / TWP))), x1 = std::max(0, std::min(gx, (int)std::ceil(xb / TWP)));
    const int y0 = std::max(0, std::min(gy, (int)std::floor(ya / THP))), y1 = std::max(0, std::min(gy, (int)std::ceil(yb / THP)));
    if (x1 <= x0 || y1 <= y0) return none;
    return HotRect{x0, y0, x1 - x0, y1 - y0};
}
template <bool CULL, int WIT, int BUILD>
static void launch_egg_t(const FrameEggStraight& F, const RowMap& M, float* out, hipStream_t s, dim3 grid, HotRect hot, size_t pad) {
    const typename EggFrame<BUILD>::type& Fb = F;            // the build's part of the frame
    hipLaunchKernelGGL((k_egg<CULL, WIT, BUILD>), grid, dim3(64 * EGG_TX), pad, s, Fb, M, out, hot);
}
template <int BUILD>
static void launch_egg_b(const FrameEggStraight& F, const RowMap& M, float* out, hipStream_t s, int variant, dim3 grid, HotRect hot, size_t pad) {
    if (variant == 1) launch_egg_t<false, 0, BUILD>(F, M, out, s, grid, hot, pad);
    else if (variant == 2) launch_egg_t<true, 2, BUILD>(F, M, out, s, grid, hot, pad);
    else if (variant == 3) launch_egg_t<true, 0, BUILD>(F, M, out, s, grid, hot, pad);
    else launch_egg_t<true, EGG_WITNESS, BUILD>(F, M, out, s, grid, hot, pad);
}

dim3 egg_grid(const RowMap& M) { return grid_for<EGG_TW, EGG_TX>(M); }

void launch_egg(const FrameEggStraight& F, const RowMap& M, float* out, hipStream_t s, int variant, int build) {
    const dim3 grid = grid_for<EGG_TW, EGG_TX>(M);
    const HotRect hot = egg_hot_rect(F, M, grid);
    static const int pad = []() { const char* e = std::getenv("SBX_DEBUG_LDS_PAD"); return e ? std::atoi(e) : EGG_LDS_PAD; }();
    if (build == EGG_STRAIGHT) launch_egg_b<EGG_STRAIGHT>(F, M, out, s, variant, grid, hot, (size_t)pad);
    else if (build == EGG_OVAL) launch_egg_b<EGG_OVAL>(F, M, out, s, variant, grid, hot, (size_t)pad);
    else launch_egg_b<EGG_DEFAULT>(F, M, out, s, variant, grid, hot, (size_t)pad);
}

}  // namespace sbx
