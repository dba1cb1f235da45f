// shaderbox_amd/csrc/sbx_vinyl.h — APP_VINYL's device functions (src/app_vinyl.h as kern_vinyl.hip's header describes it): sdf_logo,
// sdf_platter, sdf_tonearm with its exact culls, sdf, and the statements of render's loop, sdf_shadow, sdf_normal and illuminate, over a
// FrameVinyl and a witness of the square roots (sbx_sdf.h).  Shared by k_vinyl (kern_vinyl.hip: SBX_APP_VINYL, its builds and
// SBX_APP_VINYL_DECK) and k_vinyl_eval (kern_vinyl_eval.hip: sbx_vinyl_eval).
//
// THE DOMAIN OF THE CULLS AND THE HARDWARE MIN / MAX UNDER A DECK (sbx_frames.hip vinyl_deck_tame decides per launch).  Both are
// argued below from "finite points": every lower bound is computed from the SAME point, in the same frame, as the member it bounds —
// the base's box from pos, the Bezier's and the headshell's from the wobbled p — so none of them needs platter_rot or wobble to be a
// rotation, only to be finite; what they need is that no comparison meets a NaN other than the Bezier link's own 0 / 0 and that no
// squared length overflows.  The shipped apps get that from a fixed camera and a unit sun.  A deck moves three things: the camera
// (primary points eye + rd t, t <= 40 plus one step), the sun (shadow points p + sun .05 + sun ts, ts <= 5 plus one step, a step being
// at most |point| + 10) and the two matrices.  With every value of the block within 1e4 in magnitude (the three angles: 1e10,
// inside which the spec's sin / cos return finite values) and every derived frame constant finite, a primary point stays within
// 3e4, a shadow point within 1e4 * (5 + 3e4 + 5e4 + 10) < 1e9, whose squares are far inside binary32, and no NaN enters.  A NaN or
// zero-length camera (eye == look_at), a NaN sun, an inf anywhere are outside; a zero sun, a sun below the disc, fov <= 0 are inside.
// The five colours, ro_spec, a_x, a_y and shininess are read by illuminate alone, after the march, by operations that are the
// reference's in every form: they do not enter the domain.  Outside it the launch takes CULL = false and the IEEE roots.
#pragma once
#include "sbx_device.h"
#include "sbx_ldsframe.h"
#include "sbx_sdf.h"
#include "sbx_noise.h"

#ifndef VI_LDS_FRAME
#define VI_LDS_FRAME 1
#endif

namespace sbx {

// FV(field): a member of the frame block where it is used (sbx_ldsframe.h: the block lives in LDS, the read is volatile).
#if VI_LDS_FRAME
#define FV(x) lds_ld(F.x)
#else
#define FV(x) (F.x)
#endif

// HW (the CULL kernel: tame frames, fixed camera, hence finite points): the unions' min / max as v_min_f32 / v_max_f32 (sbx_sdf.h
// hmin_ / hmax_).  They differ from the spec's compare-and-select only when the FIRST operand is a NaN — the one member that can be a
// NaN, the Bezier link (0 / 0 at isolated points), enters its min as the SECOND operand — or for zeros of opposite sign in the
// order (+0, -0) for min, (-0, +0) for max: primitive values are never -0 (a length, a difference of equal numbers, |p| - b), a -0
// arises only from `max(x, -y)` with y == +0, and the places where such a value meets a +0 are first operands of a min (equal
// either way) or dmin2, which is only compared with 0 and added to a margin.
#ifndef VIN_HW_MINMAX
#define VIN_HW_MINMAX 1
#endif
template <bool HW>
__device__ __forceinline__ float vinyl_logo(const FrameVinyl& F, v3 pos, float thick) {       // :68-85
    const v3 b = V3(.25f, thick, 1.2f), d = V3(.7f, 0, 0);
    v3 p = mul(pos, FV(ry30));
    const float v1 = sd_box<HW>(p - d, b);
    p = mul(pos, FV(rym30));
    const float v2 = sd_box<HW>(p + d, b);
    const float x = sd_box<HW>(pos, V3(1.5f, thick, 1.35f));
    return hmax_<HW>(hmin_<HW>(v1, v2), x);                              // op_intersect(op_add(v1, v2), x)
}
template <bool HW, class W>      // W: the square roots' witness (sbx_sdf.h Wit)
__device__ __forceinline__ D2 vinyl_platter(const FrameVinyl& F, v3 p, W& w) {                       // :87-125
    const float thick = .1f;
    const D2 lead_in = {sd_y_cylinder<HW>(p, 6.f, thick - .05f, w), 2.f};
    const D2 groove = {sd_y_cylinder<HW>(p, 5.9f, thick, w), 1.f};
    const D2 dead_wax = {sd_y_cylinder<HW>(p, 3.f, thick, w), 2.f};
    const D2 label = {sd_y_cylinder<HW>(p, 2.f, thick, w), 3.f};
    const D2 logo = {vinyl_logo<HW>(F, p, thick - .0175f), 4.f};
    const float spc = sd_y_cylinder<HW>(p, .10f, .6f, w);
    const float sps = w.length(p - V3(0, .3f, 0)) - .10f;
    const D2 spindle = {hmin_<HW>(spc, sps), 5.f};
    const D2 d0 = op_add2(groove, lead_in);
    const D2 d1 = op_add2(d0, dead_wax);
    const D2 d2 = op_add2(label, logo);
    const D2 d3 = op_add2(d1, d2);
    const D2 d4 = op_add2(d3, spindle);
    const float defect1 = w.length(p + V3(6.05f, 0, 0)) - .1f;
    const float defect2 = w.length(p + V3(-6.05f, 0, 0)) - .1f;
    const float defect = hmin_<HW>(defect1, defect2);
    return D2{hmax_neg_<HW>(d4.d, defect), d4.m};                       // op_sub
}
// Exact culling (as in kern_egg.hip): `dmin` is the distance the platter already gives at pos; a group of the tonearm
// whose lower bound exceeds the running minimum cannot be returned by the union and enters it as +inf.
//  * base: three y-cylinders around base_p (max(.., -platter) >= its first argument); a y-cylinder is
//    max(length(xz) - r, |y| - h/2) >= the max-norm distance to its own bounding box, all inside x,z in base_p +- 3,
//    |y| <= 1.25;
//  * the Bezier link: bezier_far (sbx_sdf.h);
//  * headshell + cartridge: collar, finger lift and cartridge boxes all lie within 1.3 of a3 in the wobbled frame
//    (offsets and half-sizes of :163-232 added up); a box evaluated in a rotated frame is a max-norm distance
//    >= Euclidean / sqrt3, the collar's max(axis, slabs) form >= Euclidean / sqrt2 minus its size, and max(x, -cut) >= x:
//    every member is >= .577 (|p - a3| - 1.3) - so with K = 1.74 (dmin + 1e-3) + 1.35, |p - a3| > K puts them all above dmin.
template <bool CULL, class W>   // CULL false (sbx_set_variant 1): no culling, the reference form
__device__ __forceinline__ D2 vinyl_tonearm(const FrameVinyl& F, v3 pos, float dmin, W& w) {        // :127-255
    constexpr bool HW = CULL && VIN_HW_MINMAX;
    const float inf = u2f(0x7f800000u);
    const v3 base_p = V3(-7, 0, -5);
    D2 base = {inf, 5.f};
    {
        const v3 q = pos - base_p;
        const float lb = hmax_<HW>(abs_(q.x) - 3.01f, hmax_<HW>(abs_(q.y) - 1.26f, abs_(q.z) - 3.01f));
        if (!(CULL && dmin >= 0.f && lb > dmin * 1.001f + 2e-3f)) {
            const float platter = sd_y_cylinder<HW>(pos, 6.25f, 1.f, w);
            const float base_0 = sd_y_cylinder<HW>(pos - base_p, 3.f, .25f, w);
            const float base_1 = hmax_neg_<HW>(base_0, platter);
            const float base_2 = sd_y_cylinder<HW>(pos - base_p, 1.25f, 1.f, w);
            const float base_12 = hmin_<HW>(base_1, base_2);
            const D2 base_a = {base_12, 5.f};
            const D2 base_b = {sd_y_cylinder<HW>(pos - base_p, 0.5f, 2.5f, w), 5.f};
            base = op_add2(base_a, base_b);
        }
    }

    const v3 p = mul(pos, FV(wobble));
    const float R = .1f;
    const float arm1 = sd_capsule_f(p, FV(arm1.a), FV(arm1.ab), FV(arm1.rd), R, w);
    const float arm2 = sd_capsule_f(p, FV(arm2.a), FV(arm2.ab), FV(arm2.rd), R, w);
    const float arm3 = sd_capsule_f(p, FV(arm3.a), FV(arm3.ab), FV(arm3.rd), R, w);
    const float arm_link1 = hmin_<HW>(arm1, arm2);
    const float arm_link2 = hmin_<HW>(arm_link1, arm3);
    const float dmin2 = hmin_<HW>(hmin_<HW>(dmin, base.d), arm_link2);
    const BezierFrame abz = FV(armb);
    const float armb = (CULL && bezier_far(abz, p, R, dmin2)) ? inf : sd_bezier_x(abz, p, R, w);
    const D2 arm = {hmin_<HW>(arm_link2, armb), 5.f};
    {
        const v3 q = p - FV(a3);
        const float K = (dmin2 + 1e-3f) * 1.74f + 1.35f;
        if (CULL && dmin2 >= 0.f && dot(q, q) > K * K) {
            const D2 tone1 = op_add2(base, arm);
            return op_add2(tone1, D2{inf, 5.f});
        }
    }

    const v3 clr_p = p - FV(a3);
    const float clr_r = R * 1.5f;
    const float collar = sd_cylinder0<HW>(FV(collar), clr_p, clr_r, w);
    const float fl_w = .045f, fl_h = .020f;
    const float fl_len1 = clr_r * 1.f;
    const float fl_len2 = fl_len1 * 1.2f;
    const v3 fl_p = mul(clr_p - FV(fl_sub1) - FV(fl_sub2), FV(fl_rot));
    const float fl1 = sd_box<HW>(fl_p, V3(fl_w, fl_h, fl_len1));
    const float fl2 = sd_box<HW>(mul(fl_p - V3(0, 0, fl_len1), FV(fl_rot2)) - V3(0, 0, fl_len2), V3(fl_w, fl_h, fl_len2));
    const float finger_lift = hmin_<HW>(fl1, fl2);
    const D2 headshell = {hmin_<HW>(collar, finger_lift), 5.f};

    const float ctg_w = .05f, ctg_h = .05f, ctg_len1 = .3f, ctg_len2 = .5f;
    const v3 ctg_p = mul(clr_p, FV(arm_xform));
    const float ctg1 = sd_box<HW>(ctg_p, V3(ctg_len1, ctg_h, ctg_w));
    const v3 ctg2_p = mul(ctg_p - V3(ctg_len1, 0, 0), FV(ctg_rot)) - V3(ctg_len2 - 0.03f, -.01f, 0);
    const float ctg2 = sd_box<HW>(ctg2_p, V3(ctg_len2, ctg_h, ctg_w));
    const float cut = sd_box<HW>(mul(mul(ctg2_p, FV(cut_rx10)) - V3(0, .05f, .175f), FV(cut_rym5)),
                             V3(ctg_len2 * 2.f, ctg_h * 3.f, ctg_w * 3.2f));
    const float cut2 = sd_box<HW>(mul(ctg2_p - V3(.3f, .2f, 0), FV(cut2_rz10)), V3(.4f, .2f, .3f));
    const float ctg12 = hmin_<HW>(ctg1, ctg2);
    const float ctg12c = hmax_neg_<HW>(ctg12, cut);
    const D2 cartridge = {hmax_neg_<HW>(ctg12c, cut2), 5.f};

    const D2 tone1 = op_add2(base, arm);
    const D2 tone2 = op_add2(headshell, cartridge);
    return op_add2(tone1, tone2);
}
template <bool CULL, class W>
__device__ __forceinline__ D2 vinyl_sdf(const FrameVinyl& F, v3 pos, W& w) {                   // :257-265
    const D2 plat = vinyl_platter<(CULL && VIN_HW_MINMAX)>(F, mul(pos, FV(platter_rot)), w);
    const D2 arm = vinyl_tonearm<CULL>(F, pos, plat.d, w);
    return op_add2(plat, arm);
}
__device__ __forceinline__ float saw(float x) { return x - floor_(x); }                        // :280-283
__device__ __forceinline__ float pulse(float x) { return saw(x + .5f) - saw(x); }              // :285-288

__device__ __forceinline__ v3 vinyl_base_color(int mat) {                                       // setup_scene :40-54
    switch (mat) {
    case 0: return V3(1, 1, 1);
    case 1: return V3(.01f, .01f, .01f);
    case 2: return V3(.05f, .05f, .05f);
    case 3: return V3(.5f, .5f, .0f);
    case 4: return V3(0, 0, .7f);
    case 5: return V3(.7f, .7f, .7f);
    default: return V3(0, 0, 0);                                 // unset material slots are zero (App. B5)
    }
}

// What illuminate reads beside the hit: the literals of the shipped builds (ShadeLit: compile-time constants, the code the shipped
// instantiations always had), or the caller's block (ShadeDeck over a VinylShade, sbx_frame.h: VINYL_DECK only).
struct ShadeLit {
    __device__ __forceinline__ v3 base(int mat) const { return vinyl_base_color(mat); }
    __device__ __forceinline__ float ro_spec() const { return .0725f; }
    __device__ __forceinline__ float a_x() const { return .025f; }
    __device__ __forceinline__ float a_y() const { return .5f; }
    __device__ __forceinline__ float shininess() const { return 50.f; }
};
struct ShadeDeck {
    const VinylShade& D;
    __device__ __forceinline__ v3 base(int mat) const {          // (a chain of selects over SGPR values: no indexed access)
        switch (mat) {
        case 0: return V3(1, 1, 1);                              // mat_debug stays the literal
        case 1: return D.color[0];
        case 2: return D.color[1];
        case 3: return D.color[2];
        case 4: return D.color[3];
        case 5: return D.color[4];
        default: return V3(0, 0, 0);
        }
    }
    __device__ __forceinline__ float ro_spec() const { return D.ro_spec; }
    __device__ __forceinline__ float a_x() const { return D.a_x; }
    __device__ __forceinline__ float a_y() const { return D.a_y; }
    __device__ __forceinline__ float shininess() const { return D.shininess; }
};

#ifndef VI_WITNESS
#define VI_WITNESS 1       // witnessed five-instruction square roots in sdf() (sbx_sdf.h Wit), as in k_egg: 0 = the IEEE roots only
#endif

// render's loop :427-455 up to the hit: the trace only FINDS it (t, and on a hit mat and p).  steps: 60 (C++ build) or 180 :411-416
template <bool CULL, class W>
__device__ __forceinline__ void vinyl_trace(const FrameVinyl& Fs, v3 ro, v3 rd, int steps, W& w, float& t, bool& hit, int& mat, v3& p) {
    for (int i = 0; i < steps; ++i) {
        const v3 pi = ro + rd * t;
        const D2 d = vinyl_sdf<CULL>(Fs, pi, w);
        if (t > 40.f) break;
        if (d.d < .005f) { hit = true; mat = (int)d.m; p = pi; break; }
        t += d.d;
    }
}
// sdf_shadow :379-404 over the ray (so, dir)
template <bool CULL, class W>
__device__ __forceinline__ float vinyl_shadow(const FrameVinyl& Fs, v3 so, v3 dir, W& w) {
    float sh = 1.f;
    float ts = 0.f;
    for (int k = 0; k < 20; ++k) {
        const D2 ds = vinyl_sdf<CULL>(Fs, so + dir * ts, w);
        if (ts > 5.f) break;
        if (ds.d < .005f) { sh = .05f; break; }
        ts += ds.d;
        sh = fmin_(sh, 16.f * ds.d / ts);
    }
    return sh;
}
// sdf_normal :267-278 (the IEEE normalize: flat surfaces give exact zero components, which the witness records)
template <bool CULL, class W>
__device__ __forceinline__ v3 vinyl_normal(const FrameVinyl& Fs, v3 p, W& w) {
    const float e = 0.001f;
    return normalize(V3(
        vinyl_sdf<CULL>(Fs, p + V3(e, 0, 0), w).d - vinyl_sdf<CULL>(Fs, p - V3(e, 0, 0), w).d,
        vinyl_sdf<CULL>(Fs, p + V3(0, e, 0), w).d - vinyl_sdf<CULL>(Fs, p - V3(0, e, 0), w).d,
        vinyl_sdf<CULL>(Fs, p + V3(0, 0, e), w).d - vinyl_sdf<CULL>(Fs, p - V3(0, 0, e), w).d));
}
// illuminate :293-377 for the hit (p, mat) seen from `eye`.  F: the kernel argument (sun, platter_rot: SGPRs); Fs: the block sdf()
// reads; S: ShadeLit or ShadeDeck.
// BUILD (sbx_frame.h VINYL_*): VINYL_RIDGES has the `#if 0` of the 6-tap branch on (the ridge of the label and the logo).
template <bool CULL, int BUILD, class SH, class W>
__device__ __forceinline__ v3 vinyl_illuminate(const FrameVinyl& F, const FrameVinyl& Fs, const SH& S, v3 eye, v3 p, int mat, W& w) {
    v3 L = F.sun_dir;
    v3 V = w.normalize(eye - p);
    const v3 base = S.base(mat);
    v3 lit;
    if (mat == 1 || mat == 2) {
        const v3 ho = mul(p, F.platter_rot);
        L = mul(L, F.platter_rot);
        V = mul(V, F.platter_rot);
        const float r = length(ho);
        const v3 B = ho / r;
        v3 N = V3(0, 1, 0);
        if (mat == 1) {
            const float rr = r + .07575f * noise_iq(ho * 2.456f);
            const float s = pulse(rr * 24.f);
            if (s > 0.f) {
                N = normalize(N + B);
                N = N - 2.f * dot(V3(0, 1, 0), N) * V3(0, 1, 0);      // reflect(N, (0,1,0))
            }
        }
        if (mat == 2) {
            const float s = saw(r * 4.f);
            N = normalize(N + B * ((s > .9f) ? 1.f : 0.f));
        }
        const v3 T = cross(B, N);
        const float ro_diff = 1.f, ro_spec = S.ro_spec(), a_x = S.a_x(), a_y = S.a_y();
        const v3 H = w.normalize(V + L);
        const float dotLN = dot(L, N);
        const v3 diffuse = base * (ro_diff / 3.14159265359f) * fmax_(0.f, dotLN);
        const float spec_a = ro_spec / sqrt_(dotLN * dot(V, N));
        const float spec_b = 1.f / (4.f * 3.14159265359f * a_x * a_y);
        const float ht = dot(H, T) / a_x;
        const float hb = dot(H, B) / a_y;
        const float spec_c = -2.f * (ht * ht + hb * hb) / (1.f + dot(H, N));
        const v3 specular = V3(1, 1, 1) * spec_a * spec_b * exp_(spec_c);
        lit = diffuse + specular;
    } else {
        v3 n = vinyl_normal<CULL>(Fs, p, w);
        if constexpr (BUILD == VINYL_RIDGES) {               // the `#if 0` block after sdf_normal, on: the unrotated hit.origin
            if (mat == 3 || mat == 4) {                      // mat_label, mat_logo
                const float r = length(p);
                const v3 B = p / r;
                const float s = saw(r * .9f);
                n = normalize(n + B * ((s > .975f) ? 1.f : 0.f));
            }
        }
        const v3 diffuse = base * fmax_(0.f, dot(L, n));
        const v3 H = w.normalize(V + L);
        const v3 specular = pow_(fmax_(0.f, dot(H, n)), S.shininess()) * V3(1, 1, 1);
        lit = diffuse + specular;
    }
    return lit;
}

// One pixel up to its colour — render :406-457 — with the sdf's roots of witness `w`.  F: the kernel argument (camera, sun, steps:
// SGPRs); Fs: the block sdf() reads (the LDS copy, or F itself).
// BUILD (sbx_frame.h VINYL_*): the header as shipped, or with one of two switches of its hit block the other way — VINYL_RIDGES, the
// `#if 0` of illuminate's 6-tap branch on (the ridge of the label and the logo); VINYL_NOSHADOW, the `#if 1` around render's
// sdf_shadow call off (sh stays 1.).  The close-up camera of setup_camera's `#else` is VINYL_DEFAULT over another frame block.
// The trace only FINDS the hit; the reference's hit block (`:436-452`: 20-step soft shadow, anisotropic or 6-tap-normal shading,
// `break`) runs after the loop, once per wave with all of its hit lanes instead of once per distinct hit iteration of the wave.
// Per lane the same operations on the same values in the same order.
// (The two loops stand here as statements, not as calls of vinyl_trace / vinyl_shadow above: the inlined calls are the same operations
// but not the same register allocation, and the shipped instantiations keep their listings.)
template <bool CULL, int BUILD, class SH, class W>
__device__ __forceinline__ void vinyl_pixel(const FrameVinyl& F, const FrameVinyl& Fs, const SH& S, v2 pc, W& w, v3& color) {
    const v3 ro = F.cam.eye, rd = primary_dir(F.cam, pc, w);
    color = V3(1, 1, 1);                                        // background :15-18
    float t = 0.f;
    bool hit = false;
    int mat = 0;
    v3 p = V3(0, 0, 0);
    for (int i = 0; i < F.steps; ++i) {                           // render :427-455; 60 (C++ build) or 180 steps :411-416
        const v3 pi = ro + rd * t;
        const D2 d = vinyl_sdf<CULL>(Fs, pi, w);
        if (t > 40.f) break;
        if (d.d < .005f) { hit = true; mat = (int)d.m; p = pi; break; }
        t += d.d;
    }
    {
        if (hit) {
            // sdf_shadow :379-404
            float sh = 1.f;
            if constexpr (BUILD != VINYL_NOSHADOW) {
                const v3 so = p + F.sun_dir * 0.05f;
                float ts = 0.f;
                for (int k = 0; k < 20; ++k) {
                                const D2 ds = vinyl_sdf<CULL>(Fs, so + F.sun_dir * ts, w);
                    if (ts > 5.f) break;
                    if (ds.d < .005f) { sh = .05f; break; }
                    ts += ds.d;
                    sh = fmin_(sh, 16.f * ds.d / ts);
                }
            }
            const v3 lit = vinyl_illuminate<CULL, BUILD>(F, Fs, S, ro, p, mat, w);
            if constexpr (BUILD != VINYL_NOSHADOW) color = lit * sh;
            else color = lit;                                        // lit * 1.f, bit for bit
        }
    }
}

}  // namespace sbx
