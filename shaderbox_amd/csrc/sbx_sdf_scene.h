// shaderbox_amd/csrc/sbx_sdf_scene.h — the device functions of SBX_APP_SDF_SCENE's renderer, shared by k_sdf_scene (kern_sdf_scene.hip: the
// frame, sbx_sdf_eval) and k_sdf_scene_eval_fn (kern_sdf_scene_eval.hip: sbx_sdf_scene_eval, the same functions over the caller's
// elements): the reader of the block (SdfRd), sdf(pos) as an interpreter over the postfix program (scene_sdf), and app_sdf_ao.h's renderer
// cut into its functions — scene_normal (sdf_normal :152-163), scene_ao (sdf_ao :165-181), scene_shadow (sdf_shadow :183-207),
// scene_illuminate (illuminate :211-243), scene_fog (render's height fog :287-311) — with scene_pixel, render_impl :245-285, its march
// and their composition.  kern_sdf_scene.hip's opening comment says how the block is read and what carries over to the caller's
// numbers; DESIGN.md 5.19 and 5.27 have what was measured.
#pragma once
#include "sbx_device.h"
#include "sbx_ldsframe.h"
#include "sbx_sdf.h"

#ifndef SDF_SCENE_OPERANDS_LDS
#define SDF_SCENE_OPERANDS_LDS 1
#endif

namespace sbx {

typedef const __attribute__((address_space(4))) FrameSdfScene* SdfKarg;   // the frame where it lies in the kernarg segment
#define SDS_PTR(T, r) ((const __attribute__((address_space(3))) T*)(&(r)))

// One instruction's fields.  K: the kernel argument (scalar loads); L: its LDS copy, filled by lds_frame_fill — whose closing
// __syncthreads() is what orders these plain loads behind the stores, so no read may stand before that call.
struct SdfRd {
    SdfKarg K;
    const FrameSdfScene* L;
    __device__ __forceinline__ float ld(const __attribute__((address_space(4))) float& k, const float& l) const {
        return SDF_SCENE_OPERANDS_LDS ? *SDS_PTR(float, l) : k;
    }
    __device__ __forceinline__ float s(int i) const { return ld(K->prog[i].s, L->prog[i].s); }
    __device__ __forceinline__ float c(int i) const { return ld(K->prog[i].c, L->prog[i].c); }
    __device__ __forceinline__ v3 off(int i) const {
        return V3(ld(K->prog[i].off.x, L->prog[i].off.x), ld(K->prog[i].off.y, L->prog[i].off.y), ld(K->prog[i].off.z, L->prog[i].off.z));
    }
    __device__ __forceinline__ float p(int i, int k) const { return ld(K->prog[i].p[k], L->prog[i].p[k]); }   // k: a literal at every use
    __device__ __forceinline__ v3 p3(int i, int k) const { return V3(p(i, k), p(i, k + 1), p(i, k + 2)); }
};

__device__ __forceinline__ v3 normalize_ieee(v3 v) {             // v / length(v): the IEEE root, three IEEE quotients
    const float l = sqrt_(dot(v, v));
    return V3(v.x / l, v.y / l, v.z / l);
}

// q = pos - offset, then mul(q, rotate_around_*(deg)) (util.h:44-69: v * M = dot(v, column), every zero term kept)
__device__ __forceinline__ v3 scene_q(const SdfRd& R, int i, int ax, v3 pos) {
    v3 q = pos - R.off(i);
    if (ax != 0) {
        const float s = R.s(i), c = R.c(i);
        if (ax == 1) q = mul(q, M3(1, 0, 0, 0, c, -s, 0, s, c));
        else if (ax == 2) q = mul(q, M3(c, 0, s, 0, 1, 0, -s, 0, c));
        else q = mul(q, M3(c, -s, 0, s, c, 0, 0, 0, 1));
    }
    return q;
}

// sdf(pos): the program, instruction by instruction (include/sbx.h SBX_APP_SDF_SCENE).  The host has checked the stack discipline:
// depth 0..4, empty after every OBJECT's pop, the last instruction an OBJECT, so s0..s3 are never read before they are written.
// acc starts as (NaN, 0): `acc.x < v.x ? acc : v` takes v against a NaN, which is the `first ? v : op_add(acc, v)` of the definition.
// One flat chain of scalar bit tests, every case whole — its operands, its arithmetic, its stack move — and straight to the next
// instruction: a case that joins the others before the push costs a flag and two more branches.
#define SDF_BIT(op) (1u << sdf_op_bit(op))
#define SDF_PUSH(d) { const float d_ = (d); s3 = s2; s2 = s1; s1 = s0; s0 = d_; continue; }
#define SDF_OPER(r) { const float r_ = (r); s0 = r_; s1 = s2; s2 = s3; continue; }
template <class W>
__device__ __forceinline__ D2 scene_sdf(const FrameSdfScene& F, const SdfRd& R, int n, v3 pos, W& w) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    D2 acc = {u2f(0x7fc00000u), 0.f};
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const unsigned ctl = (unsigned)R.K->prog[i].ctl;          // a scalar load at a uniform dynamic offset; one bit per op
        const int ax = (int)(ctl >> 16);
        if (ctl & SDF_BIT(SBX_SDF_BOX)) SDF_PUSH(sd_box<false>(scene_q(R, i, ax, pos), R.p3(i, 0)))                          // sdf.h:67-73
        if (ctl & (SDF_BIT(SBX_SDF_OBJECT) | SDF_BIT(SBX_SDF_ADD) | SDF_BIT(SBX_SDF_SUB) | SDF_BIT(SBX_SDF_INTERSECT) | SDF_BIT(SBX_SDF_BLEND))) {
            if (ctl & SDF_BIT(SBX_SDF_OBJECT)) {                  // vec2(d, float(material)) into the result, sdf.h:5-11; pop
                acc = op_add2(acc, D2{s0, R.p(i, 0)});
                s0 = s1; s1 = s2; s2 = s3;
                continue;
            }
            if (ctl & SDF_BIT(SBX_SDF_ADD)) SDF_OPER(fmin_(s1, s0))                                                 // :13-18 (d1, d2) = (s1, s0)
            if (ctl & SDF_BIT(SBX_SDF_SUB)) SDF_OPER(fmax_(s1, -s0))                                                // :20-28
            if (ctl & SDF_BIT(SBX_SDF_INTERSECT)) SDF_OPER(fmax_(s1, s0))                                           // :30-36
            SDF_OPER(op_blend(s1, s0, R.p(i, 0)))                                                                   // :38-47
        }
        const v3 q = scene_q(R, i, ax, pos);
        if (ctl & SDF_BIT(SBX_SDF_PLANE)) SDF_PUSH(dot(R.p3(i, 0), q) + R.p(i, 3))                                           // :49-57
        if (ctl & SDF_BIT(SBX_SDF_SPHERE)) SDF_PUSH(w.length(q) - R.p(i, 0))                                                 // :59-65
        if (ctl & SDF_BIT(SBX_SDF_Y_CYLINDER)) SDF_PUSH(sd_y_cylinder<false>(q, R.p(i, 0), R.p(i, 1), w))                    // :85-93
        if (ctl & SDF_BIT(SBX_SDF_TORUS)) SDF_PUSH(w.length(V2(w.length(V2(q.x, q.y)) - R.p(i, 0), q.z)) - R.p(i, 1))        // :75-83
        if (ctl & SDF_BIT(SBX_SDF_CYLINDER)) {                                                                               // :95-109, any P0
            const v3 dir = R.p3(i, 0);
            const float dist = w.length(cross(dir, q - R.p3(i, 5)));
            const float plane_1 = dot(dir, q) + R.p(i, 3);
            const float plane_2 = dot(-dir, q) + (-R.p(i, 4));
            SDF_PUSH(fmax_(fmax_(dist, -plane_1), -plane_2) - R.p(i, 8))
        }
        if (ctl & SDF_BIT(SBX_SDF_CAPSULE)) {                                                                                // :162-171
            const v3 a = R.p3(i, 0), ab = R.p3(i, 3);
            const float t = clamp_(dot(q - a, ab) / R.p(i, 6), 0.f, 1.f);
            SDF_PUSH(w.length((ab * t + a) - q) - R.p(i, 7))
        }
        BezierFrame B;                                                                                              // SBX_SDF_BEZIER :120-159, .x
        B.b = R.p3(i, 0); B.u = R.p3(i, 3); B.v = R.p3(i, 6); B.w = R.p3(i, 9);
        B.a2 = V2(R.p(i, 12), R.p(i, 13)); B.c2 = V2(R.p(i, 14), R.p(i, 15));
        B.bc = V3(0, 0, 0); B.br = 0.f;                           // (bezier_far's sphere: not used here)
        SDF_PUSH(sd_bezier_x(B, q, R.p(i, 16), w))
    }
    return acc;
}
#undef SDF_BIT
#undef SDF_PUSH
#undef SDF_OPER

// ---- the renderer, function by function.  F: the kernel argument (the control words: scalar loads); R: the program's reader; n: F.n_instr;
// w: the witness whose roots sdf() takes.  Directions and normals are used as given.  Each tap loop and march is ONE scene_sdf call
// site, so a pass of scene_pixel — its own march and these three — has four of them.

// sdf_normal :152-163: taps +x -x +y -y +z -z as one loop.  p + (dt, 0, 0) adds +0 to y and z as the reference does; p - (dt, 0, 0)
// is p + (-dt, -0, -0): x - dt == x + (-dt) and y - 0 == y + (-0) for every y (-0 and NaN included).  The normalize is the IEEE one
// under every witness: on a flat face two of the three differences are exactly 0.
template <class W>
__device__ __forceinline__ v3 scene_normal(const FrameSdfScene& F, const SdfRd& R, int n, v3 p, W& w) {
    const float e = 0.001f;
    float tp0 = 0.f, tp1 = 0.f, tp2 = 0.f, tm0 = 0.f, tm1 = 0.f, tm2 = 0.f;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int ax = k >> 1;
        const float sg = (k & 1) ? -1.f : 1.f;
        const v3 o = V3(ax == 0 ? e * sg : 0.f * sg, ax == 1 ? e * sg : 0.f * sg, ax == 2 ? e * sg : 0.f * sg);
        const float v = scene_sdf(F, R, n, p + o, w).d;
        if (k == 0) tp0 = v; else if (k == 1) tm0 = v; else if (k == 2) tp1 = v; else if (k == 3) tm1 = v; else if (k == 4) tp2 = v; else tm2 = v;
    }
    return normalize_ieee(V3(tp0 - tm0, tp1 - tm1, tp2 - tm2));
}

// sdf_ao :165-181 at hit (origin p, normal nrm) -> its c; 1 / pow(2, k) of the math spec is the exact power of two (kern_sdf_ao.hip)
template <class W>
__device__ __forceinline__ float scene_ao(const FrameSdfScene& F, const SdfRd& R, int n, v3 p, v3 nrm, W& w) {
    float occlusion = 0.f, inv2k = 1.f;
#pragma unroll 1
    for (int j = 1; j <= 5; ++j) {
        const float k = (float)j;
        const v3 q = p + .5f * k * nrm;
        const float dd = scene_sdf(F, R, n, q, w).d;
        inv2k *= .5f;
        occlusion += inv2k * (.5f * k - dd);
    }
    return 1.f - clamp_(occlusion, 0.f, 1.f);
}

// sdf_shadow :183-207 over the ray (o, dir), as kern_sdf_ao.hip ao_shadow
template <class W>
__device__ __forceinline__ float scene_shadow(const FrameSdfScene& F, const SdfRd& R, int n, v3 o, v3 dir, W& w) {
    float ts = 0.f, umbra = 1.f;
    bool dark = false;
#pragma unroll 1
    for (int i = 0; i < 20; ++i) {
        const v3 pi = o + dir * ts;
        const float d = scene_sdf(F, R, n, pi, w).d;
        if (ts > 20.f) break;
        if (d < .005f) { dark = true; break; }
        ts += d;
        umbra = fmin_(umbra, 32.f * d / ts);
    }
    return dark ? .05f : umbra;
}

// illuminate :220-242 at hit (origin p, normal nrm, material mat) under ao and sh (:217-219, the normals view, is the caller's).
// get_material :23-33 reads the LDS copy per lane.  ANY_ID false: ids are 0..7 by validation (what a march returns); true: mat is the
// caller's, and an id outside 0..7, where the reference's get_material leaves its result unset, gives the zero colour.
template <bool ANY_ID>
__device__ __forceinline__ v3 scene_illuminate(const FrameSdfScene& F, const SdfRd& R, v3 p, v3 nrm, int mat, float ao, float sh) {
    const v3 sun = F.sun_dir;
    v3 accum = V3(0, 0, 0);
    const float sun_ray = fmax_(0.f, dot(sun, nrm));
    accum = accum + sh * sun_ray * V3(1.2f, 1.3f, 1.f);
    accum = accum + ao * nrm.y * V3(.15f, .15f, .4f);
    const float ind = fmax_(0.f, dot(sun * V3(-1, 0, -1), nrm));
    accum = accum + ao * ind * V3(.4f, .28f, .2f);
    const v3& ms = R.L->mats[mat & 7];
    v3 mat_c = V3(*SDS_PTR(float, ms.x), *SDS_PTR(float, ms.y), *SDS_PTR(float, ms.z));
    if (ANY_ID && (unsigned)mat > 7u) mat_c = V3(0, 0, 0);
    if (mat == F.checker) {
        const float cb = mod_(floor_(p.x * .5f) + floor_(p.z * .5f), 2.0f);   // checkboard_pattern util.h:95-101
        mat_c = mix3(mat_c - .15f * mat_c, mat_c + .15f * mat_c, cb);
    }
    return accum * mat_c;
}

// One pixel up to (rgb, t) — render_impl :245-285 — with the roots of witness `w`: its march (:253-282) and the functions above.  Returns
// the hit's material, or -1 where :284 returned the background.  The march loop stands here and not in a function of its own: as one
// (the hit flag returned, or passed by reference) it compiled to other code in k_sdf_scene — one more scalar instruction per march step,
// or another register assignment throughout — where this text gives the parent's instructions.
template <class W>
__device__ __forceinline__ int scene_pixel(const FrameSdfScene& F, const SdfRd& R, v3 ro, v3 rd, W& w, v3& rgb, float& t) {
    const int n = F.n_instr;
    rgb = F.background;                                           // :9-12
    t = 0.f;
    bool hit = false;
    int mat = 0;
    v3 p = V3(0, 0, 0);
#pragma unroll 1
    for (int i = 0; i < F.steps; ++i) {                           // :253-282; the hit block runs after the loop, as in k_sdf_ao
        const v3 pi = ro + rd * t;
        const D2 d = scene_sdf(F, R, n, pi, w);
        if (t > F.end) break;
        if (d.d < .005f) { hit = true; mat = (int)d.m; p = pi; break; }
        t += d.d;
    }
    if (!hit) return -1;
    const v3 nrm = scene_normal(F, R, n, p, w);
    if (F.view != 0) { rgb = nrm; return mat; }                   // illuminate :217-219 compiled in (a NaN normal is the pixel's data)
    const float ao = scene_ao(F, R, n, p, nrm, w);
    float sh = 1.f;
    if (F.shadow != 0) {                                          // :269-274 compiled in
        const v3 sun = F.sun_dir;
        sh = scene_shadow(F, R, n, p + sun * 0.05f, sun, w);
    }
    rgb = scene_illuminate<false>(F, R, p, nrm, mat, ao, sh);
    return mat;
}

// render's height fog :287-311 over render_impl's (rgb, t) for a ray whose origin and direction have the heights ro_y, rd_y: the linear
// colour after the `abs`
__device__ __forceinline__ v3 scene_fog(const FrameSdfScene& F, float ro_y, float rd_y, v3 rgb, float t) {
    const float fog_factor = F.fog_density * exp_(-ro_y * F.fog_falloff)
                           * (1.f - exp_(-t * rd_y * F.fog_falloff))
                           / (rd_y * F.fog_falloff);
    return abs3(mix3(rgb, V3(1, 1, 1), fog_factor));
}

}  // namespace sbx
