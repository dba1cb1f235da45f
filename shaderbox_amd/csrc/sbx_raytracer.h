// shaderbox_amd/csrc/sbx_raytracer.h — APP_RAYTRACER's device functions (src/app_raytracer.h, src/intersect.h, src/light.h,
// src/util_optics.h as kern_raytracer.hip's header describes them): the reads of the scene block, the Hit, fresnel_factor, hit_plane,
// cook_torrance and phong that every raytracer kernel runs, and raytrace_iteration, get_material, illuminate and render over the CALLER'S
// scene (FrameRtScene).  Shared by k_raytracer and k_raytracer_scene (kern_raytracer.hip: SBX_APP_RAYTRACER, its builds and
// SBX_APP_RAYTRACER_SCENE) and k_raytracer_eval (kern_raytracer_eval.hip: sbx_raytracer_eval).
#pragma once
#include <cmath>
#include "sbx_device.h"
#include "sbx_ldsframe.h"
#include "sbx_witness.h"

#ifndef RT_LDS_FRAME
#define RT_LDS_FRAME 1      // the scene block (130 floats: does not fit the SGPR file) in LDS, read at its uses (sbx_ldsframe.h)
#endif

namespace sbx {

#if RT_LDS_FRAME
__device__ __forceinline__ RtPlane rt_ld(const RtPlane& r) { return RtPlane{lds_ld(r.n), lds_ld(r.d), lds_ld(r.mat)}; }
__device__ __forceinline__ RtSphere rt_ld(const RtSphere& r) { return RtSphere{lds_ld(r.o), lds_ld(r.r), lds_ld(r.mat), lds_ld(r.rr)}; }
__device__ __forceinline__ RtMaterial rt_ld(const RtMaterial& r) {
    return RtMaterial{lds_ld(r.base_color), lds_ld(r.roughness), lds_ld(r.ior), lds_ld(r.reflectivity), lds_ld(r.r0)};
}
__device__ __forceinline__ v3 rt_ld(const v3& r) { return lds_ld(r); }
__device__ __forceinline__ int rt_ld(const int& r) { return lds_ld(r); }
__device__ __forceinline__ float rt_ld(const float& r) { return lds_ld(r); }
#else
template <class T> __device__ __forceinline__ const T& rt_ld(const T& r) { return r; }
#endif

struct Hit { float t; int mat; v3 n, o; };

__device__ __forceinline__ float fresnel_factor(float n1, float n2, float VdotH) {   // util_optics.h:5-14
    float Rn = (n1 - n2) / (n1 + n2);
    float R0 = Rn * Rn;
    float F = 1.f - VdotH;
    return R0 + (1.f - R0) * (F * F * F * F * F);
}

__device__ __forceinline__ void hit_plane(v3 ro, v3 rd, const RtPlane& p, Hit& hit) {  // intersect.h:61-77
    const float denom = dot(p.n, rd);
    if (denom < 1e-6f) return;
    const v3 P0 = V3(p.d, p.d, p.d);
    const float t = dot(P0 - ro, p.n) / denom;
    if (t < 0.f || t > hit.t) return;
    hit.t = t;
    hit.mat = p.mat;
    hit.o = ro + rd * t;
    hit.n = dot(p.n, rd) < 0 ? p.n : -p.n;          // faceforward(N, I, Nref = N)  util.h:85-93
}

template <class W>      // W: the witness of the fast roots and normalisations (sbx_witness.h)
__device__ __forceinline__ v3 cook_torrance(v3 V, v3 L, const Hit& hit, const RtMaterial& mat, W& w) {   // light.h:64-92
    const v3 H = w.normalize(L + V);
    const float NdotL = dot(hit.n, L), NdotH = dot(hit.n, H), NdotV = dot(hit.n, V), VdotH = dot(V, H);
    const float geo_a = (2.f * NdotH * NdotV) / VdotH;
    const float geo_b = (2.f * NdotH * NdotL) / VdotH;
    const float geo_term = fmin_(1.f, fmin_(geo_a, geo_b));
    const float rough_sq = mat.roughness * mat.roughness;
    const float rough_a = 1.f / (rough_sq * NdotH * NdotH * NdotH * NdotH);
    const float rough_exp = (NdotH * NdotH - 1.f) / (rough_sq * NdotH * NdotH);
    const float rough_term = rough_a * exp_(rough_exp);
    const float Fc = 1.f - VdotH;                                 // fresnel_factor(1, ior, VdotH) with R0 from the frame
    const float fresnel_term = mat.r0 + (1.f - mat.r0) * (Fc * Fc * Fc * Fc * Fc);
    const float specular = (geo_term * rough_term * fresnel_term) / (3.14159265359f * NdotV * NdotL);
    return fmax_(0.f, NdotL) * (specular + mat.base_color);
}
// illum_blinn_phong, light.h:44-62 with the `#else` of :53 (the Phong specular; the Blinn branch does not compile in the C++ form).
// reflect(incident, normal) = incident - 2 * dot(normal, incident) * normal (util_optics.h:17-22) with incident = -L: the unary minus
// makes negative zeros, which stay.  `pow(..) * vec3(1, 1, 1)` is the float times each 1: the float itself.  No root.
__device__ __forceinline__ v3 phong(v3 V, v3 L, const Hit& hit, const RtMaterial& mat) {
    const v3 diffuse = fmax_(0.f, dot(L, hit.n)) * mat.base_color;          // :50
    const v3 I = -L;
    const v3 R = I - 2.f * dot(hit.n, I) * hit.n;                           // :57
    const float specular = pow_(fmax_(0.f, dot(R, V)), 50.f);               // :52, :58
    return diffuse + V3(specular, specular, specular);                      // :61
}

// ---- over the CALLER'S scene (include/sbx.h sbx_aux_raytracer_scene): SBX_APP_RAYTRACER_SCENE and sbx_raytracer_eval ------------------
// The same functions as above — hit_plane, cook_torrance, phong, fresnel_factor, the Wit roots and normalisations — over FrameRtScene:
// the plane and sphere loops run to the block's counts, and the bounce count, the lighting model, the shadow switch and the light
// type are values of the block.  All of those are read from the kernel ARGUMENT (SGPRs: the loops and branches are scalar); the
// arrays, the light and the ambient colour from the LDS copy (sbx_ldsframe.h: 1.2 KB does not fit the SGPR file), every lane at one
// address.  hit_walls is a proof about the Cornell box and stays out: a block that equals the box still takes the plane loop.
//
// CALLER'S NUMBERS.  Every shortcut inherited from k_raytracer, and what it needs of numbers that are no longer this project's:
//   - Wit<true>'s sqrt / length / normalize (sbx_witness.h) need nothing: a lane RECORDS every argument outside the interval the fast
//     form was compared on (zero, denormal, inf, NaN, negative; for normalize also a component whose square is not normal) and the
//     wave re-runs the pixel with the IEEE forms.  A scene with an axis-parallel light or mirror direction records often and pays the
//     second pass; its bits are the IEEE forms' either way.
//   - the sphere normal (impact - origin) / radius as div_by(dn, rr), rr = recip64(radius) from the host.  sbx_math.h:59-68 proves
//     it equal to the IEEE quotient where the quotient is a NORMAL binary32 number: its midpoint argument is about 25-bit midpoints.
//     In the subnormal range a quotient can BE a rounding midpoint (5 * 2^-149 / 10 = 2^-150: the IEEE quotient is 0, while the
//     binary64 product with RN64(1 / 10) > 1 / 10 lies above the tie and rounds to 2^-149), so there the identity does not hold.  The
//     fast pass therefore records a nonzero dn whose quotient came out at or below 2^-126 in magnitude (2^-126 itself can be a tie
//     rounded up) and the wave re-runs; the IEEE pass divides by the radius itself.  (For the rays k_raytracer_scene makes the record is a
//     second net: such a dn component needs an origin and a direction component that small, and a direction component whose square is
//     not a normal number is already recorded by the normalisation that made the ray.  tests/test_gpu_raytracer_scene.py drives both
//     through the centre column of an odd-width frame from an eye whose x is a denormal.)  Everything else follows the same rules on both
//     sides: radius 0 (rr = inf: dn * inf = dn / 0, NaN for dn = 0), radius inf (rr = 0), NaN, a denormal radius (its reciprocal is
//     finite in binary64), a quotient beyond FLT_MAX (the overflow threshold is a 25-bit midpoint), dn = +-0 (the sign is the
//     product's) and a normal quotient (the proof).
//   - the host's r0 = ((1 - ior) / (1 + ior))^2 (sbx_frames.hip rt_material): the two binary32 operations of fresnel_factor(1, ior, .)
//     with n1 = 1 (util_optics.h:10-11), evaluated by IEEE arithmetic on the host as on the device, for every ior: -1 gives inf,
//     NaN gives NaN (a NaN's payload is not compared anywhere in this project).
//   - hit_plane, cook_torrance, phong, to_srgb hold no shortcut with a domain: IEEE quotients, the math spec's exp and pow.
#ifndef RT_SCENE_UNROLL
#define RT_SCENE_UNROLL 2
#endif
// the primitive arrays through PLAIN LDS loads: their index is the loop's, nothing can be hoisted out of a loop of run-time length or
// kept alive across it (what the volatile reads of sbx_ldsframe.h are there to prevent), and the scheduler may batch them.
// The block was stored by lds_frame_fill as 32-bit words through a float*, and these loads read some of them as int and double: what
// orders them behind those stores is the __syncthreads() at the end of lds_frame_fill (a workgroup barrier and an LDS fence that no
// memory access is moved across), not the types — so no rts_ld may ever stand before that call.
#define RTS_PTR(T, r) ((const __attribute__((address_space(3))) T*)(&(r)))
__device__ __forceinline__ v3 rts_v3(const v3& r) { return V3(*RTS_PTR(float, r.x), *RTS_PTR(float, r.y), *RTS_PTR(float, r.z)); }
__device__ __forceinline__ RtPlane rts_ld(const RtPlane& r) { return RtPlane{rts_v3(r.n), *RTS_PTR(float, r.d), *RTS_PTR(int, r.mat)}; }
__device__ __forceinline__ RtSphere rts_ld(const RtSphere& r) { return RtSphere{rts_v3(r.o), *RTS_PTR(float, r.r), *RTS_PTR(int, r.mat), *RTS_PTR(double, r.rr)}; }
__device__ __forceinline__ RtMaterial scene_material(const FrameRtScene& Fs, int id) {   // get_material: the zero material outside 0..7
    RtMaterial m;
    m.base_color = V3(0, 0, 0); m.roughness = 0.f; m.ior = 0.f; m.reflectivity = 0.f;
    m.r0 = 1.f;                                                  // ior 0: ((1 - 0) / (1 + 0))^2
    if (id >= 0 && id < 8) m = rt_ld(Fs.mats[id]);
    return m;
}
template <class W>
__device__ __forceinline__ void scene_hit_sphere(v3 ro, v3 rd, const RtSphere& s, Hit& hit, W& w) {   // intersect.h:7-33, as hit_sphere
    const v3 rc = s.o - ro;
    const float radius2 = s.r * s.r;
    const float tca = dot(rc, rd);
    if (tca < 0.f) return;
    const float d2 = dot(rc, rc) - tca * tca;
    if (d2 > radius2) return;
    const float thc = w.sqrt(radius2 - d2);
    float t0 = tca - thc;
    const float t1 = tca + thc;
    if (t0 < 0.f) t0 = t1;
    if (t0 > hit.t) return;
    const v3 impact = ro + rd * t0;
    hit.t = t0;
    hit.mat = s.mat;
    hit.o = impact;
    const v3 dn = impact - s.o;
    if (W::fast) {                                               // (CALLER'S NUMBERS above)
        const v3 n = V3(div_by(dn.x, s.rr), div_by(dn.y, s.rr), div_by(dn.z, s.rr));
        const float mn = u2f(0x00800000u);                       // 2^-126
        w.bad |= (abs_(n.x) <= mn && dn.x != 0.f) || (abs_(n.y) <= mn && dn.y != 0.f) || (abs_(n.z) <= mn && dn.z != 0.f);
        hit.n = n;
    } else {
        hit.n = V3(dn.x / s.r, dn.y / s.r, dn.z / s.r);          // (impact - origin) / radius
    }
}
// raytrace_iteration :70-86.  Unrolled by two: the loads of one primitive ride beside the other's arithmetic (measured: 0.209 -> 0.202 ms
// on the Cornell block at 3840x2160 together with the plain LDS loads; by four no better; select forms instead of hit_plane's early
// returns LOSE, 0.231 ms — a wave whose rays all face away from a plane skips its division —, and so does deferring the hit's origin and
// normal until the loops have chosen the primitive, 0.209 ms; profiles/raytracer_scene_timing.txt)
template <class W>
__device__ __forceinline__ Hit scene_trace(const FrameRtScene& F, const FrameRtScene& Fs, v3 ro, v3 rd, int mat_to_ignore, W& w) {
    Hit hit;
    hit.t = (float)(1e8f + 1e1f); hit.mat = -1; hit.n = V3(0, 0, 0); hit.o = V3(0, 0, 0);   // no_hit def.h:78-83
#pragma unroll RT_SCENE_UNROLL
    for (int i = 0; i < F.n_planes; ++i) hit_plane(ro, rd, rts_ld(Fs.planes[i]), hit);
#pragma unroll RT_SCENE_UNROLL
    for (int i = 0; i < F.n_spheres; ++i) {
        const RtSphere sp = rts_ld(Fs.spheres[i]);
        if (sp.mat != mat_to_ignore) scene_hit_sphere(ro, rd, sp, hit, w);
    }
    return hit;
}
// illuminate :46-68 of a hit whose material `mat` = scene_material(Fs, hit.mat) and whose light direction L (get_light_direction
// light.h:18-27) come from the caller, which needs both again: the scene block's reads are volatile, so the compiler would not share them
template <class W>
__device__ __forceinline__ v3 scene_illuminate(const FrameRtScene& F, const FrameRtScene& Fs, v3 eye, const Hit& hit, const RtMaterial& mat, v3 L, W& w) {
    if (hit.mat == 0) return rt_ld(Fs.mats[0].base_color);       // mat_debug: flat
    const v3 V = w.normalize(eye - hit.o);
    return rt_ld(Fs.ambient) + (F.lighting != 0 ? phong(V, L, hit, mat) : cook_torrance(V, L, hit, mat, w));
}
// The linear colour of one ray — render :88-136 from the ray onwards — with the roots / normalisations of witness `w`.  F: the kernel
// argument; Fs: its LDS copy.  (ro, rd): the primary ray; ro stays illuminate's eye on every bounce (:105).  depth: an int that receives
// the number of bounce-loop traces that found a hit, or an RtNoDepth for a kernel that does not want it (k_raytracer_scene: a counter
// that nothing reads is removed, but late enough to move the code generator's choices, 12 bytes of code by tools/kernel_resources.py).
struct RtNoDepth {
    __device__ __forceinline__ void operator=(int) {}
    __device__ __forceinline__ void operator++() {}
};
template <class W, class D>
__device__ __forceinline__ v3 scene_radiance(const FrameRtScene& F, const FrameRtScene& Fs, v3 ro, v3 rd, W& w, D& depth) {
    const v3 eye = ro;
    const bool dir_light = F.light_type == 2;                    // LIGHT_DIR light.h:6
    depth = 0;

    v3 color = V3(0, 0, 0), accum = V3(1, 1, 1);
    for (int i = 0; i < F.bounces; ++i) {                         // :96-133
        const Hit hit = scene_trace(F, Fs, ro, rd, -1, w);
        if (hit.t >= 1e8f) {
            color = color + accum * V3(0, 0, 0);                  // background :13-16
            break;
        }
        ++depth;
        const float f = fresnel_factor(1.f, 1.f, dot(hit.n, -rd));
        const RtMaterial mat = scene_material(Fs, hit.mat);
        const v3 light = rt_ld(Fs.light);
        const bool shadow_ray = F.shadow != 0 && i == 0;
        const v3 shadow_line = light - hit.o;                     // :109: also with LIGHT_DIR (the reference's TODO)
        v3 shadow_dir = light;
        if (!dir_light || shadow_ray) shadow_dir = w.normalize(shadow_line);   // (not evaluated where nothing reads it: no record)
        const v3 L = dir_light ? light : shadow_dir;              // get_light_direction light.h:18-27
        const v3 ill = scene_illuminate(F, Fs, eye, hit, mat, L, w);   // the primary origin on every bounce (:105)
        color = color + (1.f - f) * accum * ill;
        if (shadow_ray) {                                         // :108-121
            const Hit sh = scene_trace(F, Fs, hit.o + shadow_dir * 1e-4f, shadow_dir, 0, w);
            if (sh.t < w.length(shadow_line)) color = color * 0.1f;
        }
        if (mat.reflectivity > 0.f) {
            accum = accum * f;
            // reflect(hit.normal, ray.direction): arguments swapped in the reference (:127), kept
            const v3 refl = w.normalize(hit.n - 2.f * dot(rd, hit.n) * rd);
            ro = hit.o + refl * 1e-4f;
            rd = refl;
        } else {
            break;
        }
    }
    return color;
}

}  // namespace sbx
