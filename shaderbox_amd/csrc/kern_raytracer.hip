// shaderbox_amd/csrc/kern_raytracer.hip — APP_RAYTRACER: Cornell box, Cook-Torrance, 2 bounces.
//
// Follows /root/reference/src/app_raytracer.h (render :88-136, raytrace_iteration :70-86,
// illuminate :46-68), src/intersect.h (intersect_plane :61-77, intersect_sphere :7-33),
// src/light.h (illum_cook_torrance :64-92), src/util_optics.h (fresnel_factor :5-14, reflect
// :17-22), src/material.h, src/cornell_box.h.  The whole scene (6 planes, 3 spheres, 8 material
// slots, the light) is frame-constant: it is built on the host (setup_scene :18-36 +
// setup_cornell_box cornell_box.h:39-87) and arrives as kernel arguments in SGPRs.
//
// BUILD (sbx_frame.h RT_*): the file's compile-time switches, each one the other way (include/sbx.h).
//   RT_PHONG     the `#if 0` of illuminate at :61 turned to `#if 1` (SBX_APP_RAYTRACER_PHONG): illum_blinn_phong (light.h:44-62, its
//                compiled `#else` branch, the Phong specular) stands in for illum_cook_torrance
//   RT_NOSHADOW  the `#if 1 // shadow ray` of render at :107 turned to `#if 0` (SBX_APP_RAYTRACER_NOSHADOW): :108-121 are gone
// The third switch, setup_scene's `#if 1` at :29 (SBX_APP_RAYTRACER_STATIC), changes the frame block alone (sbx_frames.hip
// build_raytracer): it runs the RT_DEFAULT kernels.
// SBX_APP_RAYTRACER_SCENE — render over the CALLER'S scene, k_raytracer_scene — is at the end of the file.
// The device functions that more than one kernel runs (the scene block's reads, Hit, fresnel_factor, hit_plane, cook_torrance, phong, and
// everything over FrameRtScene) are in sbx_raytracer.h, which k_raytracer_eval (kern_raytracer_eval.hip) shares.
#include "sbx_raytracer.h"

namespace sbx {

template <class W>      // W: the witness of the fast roots and normalisations (sbx_witness.h)
__device__ __forceinline__ void hit_sphere(v3 ro, v3 rd, const RtSphere& s, Hit& hit, W& w) {   // intersect.h:7-33
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
    hit.n = V3(div_by(dn.x, s.rr), div_by(dn.y, s.rr), div_by(dn.z, s.rr));     // (impact - origin) / radius, exact (sbx_math.h)
}
#ifndef RT_AXIS_PLANES
#define RT_AXIS_PLANES 1   // the six walls as three axis pairs, one division per axis (below); 0 = six hit_plane from the scene block
#endif
// THE CORNELL BOX'S WALLS AS AXIS PAIRS (round 5).  cornell_box.h:57-69 builds, in array order, the planes
//   0: n (0,-1,0) d 0    1: n (0,0,-1) d -2    2: n (0,0,1) d 2    3: n (0,1,0) d 4    4: n (1,0,0) d 2 (mat 2)    5: n (-1,0,0) d -2 (mat 3)
// (mat 1 for 0..3) for every frame — launch_raytracer checks the frame holds exactly these, else the generic kernel runs.  For a
// normal n = s e_c (s = +-1) and FINITE ro, rd with rd_c != 0, intersect_plane's two dot products are exact single terms: the
// other two products are zeros, and a zero added to a nonzero number changes nothing:
//   denom = dot(n, rd) = s rd_c         num = dot(P0 - ro, n) = s (d - ro_c)   (when that is nonzero)      t = num / denom = (d - ro_c) / rd_c
// (IEEE division is sign-symmetric).  `denom < 1e-6 -> no hit` admits at most ONE plane of each pair — the one rd_c points at — so a
// ray costs three divisions, not six, no normals or distances read from LDS and one hit point.  The reference's loop takes the
// planes in array order and a later plane replaces an earlier one at EQUAL t (`t > hit.t` is false), so the candidates are taken
// in that order: plane 0 (if rd_y < 0), the z plane, plane 3 (if rd_y > 0), the x plane.  hit.n = -n (faceforward: dot(n, rd) =
// denom > 0) keeps its negated zeros.  What the shortcut needs is what the witness already records for the normalisation that
// made rd (every component's square a normal number: finite, nonzero) plus a finite frame (checked on the host: then ro = eye or
// hit.o + dir * 1e-4 stays finite, t <= 1e8 + 10); a num of zero — its sign would be the generic sum's, not s * 0 — is recorded too
// and the wave re-runs with the generic IEEE kernel body like for any other record.
template <class W>
__device__ __forceinline__ void hit_walls(v3 ro, v3 rd, Hit& hit, W& w) {
    const float ty = ((rd.y > 0.f ? 4.f : 0.f) - ro.y) / rd.y;
    const float tz = ((rd.z > 0.f ? 2.f : -2.f) - ro.z) / rd.z;
    const float tx = ((rd.x > 0.f ? 2.f : -2.f) - ro.x) / rd.x;
    w.bad |= (ty == 0.f) || (tz == 0.f) || (tx == 0.f);          // a zero quotient here is a zero num (rd finite, nonzero)
    float t = hit.t;
    int ax = -1;
    const bool cy = !(abs_(rd.y) < 1e-6f) && !(ty < 0.f);
    if (cy && rd.y < 0.f && !(ty > t)) { t = ty; ax = 0; }
    if (!(abs_(rd.z) < 1e-6f) && !(tz < 0.f) && !(tz > t)) { t = tz; ax = 1; }
    if (cy && rd.y > 0.f && !(ty > t)) { t = ty; ax = 0; }
    if (!(abs_(rd.x) < 1e-6f) && !(tx < 0.f) && !(tx > t)) { t = tx; ax = 2; }
    if (ax >= 0) {
        hit.t = t;
        hit.mat = ax == 2 ? (rd.x > 0.f ? 2 : 3) : 1;
        hit.o = ro + rd * t;
        hit.n = V3(ax == 2 ? (rd.x > 0.f ? -1.f : 1.f) : -0.f, ax == 0 ? (rd.y > 0.f ? -1.f : 1.f) : -0.f, ax == 1 ? (rd.z > 0.f ? -1.f : 1.f) : -0.f);
    }
}
inline bool rt_walls_are_cornell(const FrameRaytracer& F) {
    static const float n[6][3] = {{0, -1, 0}, {0, 0, -1}, {0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {-1, 0, 0}};
    static const float d[6] = {0.f, -2.f, 2.f, 4.f, 2.f, -2.f};
    static const int mat[6] = {1, 1, 1, 1, 2, 3};
    for (int i = 0; i < 6; ++i) {
        const RtPlane& p = F.planes[i];
        // (== on the components: a -0 in a normal would change hit.n's zeros)
        if (f2u(p.n.x) != f2u(n[i][0]) || f2u(p.n.y) != f2u(n[i][1]) || f2u(p.n.z) != f2u(n[i][2]) || f2u(p.d) != f2u(d[i]) || p.mat != mat[i]) return false;
    }
    return true;
}

template <bool WALLS, class W>
__device__ __forceinline__ Hit trace(const FrameRaytracer& F, v3 ro, v3 rd, int mat_to_ignore, W& w) {   // :70-86
    Hit hit;
    hit.t = (float)(1e8f + 1e1f); hit.mat = -1; hit.n = V3(0, 0, 0); hit.o = V3(0, 0, 0);   // no_hit def.h:78-83
    if (WALLS && W::fast) {
        hit_walls(ro, rd, hit, w);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) hit_plane(ro, rd, rt_ld(F.planes[i]), hit);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
        const RtSphere sp = rt_ld(F.spheres[i]);
        if (sp.mat != mat_to_ignore) hit_sphere(ro, rd, sp, hit, w);
    }
    return hit;
}
// get_material: linear scan; an id outside 0..7 yields the zero-initialised material (App. B5)
template <int BUILD>
__device__ __forceinline__ RtMaterial material_of(const FrameRaytracer& F, int id) {
    RtMaterial m;
    m.base_color = V3(0, 0, 0); m.roughness = 0.f; m.ior = 0.f; m.reflectivity = 0.f;
    m.r0 = 1.f;                                                  // ior 0: ((1 - 0) / (1 + 0))^2
#if RT_LDS_FRAME
    if (BUILD == RT_PHONG) {                                     // illum_blinn_phong reads base_color alone, render the reflectivity
        if (id >= 0 && id < 8) { m.base_color = rt_ld(F.mats[id].base_color); m.reflectivity = rt_ld(F.mats[id].reflectivity); }
        return m;
    }
    if (id >= 0 && id < 8) m = rt_ld(F.mats[id]);               // one LDS read per member at the lane's own address
#else
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i == id) m = F.mats[i];
#endif
    return m;
}
// (mat = material_of(hit.mat) and L = normalize(light - hit.o), light.h:18-27, come from the caller, which needs both again:
// the scene block's reads are volatile, so the compiler would not share them)
template <int BUILD, class W>
__device__ __forceinline__ v3 rt_illuminate(const FrameRaytracer& F, v3 eye, const Hit& hit, const RtMaterial& mat, v3 L, W& w) {   // :46-68
    if (hit.mat == 0) return rt_ld(F.mats[0].base_color);        // mat_debug: flat
    v3 accum = V3(.01f, .01f, .01f);                              // ambient_light light.h:16
    const v3 V = w.normalize(eye - hit.o);
    if (BUILD == RT_PHONG) accum = accum + phong(V, L, hit, mat);       // :61-62
    else accum = accum + cook_torrance(V, L, hit, mat, w);
    return accum;
}

#ifndef RT_WITNESS
#define RT_WITNESS 1       // fast roots and normalisations with a recorded domain (sbx_witness.h): 0 = the IEEE forms only
#endif

// One pixel's colour — render :88-136 — with the roots / normalisations of witness `w`.  Fs: the scene block (LDS copy or F).
template <bool WALLS, int BUILD, class W>
__device__ __forceinline__ v3 rt_pixel(const FrameRaytracer& F, const FrameRaytracer& Fs, v2 pc, W& w) {
    const v3 eye = F.cam.eye;
    v3 ro = eye, rd = primary_dir(F.cam, pc, w);

    v3 color = V3(0, 0, 0), accum = V3(1, 1, 1);
    for (int i = 0; i < 2; ++i) {                                 // :96-133
        const Hit hit = trace<WALLS>(Fs, ro, rd, -1, w);
        if (hit.t >= 1e8f) {
            color = color + accum * V3(0, 0, 0);                  // background :13-16
            break;
        }
        const float f = fresnel_factor(1.f, 1.f, dot(hit.n, -rd));
        const RtMaterial mat = material_of<BUILD>(Fs, hit.mat);
        const v3 shadow_line = rt_ld(Fs.light) - hit.o;           // = illuminate's light vector (point light, light.h:18-27)
        const v3 shadow_dir = w.normalize(shadow_line);
        color = color + (1.f - f) * accum * rt_illuminate<BUILD>(Fs, eye, hit, mat, shadow_dir, w);   // primary origin on every bounce (:105)
        if (BUILD != RT_NOSHADOW && i == 0) {                     // shadow ray :108-121
            const Hit sh = trace<WALLS>(Fs, hit.o + shadow_dir * 1e-4f, shadow_dir, 0, w);
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

template <int WIT, bool WALLS = false, int BUILD = RT_DEFAULT>   // WIT: 0 IEEE forms, 1 witnessed fast forms, 2 the witness's test edge (sbx_set_variant 2); WALLS: hit_walls; BUILD: RT_*
__global__ void __launch_bounds__(WG_THREADS) k_raytracer(FrameRaytracer F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
#if RT_LDS_FRAME
    __shared__ FrameRaytracer Fs;
    lds_frame_fill<FrameRaytracer, WG_THREADS>(Fs);
#define RT_F Fs
#else
#define RT_F F
#endif
    const Pixel px = pixel_of_thread(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    v3 color;
    // (hit_walls is the fast pass's alone: the IEEE pass takes the six-plane loop)
    witnessed<WIT>(true, [&](auto& w) {
        using W = std::remove_reference_t<decltype(w)>;
        color = rt_pixel<WALLS && W::fast, BUILD>(F, RT_F, pc, w);
    });
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(color));
}

dim3 raytracer_grid(const RowMap& M) { return grid_for(M); }

template <int BUILD>
static void launch_build(const FrameRaytracer& F, const RowMap& M, float* out, hipStream_t s, int variant, bool walls) {
    // hit_walls belongs to the fast forms (the witness's test build keeps its domain too); the IEEE kernel has no use for it
    witness_dispatch<RT_WITNESS>(variant, [&](auto, auto wit) {
        if constexpr (wit.value != 0) {
            if (walls) { hipLaunchKernelGGL((k_raytracer<wit.value, true, BUILD>), grid_for(M), dim3(WG_THREADS), 0, s, F, M, out); return; }
        }
        hipLaunchKernelGGL((k_raytracer<wit.value, false, BUILD>), grid_for(M), dim3(WG_THREADS), 0, s, F, M, out);
    });
}

void launch_raytracer(const FrameRaytracer& F, const RowMap& M, float* out, hipStream_t s, int variant, int build) {
    // hit_walls' conditions on the frame: the six planes are cornell_box.h's and every number of the frame is finite
    bool walls = RT_AXIS_PLANES && rt_walls_are_cornell(F);
    for (int i = 0; i < 3; ++i) walls = walls && std::isfinite(F.spheres[i].o.x) && std::isfinite(F.spheres[i].o.y) && std::isfinite(F.spheres[i].o.z) && std::isfinite(F.spheres[i].r);
    const float chk[] = {F.cam.eye.x, F.cam.eye.y, F.cam.eye.z, F.light.x, F.light.y, F.light.z};
    for (float v : chk) walls = walls && std::isfinite(v);
    switch (build) {
    case RT_PHONG: launch_build<RT_PHONG>(F, M, out, s, variant, walls); break;
    case RT_NOSHADOW: launch_build<RT_NOSHADOW>(F, M, out, s, variant, walls); break;
    default: launch_build<RT_DEFAULT>(F, M, out, s, variant, walls); break;     // RT_STATIC: the shipped kernels over its frame block
    }
}

// ---- SBX_APP_RAYTRACER_SCENE: render (:88-136) over the CALLER'S scene (include/sbx.h sbx_aux_raytracer_scene).  Its device functions,
// and what each inherited shortcut needs of the caller's numbers, are in sbx_raytracer.h; sbx_raytracer_eval runs the same ones.
// One pixel's colour: the primary ray of the block's camera, then render from the ray onwards.
template <class W>
__device__ __forceinline__ v3 scene_pixel(const FrameRtScene& F, const FrameRtScene& Fs, v2 pc, W& w) {
    RtNoDepth depth;
    return scene_radiance(F, Fs, F.cam.eye, primary_dir(F.cam, pc, w), w, depth);
}

// amdgpu_waves_per_eu(7, 8): the allocator's own choice was 79 VGPRs (6 waves per SIMD); asked for 7 it fits 72 without scratch, and the
// launch is 1 - 6 % shorter (profiles/raytracer_scene_timing.txt; 8 waves would need scratch)
template <int WIT>   // 0 IEEE forms, 1 witnessed fast forms, 2 the witness's test edge (sbx_set_variant 2)
__global__ void __launch_bounds__(WG_THREADS) __attribute__((amdgpu_waves_per_eu(7, 8))) k_raytracer_scene(FrameRtScene F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
    __shared__ FrameRtScene Fs;
    lds_frame_fill<FrameRtScene, WG_THREADS>(Fs);
    const Pixel px = pixel_of_thread(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    v3 color;
    witnessed<WIT>(true, [&](auto& w) { color = scene_pixel(F, Fs, pc, w); });
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(color));
}

void launch_raytracer_scene(const FrameRtScene& F, const RowMap& M, float* out, hipStream_t s, int variant) {
    witness_dispatch<RT_WITNESS>(variant, [&](auto, auto wit) {
        hipLaunchKernelGGL((k_raytracer_scene<wit.value>), grid_for(M), dim3(WG_THREADS), 0, s, F, M, out);
    });
}

}  // namespace sbx
