// shaderbox_amd/csrc/kern_raytracer_eval.hip — sbx_raytracer_eval: the raytracer's trace, shading, shadow test and render
// (src/app_raytracer.h: raytrace_iteration :70-86, illuminate :46-68, the shadow test :109-116, render :88-136) over the caller's rays and
// points under the caller's scene (include/sbx.h sbx_aux_raytracer_scene).  No camera, no sRGB.
//
// k_raytracer_eval: the element wave of sbx_witness.h (witnessed_elements: the witness re-run, loads and stores) over k_raytracer_scene's
// device functions (sbx_raytracer.h) and the FrameRtScene that build_raytracer_scene (sbx_frames.hip) makes of the block.  As in
// k_raytracer_scene the block is copied to LDS (lds_frame_fill), the primitive loops read it through the plain LDS loads, and the
// counts, bounces, lighting, shadow and light type come from the kernel argument: the loops and branches stay scalar.  What is its own:
//   WHAT THE SHORTCUTS NEED OF THE CALLER'S ELEMENTS: NOTHING, so WPOS = 0 and every wave of a default launch takes the witnessed form
//     and is counted.  sbx_raytracer.h "CALLER'S NUMBERS" decides each inherited shortcut for a scene that is the caller's; here the ray's
//     origin and direction, the hit's origin and normal and the eye are the caller's too, directions of any length included:
//     - Wit<true>'s sqrt / length / normalize RECORD every argument outside the interval they were compared on — whatever made the
//       argument: a tangent ray (the root of 0), a hit straight under the light (a zero component of shadow_line), a zero, NaN, inf or
//       3e38 coordinate — and the wave re-runs with the IEEE forms.  Nothing is assumed about the ray that produced the argument.
//     - the sphere normal's div_by(dn, rr) is proved for EVERY binary32 dividend whose quotient is a normal number, and records a nonzero
//       dn whose quotient came out at or below 2^-126.  In k_raytracer_scene that record was a second net behind the normalisation that
//       made the ray; for a ray that no normalisation made it is the only one, and it is complete: zero, inf and NaN dividends and
//       quotients beyond FLT_MAX follow the same rules on both sides.
//     - r0 is IEEE arithmetic on the host over the block alone.
//     - hit_plane, fresnel_factor, cook_torrance and phong are IEEE operations and the math spec's exp and pow, which take every binary32.
//     - hit_walls, the one shortcut that needs finite, normalised rays, is a proof about the Cornell box and is not used here.
//     - a lane past n evaluates the zero element: no plane is hit (denom = 0 < 1e-6), a sphere around the origin may be, the bounce loop
//       ends within the block's count; what it records is not counted (`on`).
//     So no form of a wave depends on its elements: PLAIN (sbx_set_variant 1) is the IEEE form for every wave, variants 2 and 3 are as
//     witness_dispatch defines them.
//   int() OF THE MATERIAL IDS ("raytrace_iteration"'s mat_to_ignore, "illuminate"'s material): toward zero, saturating, a NaN gives 0
//     (include/sbx.h) — what v_cvt_i32_f32 does, stated in C++ (`re_int`, as kern_vinyl_eval.hip's ve_int) because the language leaves an
//     out-of-range conversion undefined.  The ids going OUT are the block's ints as floats.
//   "illuminate" HAS 10 INPUTS: the capacity of an element is RE_WORDS here (witnessed_elements' CAP).
//   THE WAVE BOUND: re_min_waves below, from tools/kernel_resources.py (profiles/raytracer_eval_resources.txt): no instantiation has scratch.
#include "sbx_raytracer.h"

namespace sbx {

enum { RE_TRACE = 0, RE_ILLUMINATE = 1, RE_SHADOW = 2, RE_RENDER = 3 };
constexpr int RE_WORDS = 10;

__device__ __forceinline__ int re_int(float x) {
    if (x != x) return 0;
    return (int)fmin_(fmax_(x, -2147483648.f), 2147483520.f);      // (2^31 - 128: the largest binary32 below 2^31)
}

constexpr int re_in_width(int fn) { return fn == RE_TRACE ? 7 : fn == RE_ILLUMINATE ? 10 : fn == RE_SHADOW ? 3 : 6; }
constexpr int re_out_width(int fn) { return fn == RE_TRACE ? 8 : fn == RE_ILLUMINATE ? 3 : fn == RE_SHADOW ? 2 : 4; }

// The wave bound of an instantiation (amdgpu_waves_per_eu's lower end).  "render" is scene_radiance, k_raytracer_scene's body, with the
// element's loads, the depth and the counter beside it: asked for 7 waves (72 VGPRs), as that kernel is, its witnessed forms spill 12
// bytes; at 6 they take 79 VGPRs and no scratch.  The other three fit 8 waves (19 - 47 VGPRs).
constexpr int re_min_waves(int fn) { return fn == RE_RENDER ? 6 : 8; }

// one element of FN with the roots of witness `w`; q = its inputs, r = its outputs
template <int FN, class W>
__device__ __forceinline__ void re_element(const FrameRtScene& F, const FrameRtScene& Fs, const float (&q)[RE_WORDS], W& w, float (&r)[RE_WORDS]) {
    const v3 a = V3(q[0], q[1], q[2]), b = V3(q[3], q[4], q[5]);
    if (FN == RE_TRACE) {                                          // raytrace_iteration(ray = (a, b), mat_to_ignore)
        const Hit hit = scene_trace(F, Fs, a, b, re_int(q[6]), w);
        r[0] = hit.t; r[1] = (float)hit.mat;
        r[2] = hit.o.x; r[3] = hit.o.y; r[4] = hit.o.z;
        r[5] = hit.n.x; r[6] = hit.n.y; r[7] = hit.n.z;
    } else if (FN == RE_ILLUMINATE) {                              // illuminate(eye = a, hit = (origin b, normal, material))
        Hit hit;
        hit.t = 0.f; hit.mat = re_int(q[9]); hit.n = V3(q[6], q[7], q[8]); hit.o = b;
        const RtMaterial mat = scene_material(Fs, hit.mat);
        const v3 light = rt_ld(Fs.light);
        const v3 L = F.light_type == 2 ? light : w.normalize(light - hit.o);   // get_light_direction light.h:18-27
        const v3 lit = scene_illuminate(F, Fs, a, hit, mat, L, w);
        r[0] = lit.x; r[1] = lit.y; r[2] = lit.z;
    } else if (FN == RE_SHADOW) {                                  // :109-116 at hit.origin = a, whatever the block's shadow switch says
        const v3 shadow_line = rt_ld(Fs.light) - a;
        const v3 shadow_dir = w.normalize(shadow_line);
        const Hit sh = scene_trace(F, Fs, a + shadow_dir * 1e-4f, shadow_dir, 0, w);
        r[0] = sh.t; r[1] = w.length(shadow_line);
    } else {                                                       // render :88-136 over the caller's ray (a, b)
        int depth;
        const v3 color = scene_radiance(F, Fs, a, b, w, depth);
        r[0] = color.x; r[1] = color.y; r[2] = color.z; r[3] = (float)depth;
    }
}

// PLAIN, WIT, counts: sbx_witness.h witnessed_elements
template <int FN, bool PLAIN, int WIT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(re_min_waves(FN), 8)))
k_raytracer_eval(FrameRtScene F, const float* __restrict__ in, float* __restrict__ out, size_t n, unsigned* __restrict__ counts) {
    __shared__ FrameRtScene Fs;
    lds_frame_fill<FrameRtScene, 64>(Fs);
    witnessed_elements<re_in_width(FN), 0, re_out_width(FN), PLAIN, WIT, RE_WORDS>(in, out, n, counts,
        [&](auto, const auto& q, auto& w, auto& r) { re_element<FN>(F, Fs, q, w, r); });
}

template <int FN>
static void re_launch(const FrameRtScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    witness_dispatch<1>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_raytracer_eval<FN, !cull.value, wit.value>), grid, dim3(64), 0, s, F, in, out, n, counts);
    });
}

// fn: RE_* in the order of sbx_eval.hip's names.  F: build_raytracer_scene of the caller's validated block (its camera is not read).
// variant: witness_dispatch's.  n in 1 ... 2^31.
void launch_raytracer_eval(int fn, const FrameRtScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    switch (fn) {
    case RE_TRACE: re_launch<RE_TRACE>(F, variant, in, out, n, counts, s); break;
    case RE_ILLUMINATE: re_launch<RE_ILLUMINATE>(F, variant, in, out, n, counts, s); break;
    case RE_SHADOW: re_launch<RE_SHADOW>(F, variant, in, out, n, counts, s); break;
    default: re_launch<RE_RENDER>(F, variant, in, out, n, counts, s); break;
    }
}

}  // namespace sbx
