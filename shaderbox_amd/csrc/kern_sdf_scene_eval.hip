// shaderbox_amd/csrc/kern_sdf_scene_eval.hip — sbx_sdf_scene_eval: the field, normal, ambient occlusion, soft shadow, shading, trace and
// fogged render of SBX_APP_SDF_SCENE (src/app_sdf_ao.h: sdf_normal :152-163, sdf_ao :165-181, sdf_shadow :183-207, illuminate :211-243,
// render_impl :245-285, render :287-311, with sdf(pos) the caller's postfix program over src/sdf.h) over the caller's points and rays
// under the caller's block (include/sbx.h sbx_aux_sdf_scene).  No camera, no sRGB.
//
// k_sdf_scene_eval_fn: the element wave of sbx_witness.h (witnessed_elements: the witness re-run, loads and stores) over k_sdf_scene's
// device functions (sbx_sdf_scene.h) and the FrameSdfScene that build_sdf_scene (sbx_frames.hip) makes of the block.  What is its own:
//   THE FRAME, as k_sdf_scene reads it: the control words (n_instr, each instruction's op and axis, steps, end, shadow, view, checker,
//     sun, fog, background) by scalar loads from the kernel-argument segment, the operands and materials from the workgroup's LDS copy,
//     filled (lds_frame_fill, for this kernel's 64 threads) before the first read.  The frame is the kernel's FIRST argument: SdfRd.K is
//     the segment pointer itself.
//   WHAT THE SHORTCUTS NEED OF THE CALLER'S NUMBERS: NOTHING, so WPOS = 0, there is no host judgement of the block, and every wave of a
//     default launch takes the witnessed form and is counted.  As in k_sdf_scene (kern_sdf_scene.hip "CALLER'S NUMBERS"): Wit<true>'s
//     roots RECORD every argument outside the interval they were compared on — a point at a sphere's centre or on a cylinder's or a
//     torus's axis (the root of 0), a NaN, an inf, a 3e38 or 1e-40 coordinate — and the wave re-runs with the IEEE roots; every min / max
//     is the spec's compare-and-select; sdf_normal's normalize is the IEEE one under every witness.  Here the point, the ray, the
//     normal, ao and sh are the caller's too, of any length and any bit pattern: they enter IEEE arithmetic and those roots only.
//     PLAIN (sbx_set_variant 1) is the IEEE form for every wave; variants 2 and 3 are as witness_dispatch defines them.
//   A LANE PAST n evaluates the zero element: a march from the origin with a zero direction, which ends within the block's steps; what
//     it records is not counted (`on`) and nothing of it is stored.
//   int() OF THE MATERIAL ID ("illuminate"): toward zero, saturating, a NaN gives 0 (include/sbx.h) — what v_cvt_i32_f32 does, stated
//     in C++ (`se_int`, as kern_vinyl_eval.hip's ve_int) because the language leaves an out-of-range conversion undefined.  An id outside
//     0..7 gives the zero colour (scene_illuminate<true>): the port's choice where the reference's get_material leaves its result unset.
//   FN IS A COMPILE-TIME PARAMETER, as in the other eval kernels: 7 functions x 4 forms (PLAIN, and WIT 0 / 1 / 2).  "illuminate" has no
//     field in it; "sdf", "sdf_normal", "sdf_ao" and "sdf_shadow" hold one scene_sdf call site per pass, "render_impl" and "render"
//     four.  The sizes, the registers and the build time: profiles/sdf_scene_eval_resources.txt, DESIGN.md 5.27.
//   THE WAVE BOUND: se_min_waves below, from tools/kernel_resources.py: no instantiation has scratch.
#include "sbx_sdf_scene.h"

namespace sbx {

enum { SE_SDF = 0, SE_NORMAL = 1, SE_AO = 2, SE_SHADOW = 3, SE_ILLUMINATE = 4, SE_RENDER_IMPL = 5, SE_RENDER = 6 };
constexpr int SE_WORDS = 9;                                        // "illuminate" has 9 inputs

__device__ __forceinline__ int se_int(float x) {
    if (x != x) return 0;
    return (int)fmin_(fmax_(x, -2147483648.f), 2147483520.f);      // (2^31 - 128: the largest binary32 below 2^31)
}

constexpr int se_in_width(int fn) { return fn <= SE_NORMAL ? 3 : fn == SE_ILLUMINATE ? 9 : 6; }
constexpr int se_out_width(int fn) {
    return fn == SE_SDF ? 2 : fn == SE_AO || fn == SE_SHADOW ? 1 : fn == SE_RENDER_IMPL ? 5 : fn == SE_RENDER ? 4 : 3;
}

// The wave bound of an instantiation (amdgpu_waves_per_eu's lower end): what k_sdf_scene is built for (SDF_SCENE_MIN_WAVES)
constexpr int se_min_waves(int fn) { return 4; }

// one element of FN with the roots of witness `w`; q = its inputs, r = its outputs
template <int FN, class W>
__device__ __forceinline__ void se_element(const FrameSdfScene& F, const SdfRd& R, const float (&q)[SE_WORDS], W& w, float (&r)[SE_WORDS]) {
    const v3 a = V3(q[0], q[1], q[2]), b = V3(q[3], q[4], q[5]);
    const int n = F.n_instr;
    if (FN == SE_SDF) {                                            // sdf(pos = a)
        const D2 d = scene_sdf(F, R, n, a, w);
        r[0] = d.d; r[1] = d.m;
    } else if (FN == SE_NORMAL) {                                  // sdf_normal(p = a)
        const v3 nrm = scene_normal(F, R, n, a, w);
        r[0] = nrm.x; r[1] = nrm.y; r[2] = nrm.z;
    } else if (FN == SE_AO) {                                      // sdf_ao(hit = (origin a, normal b))
        r[0] = scene_ao(F, R, n, a, b, w);
    } else if (FN == SE_SHADOW) {                                  // sdf_shadow(ray = (a, b)), whatever the block's shadow switch says
        r[0] = scene_shadow(F, R, n, a, b, w);
    } else if (FN == SE_ILLUMINATE) {                              // illuminate(hit = (origin a, normal b, material q[6]), ao q[7], sh q[8])
        const v3 lit = F.view != 0 ? b : scene_illuminate<true>(F, R, a, b, se_int(q[6]), q[7], q[8]);   // :217-219 compiled in
        r[0] = lit.x; r[1] = lit.y; r[2] = lit.z;
    } else {                                                       // render_impl / render over the ray (a, b)
        v3 rgb;
        float t;
        const int mat = scene_pixel(F, R, a, b, w, rgb, t);
        if (FN == SE_RENDER) rgb = scene_fog(F, a.y, b.y, rgb, t);
        r[0] = rgb.x; r[1] = rgb.y; r[2] = rgb.z; r[3] = t;
        if (FN == SE_RENDER_IMPL) r[4] = (float)mat;
    }
}

// PLAIN, WIT, counts: sbx_witness.h witnessed_elements
template <int FN, bool PLAIN, int WIT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(se_min_waves(FN), 8)))
k_sdf_scene_eval_fn(FrameSdfScene F, const float* __restrict__ in, float* __restrict__ out, size_t n, unsigned* __restrict__ counts) {
    __shared__ FrameSdfScene Fs;
    lds_frame_fill<FrameSdfScene, 64>(Fs);
    const SdfRd R = {(SdfKarg)__builtin_amdgcn_kernarg_segment_ptr(), &Fs};
    witnessed_elements<se_in_width(FN), 0, se_out_width(FN), PLAIN, WIT, SE_WORDS>(in, out, n, counts,
        [&](auto, const auto& q, auto& w, auto& r) { se_element<FN>(F, R, q, w, r); });
}

template <int FN>
static void se_launch(const FrameSdfScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    witness_dispatch<1>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_sdf_scene_eval_fn<FN, !cull.value, wit.value>), grid, dim3(64), 0, s, F, in, out, n, counts);
    });
}

// fn: SE_* in the order of sbx_eval.hip's names.  F: build_sdf_scene of the caller's validated block (its camera is not read).
// variant: witness_dispatch's.  n in 1 ... 2^31.
void launch_sdf_scene_eval_fn(int fn, const FrameSdfScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    switch (fn) {
    case SE_SDF: se_launch<SE_SDF>(F, variant, in, out, n, counts, s); break;
    case SE_NORMAL: se_launch<SE_NORMAL>(F, variant, in, out, n, counts, s); break;
    case SE_AO: se_launch<SE_AO>(F, variant, in, out, n, counts, s); break;
    case SE_SHADOW: se_launch<SE_SHADOW>(F, variant, in, out, n, counts, s); break;
    case SE_ILLUMINATE: se_launch<SE_ILLUMINATE>(F, variant, in, out, n, counts, s); break;
    case SE_RENDER_IMPL: se_launch<SE_RENDER_IMPL>(F, variant, in, out, n, counts, s); break;
    default: se_launch<SE_RENDER>(F, variant, in, out, n, counts, s); break;
    }
}

}  // namespace sbx
