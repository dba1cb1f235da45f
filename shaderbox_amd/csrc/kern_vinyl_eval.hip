// shaderbox_amd/csrc/kern_vinyl_eval.hip — sbx_vinyl_eval: the deck's field, normal, soft shadow, shading and trace (src/app_vinyl.h: sdf
// :251-259, sdf_normal :261-272, sdf_shadow :381-405, illuminate :287-379, render :407-458) over the caller's points and rays under the
// caller's deck (include/sbx.h sbx_aux_vinyl_deck).  No camera, no u_res, no sRGB.
//
// k_vinyl_eval: the element wave of sbx_witness.h (witnessed_elements: the form of a wave, the witness re-run, loads and stores) over
// k_vinyl's device functions (sbx_vinyl.h), the FrameVinyl that build_vinyl_deck (sbx_frames.hip) makes of the block, and the
// VinylShade beside it.  What is its own:
//   THE BOUND'S REASONS.  k_vinyl's culls and hardware min / max are proved for finite frame constants and finite points of bounded
//     scale (sbx_vinyl.h, at the top; vinyl_deck_tame, the camera's fields ignored, decides PLAIN, whose unions are compare-and-select).
//     A NaN or inf coordinate makes primitives NaN as FIRST operands of the unions, where v_min_f32 and the spec's select differ, and
//     makes a cull's comparison false where the member it skips would have been the union's NaN.  Within 1e4 per coordinate of points
//     and directions a march point stays within 1e4 + 1e4 (40 + 4.1e5) < 4.2e9 and a shadow point of "render" within
//     4.2e9 + 1e4 (5 + 4.3e9) < 4.4e13 — t leaves the loops beyond 40 and 5, and one step adds at most the field's value, which is at
//     most |point| + 10 — whose squares (2e27) are inside binary32.  The material id of "illuminate" is not a coordinate and is not
//     tested: it only selects a branch and a colour.  A point on a cylinder's axis or a sphere's centre records; sbx_debug_vinyl_eval
//     counts both kinds of wave.
//   THE FRAME BLOCK IN LDS, as k_vinyl (sbx_ldsframe.h): ~220 floats do not fit the SGPR file, an SGPR operand halves the VALU's issue
//     rate on gfx950, and the volatile per-use loads keep nothing alive across the march.  The block is the kernel's first argument;
//     the 19 words of the shading data are the second and stay scalar (read once per element, after the march).
//   sdf_normal's SIX CALLS each keep their own cull (the six points differ; a valid cull returns the full union's bits for its own
//     point) and its normalize is the IEEE one in every form: on a flat face two of the three differences are exactly 0, which the
//     witnessed normalize would record, and a wave must not re-run six fields for that (sbx_vinyl.h vinyl_normal).
//   int() OF THE MATERIAL ID ("illuminate", as :439 does): toward zero, saturating, a NaN gives 0 (include/sbx.h) — what
//     v_cvt_i32_f32 does, stated in C++ (`ve_int`) because the language leaves an out-of-range conversion undefined.
//   THE WAVE BOUND: ve_min_waves below, chosen so that no default instantiation spills (tools/kernel_resources.py).
#include "sbx_vinyl.h"

#ifndef VE_MIN_WAVES
#define VE_MIN_WAVES 3
#endif

namespace sbx {

enum { VE_SDF = 0, VE_NORMAL = 1, VE_SHADOW = 2, VE_ILLUMINATE = 3, VE_RENDER = 4 };

__device__ __forceinline__ int ve_int(float x) {
    if (x != x) return 0;
    return (int)fmin_(fmax_(x, -2147483648.f), 2147483520.f);      // (2^31 - 128: the largest binary32 below 2^31)
}

// The wave bound of an instantiation.  Every form but PLAIN holds the plain statement too (for its untame waves), and the plain field
// inside a march loop — every member of the union live at once — takes ~173 VGPRs, as k_vinyl's does: under a bound of 3 waves
// (168 VGPRs) "sdf_shadow" and "render" spill 16-68 bytes and the plain "sdf_normal" 3 KB, so those take 2 waves and spill nothing.
// (The PLAIN "sdf_normal", six plain fields the scheduler interleaves, is the one instantiation with scratch: 2.7 KB at 2 waves, 1.7 KB
// at the 1 it takes.  It is sbx_set_variant 1's kernel, run by the parity sweeps only; no default form has any.)
constexpr int ve_min_waves(int fn, bool plain) {
    return (plain && fn == VE_NORMAL) ? 1 : (fn == VE_SHADOW || fn == VE_RENDER || plain) ? 2 : VE_MIN_WAVES;
}

constexpr int ve_in_width(int fn) { return fn <= VE_NORMAL ? 3 : fn == VE_ILLUMINATE ? 7 : 6; }
constexpr int ve_out_width(int fn) { return fn == VE_SDF ? 2 : fn == VE_SHADOW ? 1 : fn == VE_RENDER ? 5 : 3; }

// one element of FN with sdf()'s CULL and the roots of witness `w`; q = its inputs, r = its outputs
template <int FN, bool CULL, class W>
__device__ __forceinline__ void ve_element(const FrameVinyl& F, const FrameVinyl& Fs, const VinylShade& D, const float (&q)[ELEM_WORDS],
                                           W& w, float (&r)[ELEM_WORDS]) {
    const v3 a = V3(q[0], q[1], q[2]), b = V3(q[3], q[4], q[5]);
    const ShadeDeck S{D};
    if (FN == VE_SDF) {
        const D2 d = vinyl_sdf<CULL>(Fs, a, w);
        r[0] = d.d; r[1] = d.m;
    } else if (FN == VE_NORMAL) {
        const v3 nrm = vinyl_normal<CULL>(Fs, a, w);
        r[0] = nrm.x; r[1] = nrm.y; r[2] = nrm.z;
    } else if (FN == VE_SHADOW) {
        r[0] = vinyl_shadow<CULL>(Fs, a, b, w);
    } else if (FN == VE_ILLUMINATE) {
        const v3 lit = vinyl_illuminate<CULL, VINYL_DECK>(F, Fs, S, a, b, ve_int(q[6]), w);
        r[0] = lit.x; r[1] = lit.y; r[2] = lit.z;
    } else {                                                       // render :407-458 over the caller's ray
        v3 color = V3(1, 1, 1);                                    // background :15-18
        float t = 0.f;
        bool hit = false;
        int mat = 0;
        v3 p = V3(0, 0, 0);
        vinyl_trace<CULL>(Fs, a, b, 60, w, t, hit, mat, p);
        if (hit) {
            const float sh = vinyl_shadow<CULL>(Fs, p + F.sun_dir * 0.05f, F.sun_dir, w);
            color = vinyl_illuminate<CULL, VINYL_DECK>(F, Fs, S, a, p, mat, w) * sh;
        }
        r[0] = color.x; r[1] = color.y; r[2] = color.z; r[3] = t; r[4] = hit ? (float)mat : 0.f;
    }
}

// PLAIN, WIT, counts: sbx_witness.h witnessed_elements
template <int FN, bool PLAIN, int WIT>
__global__ void __launch_bounds__(64, ve_min_waves(FN, PLAIN)) k_vinyl_eval(FrameVinyl F, VinylShade D, const float* __restrict__ in,
                                                                          float* __restrict__ out, size_t n, unsigned* __restrict__ counts) {
    constexpr int WIN = ve_in_width(FN);
    constexpr int WPOS = FN == VE_ILLUMINATE ? 6 : WIN;            // the inputs that are coordinates
    __shared__ FrameVinyl Fs;
    lds_frame_fill<FrameVinyl, 64>(Fs);
    witnessed_elements<WIN, WPOS, ve_out_width(FN), PLAIN, WIT>(in, out, n, counts,
        [&](auto cull, const auto& q, auto& w, auto& r) { ve_element<FN, cull.value>(F, Fs, D, q, w, r); });
}

template <int FN>
static void ve_launch(const FrameVinyl& F, const VinylShade& D, int variant, const float* in, float* out, size_t n, unsigned* counts,
                      hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    witness_dispatch<1>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_vinyl_eval<FN, !cull.value, wit.value>), grid, dim3(64), 0, s, F, D, in, out, n, counts);
    });
}

// fn: VE_* in the order of sbx_eval.hip's names.  F, D: build_vinyl_deck / vinyl_shade_of the caller's block (F's camera is not read).
// variant: witness_dispatch's.  n in 1 ... 2^31.
void launch_vinyl_eval(int fn, const FrameVinyl& F, const VinylShade& D, int variant, const float* in, float* out, size_t n,
                       unsigned* counts, hipStream_t s) {
    switch (fn) {
    case VE_SDF: ve_launch<VE_SDF>(F, D, variant, in, out, n, counts, s); break;
    case VE_NORMAL: ve_launch<VE_NORMAL>(F, D, variant, in, out, n, counts, s); break;
    case VE_SHADOW: ve_launch<VE_SHADOW>(F, D, variant, in, out, n, counts, s); break;
    case VE_ILLUMINATE: ve_launch<VE_ILLUMINATE>(F, D, variant, in, out, n, counts, s); break;
    default: ve_launch<VE_RENDER>(F, D, variant, in, out, n, counts, s); break;
    }
}

}  // namespace sbx
