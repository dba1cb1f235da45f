// shaderbox_amd/csrc/kern_sdf_scene.hip — SBX_APP_SDF_SCENE and sbx_sdf_eval: src/sdf.h over the CALLER'S field.
//
// The renderer is app_sdf_ao.h's — render_impl :245-285, sdf_normal :152-163, sdf_ao :165-181, sdf_shadow :183-207, illuminate :211-243,
// render (height fog) :287-311 — with sdf(pos) an interpreter over the postfix program of include/sbx.h sbx_aux_sdf_scene, and the
// block's values where that header has literals.  k_sdf_scene_eval is the same interpreter over a point list.  The device functions
// themselves are in sbx_sdf_scene.h, which kern_sdf_scene_eval.hip (sbx_sdf_scene_eval) runs over the caller's elements too.
//
// CONTROL FLOW.  The program is the same for every lane, so everything that steers the interpreter — n_instr, op, rot_axis, the
// renderer's switches — is read from the KERNEL ARGUMENT: op and rot_axis as one word per instruction through the segment's
// constant-address-space pointer, a scalar load at a uniform dynamic offset, then scalar bit tests and branches; no lane ever diverges
// inside sdf().  The op is ONE BIT of that word (sbx_frame.h sdf_op_bit) and the dispatch a chain of bit tests — box first, then the
// operators and OBJECT behind one mask, then the other primitives — in which every case is whole and ends in its own stack move:
// 1.87 ms on the ramp block at 3840x2160.  With the op as a number the compiler folds any chain of compares into a switch tree
// joined by boolean flags: 2.16 ms as a switch, 2.64 ms as a chain of compares; all 32 control bytes held in SGPRs and shifted out,
// no load per instruction, 2.21 ms.  The price of the chain: a program of many late kinds pays for the tests
// before them (the seeded 32-instruction scene 5.15 against 4.72 ms under the switch).  The vector unit is not the bound: the
// witnessed roots change nothing.
// The operands (offset, sin / cos, p[]) come from the workgroup's LDS copy of the block (OPERANDS_LDS = 1: every lane one address,
// VGPR operands) or from the kernel-argument segment through its constant-address-space pointer (0: scalar loads at a uniform dynamic
// offset, SGPR operands); profiles/sdf_scene_timing.txt has both.  The materials are indexed per lane and always come from the LDS copy.
// The value stack is four named registers moved on push and pop; no private array is indexed dynamically anywhere (scratch 0).
// sdf() has four call sites per pass — march, the six normal taps as one loop, the five AO taps as one loop, the shadow march — so
// that the interpreter's body, eight primitives wide, is not instantiated fourteen times.
//
// CALLER'S NUMBERS.  What carries over from k_sdf_ao / sbx_sdf.h to values that are no longer this project's literals:
//   - Wit<true>'s square roots (sbx_witness.h) need nothing: a lane RECORDS every argument outside the interval the fast form was
//     compared on and the wave re-runs the pixel with the IEEE roots.
//   - the HW min / max forms, ao_pipe_far and bezier_far are proofs about the shipped scenes (finite points, members inside known
//     boxes): not used.  Every min / max is the spec's compare-and-select (fmin_ / fmax_).
//   - sd_capsule's quotient is the IEEE division by dot(ab, ab) (div_by is not the IEEE quotient where the quotient is subnormal,
//     sbx_math.h); normalize(v) is three IEEE divisions by the root, on the device (primary ray, sdf_normal) and on the host (the camera
//     and the instruction frames), for the same reason.
//   - the host-evaluated instruction frames hold what the reference computes per call from the primitive's own arguments, by the same
//     binary32 operations (sbx_frame.h SdfOp).
#include "sbx_sdf_scene.h"

#ifndef SDF_SCENE_MIN_WAVES
#define SDF_SCENE_MIN_WAVES 4
#endif
#ifndef SDF_SCENE_WITNESS
#define SDF_SCENE_WITNESS 1
#endif

namespace sbx {

// SdfRd, scene_sdf and the renderer's functions up to scene_pixel (render_impl :245-285) and scene_fog: sbx_sdf_scene.h, which
// k_sdf_scene_eval_fn (kern_sdf_scene_eval.hip) runs over the caller's elements too.

template <int WIT>   // sbx_witness.h `witnessed`
__global__ void __launch_bounds__(WG_THREADS, SDF_SCENE_MIN_WAVES) k_sdf_scene(FrameSdfScene F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
    __shared__ FrameSdfScene Fs;
    lds_frame_fill<FrameSdfScene, WG_THREADS>(Fs);
    const SdfRd R = {(SdfKarg)__builtin_amdgcn_kernarg_segment_ptr(), &Fs};
    const Pixel px = pixel_of_thread(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    const v3 ro = F.cam.eye;
    const v3 rd = normalize_ieee(F.cam.fwd + F.cam.up * pc.y + F.cam.right * pc.x);   // util.h:17
    v3 rgb;
    float t;
    witnessed<WIT>(true, [&](auto& w) { scene_pixel(F, R, ro, rd, w, rgb, t); });
    const v3 col = scene_fog(F, ro.y, rd.y, rgb, t);               // :287-311 (t is the march length at exit)
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(col));
}

// sbx_sdf_eval: sdf(pos) at n points, out = (distance, material id as float).  Only n_instr and prog of F are read.
template <int WIT>
__global__ void __launch_bounds__(WG_THREADS) k_sdf_scene_eval(FrameSdfScene F, const float* __restrict__ xyz, float* __restrict__ out, size_t npoints) {
    __shared__ FrameSdfScene Fs;
    lds_frame_fill<FrameSdfScene, WG_THREADS>(Fs);
    const SdfRd R = {(SdfKarg)__builtin_amdgcn_kernarg_segment_ptr(), &Fs};
    const size_t i = (size_t)blockIdx.x * WG_THREADS + threadIdx.x;
    if (i >= npoints) return;
    const v3 pos = V3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    D2 d;
    witnessed<WIT>(true, [&](auto& w) { d = scene_sdf(F, R, F.n_instr, pos, w); });
    out[2 * i] = d.d;
    out[2 * i + 1] = d.m;
}

// variant: witness_dispatch's (there is nothing to cull: 1 and 3 are both the IEEE roots)
void launch_sdf_scene(const FrameSdfScene& F, const RowMap& M, float* out, hipStream_t s, int variant) {
    witness_dispatch<SDF_SCENE_WITNESS>(variant, [&](auto, auto wit) {
        hipLaunchKernelGGL((k_sdf_scene<wit.value>), grid_for(M), dim3(WG_THREADS), 0, s, F, M, out);
    });
}

void launch_sdf_scene_eval(const FrameSdfScene& F, const float* xyz, float* out, size_t n, hipStream_t s, int variant) {
    const dim3 grid((unsigned)((n + WG_THREADS - 1) / WG_THREADS));
    witness_dispatch<SDF_SCENE_WITNESS>(variant, [&](auto, auto wit) {
        hipLaunchKernelGGL((k_sdf_scene_eval<wit.value>), grid, dim3(WG_THREADS), 0, s, F, xyz, out, n);
    });
}

}  // namespace sbx
