// shaderbox_amd/csrc/kern_egg_eval.hip — sbx_egg_eval: the egg's field, normal, shadow march and trace (src/app_egg.h as shipped: sdf
// :38-144, sdf_normal :146-157, shadowmarch :161-186, render_scene :190-231 with `depth` of :188) over the caller's points and rays
// under the caller's pose, and the two bone IK solver (src/IK.h:5-52) over the caller's goals (include/sbx.h).  No camera, no u_res.
//
// k_egg_eval: the element wave of sbx_witness.h (witnessed_elements: the form of a wave, the witness re-run, loads and stores) over
// k_egg's device functions (sbx_egg.h) and the FrameEgg that build_egg_pose (sbx_frames.hip) makes of the block.  What is its own:
//   THE BOUND'S REASONS.  k_egg's culls and witnessed roots are proved for finite frame constants and sample points of the scene's
//     scale (sbx_egg.h, sbx_sdf.h; sbx_frames.hip egg_pose_tame decides PLAIN).  A cull CLAIMS "the union is the ground plane", which
//     is false where the full evaluation would return a NaN member last (a NaN or inf coordinate of P: 0 * inf in the turntable
//     product), and a coordinate near 2^64 overflows the squared lengths the culls compare.  Within 1e4 per coordinate a march stays
//     within |P| <= 1e4 + 1.8e4 * (15 + |d|) < 2^33 — t leaves the loops beyond 15 and 10, and one step adds at most the ground's
//     distance — whose squares are far inside binary32.  Off-axis points never record; a point on a primitive's axis or centre does,
//     which sbx_debug_egg_eval counts.
//   VGPR CONSTANTS.  As k_egg (EGG_VCONST = 1): the turntable matrix and the cull sphere, read first by every sdf() call, are forced
//     into VGPRs — a VALU instruction with an SGPR source issues at half rate on gfx950 (profiles/r02_ubench_issue.txt).  The toe
//     midpoints stay scalar (k_egg's EGG_VCONST > 1 lost there, and the register budget here is the same code's).
//   sdf_normal's SIX CALLS each keep their own cull: the six points differ, a valid cull returns the full union's bits for its own
//     point, and one shared test on p with a margin of .05 would be a new bound to prove for nothing measurable.
//     Its final normalize is the IEEE one in every form: over flat ground two of the three differences are exactly 0, which the
//     witnessed normalize records (a component whose square is not normal), and a wave must not re-run six fields for that.
// k_ik_eval: "ik_solver", a kernel of its own — 44 B per element and some thirty operations: bandwidth-bound, so the spec's division,
//     square root and normalisation as they stand (no witness, no short form), and the zero terms of mul(rot, v) kept as
//     sbx_frames.hip's host version keeps them (0 * inf is a NaN, (-0) + 0 is +0).  256 lanes per workgroup.
#include "sbx_egg.h"

namespace sbx {

enum { EE_SDF = 0, EE_NORMAL = 1, EE_SHADOW = 2, EE_RENDER = 3 };

constexpr int ee_in_width(int fn) { return fn <= EE_NORMAL ? 3 : 6; }
constexpr int ee_out_width(int fn) { return fn == EE_SDF ? 2 : fn == EE_NORMAL ? 3 : fn == EE_SHADOW ? 1 : 4; }

// one element of FN with sdf()'s CULL and the roots of witness `w`; q = its inputs, r = its outputs
template <int FN, bool CULL, class W>
__device__ __forceinline__ void ee_element(const FrameEgg& F, const float (&q)[ELEM_WORDS], W& w, float (&r)[ELEM_WORDS]) {
    const v3 a = V3(q[0], q[1], q[2]), b = V3(q[3], q[4], q[5]);
    if (FN == EE_SDF) {
        const D2 d = egg_sdf<CULL, EGG_DEFAULT>(F, a, w);
        r[0] = d.d; r[1] = d.m;
    } else if (FN == EE_NORMAL) {                                  // :146-157
        const float dt = 0.05f;
        const v3 x = V3(dt, 0, 0), y = V3(0, dt, 0), z = V3(0, 0, dt);
        const float gx = egg_sdf<CULL, EGG_DEFAULT>(F, a + x, w).d - egg_sdf<CULL, EGG_DEFAULT>(F, a - x, w).d;
        const float gy = egg_sdf<CULL, EGG_DEFAULT>(F, a + y, w).d - egg_sdf<CULL, EGG_DEFAULT>(F, a - y, w).d;
        const float gz = egg_sdf<CULL, EGG_DEFAULT>(F, a + z, w).d - egg_sdf<CULL, EGG_DEFAULT>(F, a - z, w).d;
        const v3 nrm = normalize(V3(gx, gy, gz));                  // (the IEEE form, whatever the witness: see the note at the top)
        r[0] = nrm.x; r[1] = nrm.y; r[2] = nrm.z;
    } else if (FN == EE_SHADOW) {
        r[0] = egg_shadowmarch<CULL, EGG_DEFAULT>(F, a, b, w);
    } else {                                                       // render_scene :190-231, k_egg's egg_pixel over the caller's ray
        float depth = -1e8f;                                       // :188, fresh per element
        v3 color = V3(.1f, .1f, .7f);                              // background :9-12
        EggRay ray;
        ray.t = 0.f; ray.done = false; ray.hit = false; ray.mat = 0; ray.hp = V3(0, 0, 0); ray.steps = 0;
        egg_trace_steps<CULL, EGG_DEFAULT>(F, a, b, ray, w);
        if (ray.hit) {
            if (ray.mat == 1 || ray.mat == 2) depth = fmax_(depth, ray.hp.z);
            float s = 1.f;
            if (ray.mat == 3) {
                const v3 sh_dir = V3(0, 1, 1);
                s = egg_shadowmarch<CULL, EGG_DEFAULT>(F, ray.hp + sh_dir * 0.05f, sh_dir, w);
            }
            v3 base = V3(1, 1, 1);                                 // illuminate :29-35
            if (ray.mat == 3) base = V3(13.f / 255.f, 104.f / 255.f, 0.f / 255.f);
            else if (ray.mat == 1) base = V3(0.9f, 0.95f, 0.95f);
            else if (ray.mat == 2) base = V3(.2f, .2f, .2f);
            color = base * s;
        }
        r[0] = color.x; r[1] = color.y; r[2] = color.z; r[3] = depth;
    }
}

// PLAIN, WIT, counts: sbx_witness.h witnessed_elements
template <int FN, bool PLAIN, int WIT>
__global__ void __launch_bounds__(64) k_egg_eval(FrameEgg F, const float* __restrict__ in, float* __restrict__ out, size_t n,
                                                 unsigned* __restrict__ counts) {
    asm volatile("" : "+v"(F.rot_y.c0.x), "+v"(F.rot_y.c0.y), "+v"(F.rot_y.c0.z), "+v"(F.rot_y.c1.x), "+v"(F.rot_y.c1.y),
                      "+v"(F.rot_y.c1.z), "+v"(F.rot_y.c2.x), "+v"(F.rot_y.c2.y), "+v"(F.rot_y.c2.z));
    asm volatile("" : "+v"(F.ocw.x), "+v"(F.ocw.y), "+v"(F.ocw.z), "+v"(F.orad));
    witnessed_elements<ee_in_width(FN), ee_in_width(FN), ee_out_width(FN), PLAIN, WIT>(in, out, n, counts,
        [&](auto cull, const auto& q, auto& w, auto& r) { ee_element<FN, cull.value>(F, q, w, r); });
}

template <int FN>
static void ee_launch(const FrameEgg& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    witness_dispatch<1>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_egg_eval<FN, !cull.value, wit.value>), grid, dim3(64), 0, s, F, in, out, n, counts);
    });
}

// fn: EE_* in the order of sbx_eval.hip's names after "ik_solver".  F: build_egg_pose of the caller's block (its camera is not read).
// variant: witness_dispatch's.  n in 1 ... 2^31.
void launch_egg_eval(int fn, const FrameEgg& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    switch (fn) {
    case EE_SDF: ee_launch<EE_SDF>(F, variant, in, out, n, counts, s); break;
    case EE_NORMAL: ee_launch<EE_NORMAL>(F, variant, in, out, n, counts, s); break;
    case EE_SHADOW: ee_launch<EE_SHADOW>(F, variant, in, out, n, counts, s); break;
    default: ee_launch<EE_RENDER>(F, variant, in, out, n, counts, s); break;
    }
}

// ik_solver(start, goal, L1, L2) IK.h:44-52 over ik_2_bone_centered_solver :18-41, statement by statement
__global__ void __launch_bounds__(256) k_ik_eval(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (!(i < n)) return;
    const float* e = in + 8 * i;
    const v3 start = V3(e[0], e[1], e[2]), goal_abs = V3(e[3], e[4], e[5]);
    const float L1 = e[6], L2 = e[7];
    const v3 goal = goal_abs - start;
    const float G = length(goal);
    const float cos_theta = (L1 * L1 + G * G - L2 * L2) / (2.f * L1 * G);
    const float sin_theta = sqrt_(1.f - cos_theta * cos_theta);
    const m3 rot = M3(cos_theta, -sin_theta, 0, sin_theta, cos_theta, 0, 0, 0, 1.f);
    const v3 knee = start + mul(rot, normalize(goal) * L1);
    out[3 * i] = knee.x; out[3 * i + 1] = knee.y; out[3 * i + 2] = knee.z;
}

void launch_ik_eval(const float* in, float* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_ik_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
}

}  // namespace sbx
