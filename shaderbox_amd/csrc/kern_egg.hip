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
// The device functions (the cull sphere, sdf(), the shadow march, the trace's steps) are csrc/sbx_egg.h's, shared with k_egg_eval;
// SBX_APP_EGG_POSE is this kernel over the frame of the caller's pose (sbx_frames.hip build_egg_pose).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "sbx_device.h"
#include "sbx_egg.h"

#ifndef EGG_TW
#define EGG_TW 16          // wave tile EGG_TW x 64/EGG_TW pixels (profiles/r01_tile_shapes.txt)
#endif
#ifndef EGG_TX
#define EGG_TX 1           // waves per workgroup: 1 (4: the same single launch, 7 % slower with frames in flight at 1080p, 3 % at 4K;
#endif                     // census round 6: 4500 instead of 5900 waves resident — a workgroup's slots come back all at once)

namespace sbx {

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

// WIT: sbx_witness.h `witnessed` (0 = IEEE roots; 1 = witnessed roots, the shipped form; 2 = the witness's test edge)
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
    witnessed<WIT>(true, [&](auto& w) { egg_pixel<CULL, BUILD>(F, pc, w, color, depth, st_trace, st_shadow); });
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
    // (a caller's camera, SBX_APP_EGG_POSE: fov = 0 or tiny divides to inf or beyond an int — NaN fails the test too — plain order)
    auto small = [](float v) { return std::fabs(v) <= 1e9f; };
    if (!(small(xa) && small(xb) && small(ya) && small(yb))) return none;
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
    witness_dispatch<EGG_WITNESS>(variant, [&](auto cull, auto wit) { launch_egg_t<cull.value, wit.value, BUILD>(F, M, out, s, grid, hot, pad); });
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
