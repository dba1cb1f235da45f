// shaderbox_amd/csrc/kern_vinyl.hip — APP_VINYL: turntable SDF with anisotropic (Ward-like) vinyl shading.
//
// Follows /root/reference/src/app_vinyl.h with the C++ build's 60 march steps (:411-416; GLSL uses 180),
// SHADERTOY undefined: sdf_logo :68-85, sdf_platter :87-125, sdf_tonearm :127-255, sdf :257-265, sdf_normal
// :267-278, illuminate :293-377, sdf_shadow :379-404, render :406-457.  Everything that depends only on u_time
// (platter and wobble rotations, the tonearm's constant-angle rotations, capsule/Bezier/cylinder frames) is in
// FrameVinyl.  SURVEY.md §8f row 4; the reference has no known answers for this app (parity vs oracle only).
#include "sbx_vinyl.h"

#ifndef VI_MIN_WAVES
#define VI_MIN_WAVES 5     // 3840x2160: 3 waves (134 VGPRs) 4.03 ms, 4 waves 3.85, 5 waves (96 VGPRs, spills outside the march) 3.71
#endif

namespace sbx {

// The wave bound of an instantiation.  The shipped build keeps VI_MIN_WAVES for every form, its plain form (no culling: every member
// live at once) with the 312 bytes of scratch that bound costs it; the plain forms of the other builds take 2 waves (173 VGPRs) and
// spill nothing.
constexpr int vinyl_min_waves(bool cull, int build) { return (!cull && build != VINYL_DEFAULT) ? 2 : VI_MIN_WAVES; }

template <bool CULL, int WIT, int BUILD>      // WIT: sbx_witness.h `witnessed`
__global__ void __launch_bounds__(WG_THREADS, vinyl_min_waves(CULL, BUILD)) k_vinyl(FrameVinyl F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
#if VI_LDS_FRAME
    // the frame block (~220 floats of rotations and primitive frames) in LDS: sbx_ldsframe.h
    __shared__ FrameVinyl Fs;
    lds_frame_fill<FrameVinyl, WG_THREADS>(Fs);
#define VI_FS Fs
#else
#define VI_FS F
#endif
    const Pixel px = pixel_of_thread(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    v3 color;
    witnessed<WIT>(true, [&](auto& w) { vinyl_pixel<CULL, BUILD>(F, VI_FS, ShadeLit{}, pc, w, color); });
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(color));
}

dim3 vinyl_grid(const RowMap& M) { return grid_for(M); }

template <int BUILD>
static void launch_vinyl_build(const FrameVinyl& F, const RowMap& M, float* out, hipStream_t s, int variant) {
    witness_dispatch<VI_WITNESS>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_vinyl<cull.value, wit.value, BUILD>), grid_for(M), dim3(WG_THREADS), 0, s, F, M, out);
    });
}
// build: VINYL_* (sbx_frame.h).  VINYL_CLOSEUP is a frame block (build_vinyl), not a kernel: the shipped instantiations run over it.
void launch_vinyl(const FrameVinyl& F, const RowMap& M, float* out, hipStream_t s, int variant, int build) {
    switch (build) {
    case VINYL_RIDGES: launch_vinyl_build<VINYL_RIDGES>(F, M, out, s, variant); break;
    case VINYL_NOSHADOW: launch_vinyl_build<VINYL_NOSHADOW>(F, M, out, s, variant); break;
    default: launch_vinyl_build<VINYL_DEFAULT>(F, M, out, s, variant); break;
    }
}

// SBX_APP_VINYL_DECK: the shipped pixel (VINYL_DECK: the hit block of VINYL_DEFAULT) with illuminate's five colours, Ward constants and
// shininess read from D, an argument of its own AFTER the frame block (lds_frame_fill copies the first argument) — a kernel of its
// own, so that k_vinyl's argument list and every shipped instantiation stay what they were (sbx_frame.h VinylShade says why).
template <bool CULL, int WIT>
__global__ void __launch_bounds__(WG_THREADS, vinyl_min_waves(CULL, VINYL_DECK)) k_vinyl_deck(FrameVinyl F, VinylShade D, RowMap M,
                                                                                             float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
#if VI_LDS_FRAME
    __shared__ FrameVinyl Fs;
    lds_frame_fill<FrameVinyl, WG_THREADS>(Fs);
#endif
    const Pixel px = pixel_of_thread(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    const ShadeDeck S{D};
    v3 color;
    witnessed<WIT>(true, [&](auto& w) { vinyl_pixel<CULL, VINYL_DECK>(F, VI_FS, S, pc, w, color); });
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(color));
}

// variant as launch_vinyl's; the caller has already turned an untame deck into 1 (sbx_frames.hip vinyl_deck_tame)
void launch_vinyl_deck(const FrameVinyl& F, const VinylShade& D, const RowMap& M, float* out, hipStream_t s, int variant) {
    witness_dispatch<VI_WITNESS>(variant, [&](auto cull, auto wit) {
        hipLaunchKernelGGL((k_vinyl_deck<cull.value, wit.value>), grid_for(M), dim3(WG_THREADS), 0, s, F, D, M, out);
    });
}

}  // namespace sbx
