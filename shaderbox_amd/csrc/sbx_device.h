// shaderbox_amd/csrc/sbx_device.h — thread->pixel mapping and framebuffer store shared by the kernels.
//
// One thread per pixel.  A workgroup is 256 threads = 4 wave64; each wave owns a small pixel tile
// (8x8 by default, lane = ly*TW + lx) so that the rays of a wave stay coherent (same lattice cells,
// same march exits); the workgroup covers 4 tiles side by side.  Every lane stores one float4 (16 B):
// a wave writes full 128..512-byte row segments, fully coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include "sbx_frame.h"
#include "../../include/sbx_test.h"   // sbx_clouds_selection: the record launch_clouds fills

namespace sbx {

// Tile shape of a wave (TW x 64/TW pixels) is chosen per kernel from measurements on MI355X
// (profiles/r01_tile_shapes.txt): wide tiles suit APP_CLOUDS (a pixel row shares dir.y, hence march
// length and lit pattern), 16x4 suits APP_EGG, 8x8 the others.  Tile heights divide the 8-row blocks of the
// multi-GPU split.
#ifndef SBX_WG_WAVES
#define SBX_WG_WAVES 4
#endif
constexpr int WG_TILES_X = SBX_WG_WAVES, WG_THREADS = 64 * SBX_WG_WAVES;

#ifndef SBX_PIXEL_POINTS
#define SBX_PIXEL_POINTS 1     // A/B switches (tools/ab_build.py): the point-list and span forms of pixel_of compiled in
#endif
#ifndef SBX_PIXEL_SPANS
#define SBX_PIXEL_SPANS 1
#endif
struct Pixel { int x, y; size_t idx; bool valid; float fx, fy; };   // (fx, fy) = fragCoord: the pixel centre, or a listed point

// TOP_FIRST: workgroups are dispatched in increasing blockIdx (x fastest, then y); with TOP_FIRST the first ones take
// the TOP rows of the launch.  For APP_CLOUDS the bottom rows never march (src/app_clouds.h:212), so the launch then ends
// on its cheapest waves and the end-of-launch drain is not a few 100-step marches on a mostly empty chip.
// the tile a workgroup renders: its own index, or — with a dispatch-order table (RowMap.order) — the tile the table names (wave-uniform)
__device__ __forceinline__ void ordered_tile(const RowMap& M, int& bx, int& by) {
    if (M.order) {
        const unsigned t = M.order[by * (int)gridDim.x + bx];
        bx = (int)(t & 0xffffu);
        by = (int)(t >> 16);
    }
}
// a wave's duration into the cost table of the next frame's dispatch order (lane 0 of the workgroup's first wave; t0: s_memrealtime
// at the kernel's start)
// (the same for a kernel with an order of its own — APP_EGG's hot-first —: (bx, by) = the tile it hands to pixel_of.  Until this
// existed k_egg's costs were filed under the WORKGROUP's index, not the tile's: the table built from them was noise, and "the
// order loses 15 % on APP_EGG" was a measurement of that)
__device__ __forceinline__ void tile_cost_store_at(const RowMap& M, unsigned long long t0, int bx, int by) {
    if (M.cost && threadIdx.x == 0) {
        ordered_tile(M, bx, by);
        M.cost[by * (int)gridDim.x + bx] = (unsigned)(__builtin_amdgcn_s_memrealtime() - t0);
    }
}
__device__ __forceinline__ void tile_cost_store(const RowMap& M, unsigned long long t0) {
    if (M.cost && threadIdx.x == 0) {
        int bx = (int)blockIdx.x, by = (int)blockIdx.y;
        ordered_tile(M, bx, by);
        M.cost[by * (int)gridDim.x + bx] = (unsigned)(__builtin_amdgcn_s_memrealtime() - t0);
    }
}
template <int TW = 8, int TX = WG_TILES_X, bool TOP_FIRST = false>
__device__ __forceinline__ Pixel pixel_of(const RowMap& M, int tid, int bx, int by_in, int grid_y) {
    constexpr int TH = 64 / TW;
    const int lane = tid & 63, wave = tid >> 6;
    ordered_tile(M, bx, by_in);
    Pixel p;
    p.x = bx * (TW * TX) + wave * TW + (lane % TW);
    // (dispatching the block rows from the middle of the launch outwards — heaviest tiles first for centred scenes — LOSES:
    // EGG 1080p 0.54 -> 0.77 ms, VINYL 4K 3.73 -> 4.07: heavy waves that run together share their SIMDs' issue slots.
    // Re-measured after the hit block left the trace loop: one EGG 1080p launch 0.269 -> 0.241 ms, but 0.160 -> 0.168 ms per
    // frame with two in flight and 4K 0.632 -> 0.648 ms: a shorter tail, lower throughput.  Not in.)
    // (so does visiting the rows with a stride: APP_CLOUDS 4K 2.86 ms in row order, 2.87 / 2.91 / 3.41 with strides 7 / 37 / 269)
    const int by = TOP_FIRST ? (grid_y - 1 - by_in) : by_in;
    const int r = by * TH + (lane / TW);
    p.valid = (p.x < M.width) && (r < M.nrows);
    if (SBX_PIXEL_POINTS && M.frag) {                        // wave-uniform (a kernel argument): point list, see RowMap
        p.idx = (size_t)r * M.width + p.x;
        p.valid = p.valid && p.idx < (size_t)M.npoints;
        p.y = r;
        p.fx = p.valid ? M.frag[2 * p.idx] : .5f;
        p.fy = p.valid ? M.frag[2 * p.idx + 1] : .5f;
        return p;
    }
    p.y = row_to_y(M, r);
    if (SBX_PIXEL_SPANS && M.span_mode) {                    // wave-uniform: the span forms of the multi-GPU split, see RowMap
        const int yc = p.y < M.height ? p.y : M.height - 1;  // (rows past the frame are invalid anyway; keep the read in range)
        const int g = yc / M.block_rows;
        const int4 T = M.span[g];
        if (M.span_mode == 1) {
            p.x += T.x;
            p.valid = p.valid && p.x < T.y;
            p.idx = (size_t)T.z + (size_t)(yc - g * M.block_rows) * (size_t)(T.y - T.x) + (size_t)(p.x - T.x);
        } else if (M.span_mode == 3) {                       // a peer of the store exchange: its spans, at their place in the owner's frame
            p.valid = p.valid && p.x >= T.x && p.x < T.y;
            p.idx = (size_t)p.y * M.width + p.x;
        } else {
            p.valid = p.valid && (T.w == 0 || p.x < T.x || p.x >= T.y);
            p.idx = (size_t)p.y * M.width + p.x;
        }
        p.fx = (float)p.x + .5f;
        p.fy = (float)p.y + .5f;
        return p;
    }
    p.idx = (size_t)(M.in_place ? p.y : r) * M.width + p.x;
    p.fx = (float)p.x + .5f;                                 // fragCoord of pixel (x, y) is its centre
    p.fy = (float)p.y + .5f;
    return p;
}
template <int TW = 8, int TX = WG_TILES_X, bool TOP_FIRST = false>
__device__ __forceinline__ Pixel pixel_of_thread(const RowMap& M) {
    return pixel_of<TW, TX, TOP_FIRST>(M, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}
template <int TW = 8, int TX = WG_TILES_X>
inline dim3 grid_for(const RowMap& M) {
    constexpr int TH = 64 / TW, W = TW * TX;
    return dim3((M.width + W - 1) / W, (M.nrows + TH - 1) / TH);
}
// float -> UNORM8 by the Direct3D rule (the write into hlsltoy's R8G8B8A8_UNORM back buffer, util/hlsltoy/src/hlsltoy.cpp:79,192):
// NaN -> 0, clamp to [0, 1], scale by 255, add .5, truncate
__device__ __forceinline__ unsigned unorm8_(float v) {
    if (!(v > 0.f)) return 0u;                       // NaN, -x, -0, +0
    if (v > 1.f) v = 1.f;
    return (unsigned)(v * 255.f + .5f);
}
__device__ __forceinline__ void store_rgba(const RowMap& M, float* out, size_t idx, v3 c) {
    if (M.rgb == 1) {                                                          // wave-uniform (a kernel argument)
        float* o = out + idx * 3;                                              // 64 lanes: 768 contiguous bytes
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    } else if (M.rgb == 2) {                                                   // SBX_FORMAT_RGBA8: one 4-byte store per pixel, alpha 255
        reinterpret_cast<unsigned*>(out)[idx] = unorm8_(c.x) | (unorm8_(c.y) << 8) | (unorm8_(c.z) << 16) | 0xff000000u;
    } else if (M.rgb == 3) {                                                   // float4 pixels whose alpha is already in the frame: one
        float* o = out + idx * 4;                                              // three-dword store (the store exchange, sbx_shared_*:
        o[0] = c.x; o[1] = c.y; o[2] = c.z;                                    // 12 instead of 16 bytes per pixel over xGMI)
    } else {
        reinterpret_cast<float4*>(out)[idx] = make_float4(c.x, c.y, c.z, 1.0f);   // main.h:52
    }
}

// the four-channel form for apps whose alpha is not the constant 1 of main.h:52 (APP_2D: app_2d.h writes `color` itself, :108):
// float4 pixels as computed, or R8G8B8A8_UNORM words with unorm8_(alpha) in the top byte (what sbx_pack_unorm8 does with c.w).
// Three-channel outputs (RowMap.rgb 1 and 3) cannot hold such a pixel: their entry points refuse these apps on the host.
__device__ __forceinline__ void store_rgba4(const RowMap& M, float* out, size_t idx, float4 c) {
    if (M.rgb == 2) reinterpret_cast<unsigned*>(out)[idx] = unorm8_(c.x) | (unorm8_(c.y) << 8) | (unorm8_(c.z) << 16) | (unorm8_(c.w) << 24);
    else reinterpret_cast<float4*>(out)[idx] = c;
}

// launchers (one per app), defined next to their kernels
// APP_CLOUDS' lattice-hash table (kern_clouds.hip GTab; owned by the context, sbx_ytab.hip): tab[i] = hash1((float)(i - bias)) for
// 0 <= i < entries, covering the lattice indices [-range, range + 271] with CLOUDS_HASHTAB_GUARD entries of slack at both ends
struct CloudsHashTab { const float* tab = nullptr; int entries = 0, bias = 0, range = 0; };
constexpr int CLOUDS_HASHTAB_MIN_RANGE = 1 << 18;   // the smallest table (2 MB; the default frame's bound is 6.4e4)
constexpr int CLOUDS_HASHTAB_MAX_RANGE = 1 << 22;   // the largest (32 MB); a frame whose bound is beyond it keeps the LDS hash cache
constexpr int CLOUDS_HASHTAB_GUARD = 512;
constexpr int clouds_hashtab_entries(int range) { return 2 * range + 272 + 2 * CLOUDS_HASHTAB_GUARD; }
int clouds_hashtab_range(const FrameClouds& F, const RowMap& M, int build);   // the range the launch needs; 0: it does not take the table kernels
void launch_clouds_hashtab(float* tab, int entries, int bias, hipStream_t s);
// The kernel a launch takes, as a pure function of the frame (kern_clouds.hip): "a y table of ytab_rows rows is at hand" (0: none),
// "a ready hash table of range table_range is at hand" (0: none).  No device, no context; launch_clouds launches what this returns.
// view_table: "a ready view table of the frame's camera is at hand" (kern_clouds.hip "the context's view table"): taken only by a hash-table kernel
sbx_clouds_selection clouds_select(const FrameClouds& F, const RowMap& M, int variant, int build, int ytab_rows, int table_range,
                                   bool view_table = false);
// returns whether the launch took a hash-table kernel (only with `ht`: a READY table; taken iff it covers the frame's index bound).
// rec: the record of what was launched (sbx_test.h), written by the launcher itself; its `ytab` is ytab_kind where a y table was read
bool launch_clouds(const FrameClouds& F, const RowMap& M, float* out, hipStream_t s, int variant, void* ytab, int ytab_rows,
                   bool build_table, int build = CLOUDS_DEFAULT,    // build: CLOUDS_* (sbx_frame.h); build_table with CLOUDS_HEIGHT also
                   const CloudsHashTab* ht = nullptr,               // writes the steps' luminances behind the y rows
                   sbx_clouds_selection* rec = nullptr, int ytab_kind = 0,
                   const float4* vtab = nullptr);                   // vtab: a view table of F's camera that is READY on `s`, or NULL
// APP_CLOUDS' view table (kern_clouds.hip "the context's view table"; owned by the context, sbx_ytab.hip): 20 bytes per frame pixel
constexpr size_t CLOUDS_VIEWTAB_PIXEL_BYTES = 20;
void launch_clouds_viewtab(const FrameClouds& F, int width, int height, float4* tab, hipStream_t s);
bool clouds_viewtab_eligible(const FrameClouds& F, const RowMap& M, int build);   // the launch may read a view table (never: points, spans, ranks' strips, SKY_SPHERE, the y-z light march)
constexpr int CLOUDS_YTAB_ROWS = 4096;      // march steps covered by a y table of the ring (208 KB per table; beyond it the one big
                                            // table below, or in a capture the table-less kernels: 1100 steps at 4K took 48 ms without a table)
constexpr int CLOUDS_YTAB_STEP_BYTES = 48 + 4;   // per march step: its YRow and, behind the frame's rows, the HEIGHT build's luminance
constexpr int CLOUDS_YTAB_BYTES = CLOUDS_YTAB_ROWS * CLOUDS_YTAB_STEP_BYTES;
constexpr int CLOUDS_YTAB_BIG_MAX = 1 << 20;   // longest march served by the context's one on-demand table (52 MB); beyond it: the table-less kernels
constexpr int CLOUDS_YTAB_RING = 8;         // eager tables: one per REBUILD (key change), round robin; reuse of a slot waits
                                            // for the launches that may still read it (sbx_ytab.hip render_clouds)
constexpr int CLOUDS_YTAB_CAPTURE = 8;      // tables used only by launches recorded into a stream capture
void launch_clouds_tex(const FrameClouds& F, const RowMap& M, float* out, hipStream_t s, const float* shape_r, int shape_size,
                       const float* detail_r, int detail_size, const float* bounds);     // bounds: {lo1, hi1, lo2, hi2} of the texels, or NULL
void launch_minmax_r(const float* r, size_t n, unsigned* res, hipStream_t s);
float minmax_key_to_float(unsigned k);
void launch_extract_r(const float* rgba, float* r, size_t n, hipStream_t s);
void launch_tex3d_eval(int size, const float* rgba, const float* xyz, float* out, size_t n, hipStream_t s);
void launch_egg(const FrameEggStraight& F, const RowMap& M, float* out, hipStream_t s, int variant, int build = EGG_DEFAULT);   // build: EGG_* (sbx_frame.h), the one F was built for
void launch_raytracer(const FrameRaytracer& F, const RowMap& M, float* out, hipStream_t s, int variant, int build = RT_DEFAULT);   // build: RT_* (sbx_frame.h)
void launch_raytracer_scene(const FrameRtScene& F, const RowMap& M, float* out, hipStream_t s, int variant);   // SBX_APP_RAYTRACER_SCENE (kern_raytracer.hip)
// sbx_raytracer_eval (kern_raytracer_eval.hip k_raytracer_eval): fn 0 raytrace_iteration, 1 illuminate, 2 shadow, 3 render; variant:
// witness_dispatch's; counts: NULL, or two zeroed words (waves that took the witnessed roots only, waves that re-ran)
void launch_raytracer_eval(int fn, const FrameRtScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s);
// fin_ok = false: the caller has found the frame outside the domain of the FIN forms (SBX_APP_ATMOSPHERE_AIR's literal tier: a sun the
// written arguments do not admit, sbx_atmosphere.h "CALLER'S AIR"); the plain kernel then runs whatever else holds
void launch_atmosphere(const FrameAtmosphere& F, const RowMap& M, float* out, hipStream_t s, int precision = 0, bool fin_ok = true);
void launch_atmosphere_ground(const FrameAtmosphere& F, const RowMap& M, float* out, hipStream_t s, int precision, int variant, bool fin_ok = true);   // kern_atmosphere.hip
// SBX_APP_ATMOSPHERE_AIR (kern_atmosphere_air.hip k_atmosphere_air): the run-time tier (fast = true: tame blocks, the fast body on the
// waves whose rays are of the class) and the plain tier (false)
void launch_atmosphere_air(const FrameAtmosphere& F, const AtmAir& K, int view, bool fast, const RowMap& M, float* out, hipStream_t s);
void launch_sdf_ao(const FrameSdfAo& F, const RowMap& M, float* out, hipStream_t s, int variant, int build = 0);   // build: 1 / 2 = the shadow / normals builds (kern_sdf_ao.hip)
void launch_sdf_scene(const FrameSdfScene& F, const RowMap& M, float* out, hipStream_t s, int variant);   // SBX_APP_SDF_SCENE (kern_sdf_scene.hip)
void launch_sdf_scene_eval(const FrameSdfScene& F, const float* xyz, float* out, size_t n, hipStream_t s, int variant);   // sbx_sdf_eval
// sbx_sdf_scene_eval (kern_sdf_scene_eval.hip): fn = the index among its names; counts NULL or two zeroed words (witnessed / re-run waves)
void launch_sdf_scene_eval_fn(int fn, const FrameSdfScene& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s);
void launch_vinyl(const FrameVinyl& F, const RowMap& M, float* out, hipStream_t s, int variant, int build = VINYL_DEFAULT);   // build: VINYL_* (sbx_frame.h)
void launch_clouds_best(const FrameCloudsBest& F, const RowMap& M, float* out, hipStream_t s);
void launch_clouds_ue4(const FrameCloudsUe4& F, const RowMap& M, float* out, hipStream_t s);
void launch_planet(const FramePlanet& F, const RowMap& M, float* out, hipStream_t s, int variant, int build = PLANET_DEFAULT);   // build: PLANET_* (sbx_frame.h)
void launch_assemble(int width, int height, int block_rows, int nranks, int root_rounds, int rounds, int rows_max,
                     const float* gathered, float* frame, hipStream_t s, bool rgba8);
void launch_assemble_peers(int width, int height, int block_rows, int nranks, int root_rounds, int rounds, int rows_max,
                           int channels, const float* peers, float* frame, hipStream_t s);
hipError_t bind_fault_clouds(unsigned* word);
hipError_t bind_fault_clouds_ue4(unsigned* word);
// SBX_APP_PLANET_WORLD's run-time tier (kern_planet_world.hip k_planet_world): fast = a tame block under a variant other than 1
void launch_planet_world(const FramePlanetWorld& F, bool fast, const RowMap& M, float* out, hipStream_t s);
hipError_t bind_fault_planet_world(unsigned* word);
hipError_t bind_fault_planet(unsigned* word);
hipError_t bind_fault_planet_eval(unsigned* word);
void launch_raise_fault(unsigned code, hipStream_t s);
void launch_assemble_spans(int width, int height, int block_rows, const int4* span, const float* peers, size_t stride_pixels,
                           float* frame, hipStream_t s, bool rgba8);
void launch_pack_unorm8(int width, int rows, int flip, const float* in, unsigned char* out, hipStream_t s);
void launch_order_build(const unsigned* cost, unsigned* cls, unsigned* ghist, unsigned* order, int gx, int gy, hipStream_t s);
size_t order_build_scratch_words();   // tiles by cost, longest first (kern_util.hip)
// the grid each launcher uses for a map (the tile shapes are private to the kernel files): what a dispatch-order table is built for
dim3 clouds_grid(const RowMap& M);
dim3 egg_grid(const RowMap& M);
dim3 raytracer_grid(const RowMap& M);
dim3 atmosphere_grid(const RowMap& M);
dim3 planet_grid(const RowMap& M);
dim3 sdf_ao_grid(const RowMap& M);
dim3 vinyl_grid(const RowMap& M);
// SBX_APP_VINYL_DECK (kern_vinyl.hip k_vinyl_deck): the shipped pixel with illuminate's literals read from D; variant as launch_vinyl's
void launch_vinyl_deck(const FrameVinyl& F, const VinylShade& D, const RowMap& M, float* out, hipStream_t s, int variant);
dim3 clouds_best_grid(const RowMap& M);
dim3 clouds_ue4_grid(const RowMap& M);
bool launch_2d(const Frame2d& F, const RowMap& M, float* out, hipStream_t s, bool tex);   // false: a three-channel map (nothing launched)
void launch_unorm8_to_float4(const unsigned* in, float4* out, size_t n, hipStream_t s);
void launch_func(const FrameFunc& F, const RowMap& M, float* out, hipStream_t s, int variant);
void launch_func_table(float4* tab, hipStream_t s);   // APP_FUNC's hash table (kern_func.hip), func_table_bytes() of device memory
size_t func_table_bytes();
int launch_noise_eval(int fn, const float* xyz, const float* par, float* out, size_t n, hipStream_t s);
void launch_worley_volume(int size, float* out, hipStream_t s);
void launch_exp4k_eval(const float* a, float* out, size_t n, hipStream_t s);
// sbx_atmosphere_eval (kern_atmosphere.hip): fn 0 get_incident_light / 1 get_sun_light; plain = the plain kernel for every wave
void launch_atmosphere_eval(int fn, bool plain, const float* rays, const float* sun_dir, float* out, size_t n, unsigned* fast_waves, hipStream_t s);
// sbx_atmosphere_air_eval (kern_atmosphere_air.hip): the same under the caller's air; fast as launch_atmosphere_air's
void launch_atmosphere_air_eval(int fn, bool fast, const float* rays, const float* sun_dir, const AtmAir& K, float* out, size_t n, unsigned* fast_waves,
                                hipStream_t s);
// sbx_clouds_eval (kern_clouds_eval.hip): fn 0 render / 1 render_clouds / 2 render_sky_color / 3 density_func / 4 illuminate_volume over F =
// build_clouds of the caller's block; plain = the per-lane statement; ht = a hash table that is ready on `s`, or NULL; counts = NULL or two
// zeroed 64-bit device words for the counting instantiation
void launch_clouds_eval(int fn, const FrameClouds& F, bool plain, const CloudsHashTab* ht, const float* in, float* out, size_t n,
                        unsigned long long* counts, hipStream_t s);
// sbx_planet_eval (kern_planet_eval.hip): fn 0 render / 1 terrain_march / 2 sdf_terrain_map / 3 sdf_terrain_map_detail / 4 sdf_terrain_normal /
// 5 clouds_density / 6 illuminate / 7 background over F = build_planet of u_time (its camera is not read); plain = the SKIP = false
// statement for every wave; counts = NULL or two zeroed device words (waves with every guarded short form on, waves that fell back)
void launch_planet_eval(int fn, const FramePlanet& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s);
// sbx_planet_world_eval: the same functions over F = build_planet_world of the caller's block (its camera is not read)
void launch_planet_world_eval(int fn, const FramePlanetWorld& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s);
// sbx_egg_eval (kern_egg_eval.hip): fn 0 sdf / 1 sdf_normal / 2 shadowmarch / 3 render_scene over build_egg_pose's frame; variant as
// launch_egg's (1 = the reference form); counts: NULL, or two zeroed device words (witnessed waves, re-run waves).  launch_ik_eval: "ik_solver"
void launch_egg_eval(int fn, const FrameEgg& F, int variant, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s);
void launch_ik_eval(const float* in, float* out, size_t n, hipStream_t s);
// sbx_vinyl_eval (kern_vinyl_eval.hip): fn 0 sdf / 1 sdf_normal / 2 sdf_shadow / 3 illuminate / 4 render over build_vinyl_deck's frame
// and vinyl_shade_of's data; variant as launch_vinyl's (1 = the reference form); counts: NULL, or two zeroed device words
void launch_vinyl_eval(int fn, const FrameVinyl& F, const VinylShade& D, int variant, const float* in, float* out, size_t n,
                       unsigned* counts, hipStream_t s);
int launch_math_eval(int fn, const float* a, const float* b, float* out, size_t n, hipStream_t s);
void launch_cl_exp_eval(const float* a, float* out, size_t n, hipStream_t s, int form);   // exp_reg_ / exp_reg128_ forms (kern_clouds.hip)

}  // namespace sbx
