// shaderbox_amd/csrc/kern_atmosphere.hip — APP_ATMOSPHERE: Rayleigh/Mie single scattering.
//
// Follows /root/reference/src/app_atmosphere.h (FROM_SPACE defined, :162): render :183-228 (sky
// dome branch :190-209), get_incident_light :78-160 (16 view samples), get_sun_light :50-76
// (8 light samples), isect_sphere :15-26, phase functions src/volumetric.h:13-33 (hg_g = .76).
// sun_dir (a _mutable global rotated by setup_scene, :177-181) is a frame constant built on the
// host from (0,1,0), i.e. it restarts from its initialiser for every pixel (GLSL semantics).
// Magnitudes are ~6.4e6 in binary32, so the evaluation order below is part of the result.
//
// k_atmosphere_ground (SBX_APP_ATMOSPHERE_GROUND) is the same file built WITHOUT FROM_SPACE (:171-174, :210-225): a perspective camera
// one metre above the ground, intersect_plane (src/intersect.h:61-77) with the flat terrain, get_incident_light along the primary
// ray where there is no hit and (.33, .33, .33) where there is.
#include <cmath>
#ifndef ATM_NO_FIN
#define ATM_NO_FIN 0
#endif
#include "sbx_atmosphere.h"

namespace sbx {

#ifndef ATM_MIN_WAVES
#define ATM_MIN_WAVES 6     // (the max-ILP strategy of this source, build.py, takes what registers it is given: 147 for the plain kernel without a bound)
#endif
template <bool FIN, int PREC = 0>
__global__ void __launch_bounds__(64 * ATM_TX, ATM_MIN_WAVES) k_atmosphere(FrameAtmosphere F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
    constexpr bool T64 = FIN && ATM_EXP_REG && ATM_EXP64 && !ATM_EXP4K;
    __shared__ double etab[32];
    __shared__ double etab64[T64 ? 64 : 1];               // exp_reg64_'s table (builds without exp_reg4k_)
    if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    if (T64 && threadIdx.x < 64) etab64[threadIdx.x] = kExp2Tab64[threadIdx.x];
    if (ATM_TX > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    const Pixel px = pixel_of_thread<8, ATM_TX>(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);

    // sky dome mapping :195-207
    const float z2 = pc.x * pc.x + pc.y * pc.y;
#ifndef ATM_FREE_EXIT
#define ATM_FREE_EXIT 1
#endif
    // Outside the dome's circle z2 = 2 the argument of acos is below -1 (z2 > 2 is a multiple of ulp(2), so 1 - z2 is exact and
    // < -1): acos_ returns its NaN, the direction is NaN in all three components, isect_sphere's `d2 < radius2` (:25) is false and
    // get_incident_light returns (0, 0, 0) (:85-88) — 28 % of a 16:9 frame.  A wave whose pixels are ALL out there (the test is
    // wave-uniform) skips the atan2 / acos / two sin / two cos of the mapping, ~600 instructions, and encodes that black.
    if (ATM_FREE_EXIT && __builtin_amdgcn_ballot_w64(!(z2 > 2.0f)) == 0ull) {
        tile_cost_store(M, tl_t0);
        store_rgba(M, out, px.idx, to_srgb(V3(0.f, 0.f, 0.f)));
        return;
    }
    const float phi = atan2_(pc.y, pc.x);
    const float theta = acos_(1.0f - z2);
    const v3 rd = V3(sin_(theta) * cos_(phi), cos_(theta), sin_(theta) * sin_(phi));
    const v3 ro = V3(0, ATM_EARTH_R + 1.f, 0);

    const v3 col = atm_incident_light<FIN, PREC>(ro, rd, F.sun_dir, etab, etab64);
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(col));
}

// ---- the ground camera: app_atmosphere.h without FROM_SPACE ---------------------------------------------------------------------
// render :211-224 around the shared atm_incident_light.  FIN = true adds the wave-level exit below and sbx_atmosphere.h's
// shortcuts (its "THE GROUND CAMERA" paragraph shows each for these rays; the dead-ray exit is compiled out: DEAD = false);
// FIN = false is the plain statement, lane by lane (sbx_set_variant 1, and non-finite uniforms).
template <bool FIN, int PREC = 0>
__global__ void __launch_bounds__(64 * ATM_TX, ATM_MIN_WAVES) k_atmosphere_ground(FrameAtmosphere F, RowMap M, float* out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
    constexpr bool T64 = FIN && ATM_EXP_REG && ATM_EXP64 && !ATM_EXP4K;
    __shared__ double etab[32];
    __shared__ double etab64[T64 ? 64 : 1];
    if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    if (T64 && threadIdx.x < 64) etab64[threadIdx.x] = kExp2Tab64[threadIdx.x];
    if (ATM_TX > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    const Pixel px = pixel_of_thread<8, ATM_TX>(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    const v3 rd = primary_dir(F.cam, pc);

    // terrain = plane((0, -1, 0), earth_radius), hit = no_hit, intersect_plane(eye, terrain, hit)   :211-218, intersect.h:61-77
    const v3 n = V3(0.f, -1.f, 0.f);
    const float max_dist = 1e8f;                                    // def.h:77
    float hit_t = max_dist + 1e1f;                                  // no_hit.t, def.h:78-83
    const float denom = dot(n, rd);                                 // (the whole dot: 0 * NaN and 0 * inf make a NaN denom)
    if (!(denom < 1e-6f)) {                                         // a NaN denom goes on, as in the reference
        const v3 P0 = V3(ATM_EARTH_R, ATM_EARTH_R, ATM_EARTH_R);
        const float t = dot(P0 - F.cam.eye, n) / denom;
        if (!(t < 0.f || t > hit_t)) hit_t = t;                     // a NaN t is recorded: a NaN direction is a GROUND pixel
    }
    const bool sky = hit_t > max_dist;                              // :220
    const v3 ground = V3(.33f, .33f, .33f);                         // :223

    // The camera has no roll, so sky / ground is a matter of the row: whole waves lie under the horizon (22 % of the frame) and
    // leave here, before any table read or march.  Wave-uniform; the waves of the horizon row's tiles are mixed and go on.
    if (FIN && __builtin_amdgcn_ballot_w64(sky) == 0ull) {
        tile_cost_store(M, tl_t0);
        store_rgba(M, out, px.idx, to_srgb(ground));
        return;
    }
    v3 col = ground;
    if (FIN) {
        // every lane of a mixed wave takes part in the march (its wave-wide tests count lanes): a ground lane marches straight up,
        // a ray inside the domain sbx_atmosphere.h shows for the sky rays, and drops the result
        const v3 rs = sky ? rd : V3(0.f, 1.f, 0.f);
        const v3 light = atm_incident_light<FIN, PREC, false>(F.cam.eye, rs, F.sun_dir, etab, etab64);
        col = sky ? light : ground;
    } else if (sky) {
        col = atm_incident_light<false, 0, false>(F.cam.eye, rd, F.sun_dir, etab, etab64);   // :221
    }
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(col));
}

// ---- the solver over the caller's rays: sbx_atmosphere_eval ------------------------------------------------------------------------
// One thread per ray (rays: n x {origin, direction}, out: n x 3, both only 4-byte aligned), FN 0 = get_incident_light (:78-160),
// FN 1 = get_sun_light (:50-76; out = {overground, optical_depthR, optical_depthM}, the partial sums where the march returns early).
// The plain statement, lane by lane, is the definition (SELECT = false).  SELECT = true carries both bodies: a wave whose 64 rays all
// lie in sbx_atmosphere.h's class ("CALLER'S RAYS": the test is made here, on the loaded rays, wave-uniformly) runs the FIN forms,
// every other wave the plain one.  (The same selection as TWO launches, in each of which the waves of the other class leave after
// the test: measured against the one kernel and not taken, profiles/atmosphere_eval_timing.txt.)
// fast_waves: NULL, or a counter of the waves that took the FIN forms (sbx_test.h).
static_assert(!ATM_BATCH, "get_sun_light's partial sums are those of the sample-by-sample march");
template <int FN, bool SELECT>
__global__ void __launch_bounds__(64, ATM_MIN_WAVES) k_atmosphere_eval(const float* __restrict__ rays, v3 sun_dir, float* __restrict__ out,
                                                                       size_t n, unsigned* fast_waves) {
    constexpr bool T64 = ATM_EXP_REG && ATM_EXP64 && !ATM_EXP4K;
    __shared__ double etab[32];
    __shared__ double etab64[T64 ? 64 : 1];
    if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    if (T64 && threadIdx.x < 64) etab64[threadIdx.x] = kExp2Tab64[threadIdx.x];
    __builtin_amdgcn_wave_barrier();
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    // a lane past n holds a ray of the class, so that it neither keeps its wave from the FIN forms nor disturbs their wave-wide tests
    v3 ro = V3(0.f, ATM_EARTH_R + 1.f, 0.f), rd = V3(1.f, 0.f, 0.f);
    if (live) {
        const float* p = rays + 6 * i;
        ro = V3(p[0], p[1], p[2]);
        rd = V3(p[3], p[4], p[5]);
    }
    const bool fast = SELECT && __builtin_amdgcn_ballot_w64(!atm_eval_class(ro, rd)) == 0ull;   // wave-uniform
    v3 r;
    if (fast) {
        if (fast_waves && threadIdx.x == 0) atomicAdd(fast_waves, 1u);
        if (FN == 0) {
            r = atm_incident_light<true, 0, true>(ro, rd, sun_dir, etab, etab64);
        } else {
            AtmDiv K{ATM_HR, 1.0f / ATM_HR, ATM_HM, 1.0f / ATM_HM};
            if (ATM_DIV3) asm volatile("" : "+v"(K.hr), "+v"(K.rhr), "+v"(K.hm), "+v"(K.rhm));
            float odR = 0.f, odM = 0.f;
            const bool over = sun_light<true>(ro, rd, odR, odM, etab, etab64, K);
            r = V3(over ? 1.f : 0.f, odR, odM);
        }
    } else {
        if (!live) return;
        if (FN == 0) {
            r = atm_incident_light<false, 0, false>(ro, rd, sun_dir, etab, etab64);
        } else {
            const AtmDiv K{ATM_HR, 1.0f / ATM_HR, ATM_HM, 1.0f / ATM_HM};
            float odR = 0.f, odM = 0.f;
            const bool over = sun_light<false>(ro, rd, odR, odM, etab, etab64, K);
            r = V3(over ? 1.f : 0.f, odR, odM);
        }
    }
    if (live) {
        float* q = out + 3 * i;
        q[0] = r.x; q[1] = r.y; q[2] = r.z;
    }
}

// the host's part of the class: a sun direction that is finite and a unit vector to ATM_EVAL_UNIT_TOL (sbx_atmosphere.h)
static bool atm_eval_sun_ok(v3 s) {
    const float ss = (s.x * s.x + s.y * s.y) + s.z * s.z;
    return std::isfinite(s.x) && std::isfinite(s.y) && std::isfinite(s.z) && std::fabs(ss - 1.0f) <= ATM_EVAL_UNIT_TOL;
}

template <int FN>
static void launch_atmosphere_eval_fn(bool select, const float* rays, v3 sun, float* out, size_t n, unsigned* fast_waves, hipStream_t s) {
    const dim3 g((unsigned)((n + 63) / 64)), b(64);
    if (select) hipLaunchKernelGGL((k_atmosphere_eval<FN, true>), g, b, 0, s, rays, sun, out, n, fast_waves);
    else hipLaunchKernelGGL((k_atmosphere_eval<FN, false>), g, b, 0, s, rays, sun, out, n, fast_waves);
}

// plain: the plain kernel for every wave (sbx_set_variant 1); a sun the class does not admit makes the launch plain by itself.  n in 1 ... 2^31.
void launch_atmosphere_eval(int fn, bool plain, const float* rays, const float* sun_dir, float* out, size_t n, unsigned* fast_waves, hipStream_t s) {
    const v3 sun = fn == 0 ? V3(sun_dir[0], sun_dir[1], sun_dir[2]) : V3(0.f, 1.f, 0.f);   // get_sun_light reads no sun
    const bool select = !plain && ATM_NO_FIN == 0 && atm_eval_sun_ok(sun);
    if (fn == 0) launch_atmosphere_eval_fn<0>(select, rays, sun, out, n, fast_waves, s);
    else launch_atmosphere_eval_fn<1>(select, rays, sun, out, n, fast_waves, s);
}

// exp_reg4k_ as a standalone function (sbx_math_eval "exp_reg4k"): the same table, read from global memory, the same instruction
// sequence as inside k_atmosphere — for the exhaustive comparison with exp_
__global__ void __launch_bounds__(256) k_exp4k_eval(const float* __restrict__ a, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = exp_reg4k_(a[i], kExp2Tab4096);
}
void launch_exp4k_eval(const float* a, float* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_exp4k_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, out, n);
}

dim3 atmosphere_grid(const RowMap& M) { return grid_for<8, ATM_TX>(M); }

void launch_atmosphere(const FrameAtmosphere& F, const RowMap& M, float* out, hipStream_t s, int precision, bool fin_ok) {
    // FIN: camera and sun direction are finite numbers (they are for every finite u_res / u_time)
    const float chk[] = {F.cam.res_x, F.cam.res_y, F.cam.aspect_x, F.cam.fov, F.sun_dir.x, F.sun_dir.y, F.sun_dir.z,
                         F.cam.fwd.x, F.cam.fwd.y, F.cam.fwd.z, F.cam.up.x, F.cam.up.y, F.cam.up.z, F.cam.right.x, F.cam.right.y, F.cam.right.z};
    bool fin = std::isfinite(F.cam.rres_x) && std::isfinite(F.cam.rres_y) && fin_ok;
    for (float v : chk) fin = fin && std::isfinite(v);
#if ATM_NO_FIN
    fin = false;
#endif
    if (fin && precision == 1) hipLaunchKernelGGL((k_atmosphere<true, 1>), (grid_for<8, ATM_TX>(M)), dim3(64 * ATM_TX), 0, s, F, M, out);   // the tolerance tier
    else if (fin) hipLaunchKernelGGL(k_atmosphere<true>, (grid_for<8, ATM_TX>(M)), dim3(64 * ATM_TX), 0, s, F, M, out);
    else hipLaunchKernelGGL(k_atmosphere<false>, (grid_for<8, ATM_TX>(M)), dim3(64 * ATM_TX), 0, s, F, M, out);
}

void launch_atmosphere_ground(const FrameAtmosphere& F, const RowMap& M, float* out, hipStream_t s, int precision, int variant, bool fin_ok) {
    // FIN as in launch_atmosphere, with the eye (a constant of the app) among the checked values; variant 1 is the plain form
    const float chk[] = {F.cam.res_x, F.cam.res_y, F.cam.aspect_x, F.cam.fov, F.sun_dir.x, F.sun_dir.y, F.sun_dir.z,
                         F.cam.fwd.x, F.cam.fwd.y, F.cam.fwd.z, F.cam.up.x, F.cam.up.y, F.cam.up.z, F.cam.right.x, F.cam.right.y, F.cam.right.z,
                         F.cam.eye.x, F.cam.eye.y, F.cam.eye.z};
    bool fin = std::isfinite(F.cam.rres_x) && std::isfinite(F.cam.rres_y) && variant != 1 && fin_ok;
    for (float v : chk) fin = fin && std::isfinite(v);
#if ATM_NO_FIN
    fin = false;
#endif
    const dim3 g = grid_for<8, ATM_TX>(M), b(64 * ATM_TX);
    if (fin && precision == 1) hipLaunchKernelGGL((k_atmosphere_ground<true, 1>), g, b, 0, s, F, M, out);   // the tolerance tier
    else if (fin) hipLaunchKernelGGL(k_atmosphere_ground<true>, g, b, 0, s, F, M, out);
    else hipLaunchKernelGGL(k_atmosphere_ground<false>, g, b, 0, s, F, M, out);
}

}  // namespace sbx
