// shaderbox_amd/csrc/kern_atmosphere_air.hip — SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval: app_atmosphere.h over the caller's air.
//
// Follows the reference's src/app_atmosphere.h as kern_atmosphere.hip does, with every number the header states read from the
// block (include/sbx.h sbx_aux_atmosphere_air; AtmAir and FrameAtmosphere in sbx_frame.h): render's two builds (VIEW 0: the sky dome
// of :190-209 from the block's eye; VIEW 1: get_primary_ray, the terrain plane and the grey of :210-225), get_incident_light and
// get_sun_light with run-time sample counts.  The tiers, their domain and the proofs: sbx_atmosphere.h "CALLER'S AIR".  The literal
// tier is not here: it launches kern_atmosphere.hip's kernels (sbx_capi.hip).
#include <cmath>
#ifndef ATM_NO_FIN
#define ATM_NO_FIN 0
#endif
#include "sbx_atmosphere.h"

namespace sbx {

#ifndef ATM_MIN_WAVES
#define ATM_MIN_WAVES 6
#endif

// the ray a lane without a march of its own holds while its wave runs the fast body: a ray of the class (sbx_atmosphere.h)
__device__ __forceinline__ void air_class_ray(v3& ro, v3& rd) { ro = V3(0.f, ATM_EARTH_R + 1.f, 0.f); rd = V3(1.f, 0.f, 0.f); }

// SELECT = false: the plain statement, lane by lane.  SELECT = true (tame blocks only): a wave whose rays all pass atm_eval_class runs
// the fast body, every other wave the plain one.
template <int VIEW, bool SELECT>
__global__ void __launch_bounds__(64, ATM_MIN_WAVES) k_atmosphere_air(FrameAtmosphere F, AtmAir K, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
    __shared__ double etab[32];
    if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    __builtin_amdgcn_wave_barrier();
    const Pixel px = pixel_of_thread<8, 1>(M);
    if (!px.valid) return;
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    const v3 ro = F.cam.eye;
    v3 rd, rest;                  // the ray, and the pixel where `march` is false
    bool march;
    if (VIEW == 0) {
        // sky dome mapping :195-207.  Outside the circle z2 = 2 acos_ returns its NaN, the direction is NaN, `d2 < radius2` is false
        // and get_incident_light returns (0, 0, 0), whatever the block holds (kern_atmosphere.hip): a wave that is all out there
        // leaves; in a mixed one the fast body treats those lanes as lanes without a march
        const float z2 = pc.x * pc.x + pc.y * pc.y;
        const bool outside = z2 > 2.0f;
        if (__builtin_amdgcn_ballot_w64(!outside) == 0ull) {
            tile_cost_store(M, tl_t0);
            store_rgba(M, out, px.idx, to_srgb(V3(0.f, 0.f, 0.f)));
            return;
        }
        const float phi = atan2_(pc.y, pc.x);
        const float theta = acos_(1.0f - z2);
        rd = V3(sin_(theta) * cos_(phi), cos_(theta), sin_(theta) * sin_(phi));
        march = !outside;
        rest = V3(0.f, 0.f, 0.f);
    } else {
        rd = primary_dir(F.cam, pc);
        // terrain = plane((0, -1, 0), earth_radius), hit = no_hit, intersect_plane(eye, terrain, hit)   :211-218, intersect.h:61-77
        const v3 n = V3(0.f, -1.f, 0.f);
        const float max_dist = 1e8f;
        float hit_t = max_dist + 1e1f;
        const float denom = dot(n, rd);
        if (!(denom < 1e-6f)) {
            const v3 P0 = V3(K.earth_r, K.earth_r, K.earth_r);
            const float t = dot(P0 - ro, n) / denom;
            if (!(t < 0.f || t > hit_t)) hit_t = t;
        }
        march = hit_t > max_dist;                                       // :220
        rest = V3(.33f, .33f, .33f);                                    // :223
        if (SELECT && __builtin_amdgcn_ballot_w64(march) == 0ull) {     // a wave under the horizon
            tile_cost_store(M, tl_t0);
            store_rgba(M, out, px.idx, to_srgb(rest));
            return;
        }
    }
    v3 col = rest;
    bool fast = false;
    if (SELECT) {
        v3 fo = ro, fd = rd;
        if (!march) air_class_ray(fo, fd);
        fast = __builtin_amdgcn_ballot_w64(!atm_eval_class(fo, fd)) == 0ull;   // wave-uniform
        if (fast) {
            const v3 light = air_incident_light<true, 16, 8>(fo, fd, F.sun_dir, etab, K);
            col = march ? light : rest;
        }
    }
    if (!fast && (march || VIEW == 0)) col = air_incident_light<false, 0, 0>(ro, rd, F.sun_dir, etab, K);   // (VIEW 0 outside the circle: the NaN ray, black)
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(col));
}

// fast: the block is tame and sbx_set_variant is not 1 (the caller decides: sbx_frames.hip atmosphere_air_tier)
void launch_atmosphere_air(const FrameAtmosphere& F, const AtmAir& K, int view, bool fast, const RowMap& M, float* out, hipStream_t s) {
    const dim3 g = grid_for<8, 1>(M), b(64);
    const bool select = fast && ATM_NO_FIN == 0;
    if (view == 0) {
        if (select) hipLaunchKernelGGL((k_atmosphere_air<0, true>), g, b, 0, s, F, K, M, out);
        else hipLaunchKernelGGL((k_atmosphere_air<0, false>), g, b, 0, s, F, K, M, out);
    } else {
        if (select) hipLaunchKernelGGL((k_atmosphere_air<1, true>), g, b, 0, s, F, K, M, out);
        else hipLaunchKernelGGL((k_atmosphere_air<1, false>), g, b, 0, s, F, K, M, out);
    }
}

// ---- the solver over the caller's rays under the caller's air: sbx_atmosphere_air_eval ---------------------------------------------
// k_atmosphere_eval's layout and selection (kern_atmosphere.hip): one thread per ray, FN 0 = get_incident_light, FN 1 = get_sun_light
// along the ray itself with the light count; fast_waves: NULL, or a counter of the waves that took the fast body.
template <int FN, bool SELECT>
__global__ void __launch_bounds__(64, ATM_MIN_WAVES) k_atmosphere_air_eval(const float* __restrict__ rays, v3 sun_dir, AtmAir K, float* __restrict__ out,
                                                                           size_t n, unsigned* fast_waves) {
    __shared__ double etab[32];
    if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab[threadIdx.x];
    __builtin_amdgcn_wave_barrier();
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    v3 ro, rd;
    air_class_ray(ro, rd);                                                 // a lane past n
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
            r = air_incident_light<true, 16, 8>(ro, rd, sun_dir, etab, K);
        } else {
            float hr_d = K.hR, hr_r = K.rhR, hm_d = K.hM, hm_r = K.rhM;
            asm volatile("" : "+v"(hr_d), "+v"(hr_r), "+v"(hm_d), "+v"(hm_r));
            float odR = 0.f, odM = 0.f;
            const bool over = air_sun_light<true, 8>(ro, rd, odR, odM, etab, K, hr_d, hr_r, hm_d, hm_r);
            r = V3(over ? 1.f : 0.f, odR, odM);
        }
    } else {
        if (!live) return;
        if (FN == 0) {
            r = air_incident_light<false, 0, 0>(ro, rd, sun_dir, etab, K);
        } else {
            float odR = 0.f, odM = 0.f;
            const bool over = air_sun_light<false, 0>(ro, rd, odR, odM, etab, K, K.hR, K.rhR, K.hM, K.rhM);
            r = V3(over ? 1.f : 0.f, odR, odM);
        }
    }
    if (live) {
        float* q = out + 3 * i;
        q[0] = r.x; q[1] = r.y; q[2] = r.z;
    }
}

template <int FN>
static void launch_atmosphere_air_eval_fn(bool select, const float* rays, v3 sun, const AtmAir& K, float* out, size_t n, unsigned* fast_waves, hipStream_t s) {
    const dim3 g((unsigned)((n + 63) / 64)), b(64);
    if (select) hipLaunchKernelGGL((k_atmosphere_air_eval<FN, true>), g, b, 0, s, rays, sun, K, out, n, fast_waves);
    else hipLaunchKernelGGL((k_atmosphere_air_eval<FN, false>), g, b, 0, s, rays, sun, K, out, n, fast_waves);
}

// fast: as launch_atmosphere_air's.  n in 1 ... 2^31.
void launch_atmosphere_air_eval(int fn, bool fast, const float* rays, const float* sun_dir, const AtmAir& K, float* out, size_t n, unsigned* fast_waves,
                                hipStream_t s) {
    const v3 sun = V3(sun_dir[0], sun_dir[1], sun_dir[2]);
    const bool select = fast && ATM_NO_FIN == 0;
    if (fn == 0) launch_atmosphere_air_eval_fn<0>(select, rays, sun, K, out, n, fast_waves, s);
    else launch_atmosphere_air_eval_fn<1>(select, rays, sun, K, out, n, fast_waves, s);
}

}  // namespace sbx
