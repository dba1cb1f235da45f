// shaderbox_amd/csrc/sbx_clouds.h — what the two translation units of APP_CLOUDS' procedural build share: the per-lane statement of
// density_func, the phase function and illuminate_volume (k_clouds_perlane of kern_clouds.hip, the plain form of kern_clouds_eval.hip),
// and the lookup into the context's lattice-hash table (kern_clouds.hip "the context's hash table"; host side: sbx_ytab.hip).
// src/app_clouds.h :62-86, :91-123, src/volumetric.h:27-33.
#pragma once
#include "sbx_device.h"
#include "sbx_noise.h"
#include "sbx_hashcache.h"

namespace sbx {

__device__ __forceinline__ float clouds_density(const FrameClouds& F, v3 pos_in) {
    v3 pos = pos_in * F.nf;                                    // cld_noise_factor, :18,20,66 (.001 unless SKY_SPHERE)
    float shape = fbm<4>(pos * 2.03f, 2.64f, .5f, .5f, [](v3 p) { return noise_iq(p); });   // :72
    return shape * smoothstep_(F.cov, F.cov_hi, shape);        // :83-84 (per-lane cross-check kernel keeps the IEEE division)
}

__device__ __forceinline__ float hg_phase(float mu, float g) {  // volumetric.h:27-33, note (4 + PI)
    return (1.f - g * g) / ((4.f + 3.14159265359f) * pow_(1.f + g * g - 2.f * g * mu, 1.5f));
}

// illuminate_volume :91-123.  `phase` = henyey_greenstein(clamp(dot(L,V),0,1)) depends only on
// the pixel's ray, so the caller evaluates it once per pixel (same inputs, same bits).
// BUILD (CLOUDS_* of sbx_frame.h): CLOUDS_LUMINANCE returns the march's transmittance itself (the `#if 0` of :118 on).
template <int BUILD>
__device__ __forceinline__ float clouds_illuminate(const FrameClouds& F, v3 origin, float phase) {
    const v3 step = F.sun_dir * F.dt;
    v3 pos = origin + step;
    float transmittance = 1.f;
    for (int i = 0; i < F.lsteps; ++i) {
        float density = clouds_density(F, pos);
        transmittance *= exp_(-density * F.sigma * F.dt);
        pos = pos + step;
    }
    if (BUILD == CLOUDS_LUMINANCE) return transmittance;
    return transmittance * F.sun_power * phase;
}

// A lookup into the context's hash table T[i] = hash1((float)(i - bias)): idx = (int)n + bias and four 8-byte loads at the corner
// offsets 0 / 157 / 113 / 270 from the table's base.  The caller shows that idx lies inside the table.
struct GTab { const float* tab; unsigned bias4; };        // bias4 = 4 * bias: the byte offset of lattice index 0
typedef float gt_f2 __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ unsigned gt_off(float n, unsigned bias4) { return ((unsigned)(int)n << 2) + bias4; }
__device__ __forceinline__ H8 gt_load(const GTab& g, unsigned off) {
    const char* p = reinterpret_cast<const char*>(g.tab) + (unsigned long long)off;     // uniform base + 32-bit lane offset + immediates
    const gt_f2 a = *reinterpret_cast<const gt_f2*>(p), b = *reinterpret_cast<const gt_f2*>(p + 157 * 4);
    const gt_f2 c = *reinterpret_cast<const gt_f2*>(p + 113 * 4), d = *reinterpret_cast<const gt_f2*>(p + 270 * 4);
    H8 h;
    h.lo = make_float4(a.x, a.y, b.x, b.y);              // the cache's corner order: +0, +1, +157, +158, +113, +114, +270, +271
    h.hi = make_float4(c.x, c.y, d.x, d.y);
    return h;
}

}  // namespace sbx
