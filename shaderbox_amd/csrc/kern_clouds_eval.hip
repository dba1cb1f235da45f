// shaderbox_amd/csrc/kern_clouds_eval.hip — sbx_clouds_eval: APP_CLOUDS' volume and sky over the caller's rays (include/sbx.h).
//
// Follows the reference's src/app_clouds.h in its procedural build (SKY_SPHERE / USE_NOISE_TEX undefined, both `#if 0` of
// illuminate_volume off): render :204-218, render_clouds :153-202, render_sky_color :36-46, density_func :62-86, illuminate_volume
// :91-123.  The ray origin stands where the reference's eye.origin does (:166), u_time enters through the wind offset alone (:167),
// directions are used as given.  One lane per element, no cross-lane step: what a lane computes depends on its own element only.
//
// k_clouds (kern_clouds.hip) cannot serve a list of unrelated rays: its y table needs one origin.y per frame, its LDS cache lives on
// the lattice cells an 8x8 pixel tile shares, and its hash-table kernels rest on an index bound the host derives from the camera.
// Two forms here:
//   PLAIN (sbx_set_variant 1): the statement of k_clouds_perlane — clouds_density / clouds_illuminate of sbx_clouds.h: hash1 in place,
//     exp_, pow_, the IEEE division in the coverage smoothstep.
//   default: the lattice hashes from the context's table, decided per lane and per cell (eval_density), and the guard-less forms whose
//     conditions are about the aux block alone (clouds_select's predicates, decided per call: launch_clouds_eval).  No form whose
//     condition involves positions is used: no sin_b40_, no Lipschitz skip, no y table.
#include "sbx_device.h"
#include "sbx_clouds.h"
#include "sbx_exp4k_table.h"
#include <cmath>

namespace sbx {

// EXPF: the march's exp.  0: exp_; 1: exp_reg4k_ (a regular block, clouds_regular: |sigma * dt| <= 80, and the density is in [0, .9375
// (1 + 1e-6)] or NaN whatever the position — a blend of hashes in [0, 1] with weights in [0, 1] — so every argument lies in [-80, 80] or
// is NaN); 2: exp_small_ (clouds_exp_small: every argument in [-.205, -0] or NaN).
template <int EXPF>
__device__ __forceinline__ float eval_exp(float x) {
    if (EXPF == 2) return exp_small_<true>(x);
    if (EXPF == 1) return exp_reg4k_(x, kExp2Tab4096);
    return exp_(x);
}

// the eight hashes of the cell with lattice index n, evaluated in place (noise_iq's own arguments, in the table's corner order)
__device__ __forceinline__ H8 eval_hashes(float n) {
    H8 h;
    h.lo = make_float4(hash1(n + 0.0f), hash1(n + 1.0f), hash1(n + 157.0f), hash1(n + 158.0f));
    h.hi = make_float4(hash1(n + 113.0f), hash1(n + 114.0f), hash1(n + 270.0f), hash1(n + 271.0f));
    return h;
}

// density_func :62-86 with the lattice hashes from the context's table where the cell lies in it.
// noise_iq forms n = px + py * 157 + 113 * pz (noise_iq.h:19).  A lane takes a cell's eight hashes from the table iff
// fabsf(n) <= range (a NaN n compares false; range < 0: no table), else it evaluates the eight hash1 itself; the blends are the same
// instructions either way.  WHY THE BITS ARE EQUAL: px, py, pz are floor() results, integer-valued binary32 numbers, and a product or
// sum of integer-valued binary32 numbers rounds to an integer-valued one, so a finite n is an integer; with |n| <= range <= 2^22 it and
// n + k for the corner offsets k = 0, 1, 157, 158, 113, 114, 270, 271 are integers below 2^24, exactly represented, so the additions
// noise_iq makes are exact and the arguments of its hash calls are the numbers (int)n + k.  The table entry (int)n + k + bias holds
// hash1((float)((int)n + k)) (k_clouds_hashtab), the same function of the same binary32 argument (n = -0 gives n + 0.0f = +0 in
// place and entry `bias` = hash1(+0) from the table).  The index lies inside the table: it holds [-range, range + 271] and a guard.
// No bound on the rays is needed on the host: the test is made where the index is formed.
// SMF: the coverage smoothstep.  0: the IEEE division (smoothstep_); 1: x_smoothstep_rd_med3 (a regular block: cov and the reciprocal
// finite); 2: x_smoothstep_d3_med3 (clouds_div3_domain; the fBm sum is in [0, .9375 (1 + 1e-6)] or NaN for every position).
// Counting (COUNT; sbx_debug_clouds_eval): cells whose hashes came from the table / were evaluated in place, per lane in registers.
template <int SMF, bool COUNT>
__device__ __forceinline__ float eval_density(const FrameClouds& F, v3 pos_in, const GTab& g, float range, unsigned& c_tab, unsigned& c_here) {
    v3 p = (pos_in * .001f) * 2.03f;                     // :66,72 (cld_noise_factor is the literal .001 in this build, :20)
    float fx[4], fy[4], fz[4], n[4];
    bool all_in = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                        // lattice part of noise_iq.h:14-19, all octaves first
        const float px = floor_(p.x), py = floor_(p.y), pz = floor_(p.z);
        const float ax = p.x - px, ay = p.y - py, az = p.z - pz;
        fx[k] = ax * ax * tm2_(ax);
        fy[k] = ay * ay * tm2_(ay);
        fz[k] = az * az * tm2_(az);
        n[k] = px + py * 157.0f + 113.0f * pz;
        all_in = all_in && (__builtin_fabsf(n[k]) <= range);
        p = p * 2.64f;                                   // fbm.h:6  p *= lacunarity
    }
    float t = 0.f, H = .5f;
    if (all_in) {
        // this lane's four cells lie in the table: the sixteen loads first, then the blends
        H8 h[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = gt_load(g, gt_off(n[k], g.bias4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t += hc_blend(h[k].lo, h[k].hi, fx[k], fy[k], fz[k]) * H;     // fbm.h:6  t += noise * H
            H *= .5f;
        }
        if (COUNT) c_tab += 4u;
    } else {
        // some cell lies outside (or there is no table): cell by cell, from the position again (the same operations on the same values)
        v3 q = (pos_in * .001f) * 2.03f;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const float px = floor_(q.x), py = floor_(q.y), pz = floor_(q.z);
            const float ax = q.x - px, ay = q.y - py, az = q.z - pz;
            const float gx = ax * ax * tm2_(ax), gy = ay * ay * tm2_(ay), gz = az * az * tm2_(az);
            const float nk = px + py * 157.0f + 113.0f * pz;
            H8 h;
            if (__builtin_fabsf(nk) <= range) {
                h = gt_load(g, gt_off(nk, g.bias4));
                if (COUNT) c_tab += 1u;
            } else {
                h = eval_hashes(nk);
                if (COUNT) c_here += 1u;
            }
            t += hc_blend(h.lo, h.hi, gx, gy, gz) * H;
            H *= .5f;
            q = q * 2.64f;
        }
    }
    if (SMF == 2) return x_smoothstep_d3_med3(F.cov, F.cov_d, F.cov_r, t);       // :83-84
    if (SMF == 1) return x_smoothstep_rd_med3(F.cov, F.cov_rd, t);
    return t * smoothstep_(F.cov, F.cov_hi, t);
}

// what the forms differ in, behind one name each: PLAIN is the per-lane statement of sbx_clouds.h
template <bool PLAIN, int EXPF, int SMF, bool COUNT>
struct EvalForm {
    const FrameClouds& F;
    GTab g;
    float range;
    unsigned c_tab = 0u, c_here = 0u;
    __device__ __forceinline__ float density(v3 pos) {
        if (PLAIN) {
            if (COUNT) c_here += 4u;
            return clouds_density(F, pos);
        }
        return eval_density<SMF, COUNT>(F, pos, g, range, c_tab, c_here);
    }
    __device__ __forceinline__ float exp_form(float x) { return PLAIN ? exp_(x) : eval_exp<EXPF>(x); }
    // illuminate_volume :91-123 with the phase function evaluated by the caller, once per ray
    __device__ __forceinline__ float illuminate(v3 origin, float phase) {
        const v3 step = F.sun_dir * F.dt;
        v3 pos = origin + step;
        float transmittance = 1.f;
        for (int i = 0; i < F.lsteps; ++i) {
            const float d = density(pos);
            transmittance *= exp_form(-d * F.sigma * F.dt);
            pos = pos + step;
        }
        return transmittance * F.sun_power * phase;
    }
};

__device__ __forceinline__ v3 eval_sky(const FrameClouds& F, v3 dir) {            // render_sky_color :36-46
    const float sun_amount = fmax_(dot(dir, F.sun_dir), 0.f);
    v3 sky = mix3(V3(.0f, .1f, .4f), V3(.3f, .6f, .8f), 1.0f - dir.y);
    sky = sky + F.sun_color * fmin_(pow_(sun_amount, 1500.0f) * 5.0f, 1.0f);
    sky = sky + F.sun_color * fmin_(pow_(sun_amount, 10.0f) * .6f, 1.0f);
    return abs3(sky);
}

enum { CE_MARCH = 0, CE_SKY = 1, CE_DENSITY = 2, CE_ILLUM = 3 };     // the kernel's FN; CE_MARCH serves "render" and "render_clouds"

// FN: which function; clouds_only (CE_MARCH, wave-uniform): "render_clouds" instead of "render".  in / out: 4-byte aligned, the
// element widths of include/sbx.h.  counts (COUNT): two 64-bit words, added to once per wave, at its end.
template <int FN, bool PLAIN, int EXPF, int SMF, bool COUNT>
__global__ void __launch_bounds__(64) k_clouds_eval(FrameClouds F, int clouds_only, const float* __restrict__ in, float* __restrict__ out,
                                                    size_t n, GTab g, float range, unsigned long long* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    EvalForm<PLAIN, EXPF, SMF, COUNT> E{F, g, range};
    if (i < n) {
        if (FN == CE_SKY) {
            const float* q = in + 3 * i;
            const v3 sky = eval_sky(F, V3(q[0], q[1], q[2]));
            float* o = out + 3 * i;
            o[0] = sky.x; o[1] = sky.y; o[2] = sky.z;
        } else if (FN == CE_DENSITY) {
            const float* q = in + 3 * i;
            out[i] = E.density(V3(q[0], q[1], q[2]));
        } else if (FN == CE_ILLUM) {
            const float* q = in + 6 * i;
            const v3 V = V3(q[3], q[4], q[5]);
            const float phase = hg_phase(clamp_(dot(F.sun_dir, V), 0.f, 1.f), .2f);          // :121, L = sun_dir
            out[i] = E.illuminate(V3(q[0], q[1], q[2]), phase);
        } else {
            const float* q = in + 6 * i;
            const v3 eye = V3(q[0], q[1], q[2]), dir = V3(q[3], q[4], q[5]);
            const float cutoff = dot(dir, V3(0, 1, 0));                                      // :200, :212
            v3 sky = V3(0, 0, 0);
            if (!clouds_only) sky = eval_sky(F, dir);
            float4 r = make_float4(sky.x, sky.y, sky.z, 0.f);                                // :212 returned the sky
            if (clouds_only || !(cutoff < 0.05f)) {
                // render_clouds :153-202
                const v3 projection = dir / dir.y;
                v3 origin = eye + projection * 150.f;
                origin = origin + F.wind_off;
                const float phase = hg_phase(clamp_(dot(F.sun_dir, dir), 0.f, 1.f), .2f);
                float transmittance = 1.f, radiance = 0.f, alpha = 0.f, t = 0.f;
                for (int s = 0; s < F.steps; ++s) {
                    const v3 pos = origin + t * projection;
                    t += F.dt;
                    const float density = E.density(pos);
                    if (!(density < .005f)) {                          // integrate_volume :132
                        const float T_i = E.exp_form(-density * F.sigma * F.dt);
                        transmittance *= T_i;
                        radiance += (density * F.sigma) * E.illuminate(pos, phase) * transmittance * F.dt;
                        alpha += (1.f - T_i) * (1.f - alpha);
                    }
                    if (alpha > .999f) break;
                }
                const float a = alpha * smoothstep_(.0f, .2f, cutoff);                       // :201
                if (clouds_only) {
                    r = make_float4(radiance, radiance, radiance, a);
                } else {
                    const v3 col = abs3(mix3(sky, V3s(radiance), a));                        // :215-217 (radiance is r = g = b)
                    r = make_float4(col.x, col.y, col.z, a);
                }
            }
            float* o = out + 4 * i;
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        }
    }
    if (COUNT) {
        // every lane of the wave arrives here (no lane returns early): the wave's sums, then one vector atomic per word from lane 0
        unsigned long long a = E.c_tab, b = E.c_here;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o);
            b += __shfl_xor(b, o);
        }
        if (threadIdx.x == 0) {
            atomicAdd(counts, a);
            atomicAdd(counts + 1, b);
        }
    }
}

struct EvalLaunch { dim3 grid; hipStream_t s; const FrameClouds* F; int clouds_only; const float* in; float* out; size_t n; GTab g; float range; unsigned long long* counts; };
template <int FN, bool PLAIN, int EXPF, int SMF>
static void eval_launch_form(const EvalLaunch& L) {
    if (L.counts) hipLaunchKernelGGL((k_clouds_eval<FN, PLAIN, EXPF, SMF, true>), L.grid, dim3(64), 0, L.s, *L.F, L.clouds_only, L.in, L.out, L.n, L.g, L.range, L.counts);
    else hipLaunchKernelGGL((k_clouds_eval<FN, PLAIN, EXPF, SMF, false>), L.grid, dim3(64), 0, L.s, *L.F, L.clouds_only, L.in, L.out, L.n, L.g, L.range, L.counts);
}
template <int FN>
static void eval_launch_fn(const EvalLaunch& L, bool plain, int expf, int smf) {
    if (FN == CE_SKY || plain) { eval_launch_form<FN, true, 0, 0>(L); return; }          // (the sky has one form)
    if constexpr (FN == CE_SKY) {
    } else if constexpr (FN == CE_DENSITY) {                                                     // (density_func evaluates no exp)
        if (smf == 0) eval_launch_form<FN, false, 0, 0>(L);
        else if (smf == 1) eval_launch_form<FN, false, 0, 1>(L);
        else eval_launch_form<FN, false, 0, 2>(L);
    } else {
        const int key = expf << 4 | smf;                                                   // (0, 0) or both non-zero: launch_clouds_eval
        if (key == 0x00) eval_launch_form<FN, false, 0, 0>(L);
        else if (key == 0x11) eval_launch_form<FN, false, 1, 1>(L);
        else if (key == 0x12) eval_launch_form<FN, false, 1, 2>(L);
        else if (key == 0x21) eval_launch_form<FN, false, 2, 1>(L);
        else eval_launch_form<FN, false, 2, 2>(L);
    }
}

// fn: 0 render, 1 render_clouds, 2 render_sky_color, 3 density_func, 4 illuminate_volume (sbx_eval.hip clouds_eval_args).  F: build_clouds
// of the caller's block and u_time (its camera is not read).  plain: sbx_set_variant 1.  ht: a table that is ready on `s`, or none — then
// every cell is hashed in place, with the same aux-only forms.  counts: NULL, or two zeroed 64-bit device words (the counting
// instantiation).  n in 1 ... 2^31.
void launch_clouds_eval(int fn, const FrameClouds& F, bool plain, const CloudsHashTab* ht, const float* in, float* out, size_t n,
                        unsigned long long* counts, hipStream_t s) {
    // the aux-only conditions are clouds_select's own: a regular block admits the guard-less exp and the one-instruction clamp, within it
    // exp_small_ under clouds_exp_small and div3_ under clouds_div3_domain
    RowMap M{};
    const sbx_clouds_selection S = clouds_select(F, M, 0, CLOUDS_DEFAULT, 0, 0);
    const int expf = !S.regular ? 0 : S.exp_small ? 2 : 1;
    const int smf = !S.regular ? 0 : S.div3_domain ? 2 : 1;
    EvalLaunch L{dim3((unsigned)((n + 63) / 64)), s, &F, fn == 1 ? 1 : 0, in, out, n, GTab{nullptr, 0u}, -1.0f, counts};
    if (!plain && ht && ht->tab) { L.g = GTab{ht->tab, 4u * (unsigned)ht->bias}; L.range = (float)ht->range; }
    if (fn <= 1) eval_launch_fn<CE_MARCH>(L, plain, expf, smf);
    else if (fn == 2) eval_launch_fn<CE_SKY>(L, plain, expf, smf);
    else if (fn == 3) eval_launch_fn<CE_DENSITY>(L, plain, expf, smf);
    else eval_launch_fn<CE_ILLUM>(L, plain, expf, smf);
}

}  // namespace sbx
