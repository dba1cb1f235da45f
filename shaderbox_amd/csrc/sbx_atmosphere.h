// shaderbox_amd/csrc/sbx_atmosphere.h — get_incident_light / get_sun_light of /root/reference/src/app_atmosphere.h:50-160 as
// device functions: APP_ATMOSPHERE's kernel (kern_atmosphere.hip) and the config-5 composite SBX_APP_PLANET_ATMOSPHERE
// (kern_planet.hip: APP_PLANET's background() replaced by this sky) share them.  The ATM_* switches and their measurements are
// kern_atmosphere.hip's; FIN = false is the plain statement of the spec (guarded exp, sqrt_n_, division by the exact reciprocal).
#pragma once
#include "sbx_device.h"
#include "sbx_exp4k_table.h"

namespace sbx {


constexpr float ATM_EARTH_R = 6360e3f, ATM_ATMOS_R = 6420e3f, ATM_HR = 7994.0f, ATM_HM = 1200.0f;   // :34-38
constexpr double ATM_HR_RD = 1.0 / (double)ATM_HR, ATM_HM_RD = 1.0 / (double)ATM_HM;   // exact division by constants (sbx_math.h div_by)

// isect_sphere with the atmosphere sphere (origin 0)                        :15-26
__device__ __forceinline__ bool isect_atmosphere(v3 ro, v3 rd, float& t1) {
    const v3 rc = V3(0, 0, 0) - ro;
    const float radius2 = ATM_ATMOS_R * ATM_ATMOS_R;
    const float tca = dot(rc, rd);
    const float d2 = dot(rc, rc) - tca * tca;
    const float thc = sqrt_n_(radius2 - d2);   // both ~4e13: the difference is a multiple of 4e6, zero or negative
    t1 = tca + thc;
    return d2 < radius2;
}

// exp_ of this kernel reads the 2^(j/32) table from LDS.  For the density terms exp(-height / H) — 288 of the 336 exp of an
// in-dome pixel — the binary32 range guard is left out when the uniforms are finite (FIN, decided on the host): a sample lies
// inside the atmosphere sphere, so -height / H is >= -60e3 / 1200 = -50.1; a light sample below the ground returns before its exp
// (:65), but a VIEW ray that dips below the horizon marches through the planet (no ground test, :119-122) with heights down to
// -6.36e6, i.e. arguments up to +5300, where exp_ (guard at 89) and the guard-less forms alike overflow to +inf.  The guard-less
// forms are shown equal to exp_ on every argument in [-80, 2^18]; a NaN passes through the guard unchanged.  exp(-tau): grazing sun
// rays reach optical depths beyond 104 (a ring of 9 % of the pixels turns NaN / inf without the guard), so the guard-less form is
// used only where a wave-wide test shows tau <= 80 for every lane (ATM_TAU4K: 4.02 -> 3.94 ms).
#ifndef ATM_EXP_REG
#define ATM_EXP_REG 1      // the density terms through exp_reg_ (sbx_math.h) when the uniforms are finite
#endif
#ifndef ATM_EXP64
#define ATM_EXP64 1        // ... in its 64-entry / degree-5 form (exp_reg64_: one binary64 fma less, exhaustively equal on |x| <= 80)
#endif
#ifndef ATM_EXP4K
#define ATM_EXP4K 1        // ... in its 4096-entry / degree-3 form (exp_reg4k_: two more fma and a register-pair move less, exhaustively equal
#endif                     // on |x| <= 80).  The 32 KB table is read where it lies, in global memory through the vector L1: 7680x4320
                           // 4.29 -> 4.03 ms.  (A copy in LDS per workgroup of 16 / 8 / 4 waves: 4.28 / 4.05 / 4.23 ms — 65 000 copies of
                           // 32 KB, and a workgroup's LDS is held until its last wave ends; per-CU persistent workgroups that copy once
                           // and walk through the tiles: the tile loop makes the compiler hoist the kernel's constants into registers,
                           // 95 VGPRs / 5 waves or 84 B of scratch at 64, 4.66 ms.  profiles/r03_log.md)
#ifndef ATM_TAU4K
#define ATM_TAU4K 1         // exp(-tau) through exp_reg4k_ where a wave's optical depths allow it
#endif
#ifndef ATM_DIV3
#define ATM_DIV3 1         // FIN kernels: -height / H through div3_ (sbx_math.h; the divisors and their reciprocals held in VGPRs) instead of
#endif                     // div_by's binary64 multiply: |height| is 0 or in [.5, 6.4e6] (a multiple of ulp(6.4e6)), the quotient only feeds exp
#ifndef ATM_SQRT_RS
#define ATM_SQRT_RS 1      // FIN kernels: length(s) of a march position through sqrt_rs_ (sbx_math.h: five instructions, exact for finite
#endif                     // x >= 2^-102): |s|^2 is ~4e13 along rays that stay above the ground; a view ray below the horizon passes through
                           // the planet, but a position's components are multiples of their own ulp, so |s|^2 is either >= 2^-40 or exactly 0,
                           // and exactly 0 needs all three components to cancel at once: rd.x = rd.z = 0 only for theta = 0, the ray straight
                           // UP (acos never returns pi exactly), and a light sample under the ground ends its march before it could reach the
                           // centre.  (isect_atmosphere keeps sqrt_n_: its argument can be exactly 0.)
#define ATM_LEN(x) ((FIN && ATM_SQRT_RS) ? sqrt_rs_(x) : sqrt_n_(x))
// THE GROUND CAMERA (k_atmosphere_ground, SBX_APP_ATMOSPHERE_GROUND: app_atmosphere.h without FROM_SPACE).  Its rays start at the same
// origin (0, R + 1, 0), R = earth_radius, but their directions come from get_primary_ray, not from the dome mapping, so the arguments
// above are restated for them.  A ray reaches atm_incident_light only when intersect_plane records no hit, i.e. when
// denom = dot((0, -1, 0), rd) < 1e-6 is TRUE: that excludes every NaN component (0 * NaN and 0 * inf are NaN) and leaves
// rd.y > -1e-6 with rd.x, rd.z finite.  With a finite camera (FIN) rd is normalize() of a vector whose length is >= 1 (the camera
// basis is fixed: |fwd + up y + right x|^2 >= 1), hence a unit vector to a few ulp — or (0, 0, 0) when the squared length overflows
// (fragCoords beyond 1e19: v / inf; -0 < 1e-6, a sky ray that stays at its origin).  For both:
//   * |s|^2 = (R + 1)^2 + 2 (R + 1) rd.y t + t^2 >= (R + 1)^2 (1 - 1e-12) for every t >= 0: a view sample is never more than 3e-6 m
//     below the camera's own height, so |s| >= 6.36e6 and height = |s| - R is within a rounding (ulp(6.36e6) = .5) of >= 1 m.
//     ATM_SQRT_RS: |s|^2 ~ 4e13, never 0, never inf (t <= t1 <= 2 atmosphere_radius).  The light march starts from such a sample
//     and is the dome's own: each of its samples is at most t1 / 8 <= 1.7e6 from one that is above the ground (or from the view
//     sample), so it stays >= 4.6e6 from the centre.
//   * ATM_DIV3: |s| >= 2^22, so |height| is 0 or a multiple of .5, at most 60e3 + a rounding: inside the dome's domain.
//   * the density exp arguments -height / H lie in [-50.1, +.001] — a sub-range of the dome's [-80, 2^18] (no ray dives into the planet).
//   * ATM_TAU4K tests its own precondition on the wave, whatever the rays are.
//   * DEAD RAYS (atm_incident_light below): no optical depth can overflow (every density term is <= e^.001 * step), so the test is
//     never true for these rays; k_atmosphere_ground compiles it OUT (DEAD = false) rather than carry a ballot per view sample.
// CALLER'S RAYS (k_atmosphere_eval, sbx_atmosphere_eval: any origin, any direction, any sun).  Nothing above holds for a ray the
// kernel has not looked at, so the FIN forms run only on a wave whose 64 rays ALL pass atm_eval_class() below, and only in a launch
// whose sun direction the host has found finite with |dot(sun, sun) - 1| <= 1e-4 (atm_eval_sun_ok); every other wave, and every wave
// of every other launch, runs the plain statement (FIN = false), which is correct for every bit pattern.  The class, in the binary32
// values isect_atmosphere itself computes (oo = dot(rc, rc), tca, d2 = oo - tca^2; R = atmosphere_radius, Re = earth_radius):
//     oo <= R^2   and   d2 >= 1e12   and   |dot(rd, rd) - 1| <= 1e-4
// A NaN fails each comparison and an inf component makes oo or dot(rd, rd) inf or NaN, so all six components are finite; |rd|^2 and
// |sun|^2 are within 1.01e-4 of 1 in exact arithmetic (the binary32 dots carry 2e-7).  Roundings of the quantities of magnitude R^2 =
// 4.1e13 (ulp 4.2e6) and of the positions (ulp .5 m at 6.4e6 m) add up to E <= 2e8 m^2 in every squared distance below.  Three facts:
//   (a) NO SAMPLE IS FAR OUTSIDE THE SPHERE.  Along p(t) = o + d t the squared distance f(t) = |o|^2 - 2 t tca + t^2 |d|^2 is convex,
//       and t1 = tca + thc with thc^2 = R^2 - oo + tca^2 gives f(t1) = R^2 + t1^2 (|d|^2 - 1).  |t1| <= 2.0006 R (|tca| <= 1.0001 R;
//       d2 >= -1.01e-4 oo, so thc <= 1.0001 R), hence every sample of a march whose origin has |o|^2 <= R^2 + 1.7e10 has
//       |p|^2 <= max(f(0), f(t1)) <= R^2 + 1.7e10 + E, i.e. |p| <= R + 1.4 km — whatever the sign of t1, for the view march (origin in
//       the class) and then for every light march (origin a view sample, direction the checked sun).
//   (b) EVERY VIEW SAMPLE IS FAR FROM THE CENTRE.  The ray's line passes the centre at squared distance oo - tca^2 / |d|^2, which
//       differs from d2 by at most 1.01e-4 oo + E <= 4.4e9: every view sample has |s| >= sqrt(1e12 - 4.4e9) - 2 > 9.97e5 m.
//   (c) A VIEW SAMPLE OF A LONG CHORD IS INSIDE THE SPHERE.  At t = lambda t1, lambda in [1/32, 31/32] (sixteen mid-points; the
//       accumulated march_pos moves lambda by 1e-6), the identity t1^2 - 2 t1 tca = R^2 - oo gives
//       f = (1 - lambda) oo + lambda R^2 - lambda (1 - lambda |d|^2) t1^2 <= R^2 - .03 t1^2: strictly inside, with room for E, once
//       t1 >= 140 km (.03 t1^2 >= 5.9e8).  The light ray of such a sample has a t1 that is a number: isect_atmosphere computes its
//       d2' = oo' - tca'^2 <= oo' (a square is subtracted and rounding is monotone), oo' is within E of |s|^2 <= R^2 - 5.9e8, so
//       R^2 - d2' >= 5.9e8 - E > 0 and the root is taken of a positive number.
// The shortcuts, one by one:
//   * ATM_SQRT_RS (|s|^2 in [2^-102, inf)).  View samples: (b) and (a), 9.9e11 <= |s|^2 <= 4.2e13.  Light samples: the first one lies
//     |t1'| / 16 * |sun| <= 2.0006 R / 16 * 1.0001 = 8.03e5 m from its view sample, so it is >= 9.97e5 - 8.03e5 = 1.9e5 m from the centre;
//     every later one is reached only if the one before it was above the ground (:65-67) and lies <= 1.61e6 m from that, >= 4.7e6 m
//     from the centre; (a) bounds them above.  A light ray that MISSES the sphere — possible only from a view sample that (a) lets lie
//     up to 1.4 km outside it — has t1' = NaN: every position, length, quotient, exp and sum of that march is NaN in both forms
//     (sqrt_rs_, div3_ and exp_reg4k_ each return NaN for a NaN: sbx_math.h; exp_reg4k_'s table index is masked), height < 0 is false
//     in both, the sample is "lit" in both, tau is NaN, the ATM_TAU4K ballot sends the wave to the guarded exp, and the pixel is NaN.
//   * ATM_DIV3 (dividend 0 or in [2^-100, 2^100]; the quotient only feeds exp, so the sign of a zero is not used).  View samples:
//     |s| >= 2^19 by (b), so |s| and Re are multiples of 1/16 and height = RN(|s| - Re) is 0 or has 1/16 <= |height| <= 5.4e6.  Light
//     samples reach the division only with height >= 0: |s| >= Re, height 0 or a multiple of .5 up to 61.4e3 (or NaN, above).
//   * exp_reg4k_ on -height / H (arguments in [-80, 2^18]).  By (a) height <= 61.4e3: -height / H >= -51.2.  By (b) a view sample has
//     height >= -5.37e6: -height / H <= 4475; a light sample's argument is <= 0.
//   * ATM_TAU4K tests its own precondition on the wave, whatever the rays are.
//   * DEAD RAYS: compiled IN (DEAD = true) — callers' rays do look below the horizon (half of a dome of them), and those are the rays
//     the exit was written for.  Its argument needs, for every sample after the overflow, (1) the light march's t1' a number (a NaN
//     tau would make the reference's pixel NaN where the exit adds nothing) and (2) hr, hm finite where the sample is lit.  An
//     optical depth overflows only with a sample more than 80 km under the ground (sixteen terms of e^(-height / hM) * step,
//     step <= 8.1e5), which is more than 140 km from the sphere: t1 >= 140 km and (c) gives (1) for every sample of the ray.  (2): the
//     height along the light ray is convex in t (a norm along a line) and is <= 61.4e3 at t1' by (a), so the first light sample, at
//     t1' / 16, is above the ground only if 15 / 16 of the view sample's depth is <= 61.4e3 / 16: a lit sample is at most 4.1 km
//     under the ground, hr and hm <= e^3.5 * step.  Lanes that do not enter the march (d2 < R^2 false: (0, 0, 0)) are not counted
//     by its ballots; lanes past n march (0, Re + 1, 0) + t (1, 0, 0), a ray of the class, and drop the result.
// get_sun_light alone (the entry's second function: sun_light<FIN> along the caller's ray) uses the same class: its samples are view
// samples in the sense of (a) and (b), its t1 is a number (d2 <= oo <= R^2), and it divides and exponentiates only with height >= 0.
constexpr float ATM_EVAL_D2_MIN = 1e12f, ATM_EVAL_UNIT_TOL = 1e-4f;
__device__ __forceinline__ bool atm_eval_class(v3 ro, v3 rd) {
    const v3 rc = V3(0, 0, 0) - ro;
    const float oo = dot(rc, rc), tca = dot(rc, rd);
    const float d2 = oo - tca * tca;
    return oo <= ATM_ATMOS_R * ATM_ATMOS_R && d2 >= ATM_EVAL_D2_MIN && fabsf(dot(rd, rd) - 1.0f) <= ATM_EVAL_UNIT_TOL;
}
// PREC = 1: the TOLERANCE tier (include/sbx.h sbx_set_precision, SBX_PRECISION_1E4; opt-in, never the default, never in bench.py's
// `value`).  north_star's bar is 1e-4 per channel, not bit-equality, and this kernel — 336 exp per in-dome pixel, each 15 instructions
// of binary64 table arithmetic — has no threshold that turns a rounding difference into a different pixel: every exp becomes
// v_exp_f32 of x * log2(e) (two instructions, ~2 ulp) and -height / H one multiply by RN(1 / H).  Everything else (the dome mapping,
// the square roots, the phase functions, the order of every sum, the overflow to +inf of a ray inside the planet) is unchanged.
// Measured against the oracle on every pixel of the 7680x4320 frame and over the sun sweep: tests/test_gpu_round5.py.
__device__ __forceinline__ float atm_exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
#ifndef ATM_TX
#define ATM_TX 1           // waves per workgroup (1: 4.03 ms, 4: 4.06)
#endif
#if ATM_EXP_REG && ATM_EXP4K
#define ATM_EXP_H0(x) (FIN ? exp_reg4k_((x), kExp2Tab4096) : exp_tab_<true>((x), etab))
#elif ATM_EXP_REG && ATM_EXP64
#define ATM_EXP_H0(x) (FIN ? exp_reg64_<false>((x), etab64) : exp_tab_<true>((x), etab))
#elif ATM_EXP_REG
#define ATM_EXP_H0(x) (FIN ? exp_reg_<false>((x), etab) : exp_tab_<true>((x), etab))
#else
#define ATM_EXP_H0(x) exp_tab_<!FIN>((x), etab)
#endif
#define ATM_EXP_H(x) (PREC ? atm_exp_fast(x) : ATM_EXP_H0(x))
#define ATM_EXP(x) (PREC ? atm_exp_fast(x) : exp_tab_<true>((x), etab))

// (march_pos + 0.5 * march_step below is written fma(.5, march_step, march_pos): the half is exact, so it is one rounding either way)
struct AtmDiv { float hr, rhr, hm, rhm; };            // H_R, RN(1 / H_R), H_M, RN(1 / H_M)
#define ATM_DIV_HR(h) (PREC ? (h) * K.rhr : (FIN && ATM_DIV3) ? div3_((h), K.hr, K.rhr) : div_by((h), ATM_HR_RD))
#define ATM_DIV_HM(h) (PREC ? (h) * K.rhm : (FIN && ATM_DIV3) ? div3_((h), K.hm, K.rhm) : div_by((h), ATM_HM_RD))
template <bool FIN, int PREC = 0>
__device__ __forceinline__ bool sun_light(v3 ro, v3 rd, float& odR, float& odM, const double (&etab)[32], const double* etab64, const AtmDiv& K) {   // :50-76
    float t1;
    isect_atmosphere(ro, rd, t1);
    float march_pos = 0.f;
    const float march_step = t1 / 8.f;
#ifndef ATM_BATCH
#define ATM_BATCH 0        // FIN kernels: the eight heights of a sun march first, then its sixteen exp (see below).  MEASURED AND NOT
#endif                     // TAKEN: 7680x4320 3.41 -> 3.57 ms (1), 3.50 (2: first height alone, then the other seven); same bits
    if (FIN && ATM_BATCH) {
        // The reference leaves the march at the first sample under the ground (:65-67) and its caller then ignores the optical
        // depths.  So the eight heights — which depend on nothing but the ray — come first, a lane with any of them negative is
        // done (it never pays for an exp; before, a lane that failed at sample 5 had paid for ten), and the sixteen exp of the
        // other lanes are independent chains of binary64 fma that the scheduler interleaves; the sums keep the reference's order.
        float h[8];
        bool under = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const v3 s = ro + rd * __builtin_fmaf(0.5f, march_step, march_pos);
            h[i] = ATM_LEN(dot(s, s)) - ATM_EARTH_R;
            under = under || (h[i] < 0.f);                      // (a NaN height is not "under": the reference marches on)
            march_pos += march_step;
            if (ATM_BATCH == 2 && i == 0 && under) return false;   // the usual failure is the first sample (far side of the planet)
        }
        if (under) return false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            odR += ATM_EXP_H(ATM_DIV_HR(-h[i])) * march_step;
            odM += ATM_EXP_H(ATM_DIV_HM(-h[i])) * march_step;
        }
        return true;
    }
    for (int i = 0; i < 8; ++i) {
        const v3 s = ro + rd * __builtin_fmaf(0.5f, march_step, march_pos);
        const float height = ATM_LEN(dot(s, s)) - ATM_EARTH_R;   // length(s), |s| ~ 6.4e6
        if (height < 0.f) return false;
        odR += ATM_EXP_H(ATM_DIV_HR(-height)) * march_step;
        odM += ATM_EXP_H(ATM_DIV_HM(-height)) * march_step;
        march_pos += march_step;
    }
    return true;
}

// get_incident_light :78-160 for the ray (ro, rd): 16 view samples, each with an 8-sample march towards the sun
template <bool FIN, int PREC = 0, bool DEAD = true>
__device__ __forceinline__ v3 atm_incident_light(v3 ro, v3 rd, v3 sun_dir, const double (&etab)[32], const double* etab64) {
    v3 col = V3(0.f, 0.f, 0.f);
    float t1;
    AtmDiv K{ATM_HR, 1.0f / ATM_HR, ATM_HM, 1.0f / ATM_HM};
    if ((FIN && ATM_DIV3) || PREC) asm volatile("" : "+v"(K.hr), "+v"(K.rhr), "+v"(K.hm), "+v"(K.rhm));      // VGPR operands: full rate
    if (isect_atmosphere(ro, rd, t1)) {                             // get_incident_light :78-160
        const v3 betaR = V3(5.5e-6f, 13.0e-6f, 22.4e-6f), betaM = V3(21e-6f, 21e-6f, 21e-6f);   // :29-30
        const float march_step = t1 / 16.f;
        const float mu = dot(rd, sun_dir);
        const float phaseR = 3.f * (1.f + mu * mu) / (16.f * 3.14159265359f);            // volumetric.h:13-19
        const float g = .76f;
        const float phaseM = (1.f - g * g) / ((4.f + 3.14159265359f) * pow_(1.f + g * g - 2.f * g * mu, 1.5f));
        float odR = 0.f, odM = 0.f, march_pos = 0.f;
        v3 sumR = V3(0, 0, 0), sumM = V3(0, 0, 0);
        for (int i = 0; i < 16; ++i) {
            const v3 s = ro + rd * __builtin_fmaf(0.5f, march_step, march_pos);
            const float height = ATM_LEN(dot(s, s)) - ATM_EARTH_R;   // length(s)
            const float hr = ATM_EXP_H(ATM_DIV_HR(-height)) * march_step;
            const float hm = ATM_EXP_H(ATM_DIV_HM(-height)) * march_step;
            odR += hr;
            odM += hm;
            // DEAD RAYS.  A view ray below the horizon dives into the planet (there is no ground test in this march, :119-122);
            // 106 km down exp(-height / hM) overflows and optical_depthM is +inf from then on (709 km: optical_depthR).  Every
            // later sample's tau = betaR (odR + lR) + 1.1 betaM (odM + lM) is then +inf in all three components — the terms are
            // non-negative, so no inf - inf — its attenuation exp(-inf) is exactly 0, and what it would add, hr * 0 and hm * 0, is
            // exactly +0: a sample is only lit when its FIRST light sample is above the ground (:65-67), which the geometry
            // allows down to ~4 km under it (a light step is at most 1/16 of the way out of the atmosphere), so the hr, hm of a
            // lit sample are finite (<= e^3.4 * step).  So a lane whose optical depth has overflowed is finished: it skips the
            // sun marches of its far-side samples (which the reference runs for nothing), and the march ends when the whole
            // wave is finished.  The band 1.09 < z2 <= 1.4 of the dome — 10 % of a 16:9 frame — paid a sky pixel's full price for
            // a black pixel before: 7680x4320 3.90 -> 3.66 ms, same bits (tools/ab_time.py; waves that mix finished and live rays still pay).
#ifndef ATM_DEAD_EXIT
#define ATM_DEAD_EXIT 1
#endif
            const float inf = u2f(0x7f800000u);
            const bool dead = DEAD && ATM_DEAD_EXIT && (odR == inf || odM == inf);
            if (DEAD && ATM_DEAD_EXIT && __builtin_amdgcn_ballot_w64(!dead) == 0ull) break;      // wave-uniform
            float lR = 0.f, lM = 0.f;
            if (!dead && sun_light<FIN, PREC>(s, sun_dir, lR, lM, etab, etab64, K)) {
                const v3 tau = betaR * (odR + lR) + betaM * 1.1f * (odM + lM);
                // exp(-tau): the guard-less form where every lane that got here has all three tau <= 80 (tau >= 0: sums of
                // non-negative terms; a NaN fails the test), exp_'s guarded form for the wave otherwise (grazing sun rays)
                v3 att;
                if (!PREC && FIN && ATM_EXP_REG && ATM_EXP4K && ATM_TAU4K &&
                    __builtin_amdgcn_ballot_w64(!(fmax_(fmax_(tau.x, tau.y), tau.z) <= 80.f)) == 0ull)
                    att = V3(exp_reg4k_(-tau.x, kExp2Tab4096), exp_reg4k_(-tau.y, kExp2Tab4096), exp_reg4k_(-tau.z, kExp2Tab4096));
                else
                    att = V3(ATM_EXP(-tau.x), ATM_EXP(-tau.y), ATM_EXP(-tau.z));
                sumR = sumR + hr * att;
                sumM = sumM + hm * att;
            }
            march_pos += march_step;
        }
        col = 20.0f * (sumR * phaseR * betaR + sumM * phaseM * betaM);   // sun_power :41
    }
    return col;
}

// CALLER'S AIR (kern_atmosphere_air.hip: SBX_APP_ATMOSPHERE_AIR, sbx_atmosphere_air_eval — every number above from the caller's block,
// AtmAir in sbx_frame.h).  Three tiers, chosen on the host (sbx_frames.hip atmosphere_air_tier):
//   LITERAL   a block whose solver numbers are the literals above bit for bit launches k_atmosphere / k_atmosphere_ground themselves
//             with the block's sun.  Their FIN forms were argued for the sun setup_scene rotates out of (0, 1, 0); for another sun
//             they run only where the host finds it finite with |dot(sun, sun) - 1| <= 1e-4 (atm_eval_sun_ok's test), and then:
//               * every view sample of a ray from (0, Re + 1, 0) lies inside the sphere (dome rays are unit vectors to a few ulp or NaN,
//                 ground-camera rays unit vectors or (0, 0, 0): above), so fact (a) holds with the view sample as origin and the checked
//                 sun as direction: no light sample is more than 1.4 km outside the sphere, -height / H >= -51.2; a view sample at
//                 lambda <= 31/32 of t1 >= 60 km - 1 has |s|^2 <= R^2 - (R^2 - (Re + 1)^2) / 32 = R^2 - 2.4e10, so its light ray's t1 is a number;
//               * ATM_SQRT_RS on light samples.  k_atmosphere carries the dead-ray exit: a view sample more than 107 km under the ground
//                 has made optical_depthM +inf (e^88.8 overflows) and its lane runs no sun march, so a light march starts >= 6.25e6 m
//                 from the centre, its first sample <= 8.03e5 m further, every later one <= 1.61e6 m from one above the ground: never
//                 within 4.7e6 m of the centre, whatever the sun's direction.  k_atmosphere_ground: no view sample is under the camera's
//                 height, the same steps (its paragraph above reads "the dome's own" with any such sun);
//               * ATM_DIV3, the density exp: heights are finite, 0 or >= 1/16 in magnitude, and >= -107 km where a sun march runs;
//               * the ground camera's direction is a unit vector only while its basis is one: the host also asks |dot(fwd, fwd) - 1| <= 1e-4
//                 of the block's look_at - eye (a difference whose squared length is subnormal normalises to something else).
//             A sun that fails the test, or such a basis, takes FIN = false.
//   RUN-TIME  k_atmosphere_air<VIEW, true> / k_atmosphere_air_eval<FN, true>: both bodies, the fast one (FAST = true below: exp_reg4k_,
//             div3_, sqrt_rs_, the tau ballot, the dead-ray exit) on a wave whose 64 rays all pass atm_eval_class, and only in a launch
//             whose block the host finds TAME (sbx_frames.hip atmosphere_air_tame):
//                 earth_radius, atmosphere_radius, hR, hM equal to ATM_EARTH_R, ATM_ATMOS_R, ATM_HR, ATM_HM bit for bit, the counts
//                 16 and 8, and a sun that is finite with |dot(sun, sun) - 1| <= 1e-4.
//             That is the domain of "CALLER'S RAYS" above with Re, R, H_R, H_M read from registers instead of literals: facts (a)-(c)
//             and the bounds of exp_reg4k_ ([-80, 2^18]), div3_ (dividend 0 or in [2^-100, 2^100], divisor 1200 or 7994) and sqrt_rs_
//             ([2^-102, inf)) are those paragraphs word for word, with the class test made on the rays the kernel itself builds from the
//             block's eye (a lane without a march — outside the dome's circle, or a ground pixel — holds the ray (0, Re + 1, 0) + t
//             (1, 0, 0) of the class and drops the result).  No other radius, scale height or count is in the domain: those proofs have
//             not been restated, such blocks run plain.  What the block may vary inside the domain enters no proof but two:
//               * the tau ballot tests its own precondition, here as |tau| <= 80 per component (a NaN or inf tau, from any beta, fails
//                 it; a negative beta's negative tau stays inside exp_reg4k_'s [-80, 2^18]);
//               * the DEAD-RAY exit needs tau = +inf in all three components once an optical depth is +inf: betaR (odR + lR) +
//                 1.1 betaM (odM + lM) with every beta > 0 (a number; 1.1 * the smallest subnormal is still > 0) is a sum of
//                 non-negative terms one of which is +inf; a zero beta would make 0 * inf, a negative one -inf.  AtmAir.dead_ok states it,
//                 and the exit is off without it.  sun_power, hg_g and the phase terms multiply the sums after the march; fov and the
//                 eye only make rays, which the class judges.
//             t1 / float(n) is the compiler's IEEE division in both bodies (17 per pixel against 336 exp).
//   PLAIN     FAST = false for every wave (sbx_set_variant 1, every untame block): the plain statement lane by lane — IEEE sqrt (sqrt_:
//             a block's radii can make arguments below sqrt_n_'s 2^-96), IEEE division by the block's hR and hM, the guarded exp — correct
//             for every bit pattern of block.
template <bool FAST>
__device__ __forceinline__ bool air_isect(v3 ro, v3 rd, float atmos_r, float& t1) {                   // isect_sphere :15-26
    const v3 rc = V3(0, 0, 0) - ro;
    const float radius2 = atmos_r * atmos_r;
    const float tca = dot(rc, rd);
    const float d2 = dot(rc, rc) - tca * tca;
    const float thc = FAST ? sqrt_n_(radius2 - d2) : sqrt_(radius2 - d2);   // (FAST: the default radii, as isect_atmosphere)
    t1 = tca + thc;
    return d2 < radius2;
}
#define AIR_LEN(x) (FAST ? sqrt_rs_(x) : sqrt_(x))
#define AIR_EXP_H(x) (FAST ? exp_reg4k_((x), kExp2Tab4096) : exp_tab_<true>((x), etab))
#define AIR_DIV_HR(h) (FAST ? div3_((h), hr_d, hr_r) : (h) / K.hR)
#define AIR_DIV_HM(h) (FAST ? div3_((h), hm_d, hm_r) : (h) / K.hM)
// get_sun_light :50-76 with the block's numbers; NL: the literal count of the fast body (the tame domain has one), 0 = K.nl
template <bool FAST, int NL>
__device__ __forceinline__ bool air_sun_light(v3 ro, v3 rd, float& odR, float& odM, const double (&etab)[32], const AtmAir& K,
                                              float hr_d, float hr_r, float hm_d, float hm_r) {
    float t1;
    air_isect<FAST>(ro, rd, K.atmos_r, t1);
    const int nl = NL ? NL : K.nl;
    float march_pos = 0.f;
    const float march_step = t1 / (float)nl;
    for (int i = 0; i < nl; ++i) {
        const v3 s = ro + rd * __builtin_fmaf(0.5f, march_step, march_pos);
        const float height = AIR_LEN(dot(s, s)) - K.earth_r;
        if (height < 0.f) return false;
        odR += AIR_EXP_H(AIR_DIV_HR(-height)) * march_step;
        odM += AIR_EXP_H(AIR_DIV_HM(-height)) * march_step;
        march_pos += march_step;
    }
    return true;
}
// get_incident_light :78-160 with the block's numbers
template <bool FAST, int NS, int NL>
__device__ __forceinline__ v3 air_incident_light(v3 ro, v3 rd, v3 sun_dir, const double (&etab)[32], const AtmAir& K) {
    v3 col = V3(0.f, 0.f, 0.f);
    float t1;
    float hr_d = K.hR, hr_r = K.rhR, hm_d = K.hM, hm_r = K.rhM;
    if (FAST) asm volatile("" : "+v"(hr_d), "+v"(hr_r), "+v"(hm_d), "+v"(hm_r));      // VGPR operands: full rate
    if (air_isect<FAST>(ro, rd, K.atmos_r, t1)) {
        const v3 betaR = K.betaR, betaM = K.betaM;
        const int ns = NS ? NS : K.ns;
        const float march_step = t1 / (float)ns;
        const float mu = dot(rd, sun_dir);
        const float phaseR = 3.f * (1.f + mu * mu) / (16.f * 3.14159265359f);            // volumetric.h:13-19
        const float g = K.g;
        const float phaseM = (1.f - g * g) / ((4.f + 3.14159265359f) * pow_(1.f + g * g - 2.f * g * mu, 1.5f));   // :27-33
        float odR = 0.f, odM = 0.f, march_pos = 0.f;
        v3 sumR = V3(0, 0, 0), sumM = V3(0, 0, 0);
        for (int i = 0; i < ns; ++i) {
            const v3 s = ro + rd * __builtin_fmaf(0.5f, march_step, march_pos);
            const float height = AIR_LEN(dot(s, s)) - K.earth_r;
            const float hr = AIR_EXP_H(AIR_DIV_HR(-height)) * march_step;
            const float hm = AIR_EXP_H(AIR_DIV_HM(-height)) * march_step;
            odR += hr;
            odM += hm;
            const float inf = u2f(0x7f800000u);
            const bool dead = FAST && K.dead_ok && (odR == inf || odM == inf);          // DEAD RAYS, above
            if (FAST && K.dead_ok && __builtin_amdgcn_ballot_w64(!dead) == 0ull) break;   // wave-uniform
            float lR = 0.f, lM = 0.f;
            if (!dead && air_sun_light<FAST, NL>(s, sun_dir, lR, lM, etab, K, hr_d, hr_r, hm_d, hm_r)) {
                const v3 tau = betaR * (odR + lR) + betaM * 1.1f * (odM + lM);
                v3 att;
                // (each component by itself and in magnitude: a caller's betas can make ONE tau a NaN, or any of them negative, and
                // exp_reg4k_'s domain ends at 2^18)
                if (FAST && __builtin_amdgcn_ballot_w64(!(fabsf(tau.x) <= 80.f && fabsf(tau.y) <= 80.f && fabsf(tau.z) <= 80.f)) == 0ull)
                    att = V3(exp_reg4k_(-tau.x, kExp2Tab4096), exp_reg4k_(-tau.y, kExp2Tab4096), exp_reg4k_(-tau.z, kExp2Tab4096));
                else
                    att = V3(exp_tab_<true>(-tau.x, etab), exp_tab_<true>(-tau.y, etab), exp_tab_<true>(-tau.z, etab));
                sumR = sumR + hr * att;
                sumM = sumM + hm * att;
            }
            march_pos += march_step;
        }
        col = K.sun_power * (sumR * phaseR * betaR + sumM * phaseM * betaM);
    }
    return col;
}

}  // namespace sbx
