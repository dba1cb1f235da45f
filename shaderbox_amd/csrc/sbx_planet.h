// shaderbox_amd/csrc/sbx_planet.h — what the two translation units of APP_PLANET share: the cooperative fBm over the per-wave
// lattice-hash cache, the cloud shell's density and integrator, both terrain maps, the paired central differences of the terrain
// normal, setup_lights and background (k_planet of kern_planet.hip, k_planet_eval of kern_planet_eval.hip), with the switches and the
// domain arguments of their short forms.  src/app_planet.h :23-41, :79-119, :175-236.
#pragma once
#ifndef SBX_WG_WAVES
#define SBX_WG_WAVES 1
#endif
#ifndef SBX_HC_SLOTS
#define SBX_HC_SLOTS 32         // 4.7 KB of LDS per wave: 5 waves per SIMD fit (64 slots: 9.3 KB, 4 waves)
#endif
#include "sbx_device.h"
#include "sbx_noise.h"
#include "sbx_hashcache.h"
#include "sbx_exp4k_table.h"
#include "sbx_atmosphere.h"

// All noise_iq evaluations go through the per-wave lattice-hash cache (sbx_hashcache.h): octave k of any fBm
// uses table k & 3.  The cross-lane steps of the cache need wave-uniform control flow, so lanes never leave
// a loop early; they carry predicates (`tm` terrain march, `cm` cloud march, `hitl` ground hit) and the loops
// test wave_any().  A predicated-off lane still evaluates the arithmetic (harmlessly) but commits nothing.

namespace sbx {

constexpr float PL_MAX_HEIGHT = .4f;                    // :20
constexpr float PL_MAX_RAY_DIST = PL_MAX_HEIGHT * 4.f;  // :21

struct Vol { v3 origin, pos; float height, transmittance, radiance, alpha; };   // volumetric.h:47-68 (radiance r=g=b)
__device__ __forceinline__ Vol make_vol(v3 o) { return Vol{o, o, 0.f, 1.f, 0.f, 0.f}; }

// smoothstep with literal edges: the division by (e1 - e0) is an exact multiply by its binary64 reciprocal — or, in the SKIP kernels,
// div3_ of sbx_math.h: three full-rate binary32 instructions with the literal divisor and its reciprocal, equal to the IEEE quotient
// for every pair of significands.  Its domain (finite dividend, zero or within 2^+-100; the sign of a zero quotient unused) holds on
// the tame frames those kernels run for: the dividends are differences of numbers of order 1 (zero or >= 2^-26), exp of a height in
// [-2.5, 2], a smoothstep value (zero or >= 2^-60) or |p| - 1 (zero — always +0 — or >= 2^-24); a NaN gives NaN either way.
#ifndef PL_DIV3
#define PL_DIV3 1
#endif
#define PL_DIVK(a, dlit) ((SKIP && PL_DIV3) ? div3_((a), (dlit), 1.0f / (dlit)) : div_by((a), 1.0 / (double)(dlit)))
#ifndef PL_MED3
#define PL_MED3 1           // the clamp of those smoothsteps as one v_med3_f32: their arguments (fBm sums of hashes, heights of finite positions)
#endif                      // are never NaN on the tame frames of the SKIP kernels (finite u_time, u_res checked by the C API, and a camera
                            // whose eye and look_at are finite constants — the shipped one and PLANET_CLOSEUP's alike: fwd, up and right are
                            // orthogonal with |fwd| = 1, so fwd + up y + right x is finite and no shorter than 1, rd and every march position
                            // are finite, and so are their heights, with either form of pl_length)
#define SMOOTHSTEP_K(e0, e1, x) ((SKIP && PL_DIV3 && PL_MED3) ? smoothstep_d3_med3((e0), (e1) - (e0), 1.0f / ((e1) - (e0)), (x)) \
                                 : (SKIP && PL_DIV3) ? smoothstep_d3((e0), (e1) - (e0), 1.0f / ((e1) - (e0)), (x)) \
                                                   : smoothstep_rd((e0), 1.0 / (double)((e1) - (e0)), (x)))
// ---- where the header's numbers come from ----------------------------------------------------------------------------------------
// clouds_density, clouds_map, terrain_map and terrain_detail_difference below read every number that src/app_planet.h states as a
// one-line literal from a POLICY, their last template parameter and last argument.  PlLit (the default: callers that name no policy
// are k_planet and k_planet_eval as they always were) holds the literals as literals, with the exact-reciprocal multiplies and the
// literal div3_ pairs of PL_DIVK / SMOOTHSTEP_K; PlCloudW and PlTerrW read the parts of a FramePlanetWorld (sbx_frame.h: the caller's
// block of SBX_APP_PLANET_WORLD and sbx_planet_world_eval), dividing by a block's value with div3_ and the host's RN(1 / d) under
// SKIP and with the IEEE division otherwise.  The domains under which SKIP may be taken with a caller's numbers are argued in
// kern_planet_world.hip.  What is NOT a policy's business stays written once, here: the fBm scales, lacunarities, gains and octave
// staging, the terrain edges .35 / .6 / 1 and the TAIL bounds, the .1876 / .06255 of the coverage early-outs, the PL_TB2 tables.
struct PlLit {
    template <bool SKIP> __device__ __forceinline__ float band(float t) const {     // band(.2, .35, .65, t)  util.h:103-112
        return SMOOTHSTEP_K(.2f, .35f, t) * (1.f - SMOOTHSTEP_K(.35f, .65f, t));
    }
    __device__ __forceinline__ v3 cloud_offset() const { return V3(.35f, 13.35f, 2.67f); }          // :107
    __device__ __forceinline__ float cov() const { return .29475675f; }                              // :110
    template <bool SKIP> __device__ __forceinline__ float cov_smoothstep(float dens) const {        // :112
        const float cov = .29475675f, fuzzy = .0335f;
        return SMOOTHSTEP_K(cov, cov + fuzzy, dens);
    }
    __device__ __forceinline__ float absorb_arg(float dens, float t_step) const { return -30.034f * dens * t_step; }   // :87
    template <bool SKIP> __device__ __forceinline__ float light_div(float e) const { return PL_DIVK(e, .055f); }       // :76
    __device__ __forceinline__ v3 terrain_offset() const { return V3(1.9489f, 2.435f, .5483f); }    // :180, :193
    __device__ __forceinline__ float max_height() const { return PL_MAX_HEIGHT; }
    template <bool SKIP> __device__ __forceinline__ float div_height(float a) const { return PL_DIVK(a, PL_MAX_HEIGHT); }
};
template <bool SKIP>
__device__ __forceinline__ float pw_div(float a, float d, float r) { return (SKIP && PL_DIV3) ? div3_(a, d, r) : a / d; }
// smoothstep(e0, e1, x) with d = e1 - e0 and r = RN(1 / d) from the host
template <bool SKIP>
__device__ __forceinline__ float pw_smoothstep(float e0, float e1, float d, float r, float x) {
    return (SKIP && PL_DIV3 && PL_MED3) ? smoothstep_d3_med3(e0, d, r, x) : (SKIP && PL_DIV3) ? smoothstep_d3(e0, d, r, x) : smoothstep_(e0, e1, x);
}
struct PlCloudW {
    const PlanetWorldCloud& c;
    template <bool SKIP> __device__ __forceinline__ float band(float t) const {
        return pw_smoothstep<SKIP>(c.band0, c.band1, c.band_d01, c.band_r01, t) * (1.f - pw_smoothstep<SKIP>(c.band1, c.band2, c.band_d12, c.band_r12, t));
    }
    __device__ __forceinline__ v3 cloud_offset() const { return c.cloud_offset; }
    __device__ __forceinline__ float cov() const { return c.cov; }
    template <bool SKIP> __device__ __forceinline__ float cov_smoothstep(float dens) const { return pw_smoothstep<SKIP>(c.cov, c.cov_hi, c.cov_d, c.cov_r, dens); }
    __device__ __forceinline__ float absorb_arg(float dens, float t_step) const { return c.neg_absorb * dens * t_step; }
    template <bool SKIP> __device__ __forceinline__ float light_div(float e) const { return pw_div<SKIP>(e, c.cloud_light, c.cloud_light_r); }
    __device__ __forceinline__ float max_height() const { return c.max_height; }
    template <bool SKIP> __device__ __forceinline__ float div_height(float a) const { return pw_div<SKIP>(a, c.max_height, c.max_height_r); }
};
struct PlTerrW {
    const PlanetWorldTerrain& t;
    __device__ __forceinline__ v3 terrain_offset() const { return t.terrain_offset; }
    __device__ __forceinline__ float max_height() const { return t.max_height; }
    template <bool SKIP> __device__ __forceinline__ float div_height(float a) const { return pw_div<SKIP>(a, t.max_height, t.max_height_r); }
};
template <bool SKIP>
__device__ __forceinline__ float band(float t) { return PlLit().band<SKIP>(t); }

// DECL_FBM_FUNC(name, OCT, basis(noise_iq(p)))  fbm.h:6 — the OCT noise values come from one cooperative batch
// MODE 0: noise(p)   1: anoise = |2 noise - 1| (:65)   2: rnoise = 1 - |2 noise - 1| (:167)
template <int MODE>
__device__ __forceinline__ float pl_basis(float n) {
    if (MODE == 0) return n;
    // (n * 2 is exact, so n * 2 - 1 is one rounding: fma(n, 2, -1) has the reference's bits)
    if (MODE == 1) return abs_(__builtin_fmaf(n, 2.f, -1.f));
    return 1.f - abs_(__builtin_fmaf(n, 2.f, -1.f));
}
template <int OCT, int MODE>
__device__ __forceinline__ float pl_fbm_from(const float (&nz)[OCT], float init_gain, float gain) {
    float H = init_gain, t = 0.f;
#pragma unroll
    for (int i = 0; i < OCT; ++i) {
        t += pl_basis<MODE>(nz[i]) * H;
        H *= gain;
    }
    return t;
}

// fBm over the cached noise: octaves START..OCT-1 are fetched in cooperative batches of <= 4 (register budget) and
// added to (t, H, q) in octave order exactly as fbm.h:6 (t += basis * H; p *= lacunarity; H *= gain)
#ifndef PL_BATCH
#define PL_BATCH 3          // octaves fetched per cooperative batch: 4 at a time (round 1) peaked at 32 hash registers and spilled; 3 (round 5): 91 VGPRs, no scratch, -0.5 % against 2
#endif
#ifndef PL_ROLL_DETAIL
#define PL_ROLL_DETAIL 1
#endif
#ifndef PL_BATCH_DETAIL
#define PL_BATCH_DETAIL 2   // the 7-octave detail maps of the hit shading (6 per hit pixel)
#endif
#ifndef PL_SPEC
#define PL_SPEC 1           // the hash pass of a lone pending cell also hashes the rest of the 2 x 2 x 2 block ahead of the march
#endif                      // (sbx_hashcache.h hc_insert SPEC; the SKIP kernels only)
#ifndef PL_TB2
#define PL_TB2 3            // table of octave k of terrain_map's SECOND fBm: (PL_TB2 + k) & 3 — with 0 its octave k shares table k with
#endif                      // the first fBm's octave k (another lattice), and the two evict each other's cells on every slot clash
template <int OCT, int MODE, int START, bool XI = false, int TB = 0>
__device__ __forceinline__ void coop_fbm_range(WaveCache& S, v3& q, float lacunarity, float& H, float gain, float& t, bool on, int lane) {
    constexpr int B = (OCT == 7) ? PL_BATCH_DETAIL : PL_BATCH;
#if PL_ROLL_DETAIL
    if (OCT == 7) {
        // the 7-octave detail maps as a REAL loop over their batches (same operations in the same order): unrolled, the six maps of
        // the hit shading are ~40 KB of straight-line code that the scheduler interleaves across octaves — the spills of the kernel
        constexpr int NB = (OCT - START) / B;
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const int base = START + b * B;
            v3 p[B]; int tab[B]; float nz[B];
#pragma unroll
            for (int i = 0; i < B; ++i) { p[i] = q; tab[i] = (TB + base + i) & 3; q = q * lacunarity; }
            coop_noise_n<B, XI, XI && PL_SPEC>(S, p, tab, on, lane, nz);
#pragma unroll
            for (int i = 0; i < B; ++i) { t += pl_basis<MODE>(nz[i]) * H; H *= gain; }
        }
        constexpr int R = (OCT - START) % B;
        if (R > 0) {
            v3 p[R > 0 ? R : 1]; int tab[R > 0 ? R : 1]; float nz[R > 0 ? R : 1];
#pragma unroll
            for (int i = 0; i < R; ++i) { p[i] = q; tab[i] = (TB + START + NB * B + i) & 3; q = q * lacunarity; }
            coop_noise_n<(R > 0 ? R : 1), XI, XI && PL_SPEC>(S, p, tab, on, lane, nz);
#pragma unroll
            for (int i = 0; i < R; ++i) { t += pl_basis<MODE>(nz[i]) * H; H *= gain; }
        }
        return;
    }
#endif
#pragma unroll
    for (int base = START; base < OCT; base += B) {
        if (base + B <= OCT) {
            v3 p[B]; int tab[B]; float nz[B];
#pragma unroll
            for (int i = 0; i < B; ++i) { p[i] = q; tab[i] = (TB + base + i) & 3; q = q * lacunarity; }
            coop_noise_n<B, XI, XI && PL_SPEC>(S, p, tab, on, lane, nz);
#pragma unroll
            for (int i = 0; i < B; ++i) { t += pl_basis<MODE>(nz[i]) * H; H *= gain; }
        } else {
            constexpr int R = (OCT - START) % B;
            v3 p[R > 0 ? R : 1]; int tab[R > 0 ? R : 1]; float nz[R > 0 ? R : 1];
#pragma unroll
            for (int i = 0; i < R; ++i) { p[i] = q; tab[i] = (TB + base + i) & 3; q = q * lacunarity; }
            coop_noise_n<(R > 0 ? R : 1), XI, XI && PL_SPEC>(S, p, tab, on, lane, nz);
#pragma unroll
            for (int i = 0; i < R; ++i) { t += pl_basis<MODE>(nz[i]) * H; H *= gain; }
        }
    }
}
template <int OCT, int MODE, bool XI = false>
__device__ __forceinline__ float coop_fbm(WaveCache& S, v3 q, float lacunarity, float init_gain, float gain, bool on, int lane) {
    float H = init_gain, t = 0.f;
    coop_fbm_range<OCT, MODE, 0, XI>(S, q, lacunarity, H, gain, t, on, lane);
    return t;
}

// The two exp of a cloud sample in the SKIP kernels: exp_reg4k_ of sbx_math.h (4096-entry table read through the vector L1, degree 3,
// no range guard: 15 instructions against exp_'s 21), equal to exp_ for |x| <= 80.  The SKIP kernels run only for tame frames
// (sbx_capi.hip tame_time: finite, bounded camera), where a sample lies within the atmosphere shell: the arguments are
// -30.034 * dens * t_step with dens in [0, .94] and t_step <= .08, i.e. [-2.26, 0], and height = (|p| - 1) / .4 in [-2.5, 1.1]; a NaN
// stays a NaN in both forms.  7680x4320: see profiles/r03_log.md.
#ifndef PL_EXP4K
#define PL_EXP4K 1
#endif
// length() of a march position in the SKIP kernels: sqrt_n_ of sbx_math.h — v_sqrt_f32 and the two-sided fix-up WITHOUT the input
// scaling and class tests of the compiler's IEEE expansion (~35 instead of ~60 issue cycles), bit-identical to it for every
// argument that is 0, not finite, negative, or >= 2^-96 (all 2^32 run: test_sqrt_n_is_ieee_sqrt).  Here the argument is |p|^2 of a
// point p = rot * (eye + s * rd) with the reference's fixed eye (0, 0, -2.5) (:47-58): lanes that miss the atmosphere keep
// o == 0 exactly (hit_o = 0, t = 0), every other lane has rd.x, rd.y either exactly 0 (the centre ray, which stops on the terrain
// at |o| >= 1) or >= 1e-6 in magnitude (pixel centres), and o.x = (t0 + t) * rd.x has no cancellation: |o|^2 >= 1e-12 >> 2^-96 = 1.3e-29.
// The SKIP kernels run only for tame frames (finite, bounded u_time); a NaN resolution gives NaN, which sqrt_n_ passes through.
// This rests on the SHIPPED camera: the rays of PLANET_CLOSEUP's (eye (0, 0, -1.93), look_at (-.1, .9, 2)) are not aligned with the
// planet's axis, so "rd.x, rd.y are 0 or >= 1e-6" does not hold for them.  A camera-free bound exists for most samples — a terrain
// sample has |o| - 1 >= df.x and the march advances by .4567 df.x, so |o| > 1 at every sample and between any two of them, and a
// cloud sample lies on the same ray no deeper than max_cld — but not for all: a march that uses up its 120 steps without a hit and
// without passing max_ray_dist leaves max_cld at 1.6, and the cloud samples beyond its last step are bounded by nothing but the
// ray's closest approach to the centre.  No frame is known to hold such a ray; no argument here excludes one.  So the CLOSEUP
// instantiation takes the IEEE root for every length (RS = false) and keeps every other short form, none of which names the eye.
#ifndef PL_SQRT_RS
#define PL_SQRT_RS 1
#endif
#ifndef PL_SQRT_N
#define PL_SQRT_N 1
#endif
template <bool RS>
__device__ __forceinline__ float pl_length(v3 v) {
    // (PL_SQRT_RS: sqrt_rs_, five instructions, exact for finite x >= 2^-102 — the lanes whose |o|^2 is exactly 0 are the ones that
    //  missed the atmosphere: they never commit a result, and what they compute here, a NaN, decides nothing)
    return (RS && PL_SQRT_RS) ? sqrt_rs_(dot(v, v)) : (RS && PL_SQRT_N) ? sqrt_n_(dot(v, v)) : length(v);
}
#define PL_EXP(x) ((SKIP && PL_EXP4K) ? exp_reg4k_((x), kExp2Tab4096) : exp_(x))
// clouds_map :102-119 + integrate_volume :79-100; `on` = lanes that commit
// SKIP = false (sbx_set_variant 1) evaluates everything: the reference form, kept for the parity sweeps
// The density part of clouds_map: false = nothing would change for any committing lane of the wave (see below), else
// dens and T_i = exp(-30.034 dens t_step) of every lane are set.
template <bool SKIP, class P = PlLit>
__device__ __forceinline__ bool clouds_density(WaveCache& S, v3 pos, float height, float t_step, bool on, int lane, float& dens_out,
                                               float& T_i_out, const P& w = P()) {
    // The cloud shell is the height band (.2, .65): outside it band() is exactly +0, so dens = fbm * 0 = +0,
    // T_i = exp(-0) = 1, and the three updates below are `*= 1`, `+= 0`, `+= 0 * (1 - alpha)`: nothing changes.
    // When that holds for every committing lane of the wave the noise is not evaluated at all (most steps of the
    // 75-step march and 2-3 of the 5 shadow steps).  A NaN height compares unequal and takes the full path.
    const float bd = w.template band<SKIP>(height);
    if (SKIP && !wave_any(on && bd != 0.f)) return false;
    // fbm of |2 noise - 1| in [0, 1], gains .5 .25 .125 .0625: evaluated in stages {0,1}, {2}, {3}; once the part so far
    // plus the largest possible rest is below the coverage edge for every committing lane, smoothstep(cov, ..) is
    // exactly 0, the density +0, and nothing below would change anything.
    // (with a caller's numbers the two early-outs below also need cld_fuzzy > 0 and a finite coverage: kern_planet_world.hip)
    const float cov = w.cov();
    v3 q = pos * 3.2343f + w.cloud_offset();
    float H = .5f, dens = 0.f;
    // (SKIP kernels run only for tame frames — sbx_capi.hip tame_time — where every lattice coordinate is a small integer: XI)
    coop_fbm_range<2, 1, 0, SKIP>(S, q, 2.0276f, H, .5f, dens, on, lane);
    if (SKIP && !wave_any(on && !(dens + .1876f < cov))) return false;
    coop_fbm_range<3, 1, 2, SKIP>(S, q, 2.0276f, H, .5f, dens, on, lane);
    if (SKIP && !wave_any(on && !(dens + .06255f < cov))) return false;
    coop_fbm_range<4, 1, 3, SKIP>(S, q, 2.0276f, H, .5f, dens, on, lane);
    dens *= w.template cov_smoothstep<SKIP>(dens);
    dens *= bd;
    // dens is exactly +0 below the coverage edge as well (smoothstep = 0): same identities, skip the two exp
    if (SKIP && !wave_any(on && dens != 0.f)) return false;
    dens_out = dens;
    T_i_out = PL_EXP(w.absorb_arg(dens, t_step));
    return true;
}
// clouds_map :102-119 + integrate_volume :79-100; `on` = lanes that commit
// SKIP = false (sbx_set_variant 1) evaluates everything: the reference form, kept for the parity sweeps
template <bool SKIP, class P = PlLit>
__device__ __forceinline__ void clouds_map(WaveCache& S, Vol& c, float t_step, bool on, int lane, const P& w = P()) {
    float dens = 0.f, T_i = 1.f;
    if (!clouds_density<SKIP, P>(S, c.pos, c.height, t_step, on, lane, dens, T_i, w)) return;
    if (on) {
        c.transmittance *= T_i;
        c.radiance += dens * w.template light_div<SKIP>(PL_EXP(c.height)) * c.transmittance * t_step;
        c.alpha += (1.f - T_i) * (1.f - c.alpha);
    }
}

// sdf_terrain_map / sdf_terrain_map_detail :175-199
template <int OCT, bool SKIP, bool RS = SKIP, class P = PlLit>
__device__ __forceinline__ v2 terrain_map(WaveCache& S, v3 pos, bool on, int lane, const P& w = P()) {
    const float h0 = coop_fbm<OCT, 0, SKIP>(S, pos * 2.0987f, 2.0244f, .454f, .454f, on, lane);
    const float n0 = SMOOTHSTEP_K(.35f, 1.f, h0);
    // Second fBm (ridged basis, values in [0, 1]): n1 = smoothstep(.6, 1, h1) is exactly +0 whenever h1 < .6.
    // After the first octave, h1 <= t + (.454^2 + ... + .454^OCT); when that bound is below .6 for every
    // committing lane of the wave the remaining octaves cannot change n1 = +0 and are not evaluated.
    v3 q = pos * 1.50987f + w.terrain_offset();
    float H = .454f, h1 = 0.f;
    coop_fbm_range<1, 2, 0, SKIP, PL_TB2>(S, q, 2.0244f, H, .454f, h1, on, lane);
    constexpr float TAIL = (OCT == 3) ? .2998f : .3745f;       // sum of .454^k, k = 2..OCT, rounded up (OCT = 3 or 7)
    static_assert(OCT == 3 || OCT == 7, "tail bound tabulated for 3 and 7 octaves");
    float n1 = 0.f;
    if (!SKIP || wave_any(on && !(h1 + TAIL * 1.0001f < .6f))) {
        coop_fbm_range<OCT, 2, 1, SKIP, PL_TB2>(S, q, 2.0244f, H, .454f, h1, on, lane);
        n1 = SMOOTHSTEP_K(.6f, 1.f, h1);
    }
    const float n = n0 + n1;
    return V2(pl_length<RS>(pos) - 1.f - n * w.max_height(), w.template div_height<SKIP>(n));
}


// ---- the central differences of sdf_terrain_normal (:201-212) as PAIRS --------------------------------------------------------
// The six detail maps of a hit pixel are three pairs pos + d, pos - d with d along one axis (e = .001): the two points of a pair
// have two coordinates in common — bit for bit, and so all the way down both fBms (the same multiplications of the same numbers) —
// and lie in the same lattice cell except where the 0.002 between them straddles a cell face.  A pair is therefore evaluated
// together: per octave the floor / fraction / smoothstep weight of the two common axes ONCE, ONE lookup where the cells coincide,
// and of the trilinear blend (x, then y, then z: noise_iq.h:20-23) everything below the differing axis once — nothing shared for an
// x pair, the four x-mixes for a y pair, the x- and y-mixes for a z pair.  Lanes whose pair straddles a face get the second point's
// own lookup and blend behind a wave-wide test.  Every value is computed by the reference's operations on the reference's operands;
// only the duplicates are gone.  (pos.c + 0 and pos.c - 0 are pos.c unless it is a zero: a wave with a zero coordinate takes the
// unpaired path.)
// (All SIX points together — they are perturbations of one centre: one lookup instead of three, the centre's x- and y-mixes shared
//  by the y and z points, 90 blend operations instead of 109 — was built and measured: same bits, 5.57 against 5.53 ms; six
//  accumulators and six perturbed coordinates through both fBms cost more than the shared work saves.  profiles/r05_log.md)
#ifndef PL_PAIRS
#define PL_PAIRS 1
#endif
template <bool XI, bool SPEC>
__device__ __forceinline__ H8 pl_lookup(WaveCache& S, int tab, unsigned nbits, int slot, bool active, int lane) {
    H8 h;
    if (wave_any(active && S.tag[tab][slot] != nbits)) {
        h = hc_slow<XI, SPEC>(S, tab, nbits, slot, active, lane);
    } else {
        h.lo = *reinterpret_cast<const float4*>(&S.h[tab][slot][0]);
        h.hi = *reinterpret_cast<const float4*>(&S.h[tab][slot][4]);
    }
    return h;
}
// one octave: qa = the pair's first point, qb_ax = the second point's coordinate on axis AX (its other two are qa's)
template <int AX, bool XI>
__device__ __forceinline__ void pl_noise_pair(WaveCache& S, v3 qa, float qb_ax, int tab, bool on, int lane, float& na, float& nb) {
    const float px = floor_(qa.x), py = floor_(qa.y), pz = floor_(qa.z);
    const float ax = qa.x - px, ay = qa.y - py, az = qa.z - pz;
    const float fx = ax * ax * tm2_(ax), fy = ay * ay * tm2_(ay), fz = az * az * tm2_(az);
    const float pb = floor_(qb_ax), ab = qb_ax - pb, fb = ab * ab * tm2_(ab);
    const float bx = AX == 0 ? pb : px, by = AX == 1 ? pb : py, bz = AX == 2 ? pb : pz;
    const float n_a = XI ? __builtin_fmaf(113.0f, pz, __builtin_fmaf(py, 157.0f, px)) : px + py * 157.0f + 113.0f * pz;
    const float n_b = XI ? __builtin_fmaf(113.0f, bz, __builtin_fmaf(by, 157.0f, bx)) : bx + by * 157.0f + 113.0f * bz;
    const unsigned ka = f2u(n_a), kb = f2u(n_b);
    const int sa = (XI && SBX_HC_MAGIC_SLOT) ? (int)(f2u(n_a + 12582912.0f) & (unsigned)(HC_SLOTS - 1)) : ((int)n_a & (HC_SLOTS - 1));
    const H8 h = pl_lookup<XI, false>(S, tab, ka, sa, on, lane);
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz, gb = 1.0f - fb;
    // the first point, and of the second whatever does not depend on the differing axis (hc_blend's operations, its order)
    if (AX == 0) {
        na = hc_blend(h.lo, h.hi, fx, fy, fz);
        nb = hc_blend(h.lo, h.hi, fb, fy, fz);
    } else {
        const float a = h.lo.x * gx + h.lo.y * fx, b = h.lo.z * gx + h.lo.w * fx;
        const float c = h.hi.x * gx + h.hi.y * fx, d = h.hi.z * gx + h.hi.w * fx;
        if (AX == 1) {
            na = (a * gy + b * fy) * gz + (c * gy + d * fy) * fz;
            nb = (a * gb + b * fb) * gz + (c * gb + d * fb) * fz;
        } else {
            const float m = a * gy + b * fy, n = c * gy + d * fy;
            na = m * gz + n * fz;
            nb = m * gb + n * fb;
        }
    }
    // lanes whose two points lie in different cells: the second point's own cell
    const bool other = ka != kb;
    if (wave_any(on && other)) {
        const int sb = (XI && SBX_HC_MAGIC_SLOT) ? (int)(f2u(n_b + 12582912.0f) & (unsigned)(HC_SLOTS - 1)) : ((int)n_b & (HC_SLOTS - 1));
        const H8 g = pl_lookup<XI, false>(S, tab, kb, sb, on && other, lane);
        const float v = hc_blend(g.lo, g.hi, AX == 0 ? fb : fx, AX == 1 ? fb : fy, AX == 2 ? fb : fz);
        if (other) nb = v;
    }
}
// octaves START .. OCT-1 of an fBm for both points of a pair: t += basis(noise) * H; p *= lacunarity; H *= gain   (fbm.h:6)
template <int OCT, int MODE, int START, int AX, bool XI, int TB>
__device__ __forceinline__ void pl_fbm_pair(WaveCache& S, v3& qa, float& qb_ax, float lacunarity, float& H, float gain, float& ta, float& tb,
                                            bool on, int lane) {
#pragma unroll 1
    for (int k = START; k < OCT; ++k) {
        float na, nb;
        pl_noise_pair<AX, XI>(S, qa, qb_ax, (TB + k) & 3, on, lane, na, nb);
        ta += pl_basis<MODE>(na) * H;
        tb += pl_basis<MODE>(nb) * H;
        qa = qa * lacunarity;
        qb_ax = qb_ax * lacunarity;
        H *= gain;
    }
}
// sdf_terrain_map_detail(pos + d).x - sdf_terrain_map_detail(pos - d).x with d = e along axis AX   (:188-199, :201-212)
template <int AX, bool SKIP, bool RS = SKIP, class P = PlLit>
__device__ __forceinline__ float terrain_detail_difference(WaveCache& S, v3 pos, float e, bool on, int lane, const P& w = P()) {
    // the two points: pos.c + e and pos.c - e on axis AX; pos.c + 0 = pos.c - 0 = pos.c on the others (no zero coordinates here)
    const float ca = (AX == 0 ? pos.x : AX == 1 ? pos.y : pos.z) + e, cb = (AX == 0 ? pos.x : AX == 1 ? pos.y : pos.z) - e;
    const v3 pa = V3(AX == 0 ? ca : pos.x, AX == 1 ? ca : pos.y, AX == 2 ? ca : pos.z);
    const v3 pb = V3(AX == 0 ? cb : pos.x, AX == 1 ? cb : pos.y, AX == 2 ? cb : pos.z);
    // first fBm: fbm(pos * 2.0987, 2.0244, .454, .454), 7 octaves of noise
    v3 q = pa * 2.0987f;
    float qb = cb * 2.0987f;
    float H = .454f, h0a = 0.f, h0b = 0.f;
    pl_fbm_pair<7, 0, 0, AX, SKIP, 0>(S, q, qb, 2.0244f, H, .454f, h0a, h0b, on, lane);
    const float n0a = SMOOTHSTEP_K(.35f, 1.f, h0a), n0b = SMOOTHSTEP_K(.35f, 1.f, h0b);
    // second fBm (ridged): pos * 1.50987 + (1.9489, 2.435, .5483); the tail bound of terrain_map for both points
    const v3 off = w.terrain_offset();
    q = pa * 1.50987f + off;
    qb = cb * 1.50987f + (AX == 0 ? off.x : AX == 1 ? off.y : off.z);
    H = .454f;
    float h1a = 0.f, h1b = 0.f;
    pl_fbm_pair<1, 2, 0, AX, SKIP, PL_TB2>(S, q, qb, 2.0244f, H, .454f, h1a, h1b, on, lane);
    float n1a = 0.f, n1b = 0.f;
    if (!SKIP || wave_any(on && !(h1a + .3745f * 1.0001f < .6f && h1b + .3745f * 1.0001f < .6f))) {
        pl_fbm_pair<7, 2, 1, AX, SKIP, PL_TB2>(S, q, qb, 2.0244f, H, .454f, h1a, h1b, on, lane);
        n1a = SMOOTHSTEP_K(.6f, 1.f, h1a);
        n1b = SMOOTHSTEP_K(.6f, 1.f, h1b);
    }
    const float va = pl_length<RS>(pa) - 1.f - (n0a + n1a) * w.max_height();
    const float vb = pl_length<RS>(pb) - 1.f - (n0b + n1b) * w.max_height();
    return va - vb;
}

__device__ __forceinline__ v3 setup_lights(v3 L, v3 normal, v3 c_L = V3(7, 5, 3)) {    // :217-236; c_L: the key light's colour (:224)
    v3 diffuse = V3(0, 0, 0);
    diffuse = diffuse + fmax_(0.f, dot(L, normal)) * c_L;
    const float hemi = clamp_(.25f + .5f * normal.y, .0f, 1.f);
    diffuse = diffuse + hemi * V3(.4f, .6f, .8f) * .2f;
    const float amb = clamp_(.12f + .8f * fmax_(0.f, dot(-L, normal)), 0.f, 1.f);
    diffuse = diffuse + amb * V3(.4f, .5f, .6f);
    return diffuse;
}

__device__ __forceinline__ v3 planet_background(v3 dir) {                              // :23-41
    const v3 sun_color = V3(1.f, .9f, .55f);
    const float sun_amount = clamp_(dot(dir, V3(0, 0, 1)), 0.f, 1.f);
    v3 sky = mix3(V3(.0f, .05f, .2f), V3(.15f, .3f, .4f), 1.0f - dir.y);
    sky = sky + sun_color * clamp_(pow_(sun_amount, 30.0f) * 5.0f, 0.f, 1.f);
    sky = sky + sun_color * clamp_(pow_(sun_amount, 10.0f) * .6f, 0.f, 1.f);
    return abs3(sky);
}

}  // namespace sbx
