// shaderbox_amd/csrc/kern_planet_world.hip — SBX_APP_PLANET_WORLD's run-time tier: src/app_planet.h as shipped (CLOUDS and LIGHT
// defined) with every number of include/sbx.h sbx_aux_planet_world arriving at run time (FramePlanetWorld, sbx_frame.h; built by
// sbx_frames.hip build_planet_world).  tests/planet_world_model.py is the definition.  k_planet's structure: one wave per workgroup,
// PL_TW tiles, the per-wave hash cache, the park area, tile_cost_store, store_rgba; and k_planet's device functions (sbx_planet.h),
// which take the header's numbers from a policy: PlLit in k_planet, PlCloudW / PlTerrW over the frame block here.  Only the pixel's
// own statement — the marches' bounds, illuminate's materials, the key light — is written in this file.
//
// k_planet_world<false> (sbx_set_variant 1, and every block planet_world_tame refuses): the plain statement, lane by lane — every
// octave and every cloud sample, IEEE roots and divisions by the block's values, exp_, lattice indices as the reference forms them.
//
// k_planet_world<true>: k_planet<true>'s short forms are argued against the header's literals and the shipped eye.  Here a short form
// stands only where (a) it is equal for every input, (b) the host's test on the block (planet_world_tame, bounds below) proves its
// domain, or (c) a wave-wide test on the wave's own operands does; the kernel holds both bodies, and a wave that fails (c) takes the
// plain one.  The rule is kern_planet_eval.hip's.  The tests:
//   HOST (F.tame): max_height in [.02, 2]; both offsets within 64 per coordinate; the band edges finite, each 0 or of magnitude in
//     [2^-20, 4], band1 - band0 and band2 - band1 >= 2^-20; cld_coverage 0 or of magnitude in [2^-20, 4]; the binary32 difference
//     (cld_coverage + cld_fuzzy) - cld_coverage in [2^-30, 8]; |absorb| * max(t_step) <= 80; |cloud_light| in [2^-20, 2^20]; the three
//     angles within 1e9 degrees (1.75e7 rad, inside the range in which the spec's sin / cos reduce exactly enough: sbx_capi.hip
//     tame_time) and rot, rot_cloud checked entry by entry to be orthonormal to 1e-5.  Colours, limits, key light and sun enter no proof.
//   WAVE: every lane that meets the atmosphere has 1 <= |hit_o|^2 <= (2 + max_height)^2 and |rd|^2 <= 1.001, NaN failing both.  The
//     camera therefore enters no proof: eye == look_at, a huge or non-finite eye, fov 0 or a fragCoord of 1e30 are this test's business.
//   Under both, with mh = max_height: a terrain sample lies at hit_o + t rd with 0 <= t <= 4 mh (`t > max_ray_dist` ends the march), a
//   cloud sample at t <= max_cld <= 4 mh, a shadow sample within mh of a terrain sample: |p| <= (2 + mh + 4.003 mh + mh) (1 + 1e-5) <
//   2 + 6.02 mh <= 14.1 after either rotation.  A terrain sample has |p| - 1 >= df.x >= .005 or ends the march, and a step is .4567 df.x:
//   |p| > 1 at every terrain sample (the first is hit_o, |p|^2 >= 1 - 2e-5), so the shadow march's normalize(lp) is finite.
// The decisions, one by one:
//   RS (sqrt_rs_ / sqrt_n_ for |p|): OFF.  A cloud sample is bounded below by nothing but the ray's closest approach to the centre.
//   XI (exact-integer lattice indices, the magic-number slot): GUARDED.  Finest terrain coordinate 14.1 * 2.0987 * 2.0244^6 < 2040, of
//     the second fBm (14.1 * 1.50987 + 64) * 2.0244^6 < 5880, of the clouds (14.1 * 3.2343 + 64) * 2.0276^3 < 920: |px + 157 py + 113 pz|
//     < 5880 * 271 < 2^21, integers below 2^22.
//   exp_reg4k_ (|x| <= 80): GUARDED.  -absorb dens t_step with dens in [0, .9375] (an fBm of |2 noise - 1| with gains summing to .9375,
//     times a smoothstep, times a band, both in [0, 1] for ordered edges) is within 80 by the host's test; height = (|p| - 1) / mh lies in
//     [-1 / mh, 1 / mh + 6.02], within 56.1.
//   div3_ with the host's RN(1 / d) (tools/div3_exhaustive.hip: equal to the IEEE quotient for EVERY divisor significand, each with
//     the reciprocal rounded from it — a variable divisor is covered) and the v_med3 clamp: GUARDED.  Divisors max_height, cloud_light,
//     band1 - band0, band2 - band1, the coverage difference: all within 2^+-60 by the host's test.  Dividends, finite and zero or within
//     2^+-100: n0 + n1 (zero or >= 2^-60, at most 2); |p| - 1 (zero, always +0, or >= 2^-25, at most 14); exp(height) in e^+-56.1 =
//     2^+-81; dens - cld_coverage and height - band edge: differences of two binary32 numbers each 0 or of magnitude in [2^-28, 64], so 0
//     or >= 2^-52.  No operand of a v_med3 is a NaN: every position, length, fBm sum and block value above is finite.
//   The coverage early-outs (`dens + .1876 < cov`, `dens + .06255 < cov`): GUARDED.  They claim smoothstep(cov, cov + fuzzy, dens) = +0,
//     which needs the quotient's divisor positive (the host's test) — with fuzzy < 0 a dens below cov gives 1 — and a finite cov, so
//     that dens * 0, then * band, -absorb * 0 * t_step and 0 * exp(height) / cloud_light are zeros and the three updates `*= 1`, `+= 0`.
//   The |o|^2 shell skip: GUARDED, over an interval the host computes in binary64.  band() is exactly +0 for height <= band0 (the
//     first quotient <= 0) and for height >= band2 (RN(h - band1) >= RN(band2 - band1), the second smoothstep exactly 1): the shell is
//     1 + band0 mh < |p| < 1 + band2 mh.  shell_lo2 / shell_hi2 are those radii squared, moved out by 1e-3 relative (k_planet's literals
//     have 3.4e-4 and 5.7e-4): 5e-4 in |p| against 1.2e-5 from rotation, dot and root, and in height 5e-4 r / mh >= 2.5e-4 r against a
//     rounding of 2^-23 * 56 — which needs the radius r itself away from 0: an edge radius below .05 makes no claim (0 / inf), as do
//     unordered or non-finite edges.
//   The terrain TAIL skip: equal for every input with a finite h1 (it names only the literal gains), GUARDED by the finiteness above.
//   hc_set_direction's look-ahead, the cooperative fBm, the paired central differences behind their own wave-wide test: block-free.
//   illuminate's smoothsteps over the block's limits, mix, setup_lights with the block's key colour, background: one form, the plain one.
#include "sbx_planet.h"
#include <type_traits>

namespace sbx {

#ifndef PW_MIN_WAVES
#define PW_MIN_WAVES 5
#endif
#ifndef PW_MIN_WAVES_PLAIN
#define PW_MIN_WAVES_PLAIN 4 // the plain kernel is not held to 96 VGPRs: it takes 93 and runs 5 waves per SIMD as it is, and a bound it
#endif                       // does not need cannot cost it a spill when the compiler changes (tools/kernel_resources.py: no scratch)
#ifndef PL_TW
#define PL_TW 8              // wave tile PL_TW x 64/PL_TW pixels (kern_planet.hip's)
#endif

// A part of FramePlanetWorld (terr, cloud, shade) read where its phase begins.  A by-value kernel argument is loaded at the kernel's
// entry and held in SGPRs to its last use: with all of the block's numbers live across both marches the kernel ran out of them
// (tools/kernel_resources.py: over a hundred SGPRs moved to VGPR lanes, read back at 1450 places against k_planet's 90; 9.25 ms).
// Where the frame block lies in the argument block is stated by a tag type, A::frame_at, that the CALLING KERNEL hands down
// (PwKernelArgs below, held to k_planet_world's parameter list by a static_assert next to it): a second kernel that wants this
// must state its own.  The empty asm makes the block's address opaque here, which keeps the loads below it and lets the part's
// registers go when its phase ends.  Wave-uniform scalar loads from constant memory, as the compiler's own.
template <class T, class A>
__device__ __forceinline__ T pw_late(size_t offset) {
    T part;
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(T) % sizeof(float) == 0 && alignof(T) == alignof(float), "copied word by word");
    typedef const __attribute__((address_space(4))) char* kernarg_ptr;
    kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    const __attribute__((address_space(4))) float* const q = (const __attribute__((address_space(4))) float*)(p + A::frame_at + offset);
    float* const d = reinterpret_cast<float*>(&part);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / sizeof(float)); ++i) d[i] = q[i];
#endif
    return part;
}
#define PW_LATE(T, member) pw_late<T, A>(offsetof(FramePlanetWorld, member))

// render :323-366 for the lanes that met the atmosphere (k_planet's body over the block) -> the ground pixel's colour; sky_r, sky_a:
// the cloud over it or over the background
template <bool SKIP, class A>
__device__ __forceinline__ v3 pw_shell(WaveCache& S, float* const pk, bool hit_atm, v3 hit_o, v3 rd, int lane,
                                       bool& cloud_sky, float& sky_r, float& sky_a) {
    // terrain march :328-342
    float t = 0.f;
    v2 df;
    float t_pos = 0.f;                                             // (k_planet's PL_TLAST)
    float max_cld;
    {
        const PlanetWorldTerrain T = PW_LATE(PlanetWorldTerrain, terr);
        df = V2(1, T.max_height);
        max_cld = T.max_ray_dist;
        bool tm = hit_atm;
        if (SKIP && PL_SPEC) hc_set_direction(S, mul(T.rot, rd), hit_atm, lane);
        for (int i = 0; i < T.terr_steps; ++i) {
            if (tm && t > T.max_ray_dist) tm = false;
            if (!wave_any(tm)) break;
            const v3 o = hit_o + t * rd;
            const v3 p = mul(T.rot, o - V3(0, 0, 0));
            const v2 d = terrain_map<3, SKIP, false>(S, p, tm, lane, PlTerrW{T});
            if (tm) {
                t_pos = t;
                df = d;
                if (df.x < .005f) { max_cld = t; tm = false; }
                else t += df.x * .4567f;
            }
        }
    }
    // clouds_march :121-141 on construct_volume(hit.origin)
    Vol cloud = make_vol(hit_o);
    {
        const PlanetWorldCloud C = PW_LATE(PlanetWorldCloud, cloud);
        const float t_step = C.t_step_cloud;
        float tc = 0.f;
        bool cm = hit_atm;
        if (SKIP && PL_SPEC) hc_set_direction(S, mul(C.rot_cloud, rd), hit_atm, lane);
        for (int i = 0; i < C.cloud_steps; ++i) {
            if (cm && (tc > max_cld || cloud.alpha >= 1.f)) cm = false;
            if (!wave_any(cm)) break;
            const v3 o = cloud.origin + tc * rd;
            {
                const float d2 = dot(o, o);                        // (the shell skip: the interval and its margins are at the top)
                if (SKIP && !wave_any(cm && !(d2 > C.shell_hi2 || d2 < C.shell_lo2))) { tc += t_step; continue; }
            }
            const v3 cp = mul(C.rot_cloud, o - V3(0, 0, 0));
            const float ch = PlCloudW{C}.div_height<SKIP>(pl_length<false>(cp) - 1.f);
            if (cm) { cloud.pos = cp; cloud.height = ch; }
            tc += t_step;
            clouds_map<SKIP>(S, cloud, t_step, cm, lane, PlCloudW{C});
        }
    }
    const bool hitl = hit_atm && (df.x < .005f);                   // :349
    if (SKIP && PL_SPEC) hc_no_direction(S, lane);
    v3 c_hit = V3(0, 0, 0);
    if (wave_any(hitl)) {
        const PlanetWorldTerrain F = PW_LATE(PlanetWorldTerrain, terr);
        v3 pos = mul(F.rot, (hit_o + t_pos * rd) - V3(0, 0, 0));   // the point of the last committed step, as the march computed it
        float h = df.y;
        const float e = 0.001f;
        // sdf_terrain_normal :201-212; the shading's state waits in LDS meanwhile (k_planet's PL_PARK, its slots)
        pk[3 * 64] = pos.x; pk[4 * 64] = pos.y; pk[5 * 64] = pos.z; pk[6 * 64] = h;
        pk[1 * 64] = cloud.radiance; pk[2 * 64] = cloud.alpha;
        asm volatile("" ::: "memory");
        const bool pairs = SKIP && PL_PAIRS && !wave_any(hitl && (pk[3 * 64] == 0.f || pk[4 * 64] == 0.f || pk[5 * 64] == 0.f));
        if (pairs) {
            pk[7 * 64] = terrain_detail_difference<0, SKIP, false>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane, PlTerrW{F});
            asm volatile("" ::: "memory");
            pk[8 * 64] = terrain_detail_difference<1, SKIP, false>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane, PlTerrW{F});
            asm volatile("" ::: "memory");
            pk[9 * 64] = terrain_detail_difference<2, SKIP, false>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane, PlTerrW{F});
            asm volatile("" ::: "memory");
        } else {
#pragma unroll 1
            for (int ax = 0; ax < 3; ++ax) {
                const v3 d = V3(ax == 0 ? e : 0.f, ax == 1 ? e : 0.f, ax == 2 ? e : 0.f);
                const float va = terrain_map<7, SKIP, false>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]) + d, hitl, lane, PlTerrW{F}).x;
                asm volatile("" ::: "memory");
                const float vb = terrain_map<7, SKIP, false>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]) - d, hitl, lane, PlTerrW{F}).x;
                pk[(7 + ax) * 64] = va - vb;
                asm volatile("" ::: "memory");
            }
        }
        pos = V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]);
        h = pk[6 * 64];
        cloud.radiance = pk[1 * 64]; cloud.alpha = pk[2 * 64];
        // illuminate :238-298
        const PlanetWorldShade Sh = PW_LATE(PlanetWorldShade, shade);
        const v3 w_normal = normalize(pos);
        const v3 normal = normalize(V3(pk[7 * 64], pk[8 * 64], pk[9 * 64]));
        const float N = dot(normal, w_normal);
        const float s = smoothstep_(.4f, 1.f, h);
        const v3 rock = mix3(Sh.c_rock, Sh.c_snow, smoothstep_(1.f - .3f * s, 1.f - .2f * s, N));
        const v3 grass = mix3(Sh.c_grass, rock, smoothstep_(Sh.l_grass, Sh.l_rock, h));
        v3 shoreline = mix3(Sh.c_beach, grass, smoothstep_(Sh.l_shore, Sh.l_grass, h));
        const v3 water = mix3(Sh.c_water_half, Sh.c_water, smoothstep_(0.f, Sh.l_water, h));
        shoreline = shoreline * setup_lights(Sh.L, normal, Sh.key_color);
        const v3 ocean = setup_lights(Sh.L, w_normal, Sh.key_color) * water;
        const v3 c_terr = mix3(ocean, shoreline, smoothstep_(Sh.l_water, Sh.l_shore, h));
        const float c_cld = cloud.radiance, alpha = cloud.alpha;
        // cloud shadow on the ground :355-360, clouds_shadow_march :143-160
        const v3 lp = mul(Sh.rot_t, pos);
        Vol sh = make_vol(lp);
        const v3 local_up = normalize(lp);
        {
            const PlanetWorldCloud C = PW_LATE(PlanetWorldCloud, cloud);
            const float t_step = C.t_step_shadow;
            float ts = 0.f;
            for (int i = 0; i < C.shadow_steps; ++i) {
                const v3 o = sh.origin + ts * local_up;
                sh.pos = mul(C.rot_cloud, o - V3(0, 0, 0));
                sh.height = PlCloudW{C}.div_height<SKIP>(pl_length<false>(sh.pos) - 1.f);
                ts += t_step;
                clouds_map<SKIP>(S, sh, t_step, hitl, lane, PlCloudW{C});
            }
        }
        const float shadow = mix_(.7f, 1.f, step_(sh.alpha, 0.33f));
        c_hit = abs3(mix3(c_terr * shadow, V3s(c_cld), alpha));
    }
    cloud_sky = !hitl;
    sky_r = cloud.radiance; sky_a = cloud.alpha;
    return c_hit;
}

// k_planet_world's argument block as pw_late reads it: the frame block is the FIRST parameter, at offset 0 (the static_assert under the
// kernel fails the build if the parameter list changes)
struct PwKernelArgs { static constexpr size_t frame_at = 0; };
template <bool SKIP>
__global__ void __launch_bounds__(WG_THREADS, SKIP ? PW_MIN_WAVES : PW_MIN_WAVES_PLAIN) k_planet_world(FramePlanetWorld F, RowMap M, float* __restrict__ out) {
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
    __shared__ WaveCache cache[WG_THREADS / 64];
    __shared__ float park[WG_THREADS / 64][10 * 64];
    const int lane = threadIdx.x & 63;
    WaveCache& S = cache[threadIdx.x >> 6];
    hc_init(S, lane);
    const Pixel px = pixel_of_thread<PL_TW>(M);
    const v2 pc = point_cam(F.cam, px.fx, px.fy);
    const v3 ro = F.cam.eye, rd = primary_dir(F.cam, pc);

    // intersect_sphere(eye, atmosphere = {0, 1 + max_height}) on no_hit      intersect.h:7-33
    bool hit_atm = false;
    v3 hit_o = V3(0, 0, 0);
    {
        const float radius = F.atm_radius;
        const v3 rc = V3(0, 0, 0) - ro;
        const float radius2 = radius * radius;
        const float tca = dot(rc, rd);
        if (!(tca < 0.f)) {
            const float d2 = dot(rc, rc) - tca * tca;
            if (!(d2 > radius2)) {
                const float thc = sqrt_(radius2 - d2);
                float t0 = tca - thc;
                const float t1 = tca + thc;
                if (t0 < 0.f) t0 = t1;
                if (!(t0 > (float)(1e8f + 1e1f))) { hit_atm = true; hit_o = ro + rd * t0; }
            }
        }
    }
    hit_atm = hit_atm && px.valid;
    v3 col = V3(0, 0, 0);
    bool cloud_sky = false;                                      // atmosphere hit, no ground hit: background under the clouds
    float sky_r = 0.f, sky_a = 0.f;
    if (wave_any(hit_atm)) {
        float* const pk = &park[threadIdx.x >> 6][lane];
        bool fast = false;
        if (SKIP) {                                              // the WAVE test (top of the file); a NaN fails it
            const float ho2 = dot(hit_o, hit_o), rd2 = dot(rd, rd);
            fast = F.tame != 0 && !wave_any(hit_atm && !(ho2 >= 1.f && ho2 <= F.hit2_max && rd2 <= 1.001f));
        }
        if (SKIP && fast) col = pw_shell<true, PwKernelArgs>(S, pk, hit_atm, hit_o, rd, lane, cloud_sky, sky_r, sky_a);
        else col = pw_shell<false, PwKernelArgs>(S, pk, hit_atm, hit_o, rd, lane, cloud_sky, sky_r, sky_a);
    }
    if (!px.valid) return;
    if (cloud_sky) col = abs3(mix3(planet_background(rd), V3s(sky_r), sky_a));   // :364-366
    if (!hit_atm) col = planet_background(rd);                   // :316-318
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, px.idx, to_srgb(col));
}

static_assert(std::is_same<decltype(&k_planet_world<true>), void (*)(FramePlanetWorld, RowMap, float*)>::value &&
              std::is_same<decltype(&k_planet_world<false>), void (*)(FramePlanetWorld, RowMap, float*)>::value && PwKernelArgs::frame_at == 0,
              "pw_late reads FramePlanetWorld at PwKernelArgs::frame_at of the argument block: it must stay k_planet_world's first parameter");

// fast: the block is tame and the context's variant is not 1 (sbx_frames.hip planet_world_tier)
void launch_planet_world(const FramePlanetWorld& F, bool fast, const RowMap& M, float* out, hipStream_t s) {
    if (fast) hipLaunchKernelGGL(k_planet_world<true>, grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
    else hipLaunchKernelGGL(k_planet_world<false>, grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
}

hipError_t bind_fault_planet_world(unsigned* word) { return hc_bind_fault_word(word); }

}  // namespace sbx
