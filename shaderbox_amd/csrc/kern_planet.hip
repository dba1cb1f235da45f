// shaderbox_amd/csrc/kern_planet.hip — APP_PLANET: fBm terrain sphere + volumetric cloud shell.
//
// Follows /root/reference/src/app_planet.h (CLOUDS and LIGHT defined, :63,249): render :303-367,
// sdf_terrain_map :175-186, sdf_terrain_map_detail :188-199, sdf_terrain_normal :201-212,
// clouds_map :102-119, clouds_march :121-141, clouds_shadow_march :143-160, integrate_volume
// :79-100, setup_lights :217-236, illuminate :238-298, background :23-41.  The three rotation
// matrices, transpose(rot) and the light vector are frame constants (FramePlanet).
// NaN policy: smoothstep(1-.3s, 1-.2s, N) with s = 0 is 0/0 for N == 1 (:270-273); NaN is data and
// flows to the framebuffer exactly as IEEE arithmetic dictates.
// Single-wave workgroups (as k_clouds): waves never talk to each other (one hash cache and one park area per wave), and a
// 4-wave workgroup keeps its four slots until its slowest wave is done — across the planet's limb and the cloud shell the waves of
// one workgroup differ a lot.  7680x4320: 7.09 -> 6.75 ms (2 waves per workgroup: 7.18).
#include "sbx_planet.h"

namespace sbx {

// Occupancy (7680x4320, tools/ab_time.py): 4 waves/SIMD with batches of 4 octaves: 128 VGPRs, 34 spills, 8.02 ms (round 1);
// batches of 2: 126 VGPRs, NO spills, 8.00 ms; held to 3 waves: 9.65 ms; 5 waves (96 VGPRs, 32-slot tables so that LDS allows
// them): 30 spills, some inside the cloud march, and still 7.3 ms — the fifth wave pays more than the spills cost (parking the
// terrain results in LDS across the cloud march removed a third of them and changed nothing).
#ifndef PL_MIN_WAVES
#define PL_MIN_WAVES 5
#endif
#ifndef PL_TW
#define PL_TW 8              // wave tile PL_TW x 64/PL_TW pixels
#endif
#ifndef PL_PARK
#define PL_PARK 1          // the hit shading's state waits in LDS while the 6 detail terrain maps run
#endif
// (6 waves per SIMD, 80 VGPRs, no parking — its LDS does not fit beside 32-slot tables then: 7.03 ms, but 176 B of scratch per lane,
//  now inside the marches, and 4.3 GB of HBM traffic per frame: 4 % of time bought with 4x the traffic; not taken.  7 waves with
//  16-slot tables: 7.21 ms.)
// (tools/ab_time.py, 7680x4320, same bits: no parking 7.36 ms, 112 B of scratch per lane, 1.72 GB of HBM traffic per frame
//  against the 0.53 GB framebuffer; hit-shading parking 7.29 ms, 60 B, ~1.0 GB; parking the cloud march's ray and integrator
//  as well: no spills there to remove, 7.66 ms; recomputing pixel and ray in the epilogue instead of keeping them: 7.54 ms)
#ifndef PL_PARK_MARCH
#define PL_PARK_MARCH 0    // the two results of the terrain march that only the shading reads (height term, t of the last step) in LDS
#endif                     // slots 10-11 during both marches instead of in registers
#define PL_PARK_N (PL_PARK_MARCH ? 12 : 10)
// ATM: the config-5 composite SBX_APP_PLANET_ATMOSPHERE (include/sbx.h; SURVEY.md §8a note: "planet background() replaced by
// get_incident_light"): wherever APP_PLANET shows its background() (app_planet.h:316-318, 364-366) the pixel shows APP_ATMOSPHERE's
// sky instead — get_incident_light (app_atmosphere.h:78-160) for a ray from 1 m above the ground (:204-207) along the VIEW
// direction, with APP_ATMOSPHERE's sun (setup_scene :177-181, FramePlanet.atm_sun).  No reference-held answers: parity unpinned.
// The sky runs k_atmosphere's exhaustively-equal forms (atm_incident_light<true>: exp_reg4k_, div3_, sqrt_rs_) in the SKIP kernels
// (tame frames: finite uniforms) where their domains hold for THIS camera too (round 5): the ray starts at (0, Re + 1, 0) whatever
// its direction, so every sample lies inside the atmosphere sphere and the exp arguments stay in [-50.1, 5300] (sbx_atmosphere.h);
// and |s|^2 of a march position cannot be 0 or tiny because the view direction normalize(pc.x, pc.y, 1) has rd.z > 0 — a wave
// checks rd.z > 1e-15 for its pixels (s.z = rd.z t with t >= 4e5 on a ray that can come near the centre, so |s|^2 >= 1e-19 against
// sqrt_rs_'s 2^-102) and takes the plain statement of the spec otherwise (fragCoords 1e15 frames below the frame, through the point
// list).  9.73 -> 8.75 ms came from the planet's own marches; this: see profiles/r05_log.md.
// (Reading the marches' two rotations from LDS at every step, so that their 15 multiply-adds per step have no SGPR source — half rate
//  on gfx950 — was measured: 5.763 against 5.759 ms, nothing; profiles/r05_log.md.)
#ifndef PL_ATM_FIN
#define PL_ATM_FIN 1
#endif
// BUILD (sbx_frame.h PLANET_*): the header as shipped, or with one of its three switches the other way.
//   PLANET_CLOUDLESS, `#define CLOUDS` (:63) gone: no clouds_march (:344-347), no clouds_shadow_march (:355-361).  `cloud` is the
//     reference's static object that nothing writes: radiance and alpha are its +0, shadow is the literal 1, and the two mix of
//     :363 / :365 run on those zeros as written — x * (1 - 0) + 0 * 0, of which the compiler folds what IEEE lets it fold (x * 1 and
//     0 * 0; the + 0 stays, it turns a -0 into +0 before the abs).  Nothing is parked in slots 1-2.
//   PLANET_UNLIT, `#define LIGHT` (:249) gone: N = w_normal.y (:254), ocean = water (:292), shoreline unlit; sdf_terrain_normal —
//     the paired and unpaired detail maps — and setup_lights are compiled out, F.L is not read and no park area exists.
//   PLANET_CLOSEUP, setup_camera's `#if 0` (:51) on: eye (0, 0, -1.93), look_at (-.1, .9, 2), written by build_planet.  The code is
//     the shipped build's but for length() of a march position, which is the IEEE root in the SKIP kernel too (RS below; the note at
//     PL_SQRT_RS says why).
// None of the three is built with ATM.
#ifndef PL_MIN_WAVES_UNLIT
#define PL_MIN_WAVES_UNLIT PL_MIN_WAVES
#endif
constexpr int planet_min_waves(int build) { return build == PLANET_UNLIT ? PL_MIN_WAVES_UNLIT : PL_MIN_WAVES; }
template <bool SKIP, bool ATM = false, int BUILD = PLANET_DEFAULT>
__global__ void __launch_bounds__(WG_THREADS, planet_min_waves(BUILD)) k_planet(FramePlanet F, RowMap M, float* __restrict__ out) {
    static_assert(!ATM || BUILD == PLANET_DEFAULT, "the builds of app_planet.h's switches are not combined with the atmosphere sky");
    constexpr bool CLD = BUILD != PLANET_CLOUDLESS, LIT = BUILD != PLANET_UNLIT;
    constexpr bool RS = SKIP && BUILD != PLANET_CLOSEUP;         // the short roots of pl_length: proved for the shipped eye only
    const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();      // (the dispatch order's cost table, RowMap.cost)
    __shared__ double etab[ATM ? 32 : 1];
    if (ATM) {
        if (threadIdx.x < 32) etab[threadIdx.x & (ATM ? 31 : 0)] = kExp2Tab[threadIdx.x];
        if (WG_THREADS > 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    }
    __shared__ WaveCache cache[WG_THREADS / 64];
#if PL_PARK
    __shared__ float park[WG_THREADS / 64][PL_PARK_N * 64];
#endif
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
        const float radius = 1.f + PL_MAX_HEIGHT;
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
        // terrain march :328-342
        float t = 0.f;
        v2 df = V2(1, PL_MAX_HEIGHT);
        v3 pos = V3(0, 0, 0);
#ifndef PL_TLAST
#define PL_TLAST 1         // the march keeps the t of its last committed step instead of the step's point (one register for three, across
#endif                     // both marches); the point is computed again — same operations, same operands — where the hit is shaded
        float t_pos = 0.f;
        float max_cld = PL_MAX_RAY_DIST;
        bool tm = hit_atm;
        if (SKIP && PL_SPEC) hc_set_direction(S, mul(F.rot, rd), hit_atm, lane);       // both terrain fBms scale the rotated point by positive factors
        for (int i = 0; i < 120; ++i) {
            if (tm && t > PL_MAX_RAY_DIST) tm = false;           // `if (t > max_ray_dist) break;`
            if (!wave_any(tm)) break;
            const v3 o = hit_o + t * rd;
            const v3 p = mul(F.rot, o - V3(0, 0, 0));
            const v2 d = terrain_map<3, SKIP, RS>(S, p, tm, lane);
            if (tm) {
#if PL_PARK && PL_PARK_MARCH && PL_TLAST
                {
                    volatile float* const pm = &park[threadIdx.x >> 6][lane];
                    pm[10 * 64] = d.y; pm[11 * 64] = t;
                    df.x = d.x;
                }
#else
                if (PL_TLAST) t_pos = t; else pos = p;
                df = d;
#endif
                if (df.x < .005f) { max_cld = t; tm = false; }
                else t += df.x * .4567f;
            }
        }
        // clouds_march :121-141 on construct_volume(hit.origin)
        Vol cloud = make_vol(hit_o);
        if constexpr (CLD) {
            const float t_step = PL_MAX_RAY_DIST / 75.f;
            float tc = 0.f;
            bool cm = hit_atm;
            if (SKIP && PL_SPEC) hc_set_direction(S, mul(F.rot_cloud, rd), hit_atm, lane);
            for (int i = 0; i < 75; ++i) {
                if (cm && (tc > max_cld || cloud.alpha >= 1.f)) cm = false;   // `return` of clouds_march
                if (!wave_any(cm)) break;
                const v3 o = cloud.origin + tc * rd;
                // The band (.2, .65) of height = (|p| - 1) / .4 is the shell 1.08 < |p| < 1.26.  |o|^2 outside
                // (1.166, 1.5885) puts the rotated point outside it with a margin (3e-4 relative) far above the rounding
                // of rotation, sqrt and division, so clouds_map() would find band() == +0 and change nothing: when that
                // holds for every committing lane the step is only `tc += t_step` (most steps of the march).
                {
                    const float d2 = dot(o, o);
                    if (SKIP && !wave_any(cm && !(d2 > 1.5885f || d2 < 1.166f))) { tc += t_step; continue; }
                }
                const v3 cp = mul(F.rot_cloud, o - V3(0, 0, 0));
                const float ch = PL_DIVK(pl_length<RS>(cp) - 1.f, PL_MAX_HEIGHT);
                if (cm) { cloud.pos = cp; cloud.height = ch; }
                tc += t_step;
                clouds_map<SKIP>(S, cloud, t_step, cm, lane);
            }
        }
        const bool hitl = hit_atm && (df.x < .005f);              // :349
        if (SKIP && PL_SPEC) hc_no_direction(S, lane);              // the hit shading samples around a point, not along a ray
        v3 c_hit = V3(0, 0, 0);
        if (wave_any(hitl)) {
#if PL_PARK && PL_PARK_MARCH && PL_TLAST
            {
                volatile float* const pm = &park[threadIdx.x >> 6][lane];
                df.y = pm[10 * 64]; t_pos = pm[11 * 64];           // (lanes without an atmosphere hit never wrote them and are not shaded)
            }
#endif
            if (PL_TLAST) pos = mul(F.rot, (hit_o + t_pos * rd) - V3(0, 0, 0));   // the point of the last committed step, as the march computed it
            // illuminate :238-298
            float h = df.y;
            const float e = 0.001f;
            float g[3] = {0.f, 0.f, 0.f};                          // sdf_terrain_normal :201-212
            if constexpr (LIT) {
#if PL_PARK
            // 6 x (7 + 7)-octave terrain_map: the second register peak.  What it does not need — the hit point, its height
            // term, the ray, the cloud integrator (already in slots 1-2) — waits in LDS, and the three differences land there.
            float* const pk = &park[threadIdx.x >> 6][lane];
            pk[3 * 64] = pos.x; pk[4 * 64] = pos.y; pk[5 * 64] = pos.z; pk[6 * 64] = h;
            if constexpr (CLD) { pk[1 * 64] = cloud.radiance; pk[2 * 64] = cloud.alpha; }
            asm volatile("" ::: "memory");
            // (a zero coordinate of the hit point: pos.c + 0 and pos.c - 0 then differ in the sign of their zero — the unpaired path)
            const bool pairs = SKIP && PL_PAIRS && !wave_any(hitl && (pk[3 * 64] == 0.f || pk[4 * 64] == 0.f || pk[5 * 64] == 0.f));
            if (pairs) {
                pk[7 * 64] = terrain_detail_difference<0, SKIP, RS>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane);
                asm volatile("" ::: "memory");
                pk[8 * 64] = terrain_detail_difference<1, SKIP, RS>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane);
                asm volatile("" ::: "memory");
                pk[9 * 64] = terrain_detail_difference<2, SKIP, RS>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]), e, hitl, lane);
                asm volatile("" ::: "memory");
            } else {
#pragma unroll 1
            for (int ax = 0; ax < 3; ++ax) {                       // one code copy for the three central differences
                const v3 d = V3(ax == 0 ? e : 0.f, ax == 1 ? e : 0.f, ax == 2 ? e : 0.f);
                const float va = terrain_map<7, SKIP, RS>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]) + d, hitl, lane).x;
                asm volatile("" ::: "memory");
                const float vb = terrain_map<7, SKIP, RS>(S, V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]) - d, hitl, lane).x;
                pk[(7 + ax) * 64] = va - vb;
                asm volatile("" ::: "memory");
            }
            }
            pos = V3(pk[3 * 64], pk[4 * 64], pk[5 * 64]);
            h = pk[6 * 64];
            if constexpr (CLD) { cloud.radiance = pk[1 * 64]; cloud.alpha = pk[2 * 64]; }
            g[0] = pk[7 * 64]; g[1] = pk[8 * 64]; g[2] = pk[9 * 64];
#else
#pragma unroll 1
            for (int ax = 0; ax < 3; ++ax) {                       // one code copy for the three central differences
                const v3 d = V3(ax == 0 ? e : 0.f, ax == 1 ? e : 0.f, ax == 2 ? e : 0.f);
                const float v = terrain_map<7, SKIP, RS>(S, pos + d, hitl, lane).x - terrain_map<7, SKIP, RS>(S, pos - d, hitl, lane).x;
                if (ax == 0) g[0] = v; else if (ax == 1) g[1] = v; else g[2] = v;
            }
#endif
            }
            const v3 w_normal = normalize(pos);
            v3 normal = w_normal;                                  // (not read in the unlit build)
            float N = w_normal.y;                                  // `#else` of LIGHT :254
            if constexpr (LIT) {
                normal = normalize(V3(g[0], g[1], g[2]));
                N = dot(normal, w_normal);
            }
            const v3 c_water = V3(.015f, .110f, .455f), c_grass = V3(.086f, .132f, .018f),
                     c_beach = V3(.153f, .172f, .121f), c_rock = V3(.080f, .050f, .030f),
                     c_snow = V3(.600f, .600f, .600f);
            const float l_water = .05f, l_shore = .17f, l_grass = .211f, l_rock = .351f;
            const float s = smoothstep_(.4f, 1.f, h);
            const v3 rock = mix3(c_rock, c_snow, smoothstep_(1.f - .3f * s, 1.f - .2f * s, N));
            const v3 grass = mix3(c_grass, rock, smoothstep_(l_grass, l_rock, h));
            v3 shoreline = mix3(c_beach, grass, smoothstep_(l_shore, l_grass, h));
            const v3 water = mix3(c_water / 2.f, c_water, smoothstep_(0.f, l_water, h));
            v3 ocean = water;                                      // `#else` of LIGHT :292
            if constexpr (LIT) {
                shoreline = shoreline * setup_lights(F.L, normal);
                ocean = setup_lights(F.L, w_normal) * water;
            }
            const v3 c_terr = mix3(ocean, shoreline, smoothstep_(l_water, l_shore, h));

            const float c_cld = cloud.radiance, alpha = cloud.alpha;
            // cloud shadow on the ground :355-360, clouds_shadow_march :143-160
            float shadow = 1.f;                                    // :353
            if constexpr (CLD) {
            const v3 lp = mul(F.rot_t, pos);
            Vol sh = make_vol(lp);
            const v3 local_up = normalize(lp);
            {
                const float t_step = PL_MAX_HEIGHT / 5.f;
                float ts = 0.f;
                for (int i = 0; i < 5; ++i) {
                    const v3 o = sh.origin + ts * local_up;
                    sh.pos = mul(F.rot_cloud, o - V3(0, 0, 0));
                    sh.height = PL_DIVK(pl_length<RS>(sh.pos) - 1.f, PL_MAX_HEIGHT);
                    ts += t_step;
                    clouds_map<SKIP>(S, sh, t_step, hitl, lane);
                }
            }
            shadow = mix_(.7f, 1.f, step_(sh.alpha, 0.33f));
            }
            c_hit = abs3(mix3(c_terr * shadow, V3s(c_cld), alpha));
        }
        cloud_sky = !hitl;
        sky_r = cloud.radiance; sky_a = cloud.alpha;
        col = c_hit;
    }
    const Pixel pxe = px;
    const v3 rde = rd;
    if (!pxe.valid) return;
    if (ATM) {
        if (cloud_sky || !hit_atm) {
            v3 sky;
            if (SKIP && PL_ATM_FIN && !wave_any(!(rde.z > 1e-15f)))       // (wave-uniform; a NaN direction takes the plain form)
                sky = atm_incident_light<true>(V3(0, ATM_EARTH_R + 1.f, 0), rde, F.atm_sun, reinterpret_cast<const double (&)[32]>(etab), nullptr);
            else
                sky = atm_incident_light<false>(V3(0, ATM_EARTH_R + 1.f, 0), rde, F.atm_sun, reinterpret_cast<const double (&)[32]>(etab), nullptr);
            col = hit_atm ? abs3(mix3(sky, V3s(sky_r), sky_a)) : sky;
        }
    } else {
        if (cloud_sky) col = abs3(mix3(planet_background(rde), V3s(sky_r), sky_a));   // :364-366
        if (!hit_atm) col = planet_background(rde);                  // :316-318
    }
    tile_cost_store(M, tl_t0);
    store_rgba(M, out, pxe.idx, to_srgb(col));
}

dim3 planet_grid(const RowMap& M) { return grid_for<PL_TW>(M); }

// build: PLANET_* (sbx_frame.h).  The plain kernel (variant 1: no skips, the IEEE forms) of PLANET_CLOSEUP is the shipped build's over
// the frame block build_planet writes for it: with SKIP false no instantiation depends on RS.
void launch_planet(const FramePlanet& F, const RowMap& M, float* out, hipStream_t s, int variant, int build) {
    switch (F.atm_sky ? PLANET_DEFAULT : build) {
    case PLANET_CLOUDLESS:
        if (variant == 1) hipLaunchKernelGGL((k_planet<false, false, PLANET_CLOUDLESS>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        else hipLaunchKernelGGL((k_planet<true, false, PLANET_CLOUDLESS>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        return;
    case PLANET_UNLIT:
        if (variant == 1) hipLaunchKernelGGL((k_planet<false, false, PLANET_UNLIT>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        else hipLaunchKernelGGL((k_planet<true, false, PLANET_UNLIT>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        return;
    case PLANET_CLOSEUP:
        if (variant != 1) { hipLaunchKernelGGL((k_planet<true, false, PLANET_CLOSEUP>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out); return; }
        break;
    default: break;
    }
    if (F.atm_sky) {
        if (variant == 1) hipLaunchKernelGGL((k_planet<false, true>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        else hipLaunchKernelGGL((k_planet<true, true>), grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
        return;
    }
    if (variant == 1) hipLaunchKernelGGL(k_planet<false>, grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
    else hipLaunchKernelGGL(k_planet<true>, grid_for<PL_TW>(M), dim3(WG_THREADS), 0, s, F, M, out);
}

hipError_t bind_fault_planet(unsigned* word) { return hc_bind_fault_word(word); }

}  // namespace sbx
