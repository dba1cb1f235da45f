// shaderbox_amd/csrc/kern_planet_eval.hip — sbx_planet_eval: APP_PLANET's terrain, cloud shell and shading over the caller's rays and
// points (include/sbx.h).  The reference's src/app_planet.h as shipped (CLOUDS and LIGHT defined): render :303-367, the terrain march
// :311-342, sdf_terrain_map :175-186, sdf_terrain_map_detail :188-199, sdf_terrain_normal :201-212, the density of clouds_map :106-114,
// illuminate :238-298, background :23-41.  No camera, no u_res, no u_mouse; u_time enters through rot / rot_cloud (FramePlanet).
//
// One lane per element, one 64-lane wave per workgroup, a ragged last wave.  Everything is built on k_planet's device functions
// (sbx_planet.h): the cooperative fBm over the per-wave lattice-hash cache, whose cross-lane steps need wave-uniform control flow — so no
// lane leaves early; a lane past n is predicated off (`on`), evaluates harmlessly and commits nothing, as k_planet's lanes outside the
// frame do.  The cache needs no coherence between lanes to be correct (a lookup returns hash1 of its own lattice index whoever put the
// cell there; sbx_render_points runs the same functions over scattered coordinates), only to be fast.
//
// PLAIN (sbx_set_variant 1, and any u_time that sbx_eval.hip does not find tame): the SKIP = false statement lane by lane — every
// octave and every cloud sample evaluated, IEEE roots and divisions, exp_, lattice indices as the reference forms them.
//
// DEFAULT: k_planet<SKIP = true>'s short forms rest on the shipped eye or on "tame frames"; over the caller's operands none of those
// proofs holds by itself.  Here a short form stands only where it is equal for every input, or where a WAVE-WIDE test on the wave's own
// operands proves its domain; a wave that fails a test takes the plain form for that part (pe_march, pe_shade and the point functions
// are instantiated for both).  The decisions, one by one:
//   RS (sqrt_rs_ / sqrt_n_ for |p|): OFF for every length, as for PLANET_CLOSEUP.  Their domain is |p|^2 >= 2^-96 at every sample of a
//     march; a test on the origin says nothing about where a ray passes, and a test per sample would cost what the form saves.
//   div3_ quotients and the v_med3 clamp (PL_DIV3, PL_MED3), exp_reg4k_ (PL_EXP4K), exact-integer lattice indices (XI): GUARDED by
//     `tame` below.  For rays: every committing lane's origin within 256 per coordinate, and for the lanes that meet the atmosphere the
//     hit origin hit_o (computed in the plain arithmetic, the same in both forms) and the direction within 4 per coordinate, NaN
//     failing every test.  Then a terrain sample lies at hit_o + t rd with 0 <= t <= 1.6 and a cloud sample at t <= 1.6 + 1.6 / 75:
//     |coordinate| <= 4 + 1.622 * 4 < 10.5 before the rotation and |p| <= 18.2 after it (rot, rot_cloud: products of two rotations of a
//     tame u_time, rows of length 1 up to rounding), the shadow march adds .4: |p| <= 18.6.  From that bound alone, whatever the eye:
//       XI — the finest lattice coordinate is |p| * 2.0987 * 2.0244^6 < 2700 (clouds: 18.6 * 3.2343 * 2.0276^3 + 13.35 < 520), so
//         |n| = |px + 157 py + 113 pz| < 2700 * 271 < 2^20: integers below 2^22, the fmas and the magic-number slot are exact;
//       exp_reg4k_ — its arguments are -30.034 dens t_step in [-2.3, 0] (dens in [0, .94]) and height = (|p| - 1) / .4 in
//         [-2.5, 44]: within |x| <= 80;
//       div3_ — its dividends are finite, and zero or within 2^+-100: differences of fBm sums of order 1 and a literal (zero or
//         >= 2^-26), a sum of two smoothstep values (zero or >= 2^-60), |p| - 1 (zero or >= 2^-25, at most 18), exp(height) <= e^44 <
//         2^64, height - .2 / - .35 (zero or >= 2^-27);
//       v_med3 — no operand is a NaN: every position, length and fBm sum above is finite.
//     For the point functions the same bound is put on the point itself: 16 per coordinate (lattice |n| < 16 * 145 * 271 < 2^20;
//     clouds_density: its height within 2^100 as well, for band()'s two quotients).
//   The shadow march (:355-360) starts at lp = transpose(rot) pos along normalize(lp): a ground hit at the exact centre (a zero
//     direction from an origin at 0 gets there) makes that 0/0, and a NaN height must not reach v_med3.  pe_shade is taken in its short
//     form only if |lp|^2 >= 1e-20 for every shaded lane of the wave (then every component of normalize(lp) is finite, at most 1).
//   The |o|^2 shell skip of the cloud march: kept under `tame` — for a finite o the margin argument beside it (sbx_planet.h's band is
//     the shell 1.08 < |p| < 1.26, |o|^2 outside (1.166, 1.5885) is outside it by 3e-4 relative) names no eye; an inf coordinate, whose
//     d2 passes the test while rot_cloud * o is NaN, fails `tame`.
//   hc_set_direction's look-ahead: kept in the short form.  It decides which cells a miss pass ALSO hashes; what a table holds never
//     changes what a lookup returns (sbx_hashcache.h), for any direction, zero and NaN included (their sign bits are read, no more).
//   The `!wave_any(...)` skips whose skipped work is `*= 1`, `+= 0`: their predicates are evaluated in the arithmetic of the form they
//     stand in, on operands that `tame` has shown finite — fbm * 0 is then +0, not NaN — so they hold for every tame wave.
//   The paired central differences: behind k_planet's own wave-wide test (no zero coordinate), unchanged.
//   illuminate's own smoothsteps, setup_lights and background have one form (smoothstep_, pow_), as in k_planet.
// sbx_debug_planet_eval counts the waves: counts[0] every guarded form on, counts[1] the plain form for at least one part.
#include "sbx_planet.h"

namespace sbx {

enum { PE_RENDER = 0, PE_MARCH = 1, PE_MAP = 2, PE_MAP_DETAIL = 3, PE_NORMAL = 4, PE_CLOUDS = 5, PE_ILLUM = 6, PE_BACKGROUND = 7 };

#ifndef PE_MIN_WAVES
#define PE_MIN_WAVES 4      // 128 VGPRs: nothing parked in LDS, no scratch (tools/kernel_resources.py; profiles/planet_eval_timing.txt)
#endif

__device__ __forceinline__ bool pe_within(v3 v, float b) {           // every coordinate finite and within b (a NaN compares false)
    return abs_(v.x) <= b && abs_(v.y) <= b && abs_(v.z) <= b;
}

// Where the numbers come from (sbx_planet.h's policies one level up: these also carry the rotations, the marches' bounds, the shell's
// |o|^2 interval, illuminate's materials and the two `tame` tests).  PeLit: sbx_planet_eval — a FramePlanet and the header's literals,
// every expression as it stood in this file before the numbers could be a caller's.  PeWorld: sbx_planet_world_eval — a
// FramePlanetWorld (sbx_frames.hip build_planet_world).  Its `tame` tests are the host's block test (F.tame, planet_world_tame) joined
// to wave-wide tests, and for rays they are k_planet_world's, not the 256 / 4 / 18.6 chain: 1 <= |hit_o|^2 <= (2 + max_height)^2 and
// |rd|^2 <= 1.001 (a direction that is no unit vector takes the plain form), under which kern_planet_world.hip's bounds hold as
// written.  For points: within 16 per coordinate — the finest lattice coordinate is (27.8 * 1.50987 + 64) * 2.0244^6 < 7300, times 271
// below 2^21 — and for clouds_density a height that is 0 or of magnitude in [2^-60, 2^100], since a block's band edge may be 0 and the
// dividend height - edge must not fall below div3_'s 2^-100.
struct PeLit {
    const FramePlanet& F;
    __device__ __forceinline__ const m3& rot() const { return F.rot; }
    __device__ __forceinline__ const m3& rot_cloud() const { return F.rot_cloud; }
    __device__ __forceinline__ const m3& rot_t() const { return F.rot_t; }
    __device__ __forceinline__ v3 L() const { return F.L; }
    __device__ __forceinline__ PlLit cloud() const { return PlLit(); }
    __device__ __forceinline__ PlLit terr() const { return PlLit(); }
    __device__ __forceinline__ float max_height() const { return PL_MAX_HEIGHT; }
    __device__ __forceinline__ float max_ray_dist() const { return PL_MAX_RAY_DIST; }
    __device__ __forceinline__ float atm_radius() const { return 1.f + PL_MAX_HEIGHT; }
    __device__ __forceinline__ int terr_steps() const { return 120; }
    __device__ __forceinline__ int cloud_steps() const { return 75; }
    __device__ __forceinline__ int shadow_steps() const { return 5; }
    __device__ __forceinline__ float t_step_cloud() const { return PL_MAX_RAY_DIST / 75.f; }
    __device__ __forceinline__ float t_step_shadow() const { return PL_MAX_HEIGHT / 5.f; }
    // the shell skip of k_planet: o is finite here (SKIP stands under `tame` only)
    __device__ __forceinline__ bool outside_shell(float d2) const { return d2 > 1.5885f || d2 < 1.166f; }
    __device__ __forceinline__ v3 c_water() const { return V3(.015f, .110f, .455f); }
    __device__ __forceinline__ v3 c_water_half() const { return V3(.015f, .110f, .455f) / 2.f; }
    __device__ __forceinline__ v3 c_grass() const { return V3(.086f, .132f, .018f); }
    __device__ __forceinline__ v3 c_beach() const { return V3(.153f, .172f, .121f); }
    __device__ __forceinline__ v3 c_rock() const { return V3(.080f, .050f, .030f); }
    __device__ __forceinline__ v3 c_snow() const { return V3(.600f, .600f, .600f); }
    __device__ __forceinline__ float l_water() const { return .05f; }
    __device__ __forceinline__ float l_shore() const { return .17f; }
    __device__ __forceinline__ float l_grass() const { return .211f; }
    __device__ __forceinline__ float l_rock() const { return .351f; }
    __device__ __forceinline__ v3 key_color() const { return V3(7, 5, 3); }
    // `tame` (the note at the top): on the wave's own origins, hit origins and directions
    __device__ __forceinline__ bool ray_tame(v3 ro, bool hit, v3 hit_o, v3 rd) const {
        return pe_within(ro, 256.f) && (!hit || (pe_within(hit_o, 4.f) && pe_within(rd, 4.f)));
    }
    // `tame` for a point: within 16 per coordinate; clouds_density's height within 2^100 (band's two quotients)
    __device__ __forceinline__ bool point_tame(v3 p, bool clouds, float h) const { return pe_within(p, 16.f) && (!clouds || abs_(h) <= 1.2676506e30f); }
};
struct PeWorld {
    const FramePlanetWorld& F;
    __device__ __forceinline__ const m3& rot() const { return F.terr.rot; }
    __device__ __forceinline__ const m3& rot_cloud() const { return F.cloud.rot_cloud; }
    __device__ __forceinline__ const m3& rot_t() const { return F.shade.rot_t; }
    __device__ __forceinline__ v3 L() const { return F.shade.L; }
    __device__ __forceinline__ PlCloudW cloud() const { return PlCloudW{F.cloud}; }
    __device__ __forceinline__ PlTerrW terr() const { return PlTerrW{F.terr}; }
    __device__ __forceinline__ float max_height() const { return F.terr.max_height; }
    __device__ __forceinline__ float max_ray_dist() const { return F.terr.max_ray_dist; }
    __device__ __forceinline__ float atm_radius() const { return F.atm_radius; }
    __device__ __forceinline__ int terr_steps() const { return F.terr.terr_steps; }
    __device__ __forceinline__ int cloud_steps() const { return F.cloud.cloud_steps; }
    __device__ __forceinline__ int shadow_steps() const { return F.cloud.shadow_steps; }
    __device__ __forceinline__ float t_step_cloud() const { return F.cloud.t_step_cloud; }
    __device__ __forceinline__ float t_step_shadow() const { return F.cloud.t_step_shadow; }
    __device__ __forceinline__ bool outside_shell(float d2) const { return d2 > F.cloud.shell_hi2 || d2 < F.cloud.shell_lo2; }
    __device__ __forceinline__ v3 c_water() const { return F.shade.c_water; }
    __device__ __forceinline__ v3 c_water_half() const { return F.shade.c_water_half; }
    __device__ __forceinline__ v3 c_grass() const { return F.shade.c_grass; }
    __device__ __forceinline__ v3 c_beach() const { return F.shade.c_beach; }
    __device__ __forceinline__ v3 c_rock() const { return F.shade.c_rock; }
    __device__ __forceinline__ v3 c_snow() const { return F.shade.c_snow; }
    __device__ __forceinline__ float l_water() const { return F.shade.l_water; }
    __device__ __forceinline__ float l_shore() const { return F.shade.l_shore; }
    __device__ __forceinline__ float l_grass() const { return F.shade.l_grass; }
    __device__ __forceinline__ float l_rock() const { return F.shade.l_rock; }
    __device__ __forceinline__ v3 key_color() const { return F.shade.key_color; }
    __device__ __forceinline__ bool ray_tame(v3 ro, bool hit, v3 hit_o, v3 rd) const {
        const float ho2 = dot(hit_o, hit_o), rd2 = dot(rd, rd);
        return F.tame != 0 && pe_within(ro, 256.f) && (!hit || (ho2 >= 1.f && ho2 <= F.hit2_max && rd2 <= 1.001f));
    }
    __device__ __forceinline__ bool point_tame(v3 p, bool clouds, float h) const {
        return F.tame != 0 && pe_within(p, 16.f) && (!clouds || (abs_(h) <= 1.2676506e30f && (h == 0.f || abs_(h) >= 0x1p-60f)));
    }
};

// what the marches leave behind for the shading and for "terrain_march"
struct PeRay {
    bool hit_atm;           // :319, committing lanes only
    v3 hit_o;               // hit.origin (0 where the ray misses)
    float t_hit;            // hit.t
    float t, t_pos;         // t at :344; t of the last committed terrain step
    v2 df;                  // :344
    float radiance, alpha;  // cloud after clouds_march
};

// intersect_sphere(eye, atmosphere = {0, 1 + max_height}) on no_hit (intersect.h:7-33), the statement of k_planet with the caller's origin
template <class E>
__device__ __forceinline__ void pe_intersect(const E& e, v3 ro, v3 rd, bool on, PeRay& R) {
    R.hit_atm = false;
    R.hit_o = V3(0, 0, 0);
    R.t_hit = (float)(1e8f + 1e1f);
    const float radius = e.atm_radius();
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
            if (!(t0 > (float)(1e8f + 1e1f)) && on) { R.hit_atm = true; R.t_hit = t0; R.hit_o = ro + rd * t0; }
        }
    }
    R.t = 0.f; R.t_pos = 0.f;
    R.df = V2(1, e.max_height());
    R.radiance = 0.f; R.alpha = 0.f;
}

// the terrain march :328-342 and clouds_march :121-141 of k_planet over the wave's rays; RS = false (the note above)
template <bool SKIP, bool CLD, class E>
__device__ __forceinline__ void pe_march(const E& e, WaveCache& S, v3 rd, PeRay& R, int lane) {
    const bool hit_atm = R.hit_atm;
    const v3 hit_o = R.hit_o;
    float t = 0.f, t_pos = 0.f;
    v2 df = V2(1, e.max_height());
    float max_cld = e.max_ray_dist();
    bool tm = hit_atm;
    if (SKIP && PL_SPEC) hc_set_direction(S, mul(e.rot(), rd), hit_atm, lane);
    for (int i = 0; i < e.terr_steps(); ++i) {
        if (tm && t > e.max_ray_dist()) tm = false;               // `if (t > max_ray_dist) break;`
        if (!wave_any(tm)) break;
        const v3 o = hit_o + t * rd;
        const v3 p = mul(e.rot(), o - V3(0, 0, 0));
        const v2 d = terrain_map<3, SKIP, false>(S, p, tm, lane, e.terr());
        if (tm) {
            t_pos = t;
            df = d;
            if (df.x < .005f) { max_cld = t; tm = false; }
            else t += df.x * .4567f;
        }
    }
    R.t = t; R.t_pos = t_pos; R.df = df;
    if constexpr (CLD) {
        Vol cloud = make_vol(hit_o);
        const float t_step = e.t_step_cloud();
        float tc = 0.f;
        bool cm = hit_atm;
        if (SKIP && PL_SPEC) hc_set_direction(S, mul(e.rot_cloud(), rd), hit_atm, lane);
        for (int i = 0; i < e.cloud_steps(); ++i) {
            if (cm && (tc > max_cld || cloud.alpha >= 1.f)) cm = false;       // `return` of clouds_march
            if (!wave_any(cm)) break;
            const v3 o = cloud.origin + tc * rd;
            {
                const float d2 = dot(o, o);
                if (SKIP && !wave_any(cm && !e.outside_shell(d2))) { tc += t_step; continue; }
            }
            const v3 cp = mul(e.rot_cloud(), o - V3(0, 0, 0));
            const float ch = e.cloud().template div_height<SKIP>(pl_length<false>(cp) - 1.f);
            if (cm) { cloud.pos = cp; cloud.height = ch; }
            tc += t_step;
            clouds_map<SKIP>(S, cloud, t_step, cm, lane, e.cloud());
        }
        R.radiance = cloud.radiance; R.alpha = cloud.alpha;
    }
    if (SKIP && PL_SPEC) hc_no_direction(S, lane);
}

// the three central differences of sdf_terrain_normal :201-212 (before its normalize): pairs behind k_planet's test, else one code copy
template <bool SKIP, class T>
__device__ __forceinline__ v3 pe_normal_differences(WaveCache& S, v3 pos, bool on, int lane, const T& w) {
    const float e = 0.001f;
    float g[3] = {0.f, 0.f, 0.f};
    // (a zero coordinate: pos.c + 0 and pos.c - 0 then differ in the sign of their zero — the unpaired path)
    const bool pairs = SKIP && PL_PAIRS && !wave_any(on && (pos.x == 0.f || pos.y == 0.f || pos.z == 0.f));
    if (pairs) {
        g[0] = terrain_detail_difference<0, SKIP, false>(S, pos, e, on, lane, w);
        g[1] = terrain_detail_difference<1, SKIP, false>(S, pos, e, on, lane, w);
        g[2] = terrain_detail_difference<2, SKIP, false>(S, pos, e, on, lane, w);
    } else {
#pragma unroll 1
        for (int ax = 0; ax < 3; ++ax) {
            const v3 d = V3(ax == 0 ? e : 0.f, ax == 1 ? e : 0.f, ax == 2 ? e : 0.f);
            const float v = terrain_map<7, SKIP, false>(S, pos + d, on, lane, w).x - terrain_map<7, SKIP, false>(S, pos - d, on, lane, w).x;
            if (ax == 0) g[0] = v; else if (ax == 1) g[1] = v; else g[2] = v;
        }
    }
    return V3(g[0], g[1], g[2]);
}

// illuminate :238-298 with local_xform = rot (F.L = rot * normalize(1, 1, 0))
template <bool SKIP, class E>
__device__ __forceinline__ v3 pe_illuminate(const E& e, WaveCache& S, v3 pos, float h, bool on, int lane) {
    const v3 w_normal = normalize(pos);
    const v3 normal = normalize(pe_normal_differences<SKIP>(S, pos, on, lane, e.terr()));
    const float N = dot(normal, w_normal);
    const v3 c_water = e.c_water(), c_grass = e.c_grass(), c_beach = e.c_beach(), c_rock = e.c_rock(), c_snow = e.c_snow();
    const float l_water = e.l_water(), l_shore = e.l_shore(), l_grass = e.l_grass(), l_rock = e.l_rock();
    const float s = smoothstep_(.4f, 1.f, h);
    const v3 rock = mix3(c_rock, c_snow, smoothstep_(1.f - .3f * s, 1.f - .2f * s, N));
    const v3 grass = mix3(c_grass, rock, smoothstep_(l_grass, l_rock, h));
    v3 shoreline = mix3(c_beach, grass, smoothstep_(l_shore, l_grass, h));
    const v3 water = mix3(e.c_water_half(), c_water, smoothstep_(0.f, l_water, h));
    shoreline = shoreline * setup_lights(e.L(), normal, e.key_color());
    const v3 ocean = setup_lights(e.L(), w_normal, e.key_color()) * water;
    return mix3(ocean, shoreline, smoothstep_(l_water, l_shore, h));
}

// :349-363 for the lanes with a ground hit: illuminate, the cloud shadow on the ground, the composite
template <bool SKIP, class E>
__device__ __forceinline__ v3 pe_shade(const E& e, WaveCache& S, v3 pos, float h, float c_cld, float alpha, bool hitl, int lane) {
    const v3 c_terr = pe_illuminate<SKIP>(e, S, pos, h, hitl, lane);
    const v3 lp = mul(e.rot_t(), pos);
    Vol sh = make_vol(lp);
    const v3 local_up = normalize(lp);
    const float t_step = e.t_step_shadow();
    float ts = 0.f;
    for (int i = 0; i < e.shadow_steps(); ++i) {
        const v3 o = sh.origin + ts * local_up;
        sh.pos = mul(e.rot_cloud(), o - V3(0, 0, 0));
        sh.height = e.cloud().template div_height<SKIP>(pl_length<false>(sh.pos) - 1.f);
        ts += t_step;
        clouds_map<SKIP>(S, sh, t_step, hitl, lane, e.cloud());
    }
    const float shadow = mix_(.7f, 1.f, step_(sh.alpha, 0.33f));
    return abs3(mix3(c_terr * shadow, V3s(c_cld), alpha));
}

// the body of one point function under one form; r = its outputs
template <int FN, bool SKIP, class E>
__device__ __forceinline__ void pe_point(const E& e, WaveCache& S, const float (&q)[6], bool on, int lane, float (&r)[4]) {
    const v3 pos = V3(q[0], q[1], q[2]);
    if (FN == PE_MAP || FN == PE_MAP_DETAIL) {
        const v2 d = terrain_map<FN == PE_MAP ? 3 : 7, SKIP, false>(S, pos, on, lane, e.terr());
        r[0] = d.x; r[1] = d.y;
    } else if (FN == PE_NORMAL) {
        const v3 nrm = normalize(pe_normal_differences<SKIP>(S, pos, on, lane, e.terr()));
        r[0] = nrm.x; r[1] = nrm.y; r[2] = nrm.z;
    } else if (FN == PE_CLOUDS) {
        // false: the density of every committing lane is exactly +0 (the skips of clouds_density, their operands finite under `tame`)
        float dens = 0.f, T_i = 1.f;
        if (!clouds_density<SKIP>(S, pos, q[3], e.t_step_cloud(), on, lane, dens, T_i, e.cloud())) dens = 0.f;
        r[0] = dens;
    } else {
        const v3 c = pe_illuminate<SKIP>(e, S, pos, q[3], on, lane);
        r[0] = c.x; r[1] = c.y; r[2] = c.z;
    }
}

constexpr int pe_in_width(int fn) { return fn <= PE_MARCH ? 6 : (fn == PE_CLOUDS || fn == PE_ILLUM) ? 4 : 3; }
constexpr int pe_out_width(int fn) { return fn <= PE_MARCH ? 4 : fn <= PE_MAP_DETAIL ? 2 : fn == PE_CLOUDS ? 1 : 3; }

// one wave of either entry: e = PeLit over k_planet_eval's FramePlanet, PeWorld over k_planet_world_eval's FramePlanetWorld
template <int FN, bool PLAIN, class E>
__device__ __forceinline__ void pe_wave(const E& e, const float* __restrict__ in, float* __restrict__ out, size_t n, unsigned* __restrict__ counts) {
    constexpr int WIN = pe_in_width(FN), WOUT = pe_out_width(FN);
    __shared__ WaveCache cache[1];
    const int lane = threadIdx.x & 63;
    WaveCache& S = cache[0];
    if (FN != PE_BACKGROUND) hc_init(S, lane);
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool on = i < n;
    float q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
#pragma unroll
        for (int k = 0; k < WIN; ++k) q[k] = in[(size_t)WIN * i + k];
    }
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    bool fast = !PLAIN;                                             // wave-uniform throughout
    if (FN == PE_BACKGROUND) {
        const v3 c = planet_background(V3(q[0], q[1], q[2]));
        r[0] = c.x; r[1] = c.y; r[2] = c.z;
    } else if (FN <= PE_MARCH) {
        const v3 ro = V3(q[0], q[1], q[2]), rd = V3(q[3], q[4], q[5]);
        PeRay R;
        pe_intersect(e, ro, rd, on, R);
        if (!PLAIN) fast = !wave_any(on && !e.ray_tame(ro, R.hit_atm, R.hit_o, rd));
        if (wave_any(R.hit_atm)) {
            if (fast) pe_march<true, FN == PE_RENDER>(e, S, rd, R, lane);
            else pe_march<false, FN == PE_RENDER>(e, S, rd, R, lane);
        }
        if (FN == PE_MARCH) {
            r[0] = R.t_hit; r[1] = R.t; r[2] = R.df.x; r[3] = R.df.y;
        } else {
            const bool hitl = R.hit_atm && (R.df.x < .005f);        // :349
            v3 col = V3(0, 0, 0);
            if (wave_any(hitl)) {
                // the point of the last committed step, as the march computed it
                const v3 pos = mul(e.rot(), (R.hit_o + R.t_pos * rd) - V3(0, 0, 0));
                const v3 lp = mul(e.rot_t(), pos);
                if (fast && wave_any(hitl && !(dot(lp, lp) >= 1e-20f))) fast = false;      // normalize(lp) of the shadow march
                if (fast) col = pe_shade<true>(e, S, pos, R.df.y, R.radiance, R.alpha, hitl, lane);
                else col = pe_shade<false>(e, S, pos, R.df.y, R.radiance, R.alpha, hitl, lane);
            }
            if (R.hit_atm && !hitl) col = abs3(mix3(planet_background(rd), V3s(R.radiance), R.alpha));   // :364-366
            if (!R.hit_atm) col = planet_background(rd);            // :316-320
            r[0] = col.x; r[1] = col.y; r[2] = col.z; r[3] = R.hit_atm ? R.alpha : 0.f;
        }
    } else {
        if (!PLAIN) fast = !wave_any(on && !e.point_tame(V3(q[0], q[1], q[2]), FN == PE_CLOUDS, q[3]));
        if (fast) pe_point<FN, true>(e, S, q, on, lane, r);
        else pe_point<FN, false>(e, S, q, on, lane, r);
    }
    if (on) {
#pragma unroll
        for (int k = 0; k < WOUT; ++k) out[(size_t)WOUT * i + k] = r[k];
    }
    if (counts && lane == 0) atomicAdd(counts + (fast ? 0 : 1), 1u);
}

template <int FN, bool PLAIN>
__global__ void __launch_bounds__(64, PE_MIN_WAVES) k_planet_eval(FramePlanet F, const float* __restrict__ in, float* __restrict__ out, size_t n,
                                                                  unsigned* __restrict__ counts) {
    pe_wave<FN, PLAIN>(PeLit{F}, in, out, n, counts);
}
// sbx_planet_world_eval: the same wave over the caller's world (the camera of F is not read)
template <int FN, bool PLAIN>
__global__ void __launch_bounds__(64, PE_MIN_WAVES) k_planet_world_eval(FramePlanetWorld F, const float* __restrict__ in, float* __restrict__ out, size_t n,
                                                                        unsigned* __restrict__ counts) {
    pe_wave<FN, PLAIN>(PeWorld{F}, in, out, n, counts);
}

template <int FN>
static void pe_launch(const FramePlanet& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    if (plain) hipLaunchKernelGGL((k_planet_eval<FN, true>), grid, dim3(64), 0, s, F, in, out, n, counts);
    else hipLaunchKernelGGL((k_planet_eval<FN, false>), grid, dim3(64), 0, s, F, in, out, n, counts);
}

// fn: PE_* in the order of sbx_eval.hip's names.  F: build_planet of u_time (its camera is not read).  plain: sbx_set_variant 1 or an
// untame u_time.  counts: NULL, or two zeroed device words.  n in 1 ... 2^31.
void launch_planet_eval(int fn, const FramePlanet& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    switch (fn) {
    case PE_RENDER: pe_launch<PE_RENDER>(F, plain, in, out, n, counts, s); break;
    case PE_MARCH: pe_launch<PE_MARCH>(F, plain, in, out, n, counts, s); break;
    case PE_MAP: pe_launch<PE_MAP>(F, plain, in, out, n, counts, s); break;
    case PE_MAP_DETAIL: pe_launch<PE_MAP_DETAIL>(F, plain, in, out, n, counts, s); break;
    case PE_NORMAL: pe_launch<PE_NORMAL>(F, plain, in, out, n, counts, s); break;
    case PE_CLOUDS: pe_launch<PE_CLOUDS>(F, plain, in, out, n, counts, s); break;
    case PE_ILLUM: pe_launch<PE_ILLUM>(F, plain, in, out, n, counts, s); break;
    default: pe_launch<PE_BACKGROUND>(F, plain, in, out, n, counts, s); break;
    }
}

template <int FN>
static void pe_world_launch(const FramePlanetWorld& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    const dim3 grid((unsigned)((n + 63) / 64));
    if (plain) hipLaunchKernelGGL((k_planet_world_eval<FN, true>), grid, dim3(64), 0, s, F, in, out, n, counts);
    else hipLaunchKernelGGL((k_planet_world_eval<FN, false>), grid, dim3(64), 0, s, F, in, out, n, counts);
}

// sbx_planet_world_eval: launch_planet_eval's contract over F = build_planet_world of the caller's block.  plain: sbx_set_variant 1; an
// untame block (F.tame == 0) sends every wave of the other kernel to its plain form as well.
void launch_planet_world_eval(int fn, const FramePlanetWorld& F, bool plain, const float* in, float* out, size_t n, unsigned* counts, hipStream_t s) {
    switch (fn) {
    case PE_RENDER: pe_world_launch<PE_RENDER>(F, plain, in, out, n, counts, s); break;
    case PE_MARCH: pe_world_launch<PE_MARCH>(F, plain, in, out, n, counts, s); break;
    case PE_MAP: pe_world_launch<PE_MAP>(F, plain, in, out, n, counts, s); break;
    case PE_MAP_DETAIL: pe_world_launch<PE_MAP_DETAIL>(F, plain, in, out, n, counts, s); break;
    case PE_NORMAL: pe_world_launch<PE_NORMAL>(F, plain, in, out, n, counts, s); break;
    case PE_CLOUDS: pe_world_launch<PE_CLOUDS>(F, plain, in, out, n, counts, s); break;
    case PE_ILLUM: pe_world_launch<PE_ILLUM>(F, plain, in, out, n, counts, s); break;
    default: pe_world_launch<PE_BACKGROUND>(F, plain, in, out, n, counts, s); break;
    }
}

hipError_t bind_fault_planet_eval(unsigned* word) { return hc_bind_fault_word(word); }

}  // namespace sbx
