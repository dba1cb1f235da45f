// shaderbox_amd/csrc/sbx_capi.hip — the core of the C ABI of libsbx (include/sbx.h): the context's life, the ONE place a render
// kernel is launched (render_mapped), the row-range entry points, the setters and the fault word.  The rest of the host layer is
// mapped in sbx_ctx.h.
//
// Host side of the drop-in: what the reference's hosts do around mainImage() — own the uniforms
// and the render target, pick the app, issue one draw per frame (util/hlsltoy/src/hlsltoy.cpp:
// 402-426, 494-516) — reduced to: validate, build the per-frame constant block for the app with the
// shared math spec, launch the app's kernel on the caller's stream.  There is NO CPU fallback: without
// a gfx950 device sbx_create fails with SBX_ERR_NO_DEVICE.
#include "sbx_ctx.h"
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace sbx;

// The sticky fault word of each device (sbx_hashcache.h g_hc_fault): pinned host memory the kernels can write and the host can
// read without synchronising; process-wide, shared by the contexts of a device, never freed.
static unsigned* g_fault_word[64] = {nullptr};
static std::mutex g_fault_lock;
static int bind_fault_word(int device) {
    std::lock_guard<std::mutex> g(g_fault_lock);
    if (device < 0 || device >= 64) return SBX_ERR_ARG;
    if (!g_fault_word[device]) {
        unsigned* w = nullptr;
        if (hipHostMalloc((void**)&w, 64, hipHostMallocMapped) != hipSuccess) return SBX_ERR_HIP;
        *w = 0u;
        g_fault_word[device] = w;
    }
    unsigned* dev = nullptr;
    if (hipHostGetDevicePointer((void**)&dev, g_fault_word[device], 0) != hipSuccess) return SBX_ERR_HIP;
    if (bind_fault_clouds(dev) != hipSuccess || bind_fault_clouds_ue4(dev) != hipSuccess || bind_fault_planet(dev) != hipSuccess ||
        bind_fault_planet_eval(dev) != hipSuccess || bind_fault_planet_world(dev) != hipSuccess)
        return SBX_ERR_HIP;
    return SBX_OK;
}

namespace sbx {
unsigned* fault_word_device(int device) {
    unsigned* dev = nullptr;
    if (device < 0 || device >= 64 || !g_fault_word[device]) return nullptr;
    if (hipHostGetDevicePointer((void**)&dev, g_fault_word[device], 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return dev;
}
int ctx_device(const sbx_ctx* ctx) { return ctx->device; }
}  // namespace sbx

namespace sbx {
int fail(sbx_ctx* ctx, int code, const char* what, hipError_t e) {
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}
int ctx_fail(sbx_ctx* ctx, int code, const char* what, hipError_t e) { return fail(ctx, code, what, e); }
int use_device(sbx_ctx* ctx) {
    const hipError_t e = hipSetDevice(ctx->device);
    return e == hipSuccess ? SBX_OK : fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
}
int launched(sbx_ctx* ctx, const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SBX_OK : fail(ctx, SBX_ERR_HIP, what, e);
}
bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}
}  // namespace sbx

static void release(Timers& T) {
    for (auto& t : T.pairs) { (void)hipEventDestroy(t.second.ev0); (void)hipEventDestroy(t.second.ev1); }
    T.pairs.clear(); T.last = -1;
}
// HostStaging's "all of the streams and events, or none": also what undoes a set-up that stopped half way
static void release_streams(HostStaging& S) {
    if (S.copy) { (void)hipStreamDestroy(S.copy); S.copy = nullptr; }
    for (auto& st : S.render) if (st) { (void)hipStreamDestroy(st); st = nullptr; }
    if (S.entry) { (void)hipEventDestroy(S.entry); S.entry = nullptr; }
    for (auto& ev : S.ev) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    S.ready = false;
}
static void release(HostStaging& S) {
    if (S.dev) (void)hipFree(S.dev);
    S.dev = nullptr; S.cap = 0;
    release_streams(S);
}
// every group's release tolerates members that were never built: this is sbx_destroy, and what a failed sbx_create leaves behind
static void destroy_ctx(sbx_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    release(ctx->ytab);
    release(ctx->hashtab);
    release(ctx->viewtab, ctx->event_pool);
    release(ctx->mi);
    tile_order_destroy(ctx->tile_orders);
    release(ctx->hs);
    release(ctx->spans);
    release(ctx->noise);
    release(ctx->tex2d);
    if (ctx->func_tab) (void)hipFree(ctx->func_tab);
    for (auto& e : ctx->event_pool) (void)hipEventDestroy(e);
    release(ctx->timers);
    delete ctx;
}

extern "C" {

int sbx_create(int device, sbx_ctx** out) {
    if (!out) return SBX_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SBX_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return SBX_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SBX_ERR_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SBX_ERR_NO_DEVICE;   // kernels exist for gfx950 only
    sbx_ctx* ctx = new sbx_ctx();
    ctx->device = device;
    ctx->tile_orders.pool = &ctx->event_pool;
    for (auto& en : ctx->mi.frames) for (auto& w : en.key) w.store(0xffffffffu, std::memory_order_relaxed);
    if (hipSetDevice(device) != hipSuccess ||
        hipMalloc((void**)&ctx->ytab.ring, (size_t)(CLOUDS_YTAB_RING + CLOUDS_YTAB_CAPTURE) * CLOUDS_YTAB_BYTES) != hipSuccess ||
        bind_fault_word(device) != SBX_OK) {
        destroy_ctx(ctx);
        return SBX_ERR_HIP;
    }
    {   // APP_2D_TEX's default t0 (256 KB): the UNORM words decoded on the host, c / 255 in binary32 as the device decode does
        constexpr int n = TEX2D_DEFAULT * TEX2D_DEFAULT;
        std::vector<uint32_t> words(n);
        std::vector<float4> texels(n);
        sbx_checkerboard_texture(TEX2D_DEFAULT, TEX2D_DEFAULT_FREQ, words.data());
        for (int i = 0; i < n; ++i) {
            const uint32_t w = words[i];
            texels[i] = make_float4((float)(w & 255u) / 255.f, (float)((w >> 8) & 255u) / 255.f, (float)((w >> 16) & 255u) / 255.f,
                                    (float)(w >> 24) / 255.f);
        }
        if (hipMalloc((void**)&ctx->tex2d.def, n * sizeof(float4)) != hipSuccess ||
            hipMemcpy(ctx->tex2d.def, texels.data(), n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess) {
            destroy_ctx(ctx);
            return SBX_ERR_HIP;
        }
    }
    if (hipMalloc((void**)&ctx->func_tab, func_table_bytes()) != hipSuccess ||
        (launch_func_table(ctx->func_tab, nullptr), hipGetLastError()) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
        destroy_ctx(ctx);
        return SBX_ERR_HIP;
    }
    *out = ctx;
    return SBX_OK;
}

void sbx_destroy(sbx_ctx* ctx) {
    if (ctx) destroy_ctx(ctx);
}

static const char* kFaultText = "an earlier launch on this device hit the bound of the hash cache's miss loop (sbx_hashcache.h): its "
                                "pixels are invalid; re-render after sbx_clear_fault";
static const char* kFaultTextWait = "a wait of the store exchange (sbx_shared_frame_begin / _end) on this device gave up: a rank's signal did not "
                                    "arrive in time, the frame is incomplete; re-render after sbx_clear_fault";
static unsigned device_fault_code(const sbx_ctx* ctx) {
    const unsigned* w = (ctx->device >= 0 && ctx->device < 64) ? g_fault_word[ctx->device] : nullptr;
    return w ? *(volatile const unsigned*)w : 0u;
}
static bool device_fault(const sbx_ctx* ctx) { return device_fault_code(ctx) != 0u; }
static const char* fault_text(const sbx_ctx* ctx) {
    const unsigned c = device_fault_code(ctx);
    return c == 2u ? kFaultTextWait : kFaultText;
}

// Domain of the margin-based culls of EGG / SDF_AO / VINYL (bounding spheres and boxes around members placed by rotations) and
// of PLANET's |o|^2 band test (a rotation preserves the norm): their proofs take the frame's rotations to BE rotations.  The
// spec's sin / cos reduce their argument with a two-term pi, which is accurate while |angle| < 2^30 or so; the fastest angle
// of any app is 400 degrees = 7 rad per second of u_time (src/app_egg.h:73), so |u_time| <= 1e8 keeps every matrix entry the
// correctly rounded sin / cos of its angle (orthonormal to 2e-7; the margins are >= 3e-4 relative).  Beyond that, and for
// NaN / inf, the reduction returns what it returns (the oracle's does the same) and the PLAIN kernels run: same operations
// as the reference on whatever the matrices are.  (APP_CLOUDS has its own per-launch checks: clouds_regular,
// clouds_lip_domain in kern_clouds.hip.)
static bool tame_time(float t) { return std::fabs(t) <= 1e8f; }      // NaN compares false

}  // extern "C"

int sbx::render_mapped(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, const RowMap& M_in, float* rgba, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    if (M_in.nrows == 0) return SBX_OK;
    if (device_fault(ctx)) return fail(ctx, SBX_ERR_FAULT, fault_text(ctx));
    // argument checks come before anything is enqueued or recorded
    if (!app_valid(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "app is not on the accelerated path");
    const AppTraits& T = kApps[app];
    if (T.own_alpha && (M_in.rgb == 1 || M_in.rgb == 3))
        return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: three-channel outputs cannot hold its pixels");
    sbx_aux_clouds AC;
    if (T.aux == AUX_CLOUDS) {
        AC = aux_clouds(aux);
        if (AC.cld_march_steps < 0 || AC.illum_march_steps < 0) return fail(ctx, SBX_ERR_ARG, "negative march steps");
    }
    sbx_aux_raytracer_scene RS;
    if (T.aux == AUX_RT_SCENE) {
        RS = aux_raytracer_scene(aux, *uni);
        if (const char* why = raytracer_scene_check(RS)) return fail(ctx, SBX_ERR_ARG, why);
    }
    sbx_aux_sdf_scene SS;
    if (T.aux == AUX_SDF_SCENE) {
        SS = aux_sdf_scene(aux, *uni);
        if (const char* why = sdf_scene_check(SS, false)) return fail(ctx, SBX_ERR_ARG, why);
    }
    sbx_aux_egg_pose EP;
    if (T.aux == AUX_EGG_POSE) EP = aux_egg_pose(aux, *uni);               // (every bit pattern is data: nothing to refuse)
    sbx_aux_vinyl_deck VD;
    if (T.aux == AUX_VINYL_DECK) VD = aux_vinyl_deck(aux, *uni);           // (likewise)
    sbx_aux_atmosphere_air AA;
    if (T.aux == AUX_ATM_AIR) {
        AA = aux_atmosphere_air(aux, *uni);
        if (const char* why = atmosphere_air_check(AA, true)) return fail(ctx, SBX_ERR_ARG, why);
    }
    sbx_aux_planet_world PW;
    if (T.aux == AUX_PLANET_WORLD) {
        PW = aux_planet_world(aux, *uni);
        if (const char* why = planet_world_check(PW)) return fail(ctx, SBX_ERR_ARG, why);
    }
    if (T.noise_volumes && !ctx->noise.shape) return fail(ctx, SBX_ERR_ARG, "APP_CLOUDS with USE_NOISE_TEX needs sbx_set_noise_volume first");
    const bool capturing = stream_is_capturing(s);
    TimingPair* tp = nullptr;
    if (ctx->timers.enabled && !capturing) {                               // events recorded into a capture would time nothing
        int idx = -1;
        for (size_t i = 0; i < ctx->timers.pairs.size(); ++i) if (ctx->timers.pairs[i].first == s) idx = (int)i;
        if (idx < 0) {
            TimingPair p;
            if ((e = hipEventCreate(&p.ev0)) != hipSuccess || (e = hipEventCreate(&p.ev1)) != hipSuccess)
                return fail(ctx, SBX_ERR_HIP, "hipEventCreate", e);
            ctx->timers.pairs.emplace_back(s, p);
            idx = (int)ctx->timers.pairs.size() - 1;
        }
        tp = &ctx->timers.pairs[idx].second;
        tp->complete = false;
        ctx->timers.last = idx;
        (void)hipEventRecord(tp->ev0, s);
    }
    int rc = SBX_OK;
    ctx->stats.launches.fetch_add(1, std::memory_order_relaxed);
    const int cull_variant = tame_time(uni->u_time) ? ctx->variant : 1;
    const int sdf_variant = witness_variant(ctx, tame_time(uni->u_time));   // EGG / SDF_AO / VINYL and their builds
    // The dispatch order of this launch (TileOrder): the tiles by the cost earlier frames of this app and shape measured, longest
    // first.  For the kernels it was measured to help (profiles/r06_tile_order.txt: CLOUDS 4K 2.41 -> 2.23 ms, CLOUDS_SKY 5.14 ->
    // 4.91, VINYL 1.25 -> 1.19, VINYL_GPU 1.24 -> 1.14, and APP_EGG 1920x1080 0.205 -> 0.134 ms back to back — its launch drags a tail
    // of ~350 silhouette waves of up to 175 us behind it, some of which the hot-first order starts 40 us into the launch; under the
    // table they are the first to start); within +-0.6 % for ATMOSPHERE, PLANET, RAYTRACER, SDF_AO, +1.6 % for CLOUDS_BEST: those
    // keep their own order (kApps: no order grid).  (Until the table is there, and with frames in flight, k_egg's hot-first order
    // stands; the per-lane variant of k_clouds takes no table.)
    const bool ordered_app = T.order_grid && !(T.aux == AUX_CLOUDS && ctx->variant == 1);
    const dim3 og = ordered_app ? T.order_grid(M_in) : dim3(0, 0, 1);
    RowMap M = M_in;
    unsigned long long scene = 1469598103934665603ull;           // FNV-1a of the frame's uniforms (and APP_CLOUDS' aux block): "the same scene"
    if (og.x) {
        auto mix = [&scene](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) scene = (scene ^ ((const unsigned char*)p)[i]) * 1099511628211ull; };
        mix(uni, sizeof(*uni));
        if (T.aux == AUX_CLOUDS) mix(&AC, sizeof(AC));
        if (T.aux == AUX_EGG_POSE) mix(&EP, sizeof(EP));                   // (the pose IS the scene: a pose that stands still gets its table)
        if (T.aux == AUX_VINYL_DECK) mix(&VD, sizeof(VD));                 // (and so is the deck: one deck is never served another's table)
    }
    TileOrder* const ordered = tile_order_begin(ctx->tile_orders, app, M, og, s, capturing, scene, T.scene_policy);
    switch (app) {
    case SBX_APP_CLOUDS: rc = render_clouds(ctx, build_clouds(*uni, AC), M, rgba, s, capturing); break;
    // the builds of illuminate_volume's two switches (include/sbx.h): the same frame constants and the same y tables
    case SBX_APP_CLOUDS_HEIGHT: rc = render_clouds(ctx, build_clouds(*uni, AC), M, rgba, s, capturing, CLOUDS_HEIGHT); break;
    case SBX_APP_CLOUDS_LUMINANCE: rc = render_clouds(ctx, build_clouds(*uni, AC), M, rgba, s, capturing, CLOUDS_LUMINANCE); break;
    case SBX_APP_CLOUDS_SKY:
        ctx->hashtab.last_used = 0;
        ctx->viewtab.last_used = 0; ctx->viewtab.last_refusal = SBX_VIEWTAB_INELIGIBLE;
        launch_clouds(build_clouds(*uni, AC, true), M, rgba, s, ctx->variant, nullptr, 0, false, CLOUDS_DEFAULT, nullptr, &ctx->hashtab.last_selection);
        break;
    case SBX_APP_CLOUDS_TEX: launch_clouds_tex(build_clouds(*uni, AC), M, rgba, s, ctx->noise.shape, ctx->noise.shape_size, ctx->noise.detail, ctx->noise.detail_size,
                                                    // a captured launch is replayed later, possibly over volumes re-bound in place with
                                                    // other texel ranges: no bounds baked into a graph (the plain exp_ / IEEE divide)
                                                    (ctx->noise.bounds_valid && !capturing) ? ctx->noise.bounds : nullptr); break;
    // one scene, three builds of app_egg.h (include/sbx.h).  The app is part of the key of a dispatch-order table (tile_order_begin) and
    // of a frame cached by sbx_main_image (mi_make_key): neither is ever served to another build
    case SBX_APP_EGG: launch_egg(build_egg(*uni, EGG_DEFAULT), M, rgba, s, sdf_variant, EGG_DEFAULT); break;
    case SBX_APP_EGG_STRAIGHT: launch_egg(build_egg(*uni, EGG_STRAIGHT), M, rgba, s, sdf_variant, EGG_STRAIGHT); break;
    case SBX_APP_EGG_OVAL: launch_egg(build_egg(*uni, EGG_OVAL), M, rgba, s, sdf_variant, EGG_OVAL); break;
    // the shipped build over the caller's pose (include/sbx.h): the same kernels over another frame block; a pose outside the domain
    // of their culls and witnessed roots (sbx_frames.hip egg_pose_tame) takes the reference form
    case SBX_APP_EGG_POSE: {
        const FrameEggStraight F = build_egg_pose(*uni, EP, EGG_DEFAULT);
        const bool tame = egg_pose_tame(EP, F);
        ctx->stats.egg_pose_launches.fetch_add(1, std::memory_order_relaxed);
        if (!tame) ctx->stats.egg_pose_untame.fetch_add(1, std::memory_order_relaxed);
        launch_egg(F, M, rgba, s, witness_variant(ctx, tame && tame_time(uni->u_time)), EGG_DEFAULT);   // (u_time as for APP_EGG)
        break;
    }
    case SBX_APP_RAYTRACER: launch_raytracer(build_raytracer(*uni), M, rgba, s, witness_variant(ctx)); break;
    // the builds of app_raytracer.h's three switches (include/sbx.h): two kernel builds over the shipped frame, one frame of its own
    case SBX_APP_RAYTRACER_PHONG: launch_raytracer(build_raytracer(*uni), M, rgba, s, witness_variant(ctx), RT_PHONG); break;
    case SBX_APP_RAYTRACER_NOSHADOW: launch_raytracer(build_raytracer(*uni), M, rgba, s, witness_variant(ctx), RT_NOSHADOW); break;
    case SBX_APP_RAYTRACER_STATIC: launch_raytracer(build_raytracer(*uni, RT_STATIC), M, rgba, s, witness_variant(ctx), RT_STATIC); break;
    // the caller's scene (validated above), always through its own kernel: a block equal to the Cornell box is no special case
    case SBX_APP_RAYTRACER_SCENE:
        launch_raytracer_scene(build_raytracer_scene(*uni, RS), M, rgba, s, witness_variant(ctx));
        ctx->stats.rt_scene_launches.fetch_add(1, std::memory_order_relaxed);
        break;
    case SBX_APP_ATMOSPHERE: launch_atmosphere(build_atmosphere(*uni), M, rgba, s, ctx->precision); break;
    case SBX_APP_ATMOSPHERE_GROUND: launch_atmosphere_ground(build_atmosphere_ground(*uni), M, rgba, s, ctx->precision, ctx->variant); break;
    // app_atmosphere.h over the caller's air (validated above).  sbx_set_precision does not enter.  The tier (sbx_atmosphere.h "CALLER'S
    // AIR"): the shipped kernels over the block's sun, the run-time kernel with its per-wave selection, or the plain statement
    case SBX_APP_ATMOSPHERE_AIR: {
        const FrameAtmosphere F = build_atmosphere_air(*uni, AA);
        const int tier = atmosphere_air_tier(AA, ctx->variant, true);
        ctx->stats.atm_air_launches.fetch_add(1, std::memory_order_relaxed);
        if (tier == ATM_AIR_LITERAL) ctx->stats.atm_air_literal.fetch_add(1, std::memory_order_relaxed);
        if (tier == ATM_AIR_PLAIN) ctx->stats.atm_air_plain.fetch_add(1, std::memory_order_relaxed);
        if (tier != ATM_AIR_LITERAL) launch_atmosphere_air(F, atmosphere_air_numbers(AA), AA.view, tier == ATM_AIR_RUNTIME, M, rgba, s);
        else if (AA.view == 0) launch_atmosphere(F, M, rgba, s, 0, atmosphere_air_literal_fin(AA, F));
        else launch_atmosphere_ground(F, M, rgba, s, 0, 0, atmosphere_air_literal_fin(AA, F));
        break;
    }
    // one scene, three builds of app_sdf_ao.h (include/sbx.h)
    case SBX_APP_SDF_AO: launch_sdf_ao(build_sdf_ao(*uni, aux_sdf_ao(aux)), M, rgba, s, sdf_variant, 0); break;
    case SBX_APP_SDF_AO_SHADOW: launch_sdf_ao(build_sdf_ao(*uni, aux_sdf_ao(aux)), M, rgba, s, sdf_variant, 1); break;
    case SBX_APP_SDF_AO_NORMALS: launch_sdf_ao(build_sdf_ao(*uni, aux_sdf_ao(aux)), M, rgba, s, sdf_variant, 2); break;
    // the caller's field (validated above) through app_sdf_ao.h's renderer
    case SBX_APP_SDF_SCENE: launch_sdf_scene(build_sdf_scene(*uni, SS), M, rgba, s, witness_variant(ctx)); break;
    case SBX_APP_PLANET: launch_planet(build_planet(*uni), M, rgba, s, cull_variant); break;
    case SBX_APP_PLANET_ATMOSPHERE: launch_planet(build_planet(*uni, true), M, rgba, s, cull_variant); break;
    // the builds of app_planet.h's three switches (include/sbx.h): kernel builds over the shipped frame, CLOSEUP over a frame of its own
    case SBX_APP_PLANET_CLOSEUP: launch_planet(build_planet(*uni, false, PLANET_CLOSEUP), M, rgba, s, cull_variant, PLANET_CLOSEUP); break;
    case SBX_APP_PLANET_CLOUDLESS: launch_planet(build_planet(*uni), M, rgba, s, cull_variant, PLANET_CLOUDLESS); break;
    case SBX_APP_PLANET_UNLIT: launch_planet(build_planet(*uni), M, rgba, s, cull_variant, PLANET_UNLIT); break;
    // app_planet.h over the caller's world (validated above; u_time is not read, so its tameness does not enter: the block's does).
    // The tier (sbx_frames.hip planet_world_tier, kern_planet_world.hip).  LITERAL: SBX_APP_PLANET's kernels over the block's camera,
    // angles and sun — the shipped instantiation, short roots and all, only for the shipped camera bit for bit; any other camera takes
    // PLANET_CLOSEUP's code (the IEEE root: sbx_planet.h PL_SQRT_RS), and a camera or angles outside planet_world_camera_tame's bounds
    // k_planet<false>.  Otherwise k_planet_world, fast for a tame block; under sbx_set_variant 1 k_planet_world<false> for every block
    case SBX_APP_PLANET_WORLD: {
        const int tier = planet_world_tier(PW, ctx->variant);
        if (tier == PLANET_WORLD_LITERAL) {
            const FramePlanet F = build_planet_world_literal(*uni, PW);
            sbx_aux_planet_world D;
            sbx_planet_world_default(uni, &D);
            const bool shipped_cam = std::memcmp(PW.eye, D.eye, 4 * sizeof(float)) == 0 && std::memcmp(PW.look_at, D.look_at, 3 * sizeof(float)) == 0;
            const bool skip = planet_world_camera_tame(PW, F);                  // (the variant is not 1 here: planet_world_tier)
            (skip ? ctx->stats.planet_world_literal : ctx->stats.planet_world_plain).fetch_add(1, std::memory_order_relaxed);
            launch_planet(F, M, rgba, s, skip ? ctx->variant : 1, shipped_cam ? PLANET_DEFAULT : PLANET_CLOSEUP);
        } else {
            (tier == PLANET_WORLD_RUNTIME ? ctx->stats.planet_world_runtime : ctx->stats.planet_world_plain).fetch_add(1, std::memory_order_relaxed);
            launch_planet_world(build_planet_world(*uni, PW), tier == PLANET_WORLD_RUNTIME, M, rgba, s);
        }
        break;
    }
    case SBX_APP_VINYL: launch_vinyl(build_vinyl(*uni, 60), M, rgba, s, sdf_variant); break;
    case SBX_APP_VINYL_GPU: launch_vinyl(build_vinyl(*uni, 180), M, rgba, s, sdf_variant); break;
    // the builds of app_vinyl.h's three switches (include/sbx.h), 60 steps each: one frame of its own for the shipped kernels, two kernel
    // builds over the shipped frame.  The app is part of the key of a dispatch-order table and of sbx_main_image's cached frame
    case SBX_APP_VINYL_CLOSEUP: launch_vinyl(build_vinyl(*uni, 60, VINYL_CLOSEUP), M, rgba, s, sdf_variant, VINYL_CLOSEUP); break;
    case SBX_APP_VINYL_RIDGES: launch_vinyl(build_vinyl(*uni, 60), M, rgba, s, sdf_variant, VINYL_RIDGES); break;
    case SBX_APP_VINYL_NOSHADOW: launch_vinyl(build_vinyl(*uni, 60), M, rgba, s, sdf_variant, VINYL_NOSHADOW); break;
    // the shipped build over the caller's deck (include/sbx.h): k_vinyl's pixel with illuminate's literals as data (k_vinyl_deck) over
    // another frame block.  u_time is not read, so its tameness does not enter: the deck's does (sbx_frames.hip vinyl_deck_tame)
    case SBX_APP_VINYL_DECK: {
        const FrameVinyl F = build_vinyl_deck(*uni, VD, 60);
        const bool tame = vinyl_deck_tame(VD, F);
        ctx->stats.vinyl_deck_launches.fetch_add(1, std::memory_order_relaxed);
        if (!tame) ctx->stats.vinyl_deck_untame.fetch_add(1, std::memory_order_relaxed);
        launch_vinyl_deck(F, vinyl_shade_of(VD), M, rgba, s, witness_variant(ctx, tame));
        break;
    }
    case SBX_APP_CLOUDS_BEST: launch_clouds_best(build_clouds_best(*uni), M, rgba, s); break;
    case SBX_APP_CLOUDS_UE4: launch_clouds_ue4(build_clouds_ue4(*uni, aux_clouds_ue4(aux)), M, rgba, s); break;
    case SBX_APP_2D: (void)launch_2d(build_2d(*uni), M, rgba, s, false); break;   // (three-channel maps were refused above)
    case SBX_APP_2D_TEX: {
        Frame2d F = build_2d(*uni);
        F.tex = ctx->tex2d.bound ? ctx->tex2d.user : ctx->tex2d.def;
        F.tw = ctx->tex2d.bound ? ctx->tex2d.w : TEX2D_DEFAULT;
        F.th = ctx->tex2d.bound ? ctx->tex2d.h : TEX2D_DEFAULT;
        F.ftw = (float)F.tw; F.fth = (float)F.th;
        F.rtw = recip64(F.ftw); F.rth = recip64(F.fth);
        (void)launch_2d(F, M, rgba, s, true);
        break;
    }
    case SBX_APP_FUNC: launch_func(FrameFunc{uni->u_res[0], uni->u_res[1], ctx->func_tab}, M, rgba, s, ctx->variant); break;
    default: break;                                                      // (unreachable: app_valid above, and kApps has a row per app)
    }
    if (tp) { (void)hipEventRecord(tp->ev1, s); tp->complete = true; }
    if (ordered) tile_order_end(ctx->tile_orders, ordered, s);           // (a table due for its refresh is rebuilt behind the launch)
    if (rc != SBX_OK) return rc;
    return launched(ctx, "kernel launch");
}

int sbx::check_common(sbx_ctx* ctx, const sbx_uniforms* uni, const float* rgba, int& W, int& H, unsigned align_mask) {
    if (!ctx) return SBX_ERR_ARG;
    if (!uni || !rgba) return fail(ctx, SBX_ERR_ARG, "NULL uniforms or framebuffer");
    W = (int)uni->u_res[0]; H = (int)uni->u_res[1];
    if (W <= 0 || H <= 0 || (float)W != uni->u_res[0] || (float)H != uni->u_res[1] || W > 65536 || H > 65536)
        return fail(ctx, SBX_ERR_ARG, "u_res must be positive integers <= 65536");
    // float4 pixels are stored with one 16-byte store; 3-channel slabs (RowMap.rgb) with three 4-byte stores: a slab piece that
    // starts at row r0 of an odd-width frame is only 4-byte aligned, and that is fine
    if (ctx->out_format) align_mask = 3u;                     // one 4-byte store per pixel
    if (((uintptr_t)rgba & align_mask) != 0) return fail(ctx, SBX_ERR_ARG, align_mask == 15u ? "framebuffer must be 16-byte aligned" : "slab must be 4-byte aligned");
    return SBX_OK;
}

// what RowMap.rgb says about the output of a frame-granular entry point: the context's format wins (sbx_set_output_format)
int sbx::out_rgb(const sbx_ctx* ctx, int rgb) { return ctx->out_format ? 2 : rgb; }

// what the row-range entry points check first.  `empty`: rows [y0, y0) of a frame — nothing to write, whatever the other arguments
static int check_rows(sbx_ctx* ctx, const sbx_uniforms* uni, const float* rgba, int y0, int y1, unsigned align_mask, int& W, int& H, bool& empty) {
    empty = ctx && uni && y0 == y1 && y0 >= 0 && (float)y0 <= uni->u_res[1];
    if (empty) return SBX_OK;
    const int rc = check_common(ctx, uni, rgba, W, H, align_mask);
    if (rc != SBX_OK) return rc;
    if (y0 < 0 || y1 < y0 || y1 > H) return fail(ctx, SBX_ERR_ARG, "bad row range");
    return SBX_OK;
}
int sbx::render_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int y0, int y1, float* rgba, void* stream,
                     bool float_pixels) {
    int W, H;
    bool empty;
    const int rc = check_rows(ctx, uni, rgba, y0, y1, 15u, W, H, empty);
    if (rc != SBX_OK || empty) return rc;
    RowMap M{W, H, y0, (y1 - y0) > 0 ? (y1 - y0) : 1, 1, 0, y1 - y0, 0, 1, 1, 0, float_pixels ? 0 : out_rgb(ctx, 0)};
    return render_mapped(ctx, app, uni, aux, M, rgba, stream);
}

extern "C" {

int sbx_render_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int y0, int y1, float* rgba,
                    void* stream) {
    return render_rows(ctx, app, uni, aux, y0, y1, rgba, stream, false);
}

// Rows [y0, y1) into HOST memory: rendered strip by strip into the context's staging buffer, every strip copied out on the context's
// copy stream while the next ones render (a frame's copy costs about what its kernel does: CLOUDS 4K 2.3 ms of copy at 57 GB/s
// beside 2.4 ms of kernel, profiles/r05_host_boundary.txt).
int sbx_render_rows_host(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int y0, int y1, void* rgba_host,
                         void* stream) {
    int W, H;
    bool empty;
    int rc = check_rows(ctx, uni, reinterpret_cast<float*>(rgba_host), y0, y1, 3u, W, H, empty);   // (a host frame needs no 16-byte alignment)
    if (rc != SBX_OK || empty) return rc;
    if (stream_is_capturing((hipStream_t)stream)) return fail(ctx, SBX_ERR_ARG, "sbx_render_rows_host cannot be captured (it waits for its copies)");
    std::lock_guard<std::mutex> lock(ctx->hs.lock);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const size_t row_bytes = (size_t)W * (ctx->out_format ? 4 : 16);
    const size_t need = row_bytes * (size_t)(y1 - y0);
    if (need > ctx->hs.cap) {
        if (ctx->hs.dev) { (void)hipDeviceSynchronize(); (void)hipFree(ctx->hs.dev); }
        ctx->hs.dev = nullptr; ctx->hs.cap = 0;
        if ((e = hipMalloc((void**)&ctx->hs.dev, need)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc (host-frame staging)", e);
        ctx->hs.cap = need;
    }
    if (!ctx->hs.ready) {
        // all of the streams and events, or none (HostStaging): a set-up that stopped half way must not leave the next call a null
        // stream (the old test was `!hs_copy`, which is set first)
        release_streams(ctx->hs);
        if ((e = hipStreamCreateWithFlags(&ctx->hs.copy, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipStreamCreateWithFlags(&ctx->hs.render[0], hipStreamNonBlocking)) != hipSuccess ||
            (e = hipStreamCreateWithFlags(&ctx->hs.render[1], hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->hs.entry, hipEventDisableTiming)) != hipSuccess) {
            release_streams(ctx->hs);
            return fail(ctx, SBX_ERR_HIP, "hipStreamCreate", e);
        }
        for (auto& ev : ctx->hs.ev)
            if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) { release_streams(ctx->hs); return fail(ctx, SBX_ERR_HIP, "hipEventCreate", e); }
        ctx->hs.ready = true;
    }
    // Pinned (or registered) memory: the copies are asynchronous, so the frame goes out in strips — whole 64-row bands (a multiple of
    // every kernel's tile height), sixteen at most — rendered alternately on two streams of the context (one strip's tail overlaps the
    // next one's ramp; one stream and eight strips: CLOUDS 4K 4.3 ms instead of 3.55, SBX_HOST_STRIPS sets the number for measurements) behind whatever `stream` holds, each copied out as soon as it is there.  Pageable memory: the runtime stages
    // such a copy synchronously, nothing overlaps, and one strip is fastest (CLOUDS 4K 5.3 ms against 6.6 with eight).
    hipPointerAttribute_t at{};
    const bool pinned = hipPointerGetAttributes(&at, rgba_host) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();                                      // (an unregistered pointer is reported as an error: it is the pageable case)
    const int rows = y1 - y0;
    static const int want = [] { const char* v = getenv("SBX_HOST_STRIPS"); const int n = v ? atoi(v) : 16; return n < 1 ? 1 : (n > 16 ? 16 : n); }();
    const int strips = !pinned ? 1 : (rows >= 64 * want ? want : (rows >= 128 ? (rows / 64 < want ? rows / 64 : want) : 1));
    const int per = ((rows + strips - 1) / strips + 63) / 64 * 64;
    if ((e = hipEventRecord(ctx->hs.entry, (hipStream_t)stream)) != hipSuccess ||
        (e = hipStreamWaitEvent(ctx->hs.render[0], ctx->hs.entry, 0)) != hipSuccess ||
        (e = hipStreamWaitEvent(ctx->hs.render[1], ctx->hs.entry, 0)) != hipSuccess)
        return fail(ctx, SBX_ERR_HIP, "sbx_render_rows_host: entry event", e);
    int g = 0;
    for (int a = 0; a < rows; a += per, ++g) {
        const int b = a + per < rows ? a + per : rows;
        char* dev = ctx->hs.dev + (size_t)a * row_bytes;
        hipStream_t rs = ctx->hs.render[g & 1];
        rc = render_rows(ctx, app, uni, aux, y0 + a, y0 + b, reinterpret_cast<float*>(dev), rs, false);
        if (rc != SBX_OK) break;
        if ((e = hipEventRecord(ctx->hs.ev[g], rs)) != hipSuccess ||
            (e = hipStreamWaitEvent(ctx->hs.copy, ctx->hs.ev[g], 0)) != hipSuccess ||
            (e = hipMemcpyAsync(static_cast<char*>(rgba_host) + (size_t)a * row_bytes, dev, (size_t)(b - a) * row_bytes, hipMemcpyDeviceToHost,
                                ctx->hs.copy)) != hipSuccess) {
            rc = fail(ctx, SBX_ERR_HIP, "sbx_render_rows_host: strip copy", e);
            break;
        }
    }
    (void)hipStreamSynchronize(ctx->hs.render[0]);
    (void)hipStreamSynchronize(ctx->hs.render[1]);
    e = hipStreamSynchronize(ctx->hs.copy);                       // the copies wait for their strips: all of it has run
    if (rc == SBX_OK && e != hipSuccess) rc = fail(ctx, SBX_ERR_HIP, "sbx_render_rows_host: copy", e);
    return rc;
}

int sbx_set_output_format(sbx_ctx* ctx, int format) {
    if (!ctx) return SBX_ERR_ARG;
    if (format != SBX_FORMAT_RGBA32F && format != SBX_FORMAT_RGBA8) return fail(ctx, SBX_ERR_ARG, "unknown output format");
    ctx->out_format = format;
    return SBX_OK;
}
int sbx_set_precision(sbx_ctx* ctx, int precision) {
    if (!ctx) return SBX_ERR_ARG;
    if (precision != SBX_PRECISION_EXACT && precision != SBX_PRECISION_1E4) return fail(ctx, SBX_ERR_ARG, "unknown precision tier");
    ctx->precision = precision;
    mi_invalidate(ctx);                    // frames cached by sbx_main_image were rendered in the other tier
    return SBX_OK;
}
int sbx_set_variant(sbx_ctx* ctx, int variant) {
    if (!ctx) return SBX_ERR_ARG;
    if (variant < 0 || variant > 3) return fail(ctx, SBX_ERR_ARG, "unknown kernel variant");
    ctx->variant = variant == 1 ? 1 : 0;
    ctx->sdf_roots = variant >= 2 ? variant : 0;
    return SBX_OK;
}
int sbx_set_timing(sbx_ctx* ctx, int enabled) {
    if (!ctx) return SBX_ERR_ARG;
    ctx->timers.enabled = enabled != 0;
    return SBX_OK;
}
int sbx_last_kernel_ms(sbx_ctx* ctx, float* ms) {
    if (!ctx || !ms) return SBX_ERR_ARG;
    if (ctx->timers.last < 0 || !ctx->timers.pairs[ctx->timers.last].second.complete) return fail(ctx, SBX_ERR_ARG, "no timed launch yet");
    TimingPair& p = ctx->timers.pairs[ctx->timers.last].second;          // the pair of the stream of the last timed launch
    hipError_t e = hipEventSynchronize(p.ev1);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipEventSynchronize", e);
    e = hipEventElapsedTime(ms, p.ev0, p.ev1);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipEventElapsedTime", e);
    return SBX_OK;
}

int sbx_fault_status(sbx_ctx* ctx) {
    if (!ctx) return SBX_ERR_ARG;
    return device_fault(ctx) ? fail(ctx, SBX_ERR_FAULT, fault_text(ctx)) : SBX_OK;
}
int sbx_clear_fault(sbx_ctx* ctx) {
    if (!ctx) return SBX_ERR_ARG;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipDeviceSynchronize", e);   // no launch may still set it
    if (ctx->device >= 0 && ctx->device < 64 && g_fault_word[ctx->device]) *(volatile unsigned*)g_fault_word[ctx->device] = 0u;
    return SBX_OK;
}
int sbx_debug_raise_fault(sbx_ctx* ctx, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_raise_fault(1u, (hipStream_t)stream);
    return launched(ctx, "fault kernel launch");
}

int sbx_debug_tile_order(sbx_ctx* ctx, int app, int* tables_built, int* launches_since, unsigned* table, size_t capacity) {
    if (!ctx || !app_valid(app)) return SBX_ERR_ARG;
    TileOrder& T = tile_order_latest(ctx->tile_orders, app);   // the shape used last
    if (tables_built) *tables_built = T.built;
    if (launches_since) *launches_since = T.age;
    if (!table || T.cur < 0) return 0;
    const size_t n = (size_t)T.key[4] * (size_t)T.key[5];
    if (n > capacity) return fail(ctx, SBX_ERR_ARG, "sbx_debug_tile_order: table larger than the buffer");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(table, T.mem + T.cap * (size_t)(2 + T.cur), n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "sbx_debug_tile_order", e);
    return (int)n;
}

// The sort of the dispatch order on cost words of the caller's: launch_order_build itself (kern_util.hip), over buffers laid out as
// tile_order_begin lays them out (cost | classes | one table | the histograms), for the test that the table is a permutation
// whatever the words hold.  gx, gy within 1 ... 0xffff as there (a table entry is x | y << 16), gx * gy within the sort's int index.
int sbx_debug_order_build(sbx_ctx* ctx, const unsigned* cost_host, int gx, int gy, unsigned* table_host, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!cost_host || !table_host) return fail(ctx, SBX_ERR_ARG, "sbx_debug_order_build: NULL cost words or table");
    if (gx < 1 || gx > 0xffff || gy < 1 || gy > 0xffff || (long long)gx * gy > 0x7fffffffll)
        return fail(ctx, SBX_ERR_ARG, "sbx_debug_order_build: gx, gy must lie in 1 ... 65535 (and gx * gy below 2^31)");
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)gx * (size_t)gy;
    unsigned* mem = nullptr;
    hipError_t e = hipMalloc((void**)&mem, (n * 3 + order_build_scratch_words()) * 4);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "sbx_debug_order_build: hipMalloc", e);
    e = hipMemcpy(mem, cost_host, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_order_build(mem, mem + n, mem + n * 3, mem + n * 2, gx, gy, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(table_host, mem + n * 2, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(mem);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "sbx_debug_order_build", e);
    return SBX_OK;
}

int sbx_debug_clouds_hashtab(sbx_ctx* ctx, int* entries, int* bias, int* tables_built, int* last_launch_used_table) {
    if (!ctx) return SBX_ERR_ARG;
    const HashTables& H = ctx->hashtab;
    if (entries) *entries = H.tabs.empty() ? 0 : H.tabs.back().entries;
    if (bias) *bias = H.tabs.empty() ? 0 : H.tabs.back().bias;
    if (tables_built) *tables_built = (int)H.tabs.size();
    if (last_launch_used_table) *last_launch_used_table = H.last_used;
    return SBX_OK;
}

int sbx_debug_clouds_last_selection(sbx_ctx* ctx, sbx_clouds_selection* out) {
    if (!ctx || !out) return SBX_ERR_ARG;
    *out = ctx->hashtab.last_selection;
    return SBX_OK;
}

// the choice alone (kern_clouds.hip clouds_select) over the frame render_mapped would build: host code only
int sbx_debug_clouds_select(int app, const sbx_uniforms* uni, const void* aux, int variant, int ytab_rows, int table_range, int point_list,
                            sbx_clouds_selection* out) {
    if (!uni || !out) return SBX_ERR_ARG;
    int build = CLOUDS_DEFAULT;
    if (app == SBX_APP_CLOUDS_HEIGHT) build = CLOUDS_HEIGHT;
    else if (app == SBX_APP_CLOUDS_LUMINANCE) build = CLOUDS_LUMINANCE;
    else if (app != SBX_APP_CLOUDS && app != SBX_APP_CLOUDS_SKY) return SBX_ERR_ARG;
    const sbx_aux_clouds AC = aux_clouds(aux);
    if (AC.cld_march_steps < 0 || AC.illum_march_steps < 0) return SBX_ERR_ARG;
    const bool sky = app == SBX_APP_CLOUDS_SKY;
    static const float one_point[2] = {.5f, .5f};
    RowMap M{};                                                        // (the choice reads `frag` alone: a point list or not)
    if (point_list) { M.frag = one_point; M.npoints = 1; }
    *out = clouds_select(build_clouds(*uni, AC, sky), M, variant, build, sky ? 0 : ytab_rows, sky ? 0 : table_range);
    return SBX_OK;
}

int sbx_debug_clouds_select_vt(int app, const sbx_uniforms* uni, const void* aux, int variant, int ytab_rows, int table_range, int point_list,
                               int view_table, sbx_clouds_selection* out) {
    if (!uni || !out) return SBX_ERR_ARG;
    int build = CLOUDS_DEFAULT;
    if (app == SBX_APP_CLOUDS_HEIGHT) build = CLOUDS_HEIGHT;
    else if (app == SBX_APP_CLOUDS_LUMINANCE) build = CLOUDS_LUMINANCE;
    else if (app != SBX_APP_CLOUDS && app != SBX_APP_CLOUDS_SKY) return SBX_ERR_ARG;
    const sbx_aux_clouds AC = aux_clouds(aux);
    if (AC.cld_march_steps < 0 || AC.illum_march_steps < 0) return SBX_ERR_ARG;
    const bool sky = app == SBX_APP_CLOUDS_SKY;
    static const float one_point[2] = {.5f, .5f};
    const int W = (int)uni->u_res[0], H = (int)uni->u_res[1];
    RowMap M{W, H, 0, H > 0 ? H : 1, 1, 0, H, 0, 1, 1, 0, 0};          // render_rows' map of the whole frame
    if (point_list) { M.frag = one_point; M.npoints = 1; }
    *out = clouds_select(build_clouds(*uni, AC, sky), M, variant, build, sky ? 0 : ytab_rows, sky ? 0 : table_range, view_table != 0);
    return SBX_OK;
}

int sbx_debug_clouds_viewtab_key(int app, const sbx_uniforms* uni, const void* aux, unsigned* key, int words) {
    if (!uni || !key || words != ViewTables::KEY_WORDS) return SBX_ERR_ARG;
    if (app != SBX_APP_CLOUDS && app != SBX_APP_CLOUDS_HEIGHT && app != SBX_APP_CLOUDS_LUMINANCE) return SBX_ERR_ARG;
    const sbx_aux_clouds AC = aux_clouds(aux);
    if (AC.cld_march_steps < 0 || AC.illum_march_steps < 0) return SBX_ERR_ARG;
    uint32_t k[ViewTables::KEY_WORDS];
    clouds_viewtab_key(build_clouds(*uni, AC), (int)uni->u_res[0], (int)uni->u_res[1], k);
    std::memcpy(key, k, sizeof(k));
    return SBX_OK;
}

int sbx_debug_clouds_viewtab(sbx_ctx* ctx, size_t* entries, int* tables_built, int* last_launch_used_table, int* last_refusal) {
    if (!ctx) return SBX_ERR_ARG;
    const ViewTables& V = ctx->viewtab;
    if (entries) *entries = V.last_entries;
    if (tables_built) *tables_built = V.built;
    if (last_launch_used_table) *last_launch_used_table = V.last_used;
    if (last_refusal) *last_refusal = V.last_used ? SBX_VIEWTAB_USED : V.last_refusal;
    return SBX_OK;
}

int sbx_debug_set_clouds_viewtab_cap(sbx_ctx* ctx, size_t bytes) {
    if (!ctx) return SBX_ERR_ARG;
    ctx->viewtab.cap_bytes = bytes;
    return SBX_OK;
}

int sbx_debug_clouds_hashtab_read(sbx_ctx* ctx, size_t first, size_t count, float* host) {
    if (!ctx) return SBX_ERR_ARG;
    const HashTables& H = ctx->hashtab;
    if (H.tabs.empty()) return fail(ctx, SBX_ERR_ARG, "sbx_debug_clouds_hashtab_read: no table has been built");
    const HashTables::Tab& t = H.tabs.back();
    if (!host || first > (size_t)t.entries || count > (size_t)t.entries - first) return fail(ctx, SBX_ERR_ARG, "sbx_debug_clouds_hashtab_read: range outside the table");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventSynchronize(t.ready);
    if (e == hipSuccess) e = hipMemcpy(host, t.dev + first, count * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "sbx_debug_clouds_hashtab_read", e);
    return SBX_OK;
}

int sbx_debug_raytracer_scene_launches(sbx_ctx* ctx, uint64_t* launches) {
    if (!ctx || !launches) return SBX_ERR_ARG;
    *launches = ctx->stats.rt_scene_launches.load(std::memory_order_relaxed);
    return SBX_OK;
}

int sbx_debug_planet_world_launches(sbx_ctx* ctx, uint64_t counts[3]) {
    if (!ctx || !counts) return SBX_ERR_ARG;
    counts[0] = ctx->stats.planet_world_literal.load(std::memory_order_relaxed);
    counts[1] = ctx->stats.planet_world_runtime.load(std::memory_order_relaxed);
    counts[2] = ctx->stats.planet_world_plain.load(std::memory_order_relaxed);
    return SBX_OK;
}

int sbx_debug_atmosphere_air_launches(sbx_ctx* ctx, uint64_t counts[3]) {
    if (!ctx || !counts) return SBX_ERR_ARG;
    counts[0] = ctx->stats.atm_air_launches.load(std::memory_order_relaxed);
    counts[1] = ctx->stats.atm_air_literal.load(std::memory_order_relaxed);
    counts[2] = ctx->stats.atm_air_plain.load(std::memory_order_relaxed);
    return SBX_OK;
}

int sbx_debug_vinyl_deck_launches(sbx_ctx* ctx, uint64_t counts[2]) {
    if (!ctx || !counts) return SBX_ERR_ARG;
    counts[0] = ctx->stats.vinyl_deck_launches.load(std::memory_order_relaxed);
    counts[1] = ctx->stats.vinyl_deck_untame.load(std::memory_order_relaxed);
    return SBX_OK;
}

int sbx_debug_egg_pose_launches(sbx_ctx* ctx, uint64_t counts[2]) {
    if (!ctx || !counts) return SBX_ERR_ARG;
    counts[0] = ctx->stats.egg_pose_launches.load(std::memory_order_relaxed);
    counts[1] = ctx->stats.egg_pose_untame.load(std::memory_order_relaxed);
    return SBX_OK;
}

const char* sbx_last_error(sbx_ctx* ctx) {
    if (!ctx) return "no context";
    if (device_fault(ctx) && ctx->err.find(fault_text(ctx)) == std::string::npos) { ctx->err += ctx->err.empty() ? "" : "; "; ctx->err += fault_text(ctx); }
    return ctx->err.c_str();
}
const char* sbx_version(void) { return "libsbx 0.2 (gfx950, ABI 2)"; }
int sbx_abi_version(void) { return SBX_ABI_VERSION; }

}  // extern "C"
