// shaderbox_amd/csrc/sbx_eval.hip — the hooks that evaluate one piece of the math spec or of a kernel on the device for the tests
// (include/sbx_test.h), the eval entries ("a function of an app over the caller's elements": sbx_atmosphere_eval, sbx_atmosphere_air_eval,
// sbx_sdf_eval, sbx_sdf_scene_eval, sbx_clouds_eval, sbx_planet_eval, sbx_egg_eval, sbx_vinyl_eval, sbx_raytracer_eval of include/sbx.h, all but
// sbx_sdf_eval with a counted twin in
// include/sbx_test.h), and the binding of what the textured apps sample: t0 of APP_2D_TEX, the noise volumes of APP_CLOUDS_TEX.
// The eval entries share one argument check (eval_args), one plain launch and one counted launch; a new one brings its name list, its
// `*_eval_args` with whatever check is its own, and its `*_eval_launch` closure, all in the section below.
#include "sbx_ctx.h"
#include <cstring>

using namespace sbx;

namespace {

// ---- what the eval entries share

// the index of fn among names, or -1 (a NULL fn too)
template <size_t N>
int name_id(const char* fn, const char* const (&names)[N]) {
    for (size_t i = 0; fn && i < N; ++i) if (std::strcmp(fn, names[i]) == 0) return (int)i;
    return -1;
}

// The checks of every eval entry: SBX_OK, or the failure.  `id` is name_id's answer for fn, `unknown` the family's words for a miss,
// `own` the entry's complaint about its own arguments (NULL: none), which holds at n == 0 too; n == 0 is SBX_OK with `in` and `out`
// not looked at, so the caller returns before its launch.
int eval_args(sbx_ctx* ctx, const char* fn, int id, const char* unknown, const char* own, const char* too_many, const void* in, const void* out,
              size_t n) {
    if (!ctx) return SBX_ERR_ARG;
    if (!fn) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    if (id < 0) return fail(ctx, SBX_ERR_ARG, unknown);
    if (own) return fail(ctx, SBX_ERR_ARG, own);
    if (n > ((size_t)1 << 31)) return fail(ctx, SBX_ERR_ARG, too_many);
    if (n == 0) return SBX_OK;
    if (!in || !out) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    return SBX_OK;
}

// the entry itself: one kernel launch and nothing else (capturable).  launch(counters, stream) with no counters.
template <class Launch>
int plain_launch(sbx_ctx* ctx, const char* what, void* stream, Launch launch) {
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch(nullptr, (hipStream_t)stream);
    return launched(ctx, what);
}

// The counted twin: the same launch with K device words of type W zeroed before it and read back into host[0..K) after it.  It
// allocates and waits, so it is not capturable: a capturing stream is refused with the capture intact.
template <class W, int K, class H, class Launch>
int counted_launch(sbx_ctx* ctx, const char* what, size_t n, H* host, void* stream, Launch launch) {
    if (!host) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    for (int k = 0; k < K; ++k) host[k] = 0;
    if (n == 0) return SBX_OK;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return fail(ctx, SBX_ERR_ARG, "the counted launch is not capturable");
    W* counts = nullptr;
    hipError_t e = hipMalloc((void**)&counts, K * sizeof(W));
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
    if ((e = hipMemsetAsync(counts, 0, K * sizeof(W), s)) == hipSuccess) {
        launch(counts, s);
        W h[K] = {};
        if ((e = hipGetLastError()) == hipSuccess && (e = hipMemcpyAsync(h, counts, sizeof(h), hipMemcpyDeviceToHost, s)) == hipSuccess)
            e = hipStreamSynchronize(s);
        for (int k = 0; k < K; ++k) host[k] = h[k];
    }
    (void)hipFree(counts);
    return e == hipSuccess ? SBX_OK : fail(ctx, SBX_ERR_HIP, what, e);
}

// a 1 x 1 frame at u_time: what the build_* of an app need to give the frame constants of a block (its camera is not read by the kernels)
sbx_uniforms frame_1x1(float u_time) { return {{1.f, 1.f}, {0.f, 0.f}, u_time, {0.f, 0.f, 0.f}}; }

// ---- each family: its names, the checks that are its own, its launch

const char* const ATMOSPHERE_FNS[] = {"get_incident_light", "get_sun_light"};

// get_incident_light needs sun_dir, and only where it has rays
int atmosphere_eval_args(sbx_ctx* ctx, const char* fn, const float* rays, const float* sun_dir, const float* out, size_t n, int& id) {
    id = name_id(fn, ATMOSPHERE_FNS);
    const int rc = eval_args(ctx, fn, id, "unknown atmosphere function", nullptr, "more than 2^31 rays", rays, out, n);
    if (rc == SBX_OK && n > 0 && id == 0 && !sun_dir) return fail(ctx, SBX_ERR_ARG, "get_incident_light needs sun_dir");
    return rc;
}
auto atmosphere_eval_launch(const sbx_ctx* ctx, int id, const float* rays, const float* sun_dir, float* out, size_t n) {
    return [=](unsigned* fast_waves, hipStream_t s) { launch_atmosphere_eval(id, ctx->variant == 1, rays, sun_dir, out, n, fast_waves, s); };
}

// the block is required and checked whatever n is
int atmosphere_air_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_atmosphere_air* air, const float* rays, const float* out, size_t n, int& id) {
    id = name_id(fn, ATMOSPHERE_FNS);
    return eval_args(ctx, fn, id, "unknown atmosphere function", !air ? "NULL argument" : atmosphere_air_check(*air, false), "more than 2^31 rays", rays,
                     out, n);
}
// the block is read here, on the host, during the call: the kernel gets its numbers as arguments
auto atmosphere_air_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_atmosphere_air* air, const float* rays, float* out, size_t n) {
    return [=](unsigned* fast_waves, hipStream_t s) {
        const sbx_aux_atmosphere_air& A = *air;
        launch_atmosphere_air_eval(id, atmosphere_air_tier(A, ctx->variant, false) == ATM_AIR_RUNTIME, rays, A.sun_dir, atmosphere_air_numbers(A), out, n,
                                   fast_waves, s);
    };
}

// a NULL aux is the defaults; AC is the block either way.  Negative march steps are refused whatever n is.
int clouds_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_clouds* aux, const float* in, const float* out, size_t n, int& id, sbx_aux_clouds& AC) {
    static const char* const names[] = {"render", "render_clouds", "render_sky_color", "density_func", "illuminate_volume"};
    id = name_id(fn, names);
    AC = aux_clouds(aux);
    const bool negative = AC.cld_march_steps < 0 || AC.illum_march_steps < 0;
    return eval_args(ctx, fn, id, "unknown clouds function", negative ? "negative march steps" : nullptr, "more than 2^31 elements", in, out, n);
}
// The frame constants of the block: build_clouds over u_time alone.  The sky reads no hash; the plain form hashes in place.  No usable
// table (a capture before one was seen complete, which only the entry itself can meet: may_capture; a failed allocation): every cell
// in place, the same bits
auto clouds_eval_launch(sbx_ctx* ctx, int id, const sbx_aux_clouds& AC, float u_time, const float* in, float* out, size_t n, bool may_capture) {
    return [=](unsigned long long* counts, hipStream_t s) {
        const bool plain = ctx->variant == 1;
        CloudsHashTab ht;
        if (!plain && id != 2) ht = clouds_hash_table_any(ctx, s, may_capture && stream_is_capturing(s));
        launch_clouds_eval(id, build_clouds(frame_1x1(u_time), AC, false), plain, &ht, in, out, n, counts, s);
    };
}

int planet_eval_args(sbx_ctx* ctx, const char* fn, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"render", "terrain_march", "sdf_terrain_map", "sdf_terrain_map_detail", "sdf_terrain_normal",
                                        "clouds_density", "illuminate", "background"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown planet function", nullptr, "more than 2^31 elements", in, out, n);
}
// The frame constants: build_planet over u_time alone.  The guarded short forms assume rotations of a finite, bounded angle
// (sbx_capi.hip tame_time, the same bound): beyond it the plain form
auto planet_eval_launch(const sbx_ctx* ctx, int id, float u_time, const float* in, float* out, size_t n) {
    return [=](unsigned* counts, hipStream_t s) {
        const bool plain = ctx->variant == 1 || !(std::fabs(u_time) <= 1e8f);
        launch_planet_eval(id, build_planet(frame_1x1(u_time)), plain, in, out, n, counts, s);
    };
}
// sbx_planet_world_eval: the same names; the block is checked as SBX_APP_PLANET_WORLD checks it and copied here (host memory, read
// during the call).  Its eye, look_at and fov land in a camera no kernel of this entry reads.  plain: sbx_set_variant 1; the host's
// block test travels in the frame block (FramePlanetWorld.tame) and joins the wave-wide tests there (kern_planet_eval.hip PeWorld)
int planet_world_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_planet_world* world, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"render", "terrain_march", "sdf_terrain_map", "sdf_terrain_map_detail", "sdf_terrain_normal",
                                        "clouds_density", "illuminate", "background"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown planet function", !world ? "NULL argument" : planet_world_check(*world), "more than 2^31 elements", in, out, n);
}
auto planet_world_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_planet_world* world, const float* in, float* out, size_t n) {
    const sbx_aux_planet_world W = *world;
    return [=](unsigned* counts, hipStream_t s) {
        launch_planet_world_eval(id, build_planet_world(frame_1x1(0.f), W), ctx->variant == 1, in, out, n, counts, s);
    };
}

// id 0 = "ik_solver", else 1 + launch_egg_eval's fn; every function but ik_solver needs a pose, whatever n is
int egg_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_egg_pose* pose, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"ik_solver", "sdf", "sdf_normal", "shadowmarch", "render_scene"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown egg function", id > 0 && !pose ? "every egg function but ik_solver needs a pose" : nullptr,
                     "more than 2^31 elements", in, out, n);
}
// the frame of the block with the shipped camera in place of the block's; a pose outside the domain of the culls and witnessed roots
// (sbx_frames.hip egg_pose_tame, the camera's fields so ignored) takes the reference form
auto egg_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_egg_pose* pose, const float* in, float* out, size_t n) {
    return [=](unsigned* counts, hipStream_t s) {
        if (id == 0) { launch_ik_eval(in, out, n, s); return; }
        sbx_aux_egg_pose A = *pose;
        A.eye[0] = 0.f; A.eye[1] = .25f; A.eye[2] = 5.25f; A.look_at[0] = 0.f; A.look_at[1] = .25f; A.look_at[2] = 0.f; A.fov = 1.f;
        const FrameEggStraight F = build_egg_pose(frame_1x1(0.f), A, EGG_DEFAULT);
        const int variant = witness_variant(ctx, egg_pose_tame(A, F));
        launch_egg_eval(id - 1, F, variant, in, out, n, counts, s);
    };
}

// id = launch_vinyl_eval's fn; the deck is required whatever n is
int vinyl_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_vinyl_deck* deck, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"sdf", "sdf_normal", "sdf_shadow", "illuminate", "render"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown vinyl function", !deck ? "NULL argument" : nullptr, "more than 2^31 elements", in, out, n);
}
// the frame of the block with the shipped camera in place of the block's (the kernel reads no camera; a deck outside the domain of the
// culls, sbx_frames.hip vinyl_deck_tame with the camera's fields so ignored, takes the reference form)
auto vinyl_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_vinyl_deck* deck, const float* in, float* out, size_t n) {
    return [=](unsigned* counts, hipStream_t s) {
        sbx_aux_vinyl_deck A = *deck;
        A.eye[0] = 0.f; A.eye[1] = 5.75f; A.eye[2] = 6.75f; A.look_at[0] = 0.f; A.look_at[1] = -2.5f; A.look_at[2] = 0.f; A.fov = 1.f;
        const FrameVinyl F = build_vinyl_deck(frame_1x1(0.f), A, 60);
        const int variant = witness_variant(ctx, vinyl_deck_tame(A, F));
        launch_vinyl_eval(id, F, vinyl_shade_of(A), variant, in, out, n, counts, s);
    };
}

// id = launch_raytracer_eval's fn; the scene is required and range-checked (the app's checks, the app's texts) whatever n is
int raytracer_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_raytracer_scene* scene, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"raytrace_iteration", "illuminate", "shadow", "render"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown raytracer function", !scene ? "NULL argument" : raytracer_scene_check(*scene), "more than 2^31 elements", in,
                     out, n);
}
// the frame of the block with the shipped camera in place of the block's (the kernel reads no camera).  No host judgement of the block:
// no shortcut of the kernel has a domain (kern_raytracer_eval.hip, at the top), so the variant is the context's own
auto raytracer_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_raytracer_scene* scene, const float* in, float* out, size_t n) {
    return [=](unsigned* counts, hipStream_t s) {
        sbx_aux_raytracer_scene A = *scene;
        A.eye[0] = 0.f; A.eye[1] = 2.f; A.eye[2] = 4.666f; A.look_at[0] = 0.f; A.look_at[1] = 2.f; A.look_at[2] = 0.f; A.fov = 1.f;
        launch_raytracer_eval(id, build_raytracer_scene(frame_1x1(0.f), A), witness_variant(ctx), in, out, n, counts, s);
    };
}

// id = launch_sdf_scene_eval_fn's fn; the block is required and checked as SBX_APP_SDF_SCENE checks it (the app's texts) whatever n is
int sdf_scene_eval_args(sbx_ctx* ctx, const char* fn, const sbx_aux_sdf_scene* scene, const float* in, const float* out, size_t n, int& id) {
    static const char* const names[] = {"sdf", "sdf_normal", "sdf_ao", "sdf_shadow", "illuminate", "render_impl", "render"};
    id = name_id(fn, names);
    return eval_args(ctx, fn, id, "unknown sdf scene function", !scene ? "NULL argument" : sdf_scene_check(*scene, false), "more than 2^31 elements", in,
                     out, n);
}
// the frame of the block with the ramp block's camera in place of the block's (the kernel reads no camera).  No host judgement of the
// block: no shortcut of the kernel has a domain (kern_sdf_scene_eval.hip, at the top), so the variant is the context's own
auto sdf_scene_eval_launch(const sbx_ctx* ctx, int id, const sbx_aux_sdf_scene* scene, const float* in, float* out, size_t n) {
    return [=](unsigned* counts, hipStream_t s) {
        sbx_aux_sdf_scene A = *scene;
        A.eye[0] = 0.f; A.eye[1] = 3.f; A.eye[2] = 5.f; A.look_at[0] = 0.f; A.look_at[1] = 0.f; A.look_at[2] = 0.f; A.fov = 1.f;
        launch_sdf_scene_eval_fn(id, build_sdf_scene(frame_1x1(0.f), A), witness_variant(ctx), in, out, n, counts, s);
    };
}

}  // namespace

extern "C" {

int sbx_pack_unorm8(sbx_ctx* ctx, int width, int rows, const float* rgba, unsigned char* out, int flip_y, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (width <= 0 || rows < 0 || (rows > 0 && (!rgba || !out))) return fail(ctx, SBX_ERR_ARG, "bad pack arguments");
    if (rows == 0) return SBX_OK;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_pack_unorm8(width, rows, flip_y != 0, rgba, out, (hipStream_t)stream);
    return launched(ctx, "pack launch");
}

int sbx_math_eval(sbx_ctx* ctx, const char* fn, const float* a, const float* b, float* out, size_t n, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!fn || !a || !out) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    static const char* const names[] = {"sin", "cos", "tan", "exp", "pow", "acos", "atan2", "hash", "div", "div_rd", "exp_h13", "pow_h", "sqrt_n", "sqrt_ieee", "exp_reg", "exp_reg_plain", "exp_reg64", "exp_reg64_plain", "exp_small", "exp_small_plain", "exp_reg4k", "sin_b40", "div3", "sqrt_rs", "divn", "srgb_pow", "pow_spec"};
    const int id = name_id(fn, names);
    if (id < 0) return fail(ctx, SBX_ERR_ARG, "unknown math function");
    if ((id == 4 || id == 6 || id == 8 || id == 9 || id == 11 || id == 22 || id == 24 || id == 26) && !b) return fail(ctx, SBX_ERR_ARG, "binary function needs b");
    if (n == 0) return SBX_OK;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    if (id >= 21) { if (launch_math_eval(id, a, b, out, n, (hipStream_t)stream) != 0) return fail(ctx, SBX_ERR_ARG, "math function not in the kernel"); }
    else if (id == 20) launch_exp4k_eval(a, out, n, (hipStream_t)stream);                 // k_atmosphere's 4096-entry form
    else if (id >= 14) launch_cl_exp_eval(a, out, n, (hipStream_t)stream, id - 14);   // exp_reg_ of sbx_math.h (|x| <= 80): k_clouds' / k_atmosphere's form
    else if (launch_math_eval(id, a, b, out, n, (hipStream_t)stream) != 0) return fail(ctx, SBX_ERR_ARG, "math function not in the kernel");
    return launched(ctx, "math_eval launch");
}

int sbx_noise_eval(sbx_ctx* ctx, const char* fn, const float* xyz, const float* params, float* out, size_t n,
                   void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!fn || !xyz || !out) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    static const char* const names[] = {"noise_iq", "hash_w", "noise_w", "fbm_worley_tile", "normalize", "wit_normalize", "wit_record",
                                        "worley_fbm"};
    const int id = name_id(fn, names);
    if (id < 0) return fail(ctx, SBX_ERR_ARG, "unknown noise function");
    const float zero[3] = {0.f, 0.f, 0.f};
    if ((id == 2 || id == 3) && !params) return fail(ctx, SBX_ERR_ARG, "noise_w / fbm_worley_tile need params");
    if (n == 0) return SBX_OK;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_noise_eval(id, xyz, params ? params : zero, out, n, (hipStream_t)stream);
    return launched(ctx, "noise_eval launch");
}

// ---- the eval entries.  Each checks its arguments (`*_eval_args`: eval_args around what is the family's own), states its launch once
// (`*_eval_launch`: a closure over the counter pointer and the stream) and hands that to plain_launch, its counted twin to counted_launch.

int sbx_atmosphere_eval(sbx_ctx* ctx, const char* fn, const float* rays, const float* sun_dir, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = atmosphere_eval_args(ctx, fn, rays, sun_dir, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "atmosphere_eval launch", stream, atmosphere_eval_launch(ctx, id, rays, sun_dir, out, n));
}

int sbx_debug_atmosphere_eval(sbx_ctx* ctx, const char* fn, const float* rays, const float* sun_dir, float* out, size_t n,
                              unsigned* fast_waves_host, void* stream) {
    int id = -1;
    const int rc = atmosphere_eval_args(ctx, fn, rays, sun_dir, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 1>(ctx, "atmosphere_eval (counted)", n, fast_waves_host, stream, atmosphere_eval_launch(ctx, id, rays, sun_dir, out, n));
}

int sbx_atmosphere_air_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_atmosphere_air* air, const float* rays, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = atmosphere_air_eval_args(ctx, fn, air, rays, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "atmosphere_air_eval launch", stream, atmosphere_air_eval_launch(ctx, id, air, rays, out, n));
}

int sbx_debug_atmosphere_air_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_atmosphere_air* air, const float* rays, float* out, size_t n,
                                  unsigned* fast_waves_host, void* stream) {
    int id = -1;
    const int rc = atmosphere_air_eval_args(ctx, fn, air, rays, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 1>(ctx, "atmosphere_air_eval (counted)", n, fast_waves_host, stream, atmosphere_air_eval_launch(ctx, id, air, rays, out, n));
}

int sbx_sdf_eval(sbx_ctx* ctx, const sbx_aux_sdf_scene* scene, const float* xyz, float* out, size_t n, void* stream) {
    // one function, so no name: the scene's complaint stands where a family's own does, before the sizes
    const int rc = eval_args(ctx, "", 0, nullptr, !scene ? "NULL argument" : sdf_scene_check(*scene, true), "more than 2^31 points", xyz, out, n);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "sdf_eval launch", stream, [=](unsigned*, hipStream_t s) {
        // only the program of the block is read: the renderer's settings are taken from the ramp block, whatever the caller's hold
        sbx_aux_sdf_scene A;
        const sbx_uniforms U = frame_1x1(0.f);
        sbx_sdf_scene_ramp(&U, &A);
        A.n_instr = scene->n_instr;
        std::memcpy(A.program, scene->program, sizeof(A.program));
        launch_sdf_scene_eval(build_sdf_scene(U, A), xyz, out, n, s, witness_variant(ctx));
    });
}

int sbx_sdf_scene_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_sdf_scene* scene, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = sdf_scene_eval_args(ctx, fn, scene, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "sdf_scene_eval launch", stream, sdf_scene_eval_launch(ctx, id, scene, in, out, n));
}

int sbx_debug_sdf_scene_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_sdf_scene* scene, const float* in, float* out, size_t n,
                             unsigned counts_host[2], void* stream) {
    int id = -1;
    const int rc = sdf_scene_eval_args(ctx, fn, scene, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "sdf_scene_eval (counted)", n, counts_host, stream, sdf_scene_eval_launch(ctx, id, scene, in, out, n));
}

int sbx_clouds_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_clouds* aux, float u_time, const float* in, float* out, size_t n,
                    void* stream) {
    int id = -1;
    sbx_aux_clouds AC;
    const int rc = clouds_eval_args(ctx, fn, aux, in, out, n, id, AC);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "clouds_eval launch", stream, clouds_eval_launch(ctx, id, AC, u_time, in, out, n, true));
}

int sbx_debug_clouds_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_clouds* aux, float u_time, const float* in, float* out, size_t n,
                          uint64_t counts_host[2], void* stream) {
    int id = -1;
    sbx_aux_clouds AC;
    const int rc = clouds_eval_args(ctx, fn, aux, in, out, n, id, AC);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned long long, 2>(ctx, "clouds_eval (counted)", n, counts_host, stream, clouds_eval_launch(ctx, id, AC, u_time, in, out, n, false));
}

int sbx_planet_eval(sbx_ctx* ctx, const char* fn, float u_time, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = planet_eval_args(ctx, fn, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "planet_eval launch", stream, planet_eval_launch(ctx, id, u_time, in, out, n));
}

int sbx_debug_planet_eval(sbx_ctx* ctx, const char* fn, float u_time, const float* in, float* out, size_t n, unsigned counts_host[2],
                          void* stream) {
    int id = -1;
    const int rc = planet_eval_args(ctx, fn, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "planet_eval (counted)", n, counts_host, stream, planet_eval_launch(ctx, id, u_time, in, out, n));
}

int sbx_planet_world_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_planet_world* world, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = planet_world_eval_args(ctx, fn, world, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "planet_world_eval launch", stream, planet_world_eval_launch(ctx, id, world, in, out, n));
}

int sbx_debug_planet_world_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_planet_world* world, const float* in, float* out, size_t n,
                                unsigned counts_host[2], void* stream) {
    int id = -1;
    const int rc = planet_world_eval_args(ctx, fn, world, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "planet_world_eval (counted)", n, counts_host, stream, planet_world_eval_launch(ctx, id, world, in, out, n));
}

int sbx_egg_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_egg_pose* pose, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = egg_eval_args(ctx, fn, pose, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "egg_eval launch", stream, egg_eval_launch(ctx, id, pose, in, out, n));
}

int sbx_debug_egg_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_egg_pose* pose, const float* in, float* out, size_t n, unsigned counts_host[2],
                       void* stream) {
    int id = -1;
    const int rc = egg_eval_args(ctx, fn, pose, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "egg_eval (counted)", n, counts_host, stream, egg_eval_launch(ctx, id, pose, in, out, n));
}

int sbx_vinyl_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_vinyl_deck* deck, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = vinyl_eval_args(ctx, fn, deck, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "vinyl_eval launch", stream, vinyl_eval_launch(ctx, id, deck, in, out, n));
}

int sbx_debug_vinyl_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_vinyl_deck* deck, const float* in, float* out, size_t n,
                         unsigned counts_host[2], void* stream) {
    int id = -1;
    const int rc = vinyl_eval_args(ctx, fn, deck, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "vinyl_eval (counted)", n, counts_host, stream, vinyl_eval_launch(ctx, id, deck, in, out, n));
}

int sbx_raytracer_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_raytracer_scene* scene, const float* in, float* out, size_t n, void* stream) {
    int id = -1;
    const int rc = raytracer_eval_args(ctx, fn, scene, in, out, n, id);
    if (rc != SBX_OK || n == 0) return rc;
    return plain_launch(ctx, "raytracer_eval launch", stream, raytracer_eval_launch(ctx, id, scene, in, out, n));
}

int sbx_debug_raytracer_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_raytracer_scene* scene, const float* in, float* out, size_t n,
                             unsigned counts_host[2], void* stream) {
    int id = -1;
    const int rc = raytracer_eval_args(ctx, fn, scene, in, out, n, id);
    if (rc != SBX_OK) return rc;
    return counted_launch<unsigned, 2>(ctx, "raytracer_eval (counted)", n, counts_host, stream, raytracer_eval_launch(ctx, id, scene, in, out, n));
}

int sbx_worley_volume(sbx_ctx* ctx, int size, float* rgba, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!rgba || size <= 0 || size > 1024) return fail(ctx, SBX_ERR_ARG, "bad volume arguments");
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_worley_volume(size, rgba, (hipStream_t)stream);
    return launched(ctx, "worley_volume launch");
}

int sbx_set_texture2d(sbx_ctx* ctx, int width, int height, int format, const void* texels, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (!texels) {                                                 // back to hlsltoy's checkerboard (kept on the device since sbx_create)
        ctx->tex2d.bound = false;
        mi_invalidate(ctx);
        return SBX_OK;
    }
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(ctx, SBX_ERR_ARG, "texture sizes run from 1 to 16384");
    if (format != SBX_FORMAT_RGBA8 && format != SBX_FORMAT_RGBA32F) return fail(ctx, SBX_ERR_ARG, "texture format must be SBX_FORMAT_RGBA8 or SBX_FORMAT_RGBA32F");
    if (((uintptr_t)texels & (format == SBX_FORMAT_RGBA8 ? 3u : 15u)) != 0) return fail(ctx, SBX_ERR_ARG, "misaligned texels");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const size_t n = (size_t)width * (size_t)height;
    if (n > ctx->tex2d.user_cap) {
        // (a larger texture frees the old copy, which an in-flight render may read: hipFree synchronises the device first)
        if (ctx->tex2d.user) (void)hipFree(ctx->tex2d.user);
        ctx->tex2d.user = nullptr; ctx->tex2d.user_cap = 0; ctx->tex2d.bound = false;
        if ((e = hipMalloc((void**)&ctx->tex2d.user, n * sizeof(float4))) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc (texture)", e);
        ctx->tex2d.user_cap = n;
    }
    if (format == SBX_FORMAT_RGBA8) launch_unorm8_to_float4(static_cast<const unsigned*>(texels), ctx->tex2d.user, n, s);
    else if ((e = hipMemcpyAsync(ctx->tex2d.user, texels, n * sizeof(float4), hipMemcpyDeviceToDevice, s)) != hipSuccess)
        return fail(ctx, SBX_ERR_HIP, "texture copy", e);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "texture copy launch", e);
    ctx->tex2d.w = width; ctx->tex2d.h = height; ctx->tex2d.bound = true;
    mi_invalidate(ctx);
    // the call returns when the copy is done (the caller's buffer is not referenced afterwards); inside a stream capture it cannot wait
    if (!stream_is_capturing(s) && (e = hipStreamSynchronize(s)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "texture copy", e);
    return SBX_OK;
}

int sbx_set_noise_volumes(sbx_ctx* ctx, int shape_size, const float* shape_rgba, int detail_size, const float* detail_rgba,
                          void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!shape_rgba || !detail_rgba || shape_size <= 0 || detail_size <= 0 || shape_size > 1024 || detail_size > 1024)
        return fail(ctx, SBX_ERR_ARG, "bad noise volume arguments");
    ctx->noise.bounds_valid = false;                                 // whatever happens below, the old volumes' bounds are gone
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const size_t n1 = (size_t)shape_size * shape_size * shape_size, n2 = (size_t)detail_size * detail_size * detail_size;
    // (re)allocation frees buffers an in-flight render may read: hipFree synchronises the device first
    if (shape_size != ctx->noise.shape_size || !ctx->noise.shape) {
        if (ctx->noise.shape) (void)hipFree(ctx->noise.shape);
        ctx->noise.shape = nullptr; ctx->noise.shape_size = 0;
        if ((e = hipMalloc((void**)&ctx->noise.shape, n1 * sizeof(float))) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
        ctx->noise.shape_size = shape_size;
    }
    if (detail_size != ctx->noise.detail_size || !ctx->noise.detail) {
        if (ctx->noise.detail) (void)hipFree(ctx->noise.detail);
        ctx->noise.detail = nullptr; ctx->noise.detail_size = 0;
        if ((e = hipMalloc((void**)&ctx->noise.detail, n2 * sizeof(float))) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
        ctx->noise.detail_size = detail_size;
    }
    mi_invalidate(ctx);                                            // cached sbx_main_image frames may have used the old volumes
    launch_extract_r(shape_rgba, ctx->noise.shape, n1, (hipStream_t)stream);
    launch_extract_r(detail_rgba, ctx->noise.detail, n2, (hipStream_t)stream);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "noise volume copy launch", e);
    // The range of the texel values: k_clouds_tex derives a bound on the density from it and, inside that bound, uses the cheaper
    // exp form that is equal to exp_ there (kern_clouds_tex.hip clouds_tex_density_bound).  The scan is read back here, so the call
    // waits for its own copies; inside a stream capture nothing can be read back and the volumes stay without bounds (exp_ itself).
    ctx->noise.bounds_valid = false;
    if (!stream_is_capturing((hipStream_t)stream)) {
        if (!ctx->noise.scan && (e = hipMalloc((void**)&ctx->noise.scan, 6 * sizeof(unsigned))) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
        launch_minmax_r(ctx->noise.shape, n1, ctx->noise.scan, (hipStream_t)stream);
        launch_minmax_r(ctx->noise.detail, n2, ctx->noise.scan + 3, (hipStream_t)stream);
        unsigned h[6];
        if ((e = hipMemcpyAsync(h, ctx->noise.scan, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream)) != hipSuccess ||
            (e = hipStreamSynchronize((hipStream_t)stream)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "noise volume scan", e);
        if (!h[2] && !h[5] && h[0] <= h[1] && h[3] <= h[4]) {
            ctx->noise.bounds[0] = minmax_key_to_float(h[0]); ctx->noise.bounds[1] = minmax_key_to_float(h[1]);
            ctx->noise.bounds[2] = minmax_key_to_float(h[3]); ctx->noise.bounds[3] = minmax_key_to_float(h[4]);
            ctx->noise.bounds_valid = true;
        }
    }
    return SBX_OK;
}

int sbx_tex3d_eval(sbx_ctx* ctx, int size, const float* rgba, const float* xyz, float* out, size_t n, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!rgba || !xyz || !out || size <= 0 || size > 1024) return fail(ctx, SBX_ERR_ARG, "bad tex3d arguments");
    if (n == 0) return SBX_OK;
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_tex3d_eval(size, rgba, xyz, out, n, (hipStream_t)stream);
    return launched(ctx, "tex3d_eval launch");
}

}  // extern "C"

void sbx::release(NoiseVolumes& N) {
    if (N.shape) (void)hipFree(N.shape);
    if (N.detail) (void)hipFree(N.detail);
    if (N.scan) (void)hipFree(N.scan);
    N = NoiseVolumes();
}
void sbx::release(Texture2d& T) {
    if (T.def) (void)hipFree(T.def);
    if (T.user) (void)hipFree(T.user);
    T = Texture2d();
}
