// shaderbox_amd/csrc/sbx_ctx.h — the context behind the C ABI (struct sbx_ctx) and what the host-side translation units share.
// Host only.  The context's state is grouped by owner: each struct below is kept by ONE file, carries its invariant, and has a
// release function that tolerates a half-built (null) member; sbx_destroy, and a failed sbx_create, is the sequence of them.
//   sbx_capi.hip        create / destroy, render_mapped (the one place a render kernel is launched), rows, setters, the fault word
//   sbx_frames.hip      the per-frame constant blocks of every app (pure host math), the aux defaults
//   sbx_ytab.hip        APP_CLOUDS' y tables and lattice-hash tables
//   sbx_main_image.hip  sbx_main_image over cached frames, the point lists, the stats
//   sbx_split.hip       the multi-GPU split: row arithmetic, the span model and its tables, split / span / assemble entry points
//   sbx_eval.hip        the eval and test hooks, texture and noise-volume binding
#pragma once
#include "../../include/sbx.h"
#include "../../include/sbx_test.h"
#include "sbx_apps.h"
#include "sbx_device.h"
#include "sbx_tile_order.h"
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

struct TimingPair { hipEvent_t ev0{}, ev1{}; bool complete = false; };

#pragma GCC visibility push(hidden)        // the groups of the context's state are internal types: nothing of them is exported

// APP_CLOUDS y tables (sbx_ytab.hip render_clouds).  `ring`: CLOUDS_YTAB_RING slots for eager launches + CLOUDS_YTAB_CAPTURE slots
// that only launches recorded into a stream capture use (a captured graph bakes the slot pointer in, so eager rebuilds must never
// touch it, and the build is always part of the graph).  The eager table depends only on (eye.y, wind.y * t, dt, steps): it is
// rebuilt, into the next ring slot, only when that key changes (default wind has no y component, so an animation reuses one table).
// INVARIANT: valid / key / steps / slot / stream describe a build that has actually been ENQUEUED on a stream that is executing
// (not capturing) — they are committed together, after the launch; the same for the big_* fields.
struct YTables {
    struct Slot {
        // streams that launched readers of this table (they may still be running), each with the event a rebuild of the slot records on it
        std::vector<std::pair<hipStream_t, hipEvent_t>> users;
    };
    char* ring = nullptr;
    unsigned next = 0, cap_next = 0;
    bool valid = false;
    float key[3] = {0, 0, 0};
    int steps = 0;
    bool lum = false;                      // the current table also holds the HEIGHT build's luminances (they depend on steps alone)
    int slot = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ready{};
    bool have_ready = false;
    Slot slots[sbx::CLOUDS_YTAB_RING];
    // march lengths beyond the ring's rows (CLOUDS_YTAB_ROWS): ONE table grown on demand (52 B per step), rebuilt when its key
    // changes after waiting for the device — such frames take tens of milliseconds, the wait is noise
    char* big = nullptr;
    int big_rows = 0;
    bool big_valid = false;
    float big_key[3] = {0, 0, 0};
    int big_steps = 0;
    bool big_lum = false;
    hipEvent_t big_ready{};
    bool have_big_ready = false;
};

// APP_CLOUDS lattice-hash tables (sbx_ytab.hip clouds_hash_table; kern_clouds.hip GTab).  A table is built lazily, on the stream of the
// first eager launch that wants it, and NEVER changes afterwards: a frame whose index bound outgrows the largest one gets a new,
// larger table (ranges are powers of two between CLOUDS_HASHTAB_MIN_RANGE and _MAX_RANGE, so all of them together stay below twice
// the largest); the old ones may still be read by launches in flight and are freed by release().  Of the building stream only the
// `ready` event is kept: a launch waits for it (a no-op on the building stream) until the host has once seen it complete.
// INVARIANT: a Tab in `tabs` has its build kernel ENQUEUED and `ready` recorded behind it; tabs is ascending in range.
struct HashTables {
    struct Tab {
        float* dev = nullptr;
        int range = 0, entries = 0, bias = 0;
        hipEvent_t ready{};
        bool seen_complete = false;
    };
    std::vector<Tab> tabs;
    int last_used = 0;                     // the last APP_CLOUDS launch of the context took a hash-table kernel (sbx_debug_clouds_hashtab)
    sbx_clouds_selection last_selection{}; // what the context's last launch of k_clouds / k_clouds_perlane took, CLOUDS_SKY included
                                           // (sbx_debug_clouds_last_selection; written by the launcher, kern_clouds.hip launch_form)
};

// APP_CLOUDS view tables (sbx_ytab.hip clouds_view_table; kern_clouds.hip "the context's view table"): per camera, the sky colour, the
// phase value and the horizon weight of every pixel of a full frame, 20 bytes per pixel.  Two slots, one key each — the meaningful
// words of the camera, the sun and the frame size (clouds_viewtab_key), never a pad, u_time, the wind or a cloud parameter.
// A table is built in line on the stream of the eager launch that is due, once the two eligible eager launches before it had the same
// key (launches that may read no table — point lists, spans, other suns, the per-lane kernel — neither count nor break the run);
// it never changes while it is valid.  Ordering as the hash tables': one `ready` event, waited for until the host has once seen it
// complete.  A slot is given another key (least recently used first) only after it has DRAINED: when it is chosen, an event is
// recorded on every stream that launched a reader of it, and the slot is free once the host has seen all of them complete — a launch
// that finds no free slot takes the table-less instantiation.  A table that a stream capture took is pinned: a graph holds its address.
// INVARIANT: `valid` means the build kernel is ENQUEUED and `ready` recorded behind it; a slot is either valid, draining or free.
struct ViewTables {
    static constexpr int KEY_WORDS = 28;
    struct Tab {
        float4* dev = nullptr;
        size_t cap_pixels = 0;             // of the allocation
        size_t pixels = 0;                 // width * height of the key
        uint32_t key[KEY_WORDS] = {};
        bool valid = false, draining = false, pinned = false, seen_complete = false;
        hipEvent_t ready{};
        bool have_ready = false;
        uint64_t last_use = 0;
        std::vector<std::pair<hipStream_t, hipEvent_t>> users;   // streams that launched readers, each with the event a drain records on it
    };
    Tab tabs[2];
    uint32_t last_key[KEY_WORDS] = {};     // of the context's last eligible eager launch, and how many in a row had it
    int streak = 0;
    uint64_t clock = 0;
    size_t cap_bytes = SBX_CLOUDS_VIEWTAB_DEFAULT_BYTES;   // sbx_debug_set_clouds_viewtab_cap
    int built = 0;                         // tables built so far
    int last_used = 0, last_refusal = 0;   // of the context's last launch of k_clouds (SBX_VIEWTAB_* of sbx_test.h)
    size_t last_entries = 0;               // pixels of the table built or used last
};

// per-stream timing events (sbx_set_timing): a pair brackets the last launch on its stream
struct Timers {
    bool enabled = false;
    std::vector<std::pair<hipStream_t, TimingPair>> pairs;
    int last = -1;                         // index of the pair of the last timed launch
};

// APP_CLOUDS_TEX: the library's R32F copies of the two bound noise volumes (sbx_eval.hip sbx_set_noise_volumes)
struct NoiseVolumes {
    float* shape = nullptr;                // t1
    float* detail = nullptr;               // t2
    int shape_size = 0, detail_size = 0;
    unsigned* scan = nullptr;              // 6 device words: min / max keys and NaN flag of the two volumes
    float bounds[4] = {0, 0, 0, 0};        // {lo1, hi1, lo2, hi2} of the texels; valid only if bounds_valid
    bool bounds_valid = false;
};

// APP_2D_TEX: t0 as RGBA32F texels (sbx_eval.hip sbx_set_texture2d).  def = hlsltoy's 128x128 checkerboard, built at sbx_create;
// user = the last texture bound (kept, and reused by a rebind of the same size, after a NULL reset)
constexpr int TEX2D_DEFAULT = 128, TEX2D_DEFAULT_FREQ = 16;   // hlsltoy's t0: CreateTextureCheckboard(dev, 128, 128, 16), hlsltoy.cpp:217
struct Texture2d {
    float4* def = nullptr;
    float4* user = nullptr;
    size_t user_cap = 0;                   // texels
    int w = 0, h = 0;                      // of user
    bool bound = false;                    // false: renders read def
};

// sbx_main_image (sbx_main_image.hip): the frames of the last FRAMES distinct (app, uniforms, aux) seen, each in pinned host memory
// behind a sequence lock — host threads that hit read their pixel WITHOUT any lock or shared write (the reference's harness calls
// mainImage from many threads, src/def.h:7-8); only a miss takes `lock` and renders.  `gen` is even while an entry is stable and odd
// while the rendering thread rewrites it; a reader that sees the same even value before and after its reads has read one frame.
// The key words are relaxed atomics because readers look at them while a writer may be storing.
struct FrameCache {
    static constexpr int FRAMES = 2;
    static constexpr int KEY_WORDS = 2 + (int)(sizeof(sbx_uniforms) + sizeof(sbx_aux_sdf_scene)) / 4;   // (the largest aux block)
    static_assert(sizeof(sbx_aux_sdf_scene) >= sizeof(sbx_aux_clouds) && sizeof(sbx_aux_sdf_scene) >= sizeof(sbx_aux_clouds_ue4) &&
                  sizeof(sbx_aux_sdf_scene) >= sizeof(sbx_aux_sdf_ao) && sizeof(sbx_aux_sdf_scene) >= sizeof(sbx_aux_raytracer_scene),
                  "KEY_WORDS holds the largest aux block (mi_make_key copies app_aux_bytes of it)");
    struct Entry {
        std::atomic<uint64_t> gen{0};
        std::atomic<float*> host{nullptr};       // pinned (hipHostMalloc): the frame comes back with one asynchronous copy
        std::atomic<uint32_t> key[KEY_WORDS];
        size_t cap_floats = 0;                   // (writer only, under lock)
        uint64_t born = 0;
        bool used = false;
    };
    Entry frames[FRAMES];
    uint64_t clock = 0;
    std::vector<float*> retired;                 // pinned buffers outgrown by a larger frame: a reader may still be inside one, so
                                                 // they outlive the resize (the oldest goes when eight are waiting; all at destroy)
    // sbx_main_image_batch / off-centre sbx_main_image: pinned staging of a point list (4 + 2 floats per point), read and written by
    // the kernel where it lies
    float* pt_host = nullptr;
    size_t pt_cap = 0;
    std::mutex lock;                             // sbx_main_image / sbx_main_image_batch may be called from several host threads
};

// sbx_get_stats; the hit counter is striped over cache lines (it is bumped once per pixel by every host thread)
struct Stats {
    struct alignas(64) Stripe { std::atomic<uint64_t> n{0}; };
    Stripe hits[16];
    std::atomic<uint64_t> launches{0}, frames{0}, points{0};
    std::atomic<uint64_t> rt_scene_launches{0};   // k_raytracer_scene launches (sbx_debug_raytracer_scene_launches; never reset)
    std::atomic<uint64_t> atm_air_launches{0}, atm_air_literal{0}, atm_air_plain{0};   // SBX_APP_ATMOSPHERE_AIR launches, those of the literal tier, those of the plain kernel (sbx_debug_atmosphere_air_launches; never reset)
    std::atomic<uint64_t> planet_world_literal{0}, planet_world_runtime{0}, planet_world_plain{0};   // SBX_APP_PLANET_WORLD launches by tier; plain counts k_planet<false> and k_planet_world<false> alike (sbx_debug_planet_world_launches; never reset)
    std::atomic<uint64_t> vinyl_deck_launches{0}, vinyl_deck_untame{0};  // SBX_APP_VINYL_DECK launches, and those an untame deck sent to the reference form (sbx_debug_vinyl_deck_launches; never reset)
    std::atomic<uint64_t> egg_pose_launches{0}, egg_pose_untame{0};       // SBX_APP_EGG_POSE launches, and those an untame pose sent to the reference form (sbx_debug_egg_pose_launches; never reset)
};

// sbx_render_rows_host: device staging of a host frame, the stream its strips are copied out on, one event per strip.
// INVARIANT: `ready` means EVERY stream and event below exists — all of them, or none: a set-up that stopped half way must not
// leave the next call a null stream.
struct HostStaging {
    char* dev = nullptr;
    size_t cap = 0;
    hipStream_t copy = nullptr, render[2] = {nullptr, nullptr};
    bool ready = false;
    hipEvent_t entry = nullptr;
    hipEvent_t ev[16] = {};
    std::mutex lock;
};

// span tables of the multi-GPU span exchange (sbx_split.hip span_table_device): a few device copies, filled round robin
struct SpanSlots {
    struct Slot { std::vector<int> key; std::vector<int> table; int4* dev = nullptr; int max_w = 0; size_t cap = 0; };
    Slot slots[4];
    unsigned next = 0;
};

#pragma GCC visibility pop

struct sbx_ctx {
    int device = 0;
    int variant = 0;
    int out_format = 0;                    // sbx_set_output_format: 0 float pixels, 1 R8G8B8A8_UNORM words
    int precision = 0;                     // sbx_set_precision: 0 bit-exact (default), 1 = SBX_PRECISION_1E4 (APP_ATMOSPHERE only)
    int sdf_roots = 0;                     // sbx_set_variant 2 / 3: the SDF kernels' square-root witness test build / IEEE roots
    YTables ytab;
    HashTables hashtab;
    ViewTables viewtab;
    Timers timers;
    NoiseVolumes noise;
    Texture2d tex2d;
    // APP_FUNC: hash_w of every cell its six periods reach (kern_func.hip), built at sbx_create by one synchronous launch — so no
    // host thread ever sees it half built and no stream has to be ordered after it
    float4* func_tab = nullptr;
    FrameCache mi;
    Stats stats;
    HostStaging hs;
    SpanSlots spans;
    sbx::TileOrderSet tile_orders;         // the dispatch order's tables (sbx_tile_order.h)
    std::vector<hipEvent_t> event_pool;    // timing-less events, shared by the y tables and the dispatch order (taken from, returned to)
    std::string err;
};

namespace sbx {

// The variant an SDF or raytracer launch takes (sbx_witness.h witness_dispatch has the table): 1, the reference form, if
// sbx_set_variant chose it or the caller found the frame outside the domain of the kernel's culls (`tame` false: u_time, a pose,
// a deck); else sbx_set_variant's 2 / 3, else 0.  A launch with nothing to judge passes no `tame`.
inline int witness_variant(const sbx_ctx* ctx, bool tame = true) { return ctx->variant == 1 || !tame ? 1 : ctx->sdf_roots; }

// exported since the store exchange (sbx_shared.hip) was a translation unit of its own
unsigned* fault_word_device(int device);   // the device's sticky fault word, as a device pointer (sbx_capi.hip)
int ctx_device(const sbx_ctx* ctx);
int ctx_fail(sbx_ctx* ctx, int code, const char* what, hipError_t e);

#pragma GCC visibility push(hidden)        // what follows is shared by the host-side files and is no part of the library's exports

// ---- sbx_capi.hip
int fail(sbx_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess);   // sets the context's error text, returns `code`
int use_device(sbx_ctx* ctx);                                  // hipSetDevice(ctx->device), or the failure
int launched(sbx_ctx* ctx, const char* what);                  // after a kernel launch: SBX_OK, or hipGetLastError as "<what>: ..."
bool stream_is_capturing(hipStream_t s);
int check_common(sbx_ctx* ctx, const sbx_uniforms* uni, const float* rgba, int& W, int& H, unsigned align_mask = 15u);
int out_rgb(const sbx_ctx* ctx, int rgb);
int render_mapped(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, const RowMap& M, float* rgba, void* stream);
int render_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int y0, int y1, float* rgba, void* stream,
                bool float_pixels);

// ---- sbx_frames.hip: the frame-constant part of setup_camera()/setup_scene()/sdf() per app
FrameClouds build_clouds(const sbx_uniforms& U, const sbx_aux_clouds& A, bool sky_sphere = false);
FrameEggStraight build_egg(const sbx_uniforms& U, int build = EGG_DEFAULT);   // (the other builds read its FrameEgg part)
// SBX_APP_EGG_POSE / sbx_egg_eval: the frame of the caller's pose (build_egg is this over sbx_egg_pose_default's block), and whether
// k_egg's culls and witnessed roots stand for it (false: the reference form, sbx_set_variant 1's kernel)
FrameEggStraight build_egg_pose(const sbx_uniforms& U, const sbx_aux_egg_pose& A, int build = EGG_DEFAULT);
bool egg_pose_tame(const sbx_aux_egg_pose& A, const FrameEgg& F);
FrameRaytracer build_raytracer(const sbx_uniforms& U, int build = RT_DEFAULT);   // build: RT_* (sbx_frame.h); RT_STATIC is the scene at rest
// SBX_APP_RAYTRACER_SCENE / sbx_raytracer_eval: NULL if the block passes the range checks of include/sbx.h, else what is wrong;
// build_raytracer_scene takes a block that passed
const char* raytracer_scene_check(const sbx_aux_raytracer_scene& A);
FrameRtScene build_raytracer_scene(const sbx_uniforms& U, const sbx_aux_raytracer_scene& A);
// SBX_APP_SDF_SCENE / sbx_sdf_eval: NULL if the block passes the checks of include/sbx.h, else what is wrong (program_only: n_instr and
// the program alone, what sbx_sdf_eval reads); build_sdf_scene takes a block that passed
const char* sdf_scene_check(const sbx_aux_sdf_scene& A, bool program_only);
FrameSdfScene build_sdf_scene(const sbx_uniforms& U, const sbx_aux_sdf_scene& A);
FrameAtmosphere build_atmosphere(const sbx_uniforms& U);
FrameAtmosphere build_atmosphere_ground(const sbx_uniforms& U);
// SBX_APP_ATMOSPHERE_AIR / sbx_atmosphere_air_eval (sbx_frames.hip): why a block is refused (nullptr: it is not; `app` false: the
// solver entry, which does not read `view`), the frame of a valid block (the default blocks give build_atmosphere's and
// build_atmosphere_ground's bit for bit), the solver's numbers, and the tier a launch takes (sbx_atmosphere.h "CALLER'S AIR")
enum { ATM_AIR_LITERAL = 0, ATM_AIR_RUNTIME = 1, ATM_AIR_PLAIN = 2 };
const char* atmosphere_air_check(const sbx_aux_atmosphere_air& A, bool app);
FrameAtmosphere build_atmosphere_air(const sbx_uniforms& U, const sbx_aux_atmosphere_air& A);
AtmAir atmosphere_air_numbers(const sbx_aux_atmosphere_air& A);
bool atmosphere_air_tame(const sbx_aux_atmosphere_air& A);
int atmosphere_air_tier(const sbx_aux_atmosphere_air& A, int variant, bool app);   // app false: never ATM_AIR_LITERAL
bool atmosphere_air_literal_fin(const sbx_aux_atmosphere_air& A, const FrameAtmosphere& F);   // the literal tier's fin_ok
FrameSdfAo build_sdf_ao(const sbx_uniforms& U, const sbx_aux_sdf_ao& A);
FrameVinyl build_vinyl(const sbx_uniforms& U, int steps, int build = VINYL_DEFAULT);   // build: VINYL_* (sbx_frame.h); VINYL_CLOSEUP is the other camera
// SBX_APP_VINYL_DECK / sbx_vinyl_eval: the frame of the caller's deck (build_vinyl is this over the default block), the shading data
// of its kernels, and whether k_vinyl's culls and hardware min / max stand for it (false: the reference form, sbx_set_variant 1's kernel)
FrameVinyl build_vinyl_deck(const sbx_uniforms& U, const sbx_aux_vinyl_deck& A, int steps);
VinylShade vinyl_shade_of(const sbx_aux_vinyl_deck& A);
bool vinyl_deck_tame(const sbx_aux_vinyl_deck& A, const FrameVinyl& F);
FramePlanet build_planet(const sbx_uniforms& U, bool atm_sky = false, int build = PLANET_DEFAULT);   // build: PLANET_* (sbx_frame.h); PLANET_CLOSEUP is the other camera
// SBX_APP_PLANET_WORLD (sbx_frames.hip): why a block is refused (nullptr: it is not), the two frame blocks made of it, the tier a launch
// takes, and the host's two domain tests (kern_planet_world.hip says what each is for)
enum { PLANET_WORLD_LITERAL = 0, PLANET_WORLD_RUNTIME = 1, PLANET_WORLD_PLAIN = 2 };
const char* planet_world_check(const sbx_aux_planet_world& W);
FramePlanet build_planet_world_literal(const sbx_uniforms& U, const sbx_aux_planet_world& W);
FramePlanetWorld build_planet_world(const sbx_uniforms& U, const sbx_aux_planet_world& W);
int planet_world_tier(const sbx_aux_planet_world& W, int variant);
bool planet_world_tame(const sbx_aux_planet_world& W);
bool planet_world_camera_tame(const sbx_aux_planet_world& W, const FramePlanet& F);
FrameCloudsBest build_clouds_best(const sbx_uniforms& U);
FrameCloudsUe4 build_clouds_ue4(const sbx_uniforms& U, const sbx_aux_clouds_ue4& A);
Frame2d build_2d(const sbx_uniforms& U);

// ---- sbx_ytab.hip
int render_clouds(sbx_ctx* ctx, const FrameClouds& F, const RowMap& M, float* rgba, hipStream_t s, bool capturing, int build = CLOUDS_DEFAULT);
// the largest lattice-hash table the context holds, or a new one of CLOUDS_HASHTAB_MIN_RANGE, made ready for stream `s` by the rules of
// clouds_hash_table — or none (tab == nullptr): inside a capture with no table the host has seen complete, or where the allocation failed
sbx::CloudsHashTab clouds_hash_table_any(sbx_ctx* ctx, hipStream_t s, bool capturing);
void release(YTables& Y);
void release(HashTables& H);
void release(ViewTables& V, std::vector<hipEvent_t>& pool);
// the key of a launch's view table (ViewTables::KEY_WORDS words): the camera, the sun and the frame size, field by field
void clouds_viewtab_key(const FrameClouds& F, int width, int height, uint32_t* key);

// ---- sbx_main_image.hip
void mi_invalidate(sbx_ctx* ctx);          // forget the cached frames (something they were rendered with changed)
void release(FrameCache& C);

// ---- sbx_split.hip
void release(SpanSlots& S);

// ---- sbx_eval.hip
void release(NoiseVolumes& N);
void release(Texture2d& T);

#pragma GCC visibility pop

}  // namespace sbx
