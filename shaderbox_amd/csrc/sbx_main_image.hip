// shaderbox_amd/csrc/sbx_main_image.hip — mainImage one fragCoord at a time: sbx_main_image over the frames it caches (FrameCache,
// sbx_ctx.h), the point lists (sbx_render_points, sbx_main_image_batch) and the counters that show which path a host took.
#include "sbx_ctx.h"
#include <cmath>
#include <cstring>

using namespace sbx;

namespace sbx {

void mi_invalidate(sbx_ctx* ctx) {
    std::lock_guard<std::mutex> g(ctx->mi.lock);
    for (auto& en : ctx->mi.frames) {
        const uint64_t g0 = en.gen.load(std::memory_order_relaxed);
        en.gen.store(g0 + 1, std::memory_order_relaxed);
        std::atomic_thread_fence(std::memory_order_release);
        for (auto& w : en.key) w.store(0xffffffffu, std::memory_order_relaxed);
        en.used = false;
        en.gen.store(g0 + 2, std::memory_order_release);
    }
}

void release(FrameCache& C) {
    for (auto& en : C.frames) if (en.host.load()) { (void)hipHostFree(en.host.load()); en.host.store(nullptr); en.cap_floats = 0; }
    for (float* h : C.retired) (void)hipHostFree(h);
    C.retired.clear();
    if (C.pt_host) (void)hipHostFree(C.pt_host);
    C.pt_host = nullptr; C.pt_cap = 0;
}

}  // namespace sbx

extern "C" {

// mainImage at `n` arbitrary fragCoords (device arrays): one launch laid out as a pseudo-frame (RowMap.frag)
static const int POINTS_ROW = 256;         // a multiple of every kernel's workgroup width in pixels
int sbx_render_points(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, size_t n, const float* frag,
                      float* rgba, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!uni) return fail(ctx, SBX_ERR_ARG, "NULL uniforms");
    if (n == 0) return SBX_OK;
    if (!frag || !rgba) return fail(ctx, SBX_ERR_ARG, "NULL point list or output");
    if (n > (size_t)0x7fffffff - POINTS_ROW) return fail(ctx, SBX_ERR_ARG, "too many points");
    // u_res is what fragCoord is divided by (main.h:40) and what the aspect ratio comes from (:33): any positive finite
    // numbers do; only the frame-granular entry points need a whole number of pixels
    if (!(uni->u_res[0] > 0.f) || !(uni->u_res[1] > 0.f) || std::isinf(uni->u_res[0]) || std::isinf(uni->u_res[1]))
        return fail(ctx, SBX_ERR_ARG, "u_res must be positive and finite");
    if (((uintptr_t)rgba & 15u) != 0) return fail(ctx, SBX_ERR_ARG, "output must be 16-byte aligned");
    // the pseudo-frame: 256 columns, wider for very long lists so that the row count stays far below the grid's y limit (65535
    // blocks of as little as 2 rows)
    const int width = POINTS_ROW * (int)((n + (size_t)POINTS_ROW * 100000 - 1) / ((size_t)POINTS_ROW * 100000));
    const int rows = (int)((n + width - 1) / width);
    RowMap M{width, rows, 0, rows, 1, 0, rows, 0, 1, 1, 0, 0, frag, (int)n};
    return render_mapped(ctx, app, uni, aux, M, rgba, stream);
}

static int stage_points(sbx_ctx* ctx, size_t n) {
    if (n <= ctx->mi.pt_cap) return SBX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    if (ctx->mi.pt_host) (void)hipHostFree(ctx->mi.pt_host);
    ctx->mi.pt_host = nullptr; ctx->mi.pt_cap = 0;
    const size_t cap = n < 1024 ? 1024 : n;
    if ((e = hipHostMalloc((void**)&ctx->mi.pt_host, cap * 6 * sizeof(float), hipHostMallocDefault)) != hipSuccess)
        return fail(ctx, SBX_ERR_HIP, "hipHostMalloc", e);
    ctx->mi.pt_cap = cap;
    return SBX_OK;
}
static int main_image_points(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, size_t n, const float* frag,
                             float* colors) {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    int rc = stage_points(ctx, n);
    if (rc != SBX_OK) return rc;
    // The pinned staging buffer is device-accessible at its host address: the kernel reads the coordinates from it and stores the
    // colours into it — one launch, one wait, no transfer before or after (round 5; until then H2D copy + launch + D2H copy).
    // Layout: the n colours (16-byte aligned) first, then the n coordinates.
    float* hcol = ctx->mi.pt_host; float* hfrag = ctx->mi.pt_host + 4 * ctx->mi.pt_cap;
    std::memcpy(hfrag, frag, n * 2 * sizeof(float));
    rc = sbx_render_points(ctx, app, uni, aux, n, hfrag, hcol, nullptr);
    if (rc != SBX_OK) return rc;
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "point list launch", e);
    std::memcpy(colors, hcol, n * 4 * sizeof(float));
    return SBX_OK;
}
int sbx_main_image_batch(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, size_t n, const float* fragCoords,
                         float* fragColors) {
    if (!ctx) return SBX_ERR_ARG;
    std::lock_guard<std::mutex> g(ctx->mi.lock);
    if (!uni) return fail(ctx, SBX_ERR_ARG, "NULL uniforms");
    if (n == 0) return SBX_OK;
    if (!fragCoords || !fragColors) return fail(ctx, SBX_ERR_ARG, "NULL argument");
    return main_image_points(ctx, app, uni, aux, n, fragCoords, fragColors);
}

// ---- sbx_main_image: the per-pixel entry over cached frames ----------------------------------------------------------------
// the cache key of a frame as words: app, aux size, the uniforms, the aux block (zero padded)
// Only the words in use are written — 2 + the uniforms + the block, what mi_lookup compares and what mi_key_words() counts: the hit path
// of an app without a block does not clear the 344 words the largest block would take.
static int mi_key_words(const uint32_t* key) { return 2 + (int)(sizeof(sbx_uniforms) / 4) + (int)(key[1] / 4); }
static void mi_make_key(int app, const sbx_uniforms* uni, const void* aux, uint32_t key[FrameCache::KEY_WORDS]) {
    const int ab = aux ? app_aux_bytes(app) : 0;   // (no block: the defaults, one frame whoever asks)
    key[0] = (uint32_t)app; key[1] = (uint32_t)ab;
    std::memcpy(key + 2, uni, sizeof(*uni));
    if (ab) std::memcpy(key + 2 + sizeof(*uni) / 4, aux, (size_t)ab);
}
// Lock-free lookup: true and the pixel if some entry holds this frame and stayed untouched while it was read.
static bool mi_lookup(sbx_ctx* ctx, const uint32_t* key, size_t pixel, float out[4]) {
    for (auto& en : ctx->mi.frames) {
        const uint64_t g1 = en.gen.load(std::memory_order_acquire);
        if (g1 & 1u) continue;                                                   // being rewritten
        bool same = true;
        // (words 0 and 1 are the app and the aux block's size: keys that agree in them have the same length, and an unused entry's
        // 0xffffffff differs in word 0)
        const int words = mi_key_words(key);
        for (int i = 0; i < words && same; ++i) same = en.key[i].load(std::memory_order_relaxed) == key[i];
        if (!same) continue;
        const float* h = en.host.load(std::memory_order_relaxed);
        if (!h) continue;
        float c[4];
        std::memcpy(c, h + pixel * 4, sizeof(c));
        std::atomic_thread_fence(std::memory_order_acquire);
        if (en.gen.load(std::memory_order_relaxed) != g1) continue;              // rewritten under us: not a hit
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
        return true;
    }
    return false;
}
static unsigned mi_stripe() {
    static std::atomic<unsigned> next{0};
    static thread_local unsigned mine = next.fetch_add(1, std::memory_order_relaxed) & 15u;
    return mine;
}

int sbx_main_image(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, const float fragCoord[2],
                   float fragColor[4]) {
    if (!ctx) return SBX_ERR_ARG;
    if (!uni || !fragCoord || !fragColor) { std::lock_guard<std::mutex> g(ctx->mi.lock); return fail(ctx, SBX_ERR_ARG, "NULL argument"); }
    // Is fragCoord the centre of a pixel of the frame?  Then the pixel comes from the frame cached for (app, uniforms, aux).
    // ANY other coordinate — off-centre (a supersampling host), outside the frame, NaN, or a frame whose u_res is not a whole
    // number of pixels — is evaluated exactly where it is, by a one-point launch: mainImage is a function of fragCoord
    // (src/main.h:40), it never snaps or clamps.
    const float W_f = uni->u_res[0], H_f = uni->u_res[1];
    const int W = (int)W_f, H = (int)H_f;
    const float fx = fragCoord[0], fy = fragCoord[1];
    const bool whole = W > 0 && H > 0 && (float)W == W_f && (float)H == H_f && W <= 65536 && H <= 65536;
    const float cx = std::floor(fx), cy = std::floor(fy);
    const bool centre = whole && fx == cx + .5f && fy == cy + .5f && cx >= 0.f && cy >= 0.f && cx < W_f && cy < H_f;
    if (!centre) {
        std::lock_guard<std::mutex> g(ctx->mi.lock);
        ctx->stats.points.fetch_add(1, std::memory_order_relaxed);
        return main_image_points(ctx, app, uni, aux, 1, fragCoord, fragColor);
    }
    uint32_t key[FrameCache::KEY_WORDS];
    mi_make_key(app, uni, aux, key);
    const size_t pixel = (size_t)(int)cy * (size_t)W + (size_t)(int)cx;
    // the hit path: no lock, no shared write but a striped counter
    if (mi_lookup(ctx, key, pixel, fragColor)) {
        ctx->stats.hits[mi_stripe()].n.fetch_add(1, std::memory_order_relaxed);
        return SBX_OK;
    }
    std::lock_guard<std::mutex> g(ctx->mi.lock);
    if (mi_lookup(ctx, key, pixel, fragColor)) {                                 // another thread rendered it while we waited
        ctx->stats.hits[mi_stripe()].n.fetch_add(1, std::memory_order_relaxed);
        return SBX_OK;
    }
    // miss: render the frame into the entry that was filled longest ago (an unused one first)
    FrameCache::Entry* en = &ctx->mi.frames[0];
    for (auto& c : ctx->mi.frames) if (!c.used || (en->used && c.born < en->born)) { en = &c; if (!c.used) break; }
    const size_t n = (size_t)W * (size_t)H * 4;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const uint64_t g0 = en->gen.load(std::memory_order_relaxed);
    en->gen.store(g0 + 1, std::memory_order_relaxed);                            // odd: readers stay away / discard what they read
    std::atomic_thread_fence(std::memory_order_release);
    for (auto& w : en->key) w.store(0xffffffffu, std::memory_order_relaxed);     // (no frame has app = -1)
    en->used = false;
    if (n > en->cap_floats) {
        float* fresh = nullptr;
        if ((e = hipHostMalloc((void**)&fresh, n * sizeof(float), hipHostMallocDefault)) != hipSuccess) { en->gen.store(g0 + 2, std::memory_order_release); return fail(ctx, SBX_ERR_HIP, "hipHostMalloc", e); }
        if (float* old = en->host.load(std::memory_order_relaxed)) {
            ctx->mi.retired.push_back(old);                                      // a reader may still be copying its pixel out of it
            if (ctx->mi.retired.size() > 8) { (void)hipHostFree(ctx->mi.retired.front()); ctx->mi.retired.erase(ctx->mi.retired.begin()); }
        }
        en->host.store(fresh, std::memory_order_relaxed);
        en->cap_floats = n;
    }
    float* host = en->host.load(std::memory_order_relaxed);
    // The kernel stores STRAIGHT into the pinned frame (hipHostMalloc memory is device-accessible at its host address): one launch,
    // no device copy of the frame, no transfer behind it — the stores cross PCIe while the rest of the frame is computed (CLOUDS 4K
    // 3.6 ms against 5.1 for launch + copy, PLANET 8K 12.2 against 15.8; profiles/r05_host_boundary.txt).  (The cache holds float
    // pixels whatever the context's output format.)
    const int rc = render_rows(ctx, app, uni, aux, 0, H, host, nullptr, true);
    if (rc != SBX_OK) { en->gen.store(g0 + 2, std::memory_order_release); return rc; }
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) {
        en->gen.store(g0 + 2, std::memory_order_release);
        return fail(ctx, SBX_ERR_HIP, "frame render", e);
    }
    ctx->stats.frames.fetch_add(1, std::memory_order_relaxed);
    for (int i = 0, words = mi_key_words(key); i < FrameCache::KEY_WORDS; ++i) en->key[i].store(i < words ? key[i] : 0u, std::memory_order_relaxed);
    en->used = true; en->born = ++ctx->mi.clock;
    en->gen.store(g0 + 2, std::memory_order_release);                            // even again: published
    std::memcpy(fragColor, host + pixel * 4, 4 * sizeof(float));
    return SBX_OK;
}

int sbx_get_stats(sbx_ctx* ctx, sbx_stats* out) {
    if (!ctx || !out) return SBX_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    out->render_launches = ctx->stats.launches.load(std::memory_order_relaxed);
    for (auto& st : ctx->stats.hits) out->main_image_hits += st.n.load(std::memory_order_relaxed);
    out->main_image_frames = ctx->stats.frames.load(std::memory_order_relaxed);
    out->main_image_points = ctx->stats.points.load(std::memory_order_relaxed);
    return SBX_OK;
}
int sbx_reset_stats(sbx_ctx* ctx) {
    if (!ctx) return SBX_ERR_ARG;
    ctx->stats.launches.store(0); ctx->stats.frames.store(0); ctx->stats.points.store(0);
    for (auto& st : ctx->stats.hits) st.n.store(0);
    return SBX_OK;
}

}  // extern "C"
