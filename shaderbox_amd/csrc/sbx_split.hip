// shaderbox_amd/csrc/sbx_split.hip — the multi-GPU split of a frame (include/sbx.h): which row-blocks a rank renders
// (sbx_split_*), which part of a block is worth sending (the span model and its tables), and the entry points that render a rank's
// share or assemble the frame from the shares.
#include "sbx_ctx.h"
#include <algorithm>
#include <cstring>

using namespace sbx;

static bool split_ok(int height, int block_rows, int nranks, int root_rounds, int rounds) {
    return height > 0 && block_rows > 0 && nranks > 0 && rounds >= 1 && root_rounds >= 0 && root_rounds <= rounds &&
           (nranks > 1 || root_rounds == rounds);          // a lone rank cannot be relieved
}
// the row-blocks of `rank` in the order they lie in its slab: f(block) for each, until one returns false (then false)
template <class F> static bool for_rank_blocks(int nblocks, int rank, int nranks, int root_rounds, int rounds, F&& f) {
    const int V = split_cycle_blocks(nranks, root_rounds, rounds);
    const int cnt = rank == 0 ? root_rounds : rounds;
    for (int cycle = 0; cycle * V < nblocks; ++cycle)
        for (int round = 0; round < cnt; ++round) {
            const int v = round < root_rounds ? round * nranks + rank
                                              : root_rounds * nranks + (round - root_rounds) * (nranks - 1) + (rank - 1);
            const int b = cycle * V + v;
            if (b < nblocks && !f(b)) return false;
        }
    return true;
}

extern "C" {

int sbx_split_rank_rows(int height, int block_rows, int rank, int nranks, int root_rounds, int rounds) {
    if (!split_ok(height, block_rows, nranks, root_rounds, rounds) || rank < 0 || rank >= nranks) return SBX_ERR_ARG;
    int rows = 0;
    for_rank_blocks((height + block_rows - 1) / block_rows, rank, nranks, root_rounds, rounds, [&](int b) {
        const int y = b * block_rows;
        rows += (y + block_rows <= height) ? block_rows : (height - y);
        return true;
    });
    return rows;
}
int sbx_split_rows_max(int height, int block_rows, int nranks, int root_rounds, int rounds) {
    if (!split_ok(height, block_rows, nranks, root_rounds, rounds)) return SBX_ERR_ARG;
    int mx = 0;                                             // the fullest slab (equal-count gather: every slab is this tall)
    for (int r = 0; r < nranks; ++r) {
        const int rows = sbx_split_rank_rows(height, block_rows, r, nranks, root_rounds, rounds);
        if (rows > mx) mx = rows;
    }
    return ((mx + block_rows - 1) / block_rows) * block_rows;
}
int sbx_rank_rows(int height, int block_rows, int rank, int nranks) {
    return sbx_split_rank_rows(height, block_rows, rank, nranks, 1, 1);
}
int sbx_rank_rows_max(int height, int block_rows, int nranks) {
    return sbx_split_rows_max(height, block_rows, nranks, 1, 1);
}

// ---------------------------------------------------------------------------------------------
// Spans: which part of a row-block is worth sending to another GPU (include/sbx.h "span exchange")
// ---------------------------------------------------------------------------------------------
// Several apps leave mainImage through an early exit for a large part of the frame: APP_CLOUDS below the horizon
// (src/app_clouds.h:212), the ground-camera build of APP_ATMOSPHERE where the primary ray hits the terrain plane
// (src/app_atmosphere.h:211-224: a constant grey), APP_ATMOSPHERE outside the dome (acos of an argument below -1 is a NaN direction, the atmosphere test
// fails, src/app_atmosphere.h:196-207,85-88), APP_PLANET where the view ray misses the atmosphere shell (src/app_planet.h:315-321).
// Such pixels cost a few hundred instructions; shipping them costs 12 bytes each on the one xGMI link between their renderer
// and the frame's owner, which at 7680x4320 is the slower of the two by far.  So the split deals out only the SPAN of each
// row-block that the host expects to be expensive, and the owner renders the rest of every block itself, in place.
// The predicate below is a HINT: it repeats the kernels' own early-exit tests with the same math spec on the host, at tile
// corners only, and widens the result by a tile — whoever renders a pixel runs the full kernel on it, so a wrong hint costs
// balance, never a pixel.
namespace {
constexpr int SPAN_ALIGN = 64;        // spans start and end on multiples of this many pixels (every kernel's workgroup width divides it)

struct SpanProbe {
    int app;
    Camera cam;
    bool model;                       // false: no early-exit model for this app, every block's span is the whole row
};
static SpanProbe span_probe(int app, const sbx_uniforms& U, const void* aux) {
    SpanProbe P;
    P.app = app;
    P.model = true;
    switch (app) {
    case SBX_APP_CLOUDS: case SBX_APP_CLOUDS_TEX: case SBX_APP_CLOUDS_SKY: case SBX_APP_CLOUDS_HEIGHT: case SBX_APP_CLOUDS_LUMINANCE: P.cam = build_clouds(U, aux_clouds(aux)).cam; break;
    case SBX_APP_ATMOSPHERE: P.cam = build_atmosphere(U).cam; break;
    case SBX_APP_ATMOSPHERE_GROUND: P.cam = build_atmosphere_ground(U).cam; break;
    case SBX_APP_PLANET: case SBX_APP_PLANET_CLOUDLESS: case SBX_APP_PLANET_UNLIT: P.cam = build_planet(U).cam; break;
    case SBX_APP_PLANET_CLOSEUP: P.cam = build_planet(U, false, PLANET_CLOSEUP).cam; break;
    default: P.model = false; P.cam = Camera{}; break;
    }
    return P;
}
// may mainImage at fragCoord (fx, fy) get past the app's early exit?
static bool span_heavy(const SpanProbe& P, float fx, float fy) {
    const v2 pc = point_cam(P.cam, fx, fy);
    switch (P.app) {
    case SBX_APP_CLOUDS: case SBX_APP_CLOUDS_TEX: case SBX_APP_CLOUDS_SKY: case SBX_APP_CLOUDS_HEIGHT: case SBX_APP_CLOUDS_LUMINANCE: {
        const v3 dir = primary_dir(P.cam, pc);
        return !(dir.y < 0.05f);                                   // app_clouds.h:212
    }
    case SBX_APP_ATMOSPHERE: {
        // app_atmosphere.h:195-207: acos(1 - z2) is a NaN beyond z2 = 2 and the atmosphere test then fails (:85-88): free pixels.
        // Below the horizon (1 < z2 <= 2) the view ray dives into the planet from 1 m above the ground: under-ground samples are
        // not lit (get_sun_light returns at its first sample, :65-67), and once exp(-height / hM) has overflowed (106 km down)
        // the kernel is finished with the ray (sbx_atmosphere.h "dead rays").  "Heavy" = some view sample is above the ground
        // BEFORE the optical depth overflows: the same march with the host copy of the math spec.
        const float z2 = pc.x * pc.x + pc.y * pc.y;
        if (z2 > 2.0f) return false;
        const float phi = atan2_(pc.y, pc.x), theta = acos_(1.0f - z2);
        const v3 rd = V3(sin_(theta) * cos_(phi), cos_(theta), sin_(theta) * sin_(phi));
        const float Re = 6360e3f, Ra = 6420e3f;
        const v3 ro = V3(0, Re + 1.f, 0);
        const float tca = dot(V3(0, 0, 0) - ro, rd);
        const float d2 = dot(ro, ro) - tca * tca;
        if (!(d2 < Ra * Ra)) return false;
        const float t1 = tca + sqrt_(Ra * Ra - d2);
        const float step = t1 / 16.f;
        float odM = 0.f;
        for (int i = 0; i < 16; ++i) {
            const v3 sp = ro + rd * (((float)i + .5f) * step);
            const float height = length(sp) - Re;
            odM += exp_(-height / 1200.0f) * step;                 // hM: the first of the two optical depths to overflow
            if (odM > 3e38f) return false;                         // (+inf, or within a rounding of it: the ray is finished)
            if (!(height < 0.f)) return true;
        }
        return false;
    }
    case SBX_APP_ATMOSPHERE_GROUND: {
        // k_atmosphere_ground's own plane test (intersect.h:61-77 with dot(P0 - eye, n) = 1): no hit <=> sky <=> the 16 x 8 march.
        // The camera has no roll, so a row-block is under the horizon as a whole or sky over its whole width.
        const v3 dir = primary_dir(P.cam, pc);
        const float denom = dot(V3(0.f, -1.f, 0.f), dir);
        if (denom < 1e-6f) return true;
        const float t = 1.f / denom;
        return t < 0.f || t > 1e8f;
    }
    case SBX_APP_PLANET: case SBX_APP_PLANET_CLOSEUP: case SBX_APP_PLANET_CLOUDLESS: case SBX_APP_PLANET_UNLIT: {   // intersect_sphere(eye, {0, 1 + max_height}), kern_planet.hip
        const v3 ro = P.cam.eye, rd = primary_dir(P.cam, pc);
        const float radius = 1.f + .4f;                            // planet.radius + max_height   app_planet.h:16-20,311-312
        const v3 rc = V3(0, 0, 0) - ro;
        const float tca = dot(rc, rd);
        if (tca < 0.f) return false;
        const float d2 = dot(rc, rc) - tca * tca;
        return !(d2 > radius * radius * 1.01f);
    }
    default: return true;
    }
}
}  // namespace

extern "C" int sbx_span_table(int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks, int root_rounds,
                              int rounds, int32_t* table, int64_t* rank_pixels, int32_t* max_width) {
    if (!uni) return SBX_ERR_ARG;
    const int W = (int)uni->u_res[0], H = (int)uni->u_res[1];
    if (W <= 0 || H <= 0 || (float)W != uni->u_res[0] || (float)H != uni->u_res[1] || W > 65536 || H > 65536) return SBX_ERR_ARG;
    if (!split_ok(H, block_rows, nranks, root_rounds, rounds)) return SBX_ERR_ARG;
    // every app whose pixels fit the exchange's three-channel slabs has a table; one without a cost model (span_probe: APP_FUNC's cost
    // is uniform over the frame, APP_SDF_AO's ramps fill it from every camera angle) gets the whole row as every block's span
    if (!app_valid(app) || kApps[app].own_alpha) return SBX_ERR_UNSUPPORTED;
    const int nblocks = (H + block_rows - 1) / block_rows;
    const int ntiles = (W + SPAN_ALIGN - 1) / SPAN_ALIGN;
    const SpanProbe P = span_probe(app, *uni, aux);
    std::vector<int> x0(nblocks, 0), x1(nblocks, W);
    // The intervals depend on (app, u_res, u_mouse, block_rows) — not on the split — and finding them is the expensive part (tile by
    // tile, nine probes each, a 16-step march per ATMOSPHERE probe: 14 ms for the 8K dome), while a host asks for the same
    // frame's table once per candidate relief and once per rank context: the last few results are kept, process-wide.
    struct Intervals { std::vector<uint32_t> key; std::vector<int> x0, x1; };
    static std::mutex cache_lock;
    static std::vector<Intervals> cache;
    std::vector<uint32_t> key(6, 0u);
    key[0] = (uint32_t)app; key[1] = (uint32_t)block_rows;
    std::memcpy(&key[2], uni->u_res, 8);
    std::memcpy(&key[4], uni->u_mouse, 8);
    bool cached = false;
    if (P.model) {
        std::lock_guard<std::mutex> g(cache_lock);
        for (const Intervals& c : cache)
            if (c.key == key && (int)c.x0.size() == nblocks) { x0 = c.x0; x1 = c.x1; cached = true; break; }
    }
    if (P.model && !cached) {
        // the heavy part of a row-block is taken to be ONE interval of tiles (a disc, a horizon)
        int prev_lo = 1, prev_hi = 0;
        for (int g = 0; g < nblocks; ++g) {
            const int ya = g * block_rows, yb = std::min(H, ya + block_rows) - 1;
            auto tile_heavy = [&](int k) {
                const int xa = k * SPAN_ALIGN, xb = std::min(W, xa + SPAN_ALIGN) - 1;
                const int xs[3] = {xa, (xa + xb) / 2, xb}, ys[3] = {ya, (ya + yb) / 2, yb};
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i)
                        if (span_heavy(P, (float)xs[i] + .5f, (float)ys[j] + .5f)) return true;
                return false;
            };
            // The interval of a disc or a horizon moves by a tile or two from one row-block to the next: start from the previous
            // block's ends and walk outwards while heavy, inwards while not (a few probes per block instead of a scan of the whole
            // row: 1.6 s -> tens of ms for the 8K dome on a slow host); blocks after an EMPTY one scan the row on a coarse grid first
            // (every fourth tile: the table is a hint about cost — a span narrower than that, missed, is rendered by the frame's
            // owner, same pixels).
            int lo, hi;
            if (g > 0 && prev_lo <= prev_hi) {
                lo = prev_lo; hi = prev_hi;
                if (tile_heavy(lo)) { while (lo > 0 && tile_heavy(lo - 1)) --lo; }
                else { while (lo <= hi && !tile_heavy(lo)) ++lo; }
                if (lo <= hi) {
                    if (tile_heavy(hi)) { while (hi < ntiles - 1 && tile_heavy(hi + 1)) ++hi; }
                    else { while (hi > lo && !tile_heavy(hi)) --hi; }
                }
            } else {
                lo = 0; hi = ntiles - 1;
                bool any = g == 0;                                 // (the first block: the full scan)
                for (int k = 0; k < ntiles && !any; k += 4) any = tile_heavy(k);
                if (!any && ntiles > 1) any = tile_heavy(ntiles - 1);
                if (!any) { lo = 1; hi = 0; }
                else {
                    while (lo <= hi && !tile_heavy(lo)) ++lo;
                    while (hi > lo && !tile_heavy(hi)) --hi;
                }
            }
            prev_lo = lo; prev_hi = hi;
            if (lo > hi) { x0[g] = 0; x1[g] = 0; continue; }
            lo = std::max(0, lo - 1); hi = std::min(ntiles - 1, hi + 1);          // one tile of slack either side
            x0[g] = lo * SPAN_ALIGN;
            x1[g] = std::min(W, (hi + 1) * SPAN_ALIGN);
        }
        std::lock_guard<std::mutex> g(cache_lock);
        if (cache.size() >= 8) cache.erase(cache.begin());
        cache.push_back(Intervals{key, x0, x1});
    }
    // owner and slab offset of every block: the ranks' local blocks in slab order (sbx_split_rank_rows' enumeration)
    std::vector<int> owner(nblocks, 0), off(nblocks, 0);
    std::vector<long long> pix(nranks, 0);
    int maxw = 0;
    for (int rank = 0; rank < nranks; ++rank) {
        const bool fits = for_rank_blocks(nblocks, rank, nranks, root_rounds, rounds, [&](int g) {
            const int rows = std::min(H, (g + 1) * block_rows) - g * block_rows;
            owner[g] = rank;
            if (pix[rank] + (long long)rows * W > 0x7fffffffLL) return false;               // offsets are 32-bit pixel counts
            off[g] = (int)pix[rank];
            pix[rank] += (long long)rows * (x1[g] - x0[g]);
            if (rank > 0) maxw = std::max(maxw, x1[g] - x0[g]);
            return true;
        });
        if (!fits) return SBX_ERR_ARG;
    }
    if (table)
        for (int g = 0; g < nblocks; ++g) { table[4 * g] = x0[g]; table[4 * g + 1] = x1[g]; table[4 * g + 2] = off[g]; table[4 * g + 3] = owner[g]; }
    if (rank_pixels) for (int r = 0; r < nranks; ++r) rank_pixels[r] = pix[r];
    if (max_width) *max_width = maxw;
    return nblocks;
}

// the device copy of the span table of (app, uniforms, aux, split): looked up among the context's few slots, else built and
// uploaded.  An upload overwrites the least recently filled slot; launches that may still read that slot are waited for
// (hipDeviceSynchronize: a table changes when the frame's geometry does, not per frame).
static int span_table_device(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks,
                             int root_rounds, int rounds, hipStream_t s, const int4** dev, int* max_w, const std::vector<int>** host) {
    // the table depends on the camera (u_res, u_mouse) and the split, not on u_time or the rest of the aux block
    std::vector<int> key = {app, block_rows, nranks, root_rounds, rounds};
    int bits[4];
    std::memcpy(bits, uni->u_res, 8); std::memcpy(bits + 2, uni->u_mouse, 8);
    key.insert(key.end(), bits, bits + 4);
    for (auto& sl : ctx->spans.slots)
        if (sl.dev && sl.key == key) { *dev = sl.dev; *max_w = sl.max_w; if (host) *host = &sl.table; return SBX_OK; }
    if (stream_is_capturing(s)) return fail(ctx, SBX_ERR_ARG, "the span table of this frame is not on the device yet: render it once outside the stream capture");
    const int H = (int)uni->u_res[1];
    if (!split_ok(H, block_rows, nranks, root_rounds, rounds)) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    const int nblocks = (H + block_rows - 1) / block_rows;
    SpanSlots::Slot& sl = ctx->spans.slots[ctx->spans.next++ % 4];
    sl.key.clear();
    sl.table.assign((size_t)nblocks * 4, 0);
    int mw = 0;
    const int rc = sbx_span_table(app, uni, aux, block_rows, nranks, root_rounds, rounds, sl.table.data(), nullptr, &mw);
    if (rc < 0) return fail(ctx, rc, "bad span table arguments");
    hipError_t e;
    if (sl.dev) (void)hipDeviceSynchronize();                      // earlier launches may still read the slot's old table
    if (sl.cap < (size_t)nblocks) {
        if (sl.dev) (void)hipFree(sl.dev);
        sl.dev = nullptr; sl.cap = 0;
        if ((e = hipMalloc((void**)&sl.dev, (size_t)nblocks * sizeof(int4))) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
        sl.cap = (size_t)nblocks;
    }
    if ((e = hipMemcpy(sl.dev, sl.table.data(), (size_t)nblocks * sizeof(int4), hipMemcpyHostToDevice)) != hipSuccess)
        return fail(ctx, SBX_ERR_HIP, "span table upload", e);
    sl.max_w = mw;
    sl.key = key;
    *dev = sl.dev; *max_w = mw; if (host) *host = &sl.table;
    return SBX_OK;
}

extern "C" int sbx_render_span_peer(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                                    int nranks, int root_rounds, int rounds, int r0, int r1, float* rgb, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, rgb, W, H, 3u);
    if (rc != SBX_OK) return rc;
    if (app_owns_alpha(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: span slabs carry R, G, B only");
    if (rank < 1 || rank >= nranks) return fail(ctx, SBX_ERR_ARG, "span slabs are rendered by ranks 1 .. nranks-1");
    const int rows = sbx_split_rank_rows(H, block_rows, rank, nranks, root_rounds, rounds);
    if (rows < 0) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (r0 < 0 || r1 < r0 || (r0 % block_rows) != 0) return fail(ctx, SBX_ERR_ARG, "bad slab row range (whole blocks)");
    if (r1 > rows) r1 = rows;
    if (r0 >= r1) return SBX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const int4* dev = nullptr; int mw = 0;
    rc = span_table_device(ctx, app, uni, aux, block_rows, nranks, root_rounds, rounds, (hipStream_t)stream, &dev, &mw, nullptr);
    if (rc != SBX_OK) return rc;
    if (mw <= 0) return SBX_OK;                                    // every span of the peers is empty: nothing to render or send
    // `rgb` is the start of the rank's packed slab: the table's offsets are absolute within it
    RowMap M{mw, H, 0, block_rows, nranks, rank, r1 - r0, r0, root_rounds, rounds, 0, out_rgb(ctx, 1), nullptr, 0, dev, 1};
    return render_mapped(ctx, app, uni, aux, M, rgb, stream);
}
extern "C" int sbx_render_span_peer_in_place(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                                             int nranks, int root_rounds, int rounds, int channels, float* frame, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, frame, W, H);
    if (rc != SBX_OK) return rc;
    if (rank < 1 || rank >= nranks) return fail(ctx, SBX_ERR_ARG, "sbx_render_span_peer_in_place is for ranks 1 .. nranks-1");
    if (channels != 3 && channels != 4) return fail(ctx, SBX_ERR_ARG, "channels must be 3 or 4");
    if (app_owns_alpha(app) && channels == 3) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: three channels cannot hold it");
    const int rows = sbx_split_rank_rows(H, block_rows, rank, nranks, root_rounds, rounds);
    if (rows < 0) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (rows == 0) return SBX_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const int4* dev = nullptr; int mw = 0;
    rc = span_table_device(ctx, app, uni, aux, block_rows, nranks, root_rounds, rounds, (hipStream_t)stream, &dev, &mw, nullptr);
    if (rc != SBX_OK) return rc;
    if (mw <= 0) return SBX_OK;                                    // every span of the peers is empty
    RowMap M{W, H, 0, block_rows, nranks, rank, rows, 0, root_rounds, rounds, 1, out_rgb(ctx, channels == 3 ? 3 : 0), nullptr, 0, dev, 3};
    return render_mapped(ctx, app, uni, aux, M, frame, stream);
}
extern "C" int sbx_render_span_root(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks,
                                    int root_rounds, int rounds, float* frame, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, frame, W, H);
    if (rc != SBX_OK) return rc;
    if (!split_ok(H, block_rows, nranks, root_rounds, rounds)) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (app_owns_alpha(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: the span exchange's slabs carry R, G, B only");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const int4* dev = nullptr; int mw = 0;
    rc = span_table_device(ctx, app, uni, aux, block_rows, nranks, root_rounds, rounds, (hipStream_t)stream, &dev, &mw, nullptr);
    if (rc != SBX_OK) return rc;
    // one launch over the whole frame, in place: rank 0's blocks in full, everybody else's outside their spans
    RowMap M{W, H, 0, H, 1, 0, H, 0, 1, 1, 1, out_rgb(ctx, 0), nullptr, 0, dev, 2};
    M.block_rows = block_rows;                                     // (row_to_y of a contiguous map: y = r for any block size)
    return render_mapped(ctx, app, uni, aux, M, frame, stream);
}
extern "C" int sbx_assemble_spans(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int nranks,
                                  int root_rounds, int rounds, const float* peers, int64_t stride_pixels, float* frame, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, frame, W, H);
    if (rc != SBX_OK) return rc;
    if (!split_ok(H, block_rows, nranks, root_rounds, rounds) || stride_pixels < 0) return fail(ctx, SBX_ERR_ARG, "bad assemble arguments");
    if (app_owns_alpha(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: span slabs carry R, G, B only");
    if (nranks == 1) return SBX_OK;
    if (!peers) return fail(ctx, SBX_ERR_ARG, "NULL peers");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipSetDevice", e);
    const int4* dev = nullptr; int mw = 0;
    rc = span_table_device(ctx, app, uni, aux, block_rows, nranks, root_rounds, rounds, (hipStream_t)stream, &dev, &mw, nullptr);
    if (rc != SBX_OK) return rc;
    if (mw <= 0) return SBX_OK;
    launch_assemble_spans(W, H, block_rows, dev, peers, (size_t)stride_pixels, frame, (hipStream_t)stream, ctx->out_format != 0);
    return launched(ctx, "assemble launch");
}

static int render_split(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank, int nranks,
                        int root_rounds, int rounds, int r0, int r1, int rgb, float* rgba, void* stream) {
    int W, H;
    if (ctx && rgb && app_owns_alpha(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: sbx_render_split_rgb carries R, G, B only");
    if (ctx && uni && r0 == r1 && r0 >= 0) return SBX_OK;
    int rc = check_common(ctx, uni, rgba, W, H, rgb ? 3u : 15u);
    if (rc != SBX_OK) return rc;
    const int rows = sbx_split_rank_rows(H, block_rows, rank, nranks, root_rounds, rounds);
    if (rows < 0) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (r0 < 0 || r1 < r0) return fail(ctx, SBX_ERR_ARG, "bad slab row range");
    if (r1 > rows) r1 = rows;                 // the slab is padded to the split's rows_max; the tail has no pixels
    if (r0 >= r1) return SBX_OK;
    RowMap M{W, H, 0, block_rows, nranks, rank, r1 - r0, r0, root_rounds, rounds, 0, out_rgb(ctx, rgb)};
    return render_mapped(ctx, app, uni, aux, M, rgba, stream);
}
int sbx_render_split(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                     int nranks, int root_rounds, int rounds, int r0, int r1, float* rgba, void* stream) {
    return render_split(ctx, app, uni, aux, block_rows, rank, nranks, root_rounds, rounds, r0, r1, 0, rgba, stream);
}
int sbx_render_split_rgb(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                         int nranks, int root_rounds, int rounds, int r0, int r1, float* rgb, void* stream) {
    return render_split(ctx, app, uni, aux, block_rows, rank, nranks, root_rounds, rounds, r0, r1, 1, rgb, stream);
}
int sbx_render_split_in_place(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                              int nranks, int root_rounds, int rounds, float* frame, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, frame, W, H);
    if (rc != SBX_OK) return rc;
    const int rows = sbx_split_rank_rows(H, block_rows, rank, nranks, root_rounds, rounds);
    if (rows < 0) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (rows == 0) return SBX_OK;
    RowMap M{W, H, 0, block_rows, nranks, rank, rows, 0, root_rounds, rounds, 1, out_rgb(ctx, 0)};
    return render_mapped(ctx, app, uni, aux, M, frame, stream);
}
int sbx_render_split_in_place_rgb(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                                  int nranks, int root_rounds, int rounds, float* frame, void* stream) {
    int W, H;
    int rc = check_common(ctx, uni, frame, W, H);
    if (rc != SBX_OK) return rc;
    if (app_owns_alpha(app)) return fail(ctx, SBX_ERR_UNSUPPORTED, "APP_2D writes its own alpha: sbx_render_split_in_place_rgb writes R, G, B only");
    const int rows = sbx_split_rank_rows(H, block_rows, rank, nranks, root_rounds, rounds);
    if (rows < 0) return fail(ctx, SBX_ERR_ARG, "bad rank split");
    if (rows == 0) return SBX_OK;
    RowMap M{W, H, 0, block_rows, nranks, rank, rows, 0, root_rounds, rounds, 1, out_rgb(ctx, 3)};      // 3: R, G, B of float4 pixels
    return render_mapped(ctx, app, uni, aux, M, frame, stream);
}
int sbx_render_rank(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                    int nranks, float* rgba, void* stream) {
    return sbx_render_split(ctx, app, uni, aux, block_rows, rank, nranks, 1, 1, 0, 0x7fffffff, rgba, stream);
}
int sbx_render_rank_rows(sbx_ctx* ctx, int app, const sbx_uniforms* uni, const void* aux, int block_rows, int rank,
                         int nranks, int r0, int r1, float* rgba, void* stream) {
    return sbx_render_split(ctx, app, uni, aux, block_rows, rank, nranks, 1, 1, r0, r1, rgba, stream);
}

int sbx_assemble_split(sbx_ctx* ctx, int width, int height, int block_rows, int nranks, int root_rounds, int rounds,
                       const float* gathered, float* frame, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!gathered || !frame || width <= 0 || !split_ok(height, block_rows, nranks, root_rounds, rounds))
        return fail(ctx, SBX_ERR_ARG, "bad assemble arguments");
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_assemble(width, height, block_rows, nranks, root_rounds, rounds,
                    sbx_split_rows_max(height, block_rows, nranks, root_rounds, rounds), gathered, frame, (hipStream_t)stream,
                    ctx->out_format != 0);
    return launched(ctx, "assemble launch");
}
int sbx_assemble_peers(sbx_ctx* ctx, int width, int height, int block_rows, int nranks, int root_rounds, int rounds,
                       int channels, const float* peers, float* frame, void* stream) {
    if (!ctx) return SBX_ERR_ARG;
    if (!frame || width <= 0 || !split_ok(height, block_rows, nranks, root_rounds, rounds) || (channels != 3 && channels != 4) ||
        (nranks > 1 && !peers))
        return fail(ctx, SBX_ERR_ARG, "bad assemble arguments");
    if (nranks == 1) return SBX_OK;                           // no peers: the frame is the root's in-place render
    const int rc = use_device(ctx);
    if (rc != SBX_OK) return rc;
    launch_assemble_peers(width, height, block_rows, nranks, root_rounds, rounds,
                          sbx_split_rows_max(height, block_rows, nranks, root_rounds, rounds), ctx->out_format ? 1 : channels, peers, frame,
                          (hipStream_t)stream);
    return launched(ctx, "assemble launch");
}
int sbx_assemble(sbx_ctx* ctx, int width, int height, int block_rows, int nranks, const float* gathered,
                 float* frame, void* stream) {
    return sbx_assemble_split(ctx, width, height, block_rows, nranks, 1, 1, gathered, frame, stream);
}

}  // extern "C"

void sbx::release(SpanSlots& S) {
    for (auto& sl : S.slots) { if (sl.dev) (void)hipFree(sl.dev); sl = SpanSlots::Slot(); }
}
