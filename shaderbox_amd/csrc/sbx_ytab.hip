// shaderbox_amd/csrc/sbx_ytab.hip — APP_CLOUDS' y tables (YTables, sbx_ctx.h): which table a launch of k_clouds reads, when one
// is rebuilt, and who has to wait for whom; its lattice-hash tables (HashTables), which are built once and never rebuilt; and its view
// tables (ViewTables), one per camera.
#include "sbx_ctx.h"
#include <cstdlib>
#include <cstring>

namespace sbx {

// APP_CLOUDS launch with the y-table bookkeeping.  Three cases:
//  (1) no table (per-lane variant, or a step count the table does not cover): nothing cached, nothing touched;
//  (2) the stream is being captured: the build goes into the capture, into a slot of the capture ring, together with
//      the render kernel; cache key, events and the eager ring are left alone (nothing has executed yet);
//  (3) eager: rebuild into the next ring slot only when the key changed — after waiting for every launch that may
//      still be reading that slot — and record, per stream, an event behind each consumer of the current slot.
// build (CLOUDS_*): the three builds share the tables.  The HEIGHT build also reads the steps' luminances, which lie behind the y rows
// and are written only by a rebuild made for it: a table without them counts as stale for that build (`lum`, `big_lum`), a table
// with them serves the other builds unchanged.
// The lattice-hash table of a launch that reads a y table (kern_clouds.hip GTab): the smallest of the context's tables that covers
// the frame's index bound, made ready for stream `s` — or none (tab == nullptr), and the launch takes the LDS hash cache:
//   the launch does not want one (clouds_hashtab_range: CL_GTAB off, a point list, the general light march, a bound beyond the cap
//   or not finite, ...);
//   the stream is being captured and no table the host has seen complete covers the frame: nothing is allocated, built, queried
//   or waited for inside a capture;
//   the allocation or the event failed (the error is dropped: the cache kernels render the same frame).
// A new table is built on `s` in front of the launch.  A table never changes, so its only ordering is "built before read": until the
// host has once seen `ready` complete (hipEventQuery), every launch waits for it on its own stream.
// (the form that takes the wanted range: `need` > 0; largest: the context's largest table whatever its range, a new one of `need` only
//  where it holds none — sbx_clouds_eval, whose lanes test every index against the table's range themselves)
static CloudsHashTab clouds_hash_table_range(sbx_ctx* ctx, int need, bool largest, hipStream_t s, bool capturing) {
    CloudsHashTab none;
    HashTables& H = ctx->hashtab;
    HashTables::Tab* t = nullptr;
    if (largest) { if (!H.tabs.empty()) t = &H.tabs.back(); }
    else for (auto& c : H.tabs) if (c.range >= need) { t = &c; break; }       // ascending: the smallest that covers
    if (t && !t->seen_complete) {
        if (capturing) return none;
        if (hipEventQuery(t->ready) == hipSuccess) t->seen_complete = true;
        else {
            (void)hipGetLastError();                                     // (hipErrorNotReady)
            if (hipStreamWaitEvent(s, t->ready, 0) != hipSuccess) { (void)hipGetLastError(); return none; }
        }
    }
    if (!t) {
        if (capturing) return none;
        HashTables::Tab n;
        n.range = need;
        n.entries = clouds_hashtab_entries(need);
        n.bias = need + CLOUDS_HASHTAB_GUARD;
        if (hipMalloc((void**)&n.dev, (size_t)n.entries * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return none; }
        if (hipEventCreateWithFlags(&n.ready, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(n.dev); return none; }
        launch_clouds_hashtab(n.dev, n.entries, n.bias, s);
        if (hipGetLastError() != hipSuccess || hipEventRecord(n.ready, s) != hipSuccess) {
            // (nothing reads the table: freeing it waits for whatever was enqueued)
            (void)hipGetLastError(); (void)hipEventDestroy(n.ready); (void)hipFree(n.dev);
            return none;
        }
        H.tabs.push_back(n);                                             // (a new table is larger than every older one: still ascending)
        t = &H.tabs.back();
    }
    CloudsHashTab r;
    r.tab = t->dev; r.entries = t->entries; r.bias = t->bias; r.range = t->range;
    return r;
}
static CloudsHashTab clouds_hash_table(sbx_ctx* ctx, const FrameClouds& F, const RowMap& M, hipStream_t s, bool capturing, int build) {
    const int need = clouds_hashtab_range(F, M, build);
    if (need <= 0) return CloudsHashTab();
    return clouds_hash_table_range(ctx, need, false, s, capturing);
}
CloudsHashTab clouds_hash_table_any(sbx_ctx* ctx, hipStream_t s, bool capturing) {
    return clouds_hash_table_range(ctx, CLOUDS_HASHTAB_MIN_RANGE, true, s, capturing);
}

// ---- the view tables (ViewTables, sbx_ctx.h) ----------------------------------------------------------------------------------
void clouds_viewtab_key(const FrameClouds& F, int width, int height, uint32_t* key) {
    const Camera& c = F.cam;
    const float f[22] = {c.res_x, c.res_y, c.aspect_x, c.fov, c.eye.x, c.eye.y, c.eye.z, c.fwd.x, c.fwd.y, c.fwd.z, c.up.x, c.up.y, c.up.z,
                         c.right.x, c.right.y, c.right.z, F.sun_dir.x, F.sun_dir.y, F.sun_dir.z, F.sun_color.x, F.sun_color.y, F.sun_color.z};
    const double d[2] = {c.rres_x, c.rres_y};
    const int wh[2] = {width, height};
    static_assert(sizeof(f) + sizeof(d) + sizeof(wh) == ViewTables::KEY_WORDS * sizeof(uint32_t), "the key is these fields, word for word");
    std::memcpy(key, f, sizeof(f));
    std::memcpy(key + 22, d, sizeof(d));
    std::memcpy(key + 26, wh, sizeof(wh));
}
static bool viewtab_enabled() {
    static const bool on = [] { const char* v = std::getenv("SBX_CLOUDS_VIEWTAB"); return !(v && v[0] == '0' && v[1] == 0); }();
    return on;
}
// has every reader of a draining slot completed?  (events recorded when the slot was chosen; queried, never waited for)
static bool viewtab_drained(ViewTables::Tab& t, std::vector<hipEvent_t>& pool) {
    for (auto& u : t.users) {
        if (hipEventQuery(u.second) != hipSuccess) { (void)hipGetLastError(); return false; }
    }
    for (auto& u : t.users) pool.push_back(u.second);
    t.users.clear();
    t.draining = false;
    return true;
}
// The view table of a launch that takes a hash-table kernel, made ready for stream `s`, or nullptr with the reason in V.last_refusal.
static const float4* clouds_view_table(sbx_ctx* ctx, const FrameClouds& F, const RowMap& M, hipStream_t s, bool capturing, int build) {
    ViewTables& V = ctx->viewtab;
    auto refuse = [&V](int why) -> const float4* { V.last_refusal = why; return nullptr; };
    if (!viewtab_enabled()) return refuse(SBX_VIEWTAB_OFF);
    if (!clouds_viewtab_eligible(F, M, build)) return refuse(SBX_VIEWTAB_INELIGIBLE);
    uint32_t key[ViewTables::KEY_WORDS];
    clouds_viewtab_key(F, M.width, M.height, key);
    int seen_before = 0;                               // eager launches in a row, just before this one, that had this key
    if (!capturing) {
        const bool same = V.streak > 0 && std::memcmp(key, V.last_key, sizeof(key)) == 0;
        seen_before = same ? V.streak : 0;
        V.streak = seen_before + 1;
        std::memcpy(V.last_key, key, sizeof(key));
    }
    ViewTables::Tab* t = nullptr;
    for (auto& c : V.tabs) if (c.valid && std::memcmp(key, c.key, sizeof(key)) == 0) t = &c;
    if (t) {
        if (!t->seen_complete) {
            if (capturing) return refuse(SBX_VIEWTAB_CAPTURE);
            if (hipEventQuery(t->ready) == hipSuccess) t->seen_complete = true;
            else {
                (void)hipGetLastError();                                     // (hipErrorNotReady)
                if (hipStreamWaitEvent(s, t->ready, 0) != hipSuccess) { (void)hipGetLastError(); return refuse(SBX_VIEWTAB_ALLOC); }
            }
        }
        if (capturing) t->pinned = true;               // the graph holds the table's address: the slot keeps its key for good
    } else {
        if (capturing) return refuse(SBX_VIEWTAB_CAPTURE);
        if (seen_before < 2) return refuse(SBX_VIEWTAB_NEW_KEY);
        const size_t pixels = (size_t)M.width * (size_t)M.height;
        if (pixels * CLOUDS_VIEWTAB_PIXEL_BYTES > V.cap_bytes) return refuse(SBX_VIEWTAB_CAP);
        // a free slot; else the least recently used one that no capture holds starts to drain
        for (auto& c : V.tabs) if (!c.valid && !c.draining) { t = &c; break; }
        if (!t) {
            for (auto& c : V.tabs) if (c.draining && viewtab_drained(c, ctx->event_pool)) { t = &c; break; }
        }
        // (while a slot drains no other is chosen: a due key that finds the drain unfinished waits for it, launch after launch, and
        //  never sends the other table after the first)
        bool draining = false;
        for (auto& c : V.tabs) draining = draining || c.draining;
        if (!t && !draining) {
            ViewTables::Tab* lru = nullptr;
            for (auto& c : V.tabs) if (c.valid && !c.pinned && (!lru || c.last_use < lru->last_use)) lru = &c;
            if (lru) {
                bool ok = true;
                for (auto& u : lru->users)
                    ok = ok && !stream_is_capturing(u.first) && hipEventRecord(u.second, u.first) == hipSuccess;
                if (!ok) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); (void)hipGetLastError(); }   // (a stream that is gone: everything has run)
                lru->valid = false;
                if (!ok) { for (auto& u : lru->users) ctx->event_pool.push_back(u.second); lru->users.clear(); t = lru; }
                else { lru->draining = true; if (viewtab_drained(*lru, ctx->event_pool)) t = lru; }
            }
        }
        if (!t) return refuse(SBX_VIEWTAB_NO_SLOT);
        if (t->cap_pixels < pixels) {
            if (t->dev) (void)hipFree(t->dev);
            t->dev = nullptr; t->cap_pixels = 0;
            if (hipMalloc((void**)&t->dev, pixels * CLOUDS_VIEWTAB_PIXEL_BYTES) != hipSuccess) { (void)hipGetLastError(); t->dev = nullptr; return refuse(SBX_VIEWTAB_ALLOC); }
            t->cap_pixels = pixels;
        }
        if (!t->have_ready) {
            if (hipEventCreateWithFlags(&t->ready, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return refuse(SBX_VIEWTAB_ALLOC); }
            t->have_ready = true;
        }
        launch_clouds_viewtab(F, M.width, M.height, t->dev, s);
        if (hipGetLastError() != hipSuccess || hipEventRecord(t->ready, s) != hipSuccess) { (void)hipGetLastError(); return refuse(SBX_VIEWTAB_ALLOC); }
        std::memcpy(t->key, key, sizeof(key));
        t->pixels = pixels;
        t->valid = true; t->seen_complete = false; t->pinned = false;
        V.built += 1;
    }
    if (!capturing) {                                  // this stream reads the slot: remembered, nothing recorded (as the y tables do)
        bool found = false;
        for (auto& u : t->users) if (u.first == s) { found = true; break; }
        if (!found) {
            hipEvent_t ev{};
            if (!ctx->event_pool.empty()) { ev = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
            else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return refuse(SBX_VIEWTAB_ALLOC); }
            t->users.emplace_back(s, ev);
        }
    }
    t->last_use = ++V.clock;
    V.last_entries = t->pixels;
    V.last_refusal = SBX_VIEWTAB_USED;
    return t->dev;
}
// after the launch: what the launcher took is what the hook reports (a table handed to a launch whose selection then takes no VT kernel
// — a build with CL_GTAB off — counts as not eligible)
static void viewtab_launched(ViewTables& V, int vt) {
    V.last_used = vt;
    if (!vt && V.last_refusal == SBX_VIEWTAB_USED) V.last_refusal = SBX_VIEWTAB_INELIGIBLE;
}
// (what every launch of render_clouds does with it: only a launch that was given a hash table asks for a view table)
static const float4* clouds_view_table_for(sbx_ctx* ctx, const CloudsHashTab& ht, const FrameClouds& F, const RowMap& M, hipStream_t s, bool capturing, int build) {
    if (!ht.tab) { ctx->viewtab.last_refusal = viewtab_enabled() ? SBX_VIEWTAB_INELIGIBLE : SBX_VIEWTAB_OFF; return nullptr; }
    return clouds_view_table(ctx, F, M, s, capturing, build);
}

int render_clouds(sbx_ctx* ctx, const FrameClouds& F, const RowMap& M, float* rgba, hipStream_t s, bool capturing, int build) {
    ctx->hashtab.last_used = 0;
    ctx->viewtab.last_used = 0;
    ctx->viewtab.last_refusal = viewtab_enabled() ? SBX_VIEWTAB_INELIGIBLE : SBX_VIEWTAB_OFF;
    sbx_clouds_selection* const rec = &ctx->hashtab.last_selection;       // (sbx_debug_clouds_last_selection; launch_clouds counts)
    const bool need_lum = build == CLOUDS_HEIGHT;
    const bool uses_table = ctx->variant == 0 && F.steps > 0 && F.steps <= CLOUDS_YTAB_ROWS;
    if (!uses_table && ctx->variant == 0 && F.steps > CLOUDS_YTAB_ROWS && F.steps <= CLOUDS_YTAB_BIG_MAX && !capturing) {
        // (4) a march longer than the ring's tables, e.g. the `long` aux set's 4200 steps: the context's one big table, allocated on
        //     demand and so never inside a capture (the table-less kernels, ~2x slower per step, are left with a capture of such
        //     a march and with marches beyond CLOUDS_YTAB_BIG_MAX)
        const float key[3] = {F.cam.eye.y, F.wind_off.y, F.dt};
        hipError_t e;
        if (!ctx->ytab.have_big_ready) {
            if ((e = hipEventCreateWithFlags(&ctx->ytab.big_ready, hipEventDisableTiming)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipEventCreate", e);
            ctx->ytab.have_big_ready = true;
        }
        const bool rebuild = !ctx->ytab.big_valid || ctx->ytab.big_steps != F.steps || std::memcmp(key, ctx->ytab.big_key, sizeof(key)) != 0 ||
                             (need_lum && !ctx->ytab.big_lum);
        if (rebuild) {
            ctx->ytab.big_valid = false;
            if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipDeviceSynchronize", e);   // readers of the old table
            if (F.steps > ctx->ytab.big_rows) {
                if (ctx->ytab.big) (void)hipFree(ctx->ytab.big);
                ctx->ytab.big = nullptr; ctx->ytab.big_rows = 0;
                const int rows = (F.steps + 4095) / 4096 * 4096;
                if ((e = hipMalloc((void**)&ctx->ytab.big, (size_t)rows * CLOUDS_YTAB_STEP_BYTES)) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipMalloc", e);
                ctx->ytab.big_rows = rows;
            }
        } else {
            (void)hipStreamWaitEvent(s, ctx->ytab.big_ready, 0);
        }
        const CloudsHashTab ht = clouds_hash_table(ctx, F, M, s, capturing, build);
        ctx->hashtab.last_used = launch_clouds(F, M, rgba, s, 0, ctx->ytab.big, ctx->ytab.big_rows, rebuild, build, &ht, rec, 2, clouds_view_table_for(ctx, ht, F, M, s, capturing, build)) ? 1 : 0;
        viewtab_launched(ctx->viewtab, rec->vt);
        if (rebuild) {
            (void)hipEventRecord(ctx->ytab.big_ready, s);
            std::memcpy(ctx->ytab.big_key, key, sizeof(key));
            ctx->ytab.big_steps = F.steps;
            ctx->ytab.big_lum = need_lum;
            ctx->ytab.big_valid = true;
        }
        return SBX_OK;
    }
    if (!uses_table) {
        launch_clouds(F, M, rgba, s, ctx->variant, nullptr, 0, false, build, nullptr, rec);
        return SBX_OK;
    }
    if (capturing) {
        char* tab = ctx->ytab.ring + (size_t)(CLOUDS_YTAB_RING + (ctx->ytab.cap_next++ % CLOUDS_YTAB_CAPTURE)) * CLOUDS_YTAB_BYTES;
        const CloudsHashTab ht = clouds_hash_table(ctx, F, M, s, capturing, build);
        ctx->hashtab.last_used = launch_clouds(F, M, rgba, s, 0, tab, CLOUDS_YTAB_ROWS, true, build, &ht, rec, 3, clouds_view_table_for(ctx, ht, F, M, s, capturing, build)) ? 1 : 0;
        viewtab_launched(ctx->viewtab, rec->vt);
        return SBX_OK;
    }
    const float key[3] = {F.cam.eye.y, F.wind_off.y, F.dt};
    const bool rebuild = !ctx->ytab.valid || F.steps != ctx->ytab.steps || std::memcmp(key, ctx->ytab.key, sizeof(key)) != 0 ||
                         (need_lum && !ctx->ytab.lum);
    if (!ctx->ytab.have_ready) {
        if (hipEventCreateWithFlags(&ctx->ytab.ready, hipEventDisableTiming) != hipSuccess)
            return fail(ctx, SBX_ERR_HIP, "hipEventCreate");
        ctx->ytab.have_ready = true;
    }
    int slot = ctx->ytab.slot;
    if (rebuild) {
        slot = (int)(ctx->ytab.next++ % CLOUDS_YTAB_RING);
        YTables::Slot& sl = ctx->ytab.slots[slot];
        // Earlier readers of the slot we are about to overwrite: every stream that launched a reader of it.  The event is recorded
        // NOW, on the reader's stream — behind everything that stream holds, its readers included — and this stream waits for it.
        // (Until round 6 every launch re-recorded its stream's event right after the kernel: a barrier packet per frame, 26 us
        // between two back-to-back 2.4 ms launches of one stream — profiles/r06_streams3_trace.txt — to protect a rebuild that an
        // animation with the default wind never does.)
        for (auto& u : sl.users) {
            if (u.first != s) {
                const bool ok = !stream_is_capturing(u.first) && hipEventRecord(u.second, u.first) == hipSuccess &&
                                hipStreamWaitEvent(s, u.second, 0) == hipSuccess;
                if (!ok) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); (void)hipGetLastError(); }   // (a stream that is gone)
            }
            ctx->event_pool.push_back(u.second);
        }
        sl.users.clear();
    } else if (s != ctx->ytab.stream) {
        (void)hipStreamWaitEvent(s, ctx->ytab.ready, 0);           // table was built on another stream
    }
    char* tab = ctx->ytab.ring + (size_t)slot * CLOUDS_YTAB_BYTES;
    const CloudsHashTab ht = clouds_hash_table(ctx, F, M, s, capturing, build);
    ctx->hashtab.last_used = launch_clouds(F, M, rgba, s, 0, tab, CLOUDS_YTAB_ROWS, rebuild, build, &ht, rec, 1, clouds_view_table_for(ctx, ht, F, M, s, capturing, build)) ? 1 : 0;
    viewtab_launched(ctx->viewtab, rec->vt);
    if (rebuild) {
        (void)hipEventRecord(ctx->ytab.ready, s);                  // the build is enqueued: now the cache state is true
        std::memcpy(ctx->ytab.key, key, sizeof(key));
        ctx->ytab.steps = F.steps;
        ctx->ytab.lum = need_lum;
        ctx->ytab.slot = slot;
        ctx->ytab.stream = s;
        ctx->ytab.valid = true;
    }
    YTables::Slot& sl = ctx->ytab.slots[slot];                               // this stream reads the slot: remembered, nothing recorded
    bool found = false;
    for (auto& u : sl.users) if (u.first == s) { found = true; break; }
    if (!found) {
        hipEvent_t ev{};
        if (!ctx->event_pool.empty()) { ev = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail(ctx, SBX_ERR_HIP, "hipEventCreate");
        sl.users.emplace_back(s, ev);
    }
    return SBX_OK;
}

void release(YTables& Y) {
    if (Y.ring) (void)hipFree(Y.ring);
    if (Y.big) (void)hipFree(Y.big);
    if (Y.have_big_ready) (void)hipEventDestroy(Y.big_ready);
    if (Y.have_ready) (void)hipEventDestroy(Y.ready);
    for (auto& sl : Y.slots) for (auto& u : sl.users) (void)hipEventDestroy(u.second);
    Y = YTables();
}

void release(ViewTables& V, std::vector<hipEvent_t>& pool) {
    for (auto& t : V.tabs) {
        if (t.dev) (void)hipFree(t.dev);
        if (t.have_ready) (void)hipEventDestroy(t.ready);
        for (auto& u : t.users) pool.push_back(u.second);            // (destroyed with the pool, after this: sbx_capi.hip destroy_ctx)
    }
    V = ViewTables();
}

void release(HashTables& H) {
    for (auto& t : H.tabs) {
        if (t.dev) (void)hipFree(t.dev);
        (void)hipEventDestroy(t.ready);
    }
    H = HashTables();
}

}  // namespace sbx
