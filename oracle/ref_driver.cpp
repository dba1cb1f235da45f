/* oracle/ref_driver.cpp — C entry points of one `_ref` build: ONE reference header, compiled verbatim over oracle/glsl_env.h.
 *
 * TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * oracle/Makefile compiles this file once per reference build into oracle/_ref/libsbx_ref_<name>.so (mainImage and the
 * shader's globals have the same names in every app, so each build is a library of its own), with
 *     -DSBX_REF_HEADER='"_ref/src/<header>"'   the header to include: a copy the make rule generates, never committed
 *     -DSBX_REF_RESET='<statement>'            optional: puts back the globals the shader mutates, run before every pixel
 *     -DSBX_REF_NOISE                          the header is the noise library: export sbxr_noise, not mainImage
 * plus whatever defines the reference header itself reads (-DAPP_CLOUDS, -DSKY_SPHERE, -DUSE_TEXTURE, ...).
 *
 * The entry points mirror sbx_oracle.cpp's: sbxr_main_image / sbxr_render_rows take the same uniforms array
 * {u_res.x, u_res.y, u_mouse.x, u_mouse.y, u_time}, fragCoord = (x + .5, y + .5), row 0 = bottom.  GLSL per-invocation
 * semantics: the reference's `_mutable` globals are thread_local in C++ and would carry a pixel's
 * writes into the next one, so SBX_REF_RESET re-initialises the ones a shader writes and reads (`depth` in app_egg.h:188,210,
 * `sun_dir` in app_atmosphere.h:40,180; the others are assigned before use every pixel).
 */
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "glsl_env.h"

namespace glsl {
thread_local vec2 iResolution;
thread_local float iGlobalTime;
thread_local vec4 iMouse;
tex2d_binding g_tex2d = {nullptr, 0, 0};

#include SBX_REF_HEADER

#ifdef SBX_REF_NOISE
static int sbxr_noise_impl(const char* fn, const float* xyz, const float* par, float* out, long n) {
    for (long i = 0; i < n; ++i) {
        vec3 p_(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        vec3 r_(0, 0, 0);
        if (!strcmp(fn, "noise_iq")) r_.x = noise_iq(p_);
        else if (!strcmp(fn, "hash")) r_.x = hash(p_.x);
        else if (!strcmp(fn, "hash_w")) r_ = hash_w(p_);
        else if (!strcmp(fn, "noise_w")) r_ = noise_w(p_, par[0]);
        else if (!strcmp(fn, "fbm_worley_tile")) r_.x = fbm_worley_tile(p_, par[0], par[1], par[2]);
        else return -1;
        out[3 * i] = r_.x; out[3 * i + 1] = r_.y; out[3 * i + 2] = r_.z;
    }
    return 0;
}
#else
static void sbxr_pixel(const float* uniforms, float fx, float fy, float* rgba) {
    iResolution = vec2(uniforms[0], uniforms[1]);
    iMouse = vec4(uniforms[2], uniforms[3], 0, 0);
    iGlobalTime = uniforms[4];
#ifdef SBX_REF_RESET
    SBX_REF_RESET;
#endif
    vec4 c_;
    mainImage(c_, vec2(fx, fy));
    rgba[0] = c_.x; rgba[1] = c_.y; rgba[2] = c_.z; rgba[3] = c_.w;
}
#endif
} /* namespace glsl */

extern "C" {

#ifdef SBX_REF_NOISE
/* same contract as sbxo_noise (sbx_oracle.cpp), plus "hash" (noise_iq.h's scalar hash of xyz[.][0]) */
int sbxr_noise(const char* fn, const float* xyz, const float* par, float* out, long n) {
    return glsl::sbxr_noise_impl(fn, xyz, par, out, n);
}
#else
/* bind the RGBA32F image [height][width][4] (row 0 at v = 0) every sampler2D reads; the pointer is kept, not copied */
int sbxr_set_texture2d(int width, int height, const float* rgba) {
    glsl::g_tex2d.rgba = rgba; glsl::g_tex2d.width = width; glsl::g_tex2d.height = height;
    return 0;
}

int sbxr_main_image(const float* uniforms, float fx, float fy, float* rgba) {
    glsl::sbxr_pixel(uniforms, fx, fy, rgba);
    return 0;
}

/* the listed rows (global indices, 0 = bottom) of the frame into out[nrows][W][4]; tiles of 64 pixels dealt to threads */
int sbxr_render_rows(const float* uniforms, const int* rows, int nrows, float* out, int nthreads) {
    const int W = (int)uniforms[0];
    if (nthreads < 1) nthreads = 1;
    const int TILE = 64;
    const int tiles_x = (W + TILE - 1) / TILE;
    const long ntiles = (long)nrows * tiles_x;
    std::atomic<long> next(0);
    auto work = [&]() {
        for (;;) {
            const long i = next.fetch_add(1);
            if (i >= ntiles) break;
            const int r = (int)(i / tiles_x), x0 = (int)(i % tiles_x) * TILE;
            const int x1 = x0 + TILE < W ? x0 + TILE : W;
            float* dst = out + (size_t)r * W * 4;
            for (int x = x0; x < x1; ++x) glsl::sbxr_pixel(uniforms, (float)x + .5f, (float)rows[r] + .5f, dst + 4 * x);
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < nthreads; ++i) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return 0;
}
#endif

} /* extern "C" */
