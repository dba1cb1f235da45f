// include/sbx_mainimage.hpp — C++ drop-in for the reference's C++/VML build of an app.
//
// In the reference, a C++ host includes one app header chosen by a global APP_* define
// (/root/reference/README.md:11-22, src/Makefile:9), gets the globals iResolution / iGlobalTime /
// iMouse (src/uniform_buffer.h:32-36) and the entry point
//     void mainImage(out vec4 fragColor, in vec2 fragCoord)            (src/main.h:6-9)
// and loops over the pixels itself.  This header keeps exactly that surface — same define, same
// globals, same entry point — but evaluates the frame on an MI355X through the C ABI of libsbx:
// the first mainImage() call after the uniforms change renders the WHOLE frame with one HIP kernel
// launch and copies it to the host; every call then returns its pixel from that frame.  So an
// unmodified per-pixel host loop keeps working and costs one GPU frame per frame.
//
// Threads.  The reference's globals are thread_local (src/def.h:7-8) because its harness may call mainImage()
// from many threads at once, each with private scene state.  Here the UNIFORMS are thread_local too, but the
// library context is ONE per process: all host threads that ask for pixels of the same frame share one launch
// and one host copy (sbx_main_image serves hits without a lock, include/sbx.h), instead of one context, one
// launch and one 133 MB frame per thread.  Threads with different uniforms at the same time are served from
// the context's two cached frames; more than two distinct frames in flight re-render on every switch.
//
//   g++ -std=c++17 -DAPP_CLOUDS host.cpp -I include -L shaderbox_amd/lib -lsbx -L /opt/rocm/lib -lamdhip64
//                                                                       (see host/Makefile; no HIP headers needed)
//
// Vector types: anything indexable with operator[] (VML's vector<float,...> is); see host/sbx_render.cpp
// for a complete host.  Errors (no GPU, HIP failure) throw std::runtime_error — there is no CPU path.
#pragma once
#include <stdexcept>
#include <string>

#include "sbx.h"

#if defined(APP_PLANET_ATMOSPHERE)   /* config 5's composite (include/sbx.h): not an APP_* define of the reference */
#define SBX_SELECTED_APP SBX_APP_PLANET_ATMOSPHERE
#elif defined(APP_2D_TEX)   /* src/app_2d.h with USE_TEXTURE, t0 = sbx_set_texture2d's (default: hlsltoy's checkerboard): not an APP_* define of the reference */
#define SBX_SELECTED_APP SBX_APP_2D_TEX
#elif defined(APP_2D)       /* src/app_2d.h, the tunnel / road UV demo (own mainImage :70-111): not an APP_* define of the reference */
#define SBX_SELECTED_APP SBX_APP_2D
#elif defined(APP_FUNC)     /* src/app_func.h's compiled 2D branch, the tiled Worley fBm (own mainImage :63-111): not an APP_* define of the reference */
#define SBX_SELECTED_APP SBX_APP_FUNC
#elif defined(APP_ATMOSPHERE_GROUND)   /* src/app_atmosphere.h built without FROM_SPACE (the ground camera, include/sbx.h); tested before APP_ATMOSPHERE */
#define SBX_SELECTED_APP SBX_APP_ATMOSPHERE_GROUND
#elif defined(APP_SDF_AO_SHADOW)    /* src/app_sdf_ao.h with the `#if 0` at :269 on (the soft-shadow march, include/sbx.h); tested before APP_SDF_AO */
#define SBX_SELECTED_APP SBX_APP_SDF_AO_SHADOW
#elif defined(APP_SDF_AO_NORMALS)   /* src/app_sdf_ao.h with the `#if 0` at :217 on (the normals view, include/sbx.h); tested before APP_SDF_AO */
#define SBX_SELECTED_APP SBX_APP_SDF_AO_NORMALS
#elif defined(APP_EGG_STRAIGHT)     /* src/app_egg.h without its `#define BEZIER` (:37; the cylinder legs, include/sbx.h); tested before APP_EGG */
#define SBX_SELECTED_APP SBX_APP_EGG_STRAIGHT
#elif defined(APP_EGG_OVAL)         /* src/app_egg.h with the `#if 1` at :46 off (the one scaled sphere, include/sbx.h); tested before APP_EGG */
#define SBX_SELECTED_APP SBX_APP_EGG_OVAL
#elif defined(APP_CLOUDS_HEIGHT)    /* src/app_clouds.h with the `#if 0` at :97 on (lit by height, no light march; include/sbx.h); tested before APP_CLOUDS */
#define SBX_SELECTED_APP SBX_APP_CLOUDS_HEIGHT
#elif defined(APP_CLOUDS_LUMINANCE) /* src/app_clouds.h with the `#if 0` at :118 on (the light march's transmittance itself); tested before APP_CLOUDS */
#define SBX_SELECTED_APP SBX_APP_CLOUDS_LUMINANCE
#elif defined(APP_RAYTRACER_PHONG)    /* src/app_raytracer.h with the `#if 0` at :61 on (illum_blinn_phong's Phong specular; include/sbx.h); tested before APP_RAYTRACER */
#define SBX_SELECTED_APP SBX_APP_RAYTRACER_PHONG
#elif defined(APP_RAYTRACER_NOSHADOW) /* src/app_raytracer.h with the `#if 1` at :107 off (no shadow ray); tested before APP_RAYTRACER */
#define SBX_SELECTED_APP SBX_APP_RAYTRACER_NOSHADOW
#elif defined(APP_RAYTRACER_STATIC)   /* src/app_raytracer.h with the `#if 1` at :29 off (the Cornell box at rest); tested before APP_RAYTRACER */
#define SBX_SELECTED_APP SBX_APP_RAYTRACER_STATIC
#elif defined(APP_VINYL_CLOSEUP)  /* src/app_vinyl.h with the `#if 1` of setup_camera at :60 off (the close-up camera of :64-65; include/sbx.h); tested before APP_VINYL */
#define SBX_SELECTED_APP SBX_APP_VINYL_CLOSEUP
#elif defined(APP_VINYL_RIDGES)   /* src/app_vinyl.h with the `#if 0` of illuminate at :357 on (the ridge of label and logo); tested before APP_VINYL */
#define SBX_SELECTED_APP SBX_APP_VINYL_RIDGES
#elif defined(APP_VINYL_NOSHADOW) /* src/app_vinyl.h with the `#if 1` of render at :445 off (no sdf_shadow march); tested before APP_VINYL */
#define SBX_SELECTED_APP SBX_APP_VINYL_NOSHADOW
#elif defined(APP_PLANET_CLOSEUP)   /* src/app_planet.h with the `#if 0` of setup_camera at :51 on (the camera of :52-53; include/sbx.h); tested before APP_PLANET */
#define SBX_SELECTED_APP SBX_APP_PLANET_CLOSEUP
#elif defined(APP_PLANET_CLOUDLESS) /* src/app_planet.h without the `#define CLOUDS` of :63 (no cloud march, no cloud shadow); tested before APP_PLANET */
#define SBX_SELECTED_APP SBX_APP_PLANET_CLOUDLESS
#elif defined(APP_PLANET_UNLIT)     /* src/app_planet.h without the `#define LIGHT` of :249 (N = w_normal.y, ocean = water); tested before APP_PLANET */
#define SBX_SELECTED_APP SBX_APP_PLANET_UNLIT
#elif defined(APP_PLANET)           /* (APP_PLANET_ATMOSPHERE was tested first, above: it is not combined with the three builds) */
#define SBX_SELECTED_APP SBX_APP_PLANET
#elif defined(APP_CLOUDS)
#define SBX_SELECTED_APP SBX_APP_CLOUDS
#elif defined(APP_EGG)
#define SBX_SELECTED_APP SBX_APP_EGG
#elif defined(APP_RAYTRACER)
#define SBX_SELECTED_APP SBX_APP_RAYTRACER
#elif defined(APP_ATMOSPHERE)      /* (SBX_APP_ATMOSPHERE_AIR, the same header over the caller's air, has no define here: this header has no way to state a block; include/sbx.h) */
#define SBX_SELECTED_APP SBX_APP_ATMOSPHERE
#elif defined(APP_SDF_AO)
#define SBX_SELECTED_APP SBX_APP_SDF_AO
#elif defined(APP_VINYL)          /* (SBX_APP_VINYL_DECK, the same header over the caller's deck, has no define here: this header has no way to state a block; include/sbx.h) */
#define SBX_SELECTED_APP SBX_APP_VINYL
#elif defined(APP_CLOUDS_BEST)   /* src/app_clouds_best.h, the stand-alone shader (no APP_* define in the reference) */
#define SBX_SELECTED_APP SBX_APP_CLOUDS_BEST
#else
#error "define one of APP_PLANET APP_CLOUDS APP_VINYL APP_EGG APP_RAYTRACER APP_ATMOSPHERE APP_SDF_AO (or APP_CLOUDS_BEST APP_PLANET_ATMOSPHERE APP_2D APP_2D_TEX APP_FUNC APP_ATMOSPHERE_GROUND APP_SDF_AO_SHADOW APP_SDF_AO_NORMALS APP_EGG_STRAIGHT APP_EGG_OVAL APP_CLOUDS_HEIGHT APP_CLOUDS_LUMINANCE APP_RAYTRACER_PHONG APP_RAYTRACER_NOSHADOW APP_RAYTRACER_STATIC APP_VINYL_CLOSEUP APP_VINYL_RIDGES APP_VINYL_NOSHADOW APP_PLANET_CLOSEUP APP_PLANET_CLOUDLESS APP_PLANET_UNLIT)"
#endif

namespace sbx_host {

struct float2_t { float v[2]; float& operator[](int i) { return v[i]; } float operator[](int i) const { return v[i]; } };
struct float4_t { float v[4]; float& operator[](int i) { return v[i]; } float operator[](int i) const { return v[i]; } };

// the reference's C++ globals (src/uniform_buffer.h:32-36)
inline thread_local float2_t iResolution{{0, 0}};
inline thread_local float iGlobalTime = 0.f;
inline thread_local float4_t iMouse{{0, 0, 0, 0}};

// ONE library context per process, created by whichever thread asks first (C++11 guarantees the one-time, thread-safe
// construction of a function-local static); the library's ABI is checked against this header's.
struct Context {
    sbx_ctx* ctx = nullptr;
    Context() {
        if (sbx_abi_version() != SBX_ABI_VERSION)
            throw std::runtime_error("libsbx.so has ABI " + std::to_string(sbx_abi_version()) + ", this header was written for ABI " +
                                     std::to_string(SBX_ABI_VERSION));
        const int rc = sbx_create(0, &ctx);
        if (rc != SBX_OK) throw std::runtime_error("sbx_create failed (" + std::to_string(rc) + "): a gfx950 GPU is required");
    }
    ~Context() { if (ctx) sbx_destroy(ctx); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    sbx_ctx* get() { return ctx; }
};
inline Context& context() { static Context c; return c; }

}  // namespace sbx_host

using sbx_host::iGlobalTime;
using sbx_host::iMouse;
using sbx_host::iResolution;

// void mainImage(out vec4 fragColor, in vec2 fragCoord)   — src/main.h:6-9
template <class Vec4, class Vec2>
inline void mainImage(Vec4& fragColor, const Vec2& fragCoord) {
    sbx_uniforms u{};
    u.u_res[0] = iResolution[0]; u.u_res[1] = iResolution[1];
    u.u_mouse[0] = iMouse[0]; u.u_mouse[1] = iMouse[1];
    u.u_time = iGlobalTime;
    const float fc[2] = {fragCoord[0], fragCoord[1]};
    float c[4];
    sbx_ctx* ctx = sbx_host::context().get();
    const int rc = sbx_main_image(ctx, SBX_SELECTED_APP, &u, nullptr, fc, c);    // renders the frame on first use
    if (rc != SBX_OK) throw std::runtime_error(std::string("sbx_main_image: ") + sbx_last_error(ctx));
    fragColor[0] = c[0]; fragColor[1] = c[1]; fragColor[2] = c[2]; fragColor[3] = c[3];
}
