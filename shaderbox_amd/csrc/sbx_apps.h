// shaderbox_amd/csrc/sbx_apps.h — what an app IS on the host side: one row of kApps per value of enum sbx_app (include/sbx.h).
// Host only: no kern_*.hip includes it.  A new app is a new enum value, a row here and a case in render_mapped's launch switch
// (sbx_capi.hip); the range checks, the aux block's defaults and cache key, the alpha refusals and the dispatch order all read the row.
// (The Python APPS dict and the name list of host/sbx_render.cpp are kept by hand: sharing the table with them would need an export.)
#pragma once
#include "../../include/sbx.h"
#include "sbx_device.h"

namespace sbx {

constexpr int SBX_APP_COUNT = SBX_APP_PLANET_WORLD + 1;
// (sbx_debug_tile_order, include/sbx_test.h, answers for every app — the builds after SBX_APP_FUNC that have an order grid below
// included; an app without one never has a table: 0 tables, 0 launches, nothing to copy)

// What a MOVING scene means for an app's dispatch-order table (sbx_tile_order.h; measured on animated frames,
// profiles/r06_tile_order.txt section 11):
//   TILE_SCENE_FREE    the costs do not follow the scene (APP_VINYL: -7 % standing or moving): the plain refresh schedule
//   TILE_SCENE_REFRESH they drift with it (APP_CLOUDS: a table 8-64 frames old keeps 0.6-3 % of the 6 % a fresh one gives): while the
//                      scene moves the table is rebuilt behind EVERY launch (23 us of a 2.2-3.4 ms frame: -3.6 ... -4.5 %)
//   TILE_SCENE_KEYED   they jump with it (APP_EGG: the silhouette's 16 x 4-pixel tiles are others a frame later; with tables even one
//                      frame old an animated launch is 8-27 % SLOWER than in the kernel's own hot-first order): the scene is part of
//                      the table's key — a scene that stands still gets its table, a moving one never does
enum { TILE_SCENE_FREE = 0, TILE_SCENE_REFRESH = 1, TILE_SCENE_KEYED = 2 };

enum AuxKind { AUX_NONE, AUX_CLOUDS, AUX_SDF_AO, AUX_CLOUDS_UE4, AUX_RT_SCENE, AUX_SDF_SCENE, AUX_EGG_POSE, AUX_VINYL_DECK, AUX_ATM_AIR, AUX_PLANET_WORLD };   // which block `aux` points to: sbx_aux_clouds, sbx_aux_sdf_ao, sbx_aux_clouds_ue4, sbx_aux_raytracer_scene, sbx_aux_sdf_scene, sbx_aux_egg_pose, sbx_aux_vinyl_deck, sbx_aux_atmosphere_air, sbx_aux_planet_world

struct AppTraits {
    AuxKind aux;
    bool noise_volumes;                    // the app samples the bound noise volumes (sbx_set_noise_volumes): refused until they are bound
    bool own_alpha;                        // the app writes its own alpha (src/app_2d.h:108): three-channel outputs cannot hold its pixels
    dim3 (*order_grid)(const RowMap&);     // the grid its dispatch-order table is built for; nullptr: the kernel keeps its own order
                                           // (measured to gain nothing there, see render_mapped)
    int scene_policy;                      // TILE_SCENE_*
};

constexpr AppTraits kApps[] = {
    /* SBX_APP_PLANET            */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_CLOUDS            */ {AUX_CLOUDS, false, false, clouds_grid, TILE_SCENE_REFRESH},
    /* SBX_APP_VINYL             */ {AUX_NONE, false, false, vinyl_grid, TILE_SCENE_FREE},
    /* SBX_APP_EGG               */ {AUX_NONE, false, false, egg_grid, TILE_SCENE_KEYED},
    /* SBX_APP_RAYTRACER         */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_ATMOSPHERE        */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_SDF_AO            */ {AUX_SDF_AO, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_CLOUDS_BEST       */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_CLOUDS_TEX        */ {AUX_CLOUDS, true, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_CLOUDS_UE4        */ {AUX_CLOUDS_UE4, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_CLOUDS_SKY        */ {AUX_CLOUDS, false, false, clouds_grid, TILE_SCENE_REFRESH},
    /* SBX_APP_VINYL_GPU         */ {AUX_NONE, false, false, vinyl_grid, TILE_SCENE_FREE},
    /* SBX_APP_PLANET_ATMOSPHERE */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_2D                */ {AUX_NONE, false, true, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_2D_TEX            */ {AUX_NONE, false, true, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_FUNC              */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_ATMOSPHERE_GROUND */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_SDF_AO_SHADOW     */ {AUX_SDF_AO, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_SDF_AO_NORMALS    */ {AUX_SDF_AO, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_EGG_STRAIGHT      */ {AUX_NONE, false, false, egg_grid, TILE_SCENE_KEYED},
    /* SBX_APP_EGG_OVAL          */ {AUX_NONE, false, false, egg_grid, TILE_SCENE_KEYED},
    /* SBX_APP_CLOUDS_HEIGHT     */ {AUX_CLOUDS, false, false, clouds_grid, TILE_SCENE_REFRESH},
    /* SBX_APP_CLOUDS_LUMINANCE  */ {AUX_CLOUDS, false, false, clouds_grid, TILE_SCENE_REFRESH},
    /* SBX_APP_RAYTRACER_PHONG   */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_RAYTRACER_NOSHADOW*/ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_RAYTRACER_STATIC  */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_VINYL_CLOSEUP     */ {AUX_NONE, false, false, vinyl_grid, TILE_SCENE_FREE},
    /* SBX_APP_VINYL_RIDGES      */ {AUX_NONE, false, false, vinyl_grid, TILE_SCENE_FREE},
    /* SBX_APP_VINYL_NOSHADOW    */ {AUX_NONE, false, false, vinyl_grid, TILE_SCENE_FREE},
    /* SBX_APP_PLANET_CLOSEUP    */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_PLANET_CLOUDLESS  */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_PLANET_UNLIT      */ {AUX_NONE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_RAYTRACER_SCENE   */ {AUX_RT_SCENE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_SDF_SCENE         */ {AUX_SDF_SCENE, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_EGG_POSE          */ {AUX_EGG_POSE, false, false, egg_grid, TILE_SCENE_KEYED},
    /* SBX_APP_VINYL_DECK        */ {AUX_VINYL_DECK, false, false, vinyl_grid, TILE_SCENE_KEYED},
    /* SBX_APP_ATMOSPHERE_AIR    */ {AUX_ATM_AIR, false, false, nullptr, TILE_SCENE_FREE},
    /* SBX_APP_PLANET_WORLD      */ {AUX_PLANET_WORLD, false, false, nullptr, TILE_SCENE_FREE},   // (as SBX_APP_PLANET: no order grid, so no table the block could be a key of)
};
static_assert(sizeof(kApps) / sizeof(kApps[0]) == SBX_APP_COUNT, "every value of enum sbx_app needs its row in kApps");

inline bool app_valid(int app) { return (unsigned)app < (unsigned)SBX_APP_COUNT; }
inline bool app_owns_alpha(int app) { return app_valid(app) && kApps[app].own_alpha; }
// bytes of the block an app's `aux` points to (0: the app reads none, or is none)
inline int app_aux_bytes(int app) {
    switch (app_valid(app) ? kApps[app].aux : AUX_NONE) {
    case AUX_CLOUDS: return (int)sizeof(sbx_aux_clouds);
    case AUX_SDF_AO: return (int)sizeof(sbx_aux_sdf_ao);
    case AUX_CLOUDS_UE4: return (int)sizeof(sbx_aux_clouds_ue4);
    case AUX_RT_SCENE: return (int)sizeof(sbx_aux_raytracer_scene);
    case AUX_SDF_SCENE: return (int)sizeof(sbx_aux_sdf_scene);
    case AUX_EGG_POSE: return (int)sizeof(sbx_aux_egg_pose);
    case AUX_VINYL_DECK: return (int)sizeof(sbx_aux_vinyl_deck);
    case AUX_ATM_AIR: return (int)sizeof(sbx_aux_atmosphere_air);
    case AUX_PLANET_WORLD: return (int)sizeof(sbx_aux_planet_world);
    default: return 0;
    }
}
// the caller's aux block, or the reference's defaults where the caller passed none
template <class A> inline A aux_or(const void* aux, void (*defaults)(A*)) {
    A a;
    if (aux) a = *(const A*)aux; else defaults(&a);
    return a;
}
inline sbx_aux_clouds aux_clouds(const void* aux) { return aux_or<sbx_aux_clouds>(aux, sbx_aux_clouds_defaults); }
inline sbx_aux_sdf_ao aux_sdf_ao(const void* aux) { return aux_or<sbx_aux_sdf_ao>(aux, sbx_aux_sdf_ao_defaults); }
inline sbx_aux_clouds_ue4 aux_clouds_ue4(const void* aux) { return aux_or<sbx_aux_clouds_ue4>(aux, sbx_aux_clouds_ue4_defaults); }
// SBX_APP_RAYTRACER_SCENE: the caller's scene, or the Cornell box of these uniforms (its defaults depend on them)
inline sbx_aux_raytracer_scene aux_raytracer_scene(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_raytracer_scene a;
    if (aux) a = *(const sbx_aux_raytracer_scene*)aux; else sbx_raytracer_scene_cornell(&uni, 0, &a);
    return a;
}
// SBX_APP_SDF_SCENE: the caller's field, or the ramp block of these uniforms
inline sbx_aux_sdf_scene aux_sdf_scene(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_sdf_scene a;
    if (aux) a = *(const sbx_aux_sdf_scene*)aux; else sbx_sdf_scene_ramp(&uni, &a);
    return a;
}
// SBX_APP_EGG_POSE: the caller's pose, or what app_egg.h makes of these uniforms
inline sbx_aux_egg_pose aux_egg_pose(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_egg_pose a;
    if (aux) a = *(const sbx_aux_egg_pose*)aux; else sbx_egg_pose_default(&uni, &a);
    return a;
}
// SBX_APP_VINYL_DECK: the caller's deck, or what app_vinyl.h makes of these uniforms
inline sbx_aux_vinyl_deck aux_vinyl_deck(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_vinyl_deck a;
    if (aux) a = *(const sbx_aux_vinyl_deck*)aux; else sbx_vinyl_deck_default(&uni, &a);
    return a;
}
// SBX_APP_ATMOSPHERE_AIR: the caller's air, or the reference's numbers with the sun setup_scene makes of these uniforms (view 0)
inline sbx_aux_atmosphere_air aux_atmosphere_air(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_atmosphere_air a;
    if (aux) a = *(const sbx_aux_atmosphere_air*)aux; else sbx_atmosphere_air_default(&uni, 0, &a);
    return a;
}
// SBX_APP_PLANET_WORLD: the caller's world, or app_planet.h's numbers with the spins of these uniforms
inline sbx_aux_planet_world aux_planet_world(const void* aux, const sbx_uniforms& uni) {
    sbx_aux_planet_world a;
    if (aux) a = *(const sbx_aux_planet_world*)aux; else sbx_planet_world_default(&uni, &a);
    return a;
}

}  // namespace sbx
