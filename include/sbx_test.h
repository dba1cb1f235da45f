/* include/sbx_test.h — TEST HOOKS of libsbx.  Not part of the drop-in surface.
 *
 * include/sbx.h is what a host binds (the replacement of the reference's per-pixel mainImage() loop, src/main.h:6-53).  The entry
 * points below exist so that tests/ and tools/ can (a) run the cross-check builds of the kernels against the default ones,
 * (b) evaluate single functions of the math spec on the device against the CPU oracle, (c) drive paths that ordinary frames
 * never reach (the fault path, the witness re-run, a store-exchange wait that times out).  They are exported by the same
 * libsbx.so, keep no compatibility promise across SBX_ABI_VERSION, and no reference interface corresponds to them.
 */
#ifndef SBX_TEST_H
#define SBX_TEST_H

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic knob: 0 = default kernels; 1 = the plain cross-check kernels where one exists: APP_CLOUDS with every
 * lane hashing its own lattice corners (no cache, no staging, no tables); APP_EGG / APP_SDF_AO / APP_VINYL with every
 * member of the SDF union evaluated everywhere (no culling); APP_PLANET without its exact skips.
 * 2 / 3 = the default kernels, except APP_EGG / APP_SDF_AO / APP_VINYL(_GPU): 2 = their square-root witness with the recording
 * edge raised to 1.0, so that the re-run path (csrc/sbx_witness.h `witnessed`) executes on ordinary frames; 3 = the culled
 * kernels with the IEEE roots only.  For every app and eval entry below that has a witness, the one table from 1 / 2 / 3 to the
 * kernel's CULL and WIT is witness_dispatch's in that header; a kernel with nothing to cull folds 1 and 3 together.
 * APP_FUNC: 1 = hash_w in place for every cell (no hash table; worley_fbm as src/app_func.h writes it).
 * SBX_APP_ATMOSPHERE_GROUND: 1 = the plain statement of src/app_atmosphere.h:211-224 lane by lane (no wave-level exit, guarded exp,
 * sqrt_n_, division by the exact reciprocal; exact, whatever sbx_set_precision says).  SBX_APP_ATMOSPHERE ignores the knob.
 * SBX_APP_SDF_AO_SHADOW / SBX_APP_SDF_AO_NORMALS: every value as for APP_SDF_AO, the shadow march included — 1 = no culling, the spec's
 * compare-and-select min / max and the IEEE roots along the shadow ray too; 2 / 3 = the witness's test edge / the IEEE roots only.
 * SBX_APP_EGG_STRAIGHT / SBX_APP_EGG_OVAL: every value as for APP_EGG, over the build's own members and bounds.
 * SBX_APP_CLOUDS_HEIGHT / SBX_APP_CLOUDS_LUMINANCE: as for APP_CLOUDS, 1 = the per-lane kernel of the build.
 * APP_RAYTRACER and SBX_APP_RAYTRACER_PHONG / _NOSHADOW / _STATIC alike: 1 = the IEEE roots and normalisations with the six-plane loop of
 * raytrace_iteration; 2 = the witness's test edge; 3 = the IEEE roots and normalisations; each over the build's own code and frame.
 * SBX_APP_RAYTRACER_SCENE: 1 and 3 = the IEEE roots, normalisations and sphere-normal quotients; 2 = the witness's test edge.
 * SBX_APP_SDF_SCENE and sbx_sdf_eval: 1 and 3 = the IEEE roots; 2 = the witness's test edge.
 * SBX_APP_VINYL_CLOSEUP / _RIDGES / _NOSHADOW: every value as for APP_VINYL, over the build's own code and frame.
 * SBX_APP_PLANET_CLOSEUP / _CLOUDLESS / _UNLIT: as for APP_PLANET, 1 = the build without its exact skips.
 * sbx_atmosphere_eval: 1 = the plain statement of src/app_atmosphere.h:50-160 lane by lane for every wave (no class test, guarded exp,
 * sqrt_n_, division by the exact reciprocal); 0 runs it only on the waves whose rays are outside the class of csrc/sbx_atmosphere.h.
 * sbx_clouds_eval: 1 = the statement of k_clouds_perlane lane by lane (hash1 in place, exp_, pow_, the IEEE division in the coverage
 * smoothstep); 0 takes the lattice hashes from the context's table and the guard-less forms the aux block admits.
 * sbx_planet_eval: 1 = the SKIP = false statement of k_planet lane by lane for every wave (every fBm octave and cloud sample evaluated,
 * the IEEE roots and divisions, exp_, lattice indices as the reference forms them); 0 runs it only on the waves whose own operands fail
 * a guard of csrc/kern_planet_eval.hip, and for any u_time beyond 1e8 in magnitude or NaN.
 * SBX_APP_EGG_POSE: every value as for APP_EGG; a pose outside the domain of the culls and witnessed roots (a non-finite frame constant, a
 * value of the block beyond 1e4, 1e10 for the angle) takes 1 whatever is set; sbx_debug_egg_pose_launches counts such launches.  sbx_egg_eval: 1 = CULL = false and the IEEE roots for every
 * wave; 2 / 3 = the witness's test edge / the IEEE roots; 0 takes the plain form only for such a pose and for the waves whose own inputs
 * hold a value beyond 1e4 or a NaN (csrc/kern_egg_eval.hip).  "ik_solver" has one form.
 * SBX_APP_VINYL_DECK: every value as for APP_VINYL; a deck outside the domain of the culls and the hardware min / max (a value of the
 * block's first sixteen beyond 1e4, 1e10 for the three angles, a non-finite camera or matrix: csrc/sbx_vinyl.h, sbx_frames.hip
 * vinyl_deck_tame) takes 1 whatever is set; sbx_debug_vinyl_deck_launches counts such launches.  sbx_vinyl_eval: 1 = CULL = false, the IEEE roots and
 * compare-and-select unions for every wave; 2 / 3 = the witness's test edge / the IEEE roots; 0 takes the plain form only for such a deck
 * (the camera's fields ignored) and for the waves whose own points or directions hold a value beyond 1e4 or a NaN
 * (csrc/kern_vinyl_eval.hip).
 * sbx_raytracer_eval: 1 and 3 = the IEEE roots for every wave, 2 = the witness's test edge, 0 the witnessed roots; no block and no
 * element changes a wave's form (csrc/kern_raytracer_eval.hip).
 * sbx_sdf_scene_eval: 1 and 3 = the IEEE roots for every wave, 2 = the witness's test edge, 0 the witnessed roots; no block and no
 * element changes a wave's form (csrc/kern_sdf_scene_eval.hip).
 * SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval: 1 = the plain statement for every wave, whatever the block; every other value
 * leaves the tier to the block (csrc/sbx_frames.hip atmosphere_air_tier).
 * SBX_APP_PLANET_WORLD: 1 = k_planet_world<false>, the plain statement over the block's numbers, for every block, one that differs from the
 * default in camera, angles and sun only included; every other value leaves the tier to the block (planet_world_tier).
 * sbx_planet_world_eval: 1 = the plain form for every wave; 0 runs it for the waves whose own operands fail a guard and for every wave
 * of a block outside planet_world_tame (csrc/kern_planet_eval.hip PeWorld).
 * All variants are specified to produce identical bits (tests/test_gpu_parity.py sweeps them against each other). */
int sbx_set_variant(sbx_ctx* ctx, int variant);

/* sbx_atmosphere_eval (sbx.h) with a count: the same launch (the context's variant included), after which the call waits and
 * stores in `fast_waves_host` the number of 64-lane waves that ran the fast forms (0 under variant 1, and for a sun direction the
 * host refuses).  It allocates and synchronises, so it is not capturable.  For the test that the fast forms run where the default
 * kernel is compared with the plain one (tests/test_gpu_atmosphere_eval.py) and for tools/time_atmosphere_eval.py. */
int sbx_debug_atmosphere_eval(sbx_ctx* ctx, const char* fn, const float* rays, const float* sun_dir, float* out, size_t n,
                              unsigned* fast_waves_host, void* stream);

/* sbx_clouds_eval (sbx.h) with counts: the same launch (the context's variant and the same choice of hash table included) in a counting
 * instantiation of the kernel, after which the call waits and stores in counts_host[0] the noise cells (one noise_iq call = one cell,
 * four per density_func) whose eight lattice hashes came from the context's table and in counts_host[1] the cells whose hashes were
 * evaluated in place (all of them under variant 1 and where no table is usable).  It allocates and synchronises, so it is not
 * capturable.  For tests/test_gpu_clouds_eval.py and tools/time_clouds_eval.py. */
int sbx_debug_clouds_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_clouds* aux, float u_time, const float* in, float* out, size_t n,
                          uint64_t counts_host[2], void* stream);

/* sbx_planet_eval (sbx.h) with counts: the same launch (the context's variant included) followed by a wait, after which counts_host[0]
 * holds the waves that ran with every guarded short form on and counts_host[1] the waves that took the plain form for at least one
 * part (all of them under variant 1 or an untame u_time).  It allocates and synchronises, so it is not capturable.  For
 * tests/test_gpu_planet_eval.py and tools/time_planet_eval.py. */
int sbx_debug_planet_eval(sbx_ctx* ctx, const char* fn, float u_time, const float* in, float* out, size_t n, unsigned counts_host[2],
                          void* stream);

/* sbx_planet_world_eval (sbx.h) with counts: as sbx_debug_planet_eval — counts_host[0] the waves that ran with every guarded short form
 * on, counts_host[1] the waves that took the plain form for at least one part: all of them under variant 1 or a block outside
 * planet_world_tame (csrc/sbx_frames.hip).  It allocates and synchronises, so it is not capturable. */
int sbx_debug_planet_world_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_planet_world* world, const float* in, float* out, size_t n,
                                unsigned counts_host[2], void* stream);

/* sbx_egg_eval (sbx.h) with counts: the same launch (the context's variant included) followed by a wait, after which counts_host[0]
 * holds the waves that took the witnessed roots only and counts_host[1] the waves that re-ran with the IEEE roots because a lane
 * recorded a root outside the witness's interval.  A wave given the plain form (variant 1 or 3, an untame pose, an untame input) and
 * "ik_solver" are in neither.  It allocates and synchronises, so it is not capturable.  For tests/test_gpu_egg_eval.py and
 * tools/time_egg_eval.py. */
int sbx_debug_egg_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_egg_pose* pose, const float* in, float* out, size_t n,
                       unsigned counts_host[2], void* stream);

/* sbx_vinyl_eval (sbx.h) with counts: the same launch (the context's variant included) followed by a wait, after which counts_host[0]
 * holds the waves that took the witnessed roots only and counts_host[1] the waves that re-ran with the IEEE roots because a lane
 * recorded a root outside the witness's interval.  A wave given the plain form (variant 1 or 3, an untame deck, an untame input) is in
 * neither.  It allocates and synchronises, so it is not capturable.  For tests/test_gpu_vinyl_eval.py and tools/time_vinyl_eval.py. */
int sbx_debug_vinyl_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_vinyl_deck* deck, const float* in, float* out, size_t n,
                         unsigned counts_host[2], void* stream);
/* sbx_raytracer_eval (sbx.h) with counts: the same launch (the context's variant included) followed by a wait, after which
 * counts_host[0] holds the waves that took the witnessed roots only and counts_host[1] the waves that re-ran with the IEEE roots because
 * a lane recorded an argument outside the witness's interval.  No wave's form depends on its elements or on the block, so under
 * variants 0 and 2 the two add up to the waves of the launch; under 1 and 3 (the IEEE roots) both are 0.  It allocates and synchronises,
 * so it is not capturable.  For tests/test_gpu_raytracer_eval.py and tools/time_raytracer_eval.py. */
int sbx_debug_raytracer_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_raytracer_scene* scene, const float* in, float* out, size_t n,
                             unsigned counts_host[2], void* stream);
/* sbx_sdf_scene_eval (sbx.h) with counts: the same launch (the context's variant included) followed by a wait, after which
 * counts_host[0] holds the waves that took the witnessed roots only and counts_host[1] the waves that re-ran with the IEEE roots because
 * a lane recorded an argument outside the witness's interval.  No wave's form depends on its elements or on the block, so under
 * variants 0 and 2 the two add up to the waves of the launch ("illuminate" takes no root: all of its waves are in the first); under 1
 * and 3 (the IEEE roots) both are 0.  It allocates and synchronises, so it is not capturable: a capturing stream is refused with the
 * capture intact, a NULL counts_host too.  For tests/test_gpu_sdf_scene_eval.py and tools/time_sdf_scene_eval.py. */
int sbx_debug_sdf_scene_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_sdf_scene* scene, const float* in, float* out, size_t n,
                             unsigned counts_host[2], void* stream);
/* sbx_atmosphere_air_eval (sbx.h) with a count: the same launch (the context's variant included) followed by a wait, after which
 * *fast_waves_host holds the waves that took the fast body (csrc/sbx_atmosphere.h "CALLER'S AIR"): 0 under an untame block or
 * sbx_set_variant 1.  It allocates and synchronises, so it is not capturable. */
int sbx_debug_atmosphere_air_eval(sbx_ctx* ctx, const char* fn, const sbx_aux_atmosphere_air* air, const float* rays, float* out, size_t n,
                                  unsigned* fast_waves_host, void* stream);
/* SBX_APP_ATMOSPHERE_AIR launches of this context so far: counts[0] all of them, counts[1] those that took the literal tier (the shipped
 * kernels over the block's sun), counts[2] those that took the plain kernel (sbx_set_variant 1, or a block that is neither literal nor
 * tame).  The rest took the run-time kernel with its per-wave selection. */
int sbx_debug_atmosphere_air_launches(sbx_ctx* ctx, uint64_t counts[3]);
/* SBX_APP_PLANET_WORLD launches of this context so far, by what ran: counts[0] the literal tier with its short forms (k_planet<true>'s
 * instantiations over the block's camera, angles and sun), counts[1] the run-time kernel k_planet_world<true>, counts[2] a plain
 * kernel: k_planet_world<false> (sbx_set_variant 1, whatever the block; a block outside planet_world_tame) or k_planet<false> (a
 * literal-tier block whose camera or angles are outside planet_world_camera_tame; csrc/sbx_frames.hip). */
int sbx_debug_planet_world_launches(sbx_ctx* ctx, uint64_t counts[3]);
/* SBX_APP_VINYL_DECK launches of this context so far, and how many of them took the reference form because their deck was outside the
 * domain of the culls (whatever variant was set; a launch under sbx_set_variant 1 with a tame deck is not among the latter). */
int sbx_debug_vinyl_deck_launches(sbx_ctx* ctx, uint64_t counts[2]);
/* The same record for SBX_APP_EGG_POSE: counts[0] its launches of this context so far, counts[1] those of them that took the reference
 * form because their pose was outside the domain of the culls and witnessed roots (csrc/sbx_frames.hip egg_pose_tame), whatever variant
 * was set; a launch under sbx_set_variant 1 with a tame pose is not among the latter.  Host bookkeeping: one launch adds one to
 * counts[0] whatever rows or points it renders.  For the tests that a pose compared with the plain kernel did not take it itself
 * (tests/test_gpu_caller_sweeps.py). */
int sbx_debug_egg_pose_launches(sbx_ctx* ctx, uint64_t counts[2]);

/* Device evaluation of the math spec, elementwise over device arrays (for parity tests):
 * fn in {"sin","cos","tan","exp","pow","acos","atan2","hash","div","div_rd","exp_h13","pow_h","sqrt_n","sqrt_ieee","exp_reg","exp_reg_plain","exp_reg64","exp_reg64_plain","exp_small","exp_small_plain","exp_reg4k","sin_b40","div3","sqrt_rs","divn","srgb_pow","pow_spec"}; b may be NULL
 * for unary fns ("exp_reg*": kernel-internal forms of exp — 32-entry table / degree 6 and 64-entry / degree 5, each with and without
 * the three-address asm — used by the regular-frame k_clouds and by k_atmosphere's density terms, equal to
 * "exp" for |x| <= 80; "exp_reg4k": the 4096-entry / degree-3 form of k_atmosphere's density terms, equal to "exp" for |x| <= 80;
 * "sin_b40": sin with a degree-15 polynomial, the hash passes' form, equal to "sin" for |x| <= 2^40;
 * "exp_small*": the degree-8 polynomial without argument reduction that the regular-frame k_clouds uses when
 * every argument lies in [-0.205, -0], equal to "exp" on that whole interval and at +0).
 * "div3" = a/b as q0 = a * RN(1/b), q = fma(fma(-q0, b, a), RN(1/b), q0): equal to "div" away from overflow and underflow;
 * "divn" = a/b through v_rcp_f32, one Newton step and div3's three instructions (equal to "div" away from overflow / underflow);
 * "pow_spec" = pow exactly as stated in the oracle ("pow" is the device's shorter instruction sequence for the same operations);
 * "srgb_pow" = pow(x, 1/2.2f) in the short form to_srgb uses on the device (equal to "pow" with b = 1/2.2f on all 2^32 arguments);
 * "sqrt_rs" = v_rsq_f32 and one corrected step: equal to "sqrt_ieee" for finite x >= 2^-102;
 * "div" = IEEE a/b, "div_rd" = the same quotient through the binary64 reciprocal of b (must be identical). */
int sbx_math_eval(sbx_ctx* ctx, const char* fn, const float* a, const float* b, float* out,
                  size_t n, void* stream);

int sbx_multi_set_variant(sbx_multi* m, int variant);

/* sbx_noise_eval (sbx.h) also answers three names that exist for the parity tests of the recorded-domain forms
 * (csrc/sbx_witness.h): "normalize" = v / length(v) in the IEEE form, "wit_normalize" = the fast form (sqrt_rs_, v_rcp_f32 + one
 * Newton step, three div3_), "wit_record" = out[0] 1 where that form's domain record fires. */

/* SampleLevel(linear, wrap, lod 0).r of a size^3 RGBA32F device volume at n points (xyz interleaved, device):
 * the texture-filter spec on its own, for parity tests. */
int sbx_tex3d_eval(sbx_ctx* ctx, int size, const float* rgba, const float* xyz, float* out, size_t n, void* stream);


/* One wave through the fault path of the hash cache (sbx_fault_status then reports SBX_ERR_FAULT until sbx_clear_fault). */
int sbx_debug_raise_fault(sbx_ctx* ctx, void* stream);

/* The store exchange's waits (sbx_shared_frame_begin / _end) give up after this many milliseconds and raise the device's fault
 * word (default 10 000); tests shorten it to see the fault. */
int sbx_shared_set_timeout_ms(sbx_shared* s, int ms);

/* MODEL of what RCCL's point-to-point receive kernels cost the frame's owner while the peers' slabs land (bench.py --emulate-ranks,
 * tools/strip_scaling.py; nothing in the product calls it): `workgroups` workgroups of 256 threads stay resident for
 * `duration_us` microseconds and copy `bytes` bytes from `src` to `dst` (device memory, 16-byte aligned) at that pace — the CUs
 * a grouped ncclRecv from N-1 peers holds for the time the links need, and the HBM writes of the landing. */
int sbx_model_landing(sbx_ctx* ctx, const void* src, void* dst, size_t bytes, int workgroups, float duration_us, void* stream);

/* The dispatch-order table of an app (csrc/sbx_tile_order.h TileOrder: a full launch's tiles sorted by the cost earlier frames measured,
 * longest first — a hint about cost, never about pixels): tables built so far for the current launch shape (0 = the launches still
 * run in plain order), launches since the last one, and — if `table` is not NULL and one exists — the current table copied to the
 * host (`capacity` words; returns the number of tiles, or a negative sbx_status).  For the test that every table is a permutation.
 * Answers for every app; one without a dispatch order (csrc/sbx_apps.h kApps) never has a table. */
int sbx_debug_tile_order(sbx_ctx* ctx, int app, int* tables_built, int* launches_since, unsigned* table, size_t capacity);

/* The sort behind that table (csrc/kern_util.hip launch_order_build: k_order_count / _scan / _place) run once on `gx * gy` cost words
 * of the caller's (host memory), the table of `gx * gy` words x | y << 16 copied back to `table_host`; synchronous.  Device buffers
 * of its own, nothing of the context's tables is touched.  gx, gy outside 1 ... 0xffff (the bound of a launch that takes a table): SBX_ERR_ARG.
 * For the test that the table is a permutation, longest cost class first, whatever the words hold (tests/test_gpu_tile_order.py). */
int sbx_debug_order_build(sbx_ctx* ctx, const unsigned* cost_host, int gx, int gy, unsigned* table_host, void* stream);

/* Launches of k_raytracer_scene (SBX_APP_RAYTRACER_SCENE's kernel, csrc/kern_raytracer.hip) this context has enqueued since its
 * creation: for the test that a scene block equal to the Cornell box is rendered by the scene kernel, not handed to k_raytracer. */
int sbx_debug_raytracer_scene_launches(sbx_ctx* ctx, uint64_t* launches);

/* APP_CLOUDS' lattice-hash tables (csrc/sbx_ctx.h HashTables; csrc/kern_clouds.hip GTab): the newest — largest — table's size in entries and
 * its bias (entry i holds hash(float(i - bias))), 0 / 0 before the first one; how many tables this context has built; and whether its last
 * launch of APP_CLOUDS, of its HEIGHT / LUMINANCE builds or of CLOUDS_SKY took a hash-table kernel (1) or another one (0): `gt != 0` of
 * sbx_debug_clouds_last_selection's record.  Any
 * pointer may be NULL.  For the tests that the table kernels run where their frames are compared with the per-lane kernel's, and that
 * the launches which must not touch a table do not (tests/test_gpu_clouds_hashtab.py). */
int sbx_debug_clouds_hashtab(sbx_ctx* ctx, int* entries, int* bias, int* tables_built, int* last_launch_used_table);

/* `count` entries of the newest table from entry `first` on, copied to host memory after waiting for its build. */
int sbx_debug_clouds_hashtab_read(sbx_ctx* ctx, size_t first, size_t count, float* host);

/* WHICH KERNEL a launch of APP_CLOUDS, of its HEIGHT / LUMINANCE builds or of CLOUDS_SKY took (csrc/kern_clouds.hip: clouds_select is
 * the host's choice, launch_form<> the one place a k_clouds / k_clouds_perlane launch is made — it writes perlane, ytab_used, reg, lm,
 * sm, gt and build from its own template arguments). */
typedef struct sbx_clouds_selection {
    int build;          /* 0 the shipped build, 1 HEIGHT, 2 LUMINANCE */
    int perlane;        /* 1: k_clouds_perlane<build>; every field of the next line is 0 then */
    int ytab_used, reg, lm, sm, gt;   /* k_clouds<YTAB, REG, LM, SM, BUILD, GT> as instantiated (gt: 0, or 1 + the first octave read from the hash table) */
    int ytab;           /* the y table the launch read: 0 none, 1 a slot of the eager ring, 2 the context's big table, 3 a slot of the capture ring
                           (sbx_debug_clouds_select, which has no context: 1 for a table of up to 4096 rows, 2 for a longer one) */
    int sky;            /* the frame is SKY_SPHERE's (CLOUDS_SKY) */
    /* the host predicates as evaluated for the frame, whether or not the choice came to depend on them */
    int regular, exp_small, index_domain, div3_domain, lip_ok;
    int light;          /* the form of sun_dir * dt: 1 z-only (x == 0 and y == 0), 2 y-z (x == 0), 0 general (NaN included) */
    int need_range;     /* clouds_hashtab_range: the hash-table range the frame needs, 0: it takes no table kernel */
    int table_range;    /* the range of the ready table the launch was given, 0: none */
    int vt;             /* 1: k_clouds<..., VT = true>, the instantiation that reads the context's view table (gt != 0 only) */
    uint64_t launches;  /* launches of these apps by the context so far, this one included (sbx_debug_clouds_select: 0) */
} sbx_clouds_selection;

/* The record of the context's last launch of APP_CLOUDS, SBX_APP_CLOUDS_HEIGHT / _LUMINANCE or SBX_APP_CLOUDS_SKY (all zero before the
 * first one).  `last_launch_used_table` of sbx_debug_clouds_hashtab is `gt != 0` of this record. */
int sbx_debug_clouds_last_selection(sbx_ctx* ctx, sbx_clouds_selection* out);

/* The choice alone: host only, no context, no device, nothing launched (callable on a machine without a GPU, like sbx_span_table).
 * app: one of the four apps above; variant as sbx_set_variant; "a y table of `ytab_rows` rows is at hand" (0: none), "a ready hash
 * table of range `table_range` is at hand" (0: none); point_list != 0: the launch is a point list's (sbx_render_points).  Returns
 * SBX_OK, or SBX_ERR_ARG for another app, a NULL pointer or negative march steps. */
int sbx_debug_clouds_select(int app, const sbx_uniforms* uni, const void* aux, int variant, int ytab_rows, int table_range, int point_list,
                            sbx_clouds_selection* out);

/* APP_CLOUDS' view tables (include/sbx.h "THE VIEW TABLE"; csrc/sbx_ctx.h ViewTables): the entries (frame pixels) of the table built or
 * used last, 0 before the first one; how many tables this context has built; whether its last launch of APP_CLOUDS or of its HEIGHT /
 * LUMINANCE builds took a view-table kernel (`vt` of sbx_debug_clouds_last_selection's record); and, where it did not, why
 * (SBX_VIEWTAB_*).  Any pointer may be NULL. */
enum {
    SBX_VIEWTAB_USED = 0,        /* the launch read a table */
    SBX_VIEWTAB_OFF = 1,         /* SBX_CLOUDS_VIEWTAB=0 */
    SBX_VIEWTAB_INELIGIBLE = 2,  /* not a launch that may read one: a point list, a span, a multi-rank strip, SKY_SPHERE, the per-lane kernel, a sun
                                    off the z axis (the y-z and the general light march), or a frame that takes no hash-table kernel */
    SBX_VIEWTAB_NEW_KEY = 3,     /* the key has not been seen on the two eager launches before this one */
    SBX_VIEWTAB_CAP = 4,         /* the table would exceed the byte cap */
    SBX_VIEWTAB_NO_SLOT = 5,     /* both slots hold other keys that are still read (or pinned by a capture) */
    SBX_VIEWTAB_CAPTURE = 6,     /* a stream capture, and no table of the key that the host has seen complete */
    SBX_VIEWTAB_ALLOC = 7        /* the allocation or an event failed (the error is dropped) */
};
int sbx_debug_clouds_viewtab(sbx_ctx* ctx, size_t* entries, int* tables_built, int* last_launch_used_table, int* last_refusal);

/* The byte cap of one view table (default SBX_CLOUDS_VIEWTAB_DEFAULT_BYTES), so that tests reach the refusal at small shapes. */
int sbx_debug_set_clouds_viewtab_cap(sbx_ctx* ctx, size_t bytes);

/* The key of the view table a launch of `app` (SBX_APP_CLOUDS or its HEIGHT / LUMINANCE builds) under these uniforms and this aux block
 * would ask for: `words` (28) 32-bit words.  Host only, no context.  SBX_ERR_ARG as sbx_debug_clouds_select. */
int sbx_debug_clouds_viewtab_key(int app, const sbx_uniforms* uni, const void* aux, unsigned* key, int words);

/* sbx_debug_clouds_select with the further input "a ready view table of the frame's camera is at hand" (view_table != 0), for a
 * full-frame one-rank launch (or a point list): `vt` of the record. */
int sbx_debug_clouds_select_vt(int app, const sbx_uniforms* uni, const void* aux, int variant, int ytab_rows, int table_range, int point_list,
                               int view_table, sbx_clouds_selection* out);

#ifdef __cplusplus
}
#endif
#endif /* SBX_TEST_H */
