"""shaderbox_amd — MI355X-native renderer for shaderbox's mainImage() hot path.

Python host layer over the C ABI of libsbx.so (include/sbx.h).  PyTorch is used only as plumbing:
device memory (framebuffers are torch CUDA tensors), streams and torch.distributed.  All pixels
are produced by the hand-written HIP kernels in shaderbox_amd/csrc; there is no CPU or PyTorch
fallback — if the library or a gfx950 device is missing, construction raises.

The surface mirrors the reference's: an app is chosen by its APP_* project define
(/root/reference/README.md:11-22), a frame is a pure function of the uniforms u_res / u_time /
u_mouse (+ the per-app aux block with the defaults of /root/reference/src/uniform_buffer.h:39-60).
"""
import ctypes
import os

from . import shard  # noqa: F401  (pure-python row-block arithmetic, no GPU needed)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsbx.so")

APP_PLANET, APP_CLOUDS, APP_VINYL, APP_EGG, APP_RAYTRACER, APP_ATMOSPHERE, APP_SDF_AO, APP_CLOUDS_BEST, APP_CLOUDS_TEX, APP_CLOUDS_UE4, APP_CLOUDS_SKY, APP_VINYL_GPU, APP_PLANET_ATMOSPHERE, APP_2D, APP_2D_TEX, APP_FUNC, APP_ATMOSPHERE_GROUND, APP_SDF_AO_SHADOW, APP_SDF_AO_NORMALS, APP_EGG_STRAIGHT, APP_EGG_OVAL, APP_CLOUDS_HEIGHT, APP_CLOUDS_LUMINANCE, APP_RAYTRACER_PHONG, APP_RAYTRACER_NOSHADOW, APP_RAYTRACER_STATIC, APP_VINYL_CLOSEUP, APP_VINYL_RIDGES, APP_VINYL_NOSHADOW, APP_PLANET_CLOSEUP, APP_PLANET_CLOUDLESS, APP_PLANET_UNLIT, APP_RAYTRACER_SCENE, APP_SDF_SCENE, APP_EGG_POSE, APP_VINYL_DECK, APP_ATMOSPHERE_AIR, APP_PLANET_WORLD = range(38)
APPS = {"APP_PLANET": APP_PLANET, "APP_CLOUDS": APP_CLOUDS, "APP_VINYL": APP_VINYL, "APP_EGG": APP_EGG,
        "APP_RAYTRACER": APP_RAYTRACER, "APP_ATMOSPHERE": APP_ATMOSPHERE, "APP_SDF_AO": APP_SDF_AO,
        "APP_CLOUDS_BEST": APP_CLOUDS_BEST,    # src/app_clouds_best.h (stand-alone shader, not an APP_* define)
        "APP_CLOUDS_TEX": APP_CLOUDS_TEX,      # APP_CLOUDS + USE_NOISE_TEX (src/app_clouds.h:9)
        "APP_CLOUDS_UE4": APP_CLOUDS_UE4,      # ue4/volumetric_clouds/Shaders/app_clouds.usf (host mapping: include/sbx.h)
        "APP_CLOUDS_SKY": APP_CLOUDS_SKY,      # APP_CLOUDS + SKY_SPHERE (src/app_clouds.h:8,14-19,154-162)
        "APP_VINYL_GPU": APP_VINYL_GPU,        # APP_VINYL with the 180 march steps of its GLSL / HLSL builds (src/app_vinyl.h:411-416)
        "APP_PLANET_ATMOSPHERE": APP_PLANET_ATMOSPHERE,   # config 5's composite: APP_PLANET with APP_ATMOSPHERE's sky as background (include/sbx.h)
        "APP_2D": APP_2D,                      # src/app_2d.h, the tunnel / road UV demo (own mainImage; alpha is not 1, include/sbx.h)
        "APP_2D_TEX": APP_2D_TEX,              # APP_2D + USE_TEXTURE (src/app_2d.h:3-30): sample() reads t0 (Renderer.set_texture2d)
        "APP_FUNC": APP_FUNC,                  # src/app_func.h's 2D branch, the tiled Worley fBm (own mainImage; alpha 1, include/sbx.h)
        "APP_ATMOSPHERE_GROUND": APP_ATMOSPHERE_GROUND,   # APP_ATMOSPHERE without FROM_SPACE: the camera 1 m above the ground (include/sbx.h)
        "APP_SDF_AO_SHADOW": APP_SDF_AO_SHADOW,    # APP_SDF_AO with the soft-shadow march compiled in (src/app_sdf_ao.h:269-274, 183-207)
        "APP_SDF_AO_NORMALS": APP_SDF_AO_NORMALS}  # APP_SDF_AO with the normals view compiled in (src/app_sdf_ao.h:217-219)
# The apps appended after those.  A table of its own: tests/test_sdf_ao_builds_cpu.py pins APPS to the nineteen values above, so APPS
# stays what it was; app_id() and every entry point that takes a name look in both tables, ALL_APPS is their union.
MORE_APPS = {"APP_EGG_STRAIGHT": APP_EGG_STRAIGHT,  # APP_EGG without `#define BEZIER`: four cylinder legs (src/app_egg.h:37, 86-109)
             "APP_EGG_OVAL": APP_EGG_OVAL,          # APP_EGG with the `#if 1` at src/app_egg.h:46 off: the one scaled sphere (:53-66)
             "APP_CLOUDS_HEIGHT": APP_CLOUDS_HEIGHT,        # APP_CLOUDS with the `#if 0` at src/app_clouds.h:97 on: lit by height, no light march
             "APP_CLOUDS_LUMINANCE": APP_CLOUDS_LUMINANCE,  # APP_CLOUDS with the `#if 0` at src/app_clouds.h:118 on: the light march's transmittance
             "APP_RAYTRACER_PHONG": APP_RAYTRACER_PHONG,        # APP_RAYTRACER with the `#if 0` at src/app_raytracer.h:61 on: illum_blinn_phong (Phong specular)
             "APP_RAYTRACER_NOSHADOW": APP_RAYTRACER_NOSHADOW,  # APP_RAYTRACER with the `#if 1` at src/app_raytracer.h:107 off: no shadow ray
             "APP_RAYTRACER_STATIC": APP_RAYTRACER_STATIC,      # APP_RAYTRACER with the `#if 1` at src/app_raytracer.h:29 off: the Cornell box at rest
             "APP_VINYL_CLOSEUP": APP_VINYL_CLOSEUP,    # APP_VINYL with the `#if 1` at src/app_vinyl.h:60 off: the close-up camera of :64-65
             "APP_VINYL_RIDGES": APP_VINYL_RIDGES,      # APP_VINYL with the `#if 0` at src/app_vinyl.h:357 on: the ridge of label and logo
             "APP_VINYL_NOSHADOW": APP_VINYL_NOSHADOW,  # APP_VINYL with the `#if 1` at src/app_vinyl.h:445 off: no sdf_shadow march
             "APP_PLANET_CLOSEUP": APP_PLANET_CLOSEUP,      # APP_PLANET with the `#if 0` at src/app_planet.h:51 on: the camera of :52-53
             "APP_PLANET_CLOUDLESS": APP_PLANET_CLOUDLESS,  # APP_PLANET without the `#define CLOUDS` of src/app_planet.h:63: no cloud march, no cloud shadow
             "APP_PLANET_UNLIT": APP_PLANET_UNLIT,          # APP_PLANET without the `#define LIGHT` of src/app_planet.h:249: N = w_normal.y, ocean = water
             "APP_RAYTRACER_SCENE": APP_RAYTRACER_SCENE,    # src/app_raytracer.h's render over the caller's scene: aux = a RaytracerScene (cornell_scene, raytracer_scene)
             "APP_ATMOSPHERE_AIR": APP_ATMOSPHERE_AIR,      # src/app_atmosphere.h over the caller's air (coefficients, scale heights, radii, sun, counts, observer; view 0 = the sky dome, 1 = the ground camera): aux = an AtmosphereAir (atmosphere_air_default, atmosphere_air)
             "APP_PLANET_WORLD": APP_PLANET_WORLD,          # src/app_planet.h as shipped over the caller's world (camera, tilt and spins, sun and key light, max_height, noise offsets, cloud cover, colours, limits, step counts): aux = a PlanetWorld (planet_world_default, planet_world)
             "APP_VINYL_DECK": APP_VINYL_DECK,              # src/app_vinyl.h as shipped over the caller's deck (platter angle, tilts, sun, colours, groove BRDF): aux = a VinylDeck (vinyl_deck_default, vinyl_deck)
             "APP_EGG_POSE": APP_EGG_POSE,                  # src/app_egg.h as shipped with the rider posed by the caller (src/IK.h at work): aux = an EggPose (egg_pose_default, egg_pose)
             "APP_SDF_SCENE": APP_SDF_SCENE}                # src/app_sdf_ao.h's renderer over the caller's field, a program of src/sdf.h's primitives and operators: aux = an SdfScene (sdf_ramp_scene, SdfSceneBuilder)
ALL_APPS = {**APPS, **MORE_APPS}

SBX_OK, SBX_ERR_ARG, SBX_ERR_UNSUPPORTED, SBX_ERR_HIP, SBX_ERR_NO_DEVICE, SBX_ERR_FAULT = 0, -1, -2, -3, -4, -5
SBX_FORMAT_RGBA32F, SBX_FORMAT_RGBA8 = 0, 1
SBX_ABI_VERSION = 2                          # include/sbx.h; load_library() refuses a libsbx.so built from another header


class SbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libsbx error %d: %s" % (code, msg))
        self.code = code


class Uniforms(ctypes.Structure):           # sbx_uniforms (cbuffer b0)
    _fields_ = [("u_res", ctypes.c_float * 2), ("u_mouse", ctypes.c_float * 2), ("u_time", ctypes.c_float),
                ("_pad", ctypes.c_float * 3)]


class AuxClouds(ctypes.Structure):          # sbx_aux_clouds (cbuffer b1, APP_CLOUDS)
    _fields_ = [("wind_dir", ctypes.c_float * 3), ("_pad0", ctypes.c_float),
                ("sun_dir", ctypes.c_float * 3), ("_pad1", ctypes.c_float),
                ("sun_color", ctypes.c_float * 3), ("_pad2", ctypes.c_float),
                ("sun_power", ctypes.c_float), ("cld_march_steps", ctypes.c_int32),
                ("illum_march_steps", ctypes.c_int32), ("sigma_scattering", ctypes.c_float),
                ("cld_coverage", ctypes.c_float), ("cld_thick", ctypes.c_float),
                ("atm_radius", ctypes.c_float), ("atm_ground_y", ctypes.c_float)]


class CloudsSelection(ctypes.Structure):    # sbx_clouds_selection (include/sbx_test.h): the kernel a launch of APP_CLOUDS took
    _fields_ = [(n, ctypes.c_int) for n in ("build", "perlane", "ytab_used", "reg", "lm", "sm", "gt", "ytab", "sky", "regular", "exp_small",
                                            "index_domain", "div3_domain", "lip_ok", "light", "need_range", "table_range", "vt")] + \
               [("launches", ctypes.c_uint64)]

    def as_dict(self):
        # (`vt`, the view-table instantiation, is reported by Renderer.clouds_viewtab and clouds_select(view_table=True): the records
        #  the selection cases compare are these fields)
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "vt"}


class AuxCloudsUe4(ctypes.Structure):       # sbx_aux_clouds_ue4
    _fields_ = [("coverage", ctypes.c_float), ("thickness", ctypes.c_float), ("absorbtion", ctypes.c_float),
                ("fuzziness", ctypes.c_float), ("sun_dir", ctypes.c_float * 3), ("_pad1", ctypes.c_float),
                ("wind_dir", ctypes.c_float * 3), ("use_dirs", ctypes.c_int32)]


class AuxSdfAo(ctypes.Structure):           # sbx_aux_sdf_ao (cbuffer b1, APP_SDF_AO)
    _fields_ = [("fog_density", ctypes.c_float), ("fog_falloff", ctypes.c_float), ("_pad", ctypes.c_float * 2)]


class RtMaterial(ctypes.Structure):         # sbx_rt_material (material.h:5-12)
    _fields_ = [("base_color", ctypes.c_float * 3), ("metallic", ctypes.c_float), ("roughness", ctypes.c_float),
                ("ior", ctypes.c_float), ("reflectivity", ctypes.c_float), ("translucency", ctypes.c_float)]


class RtPlane(ctypes.Structure):            # sbx_rt_plane
    _fields_ = [("direction", ctypes.c_float * 3), ("distance", ctypes.c_float), ("material", ctypes.c_int32),
                ("_pad", ctypes.c_int32 * 3)]


class RtSphere(ctypes.Structure):           # sbx_rt_sphere
    _fields_ = [("origin", ctypes.c_float * 3), ("radius", ctypes.c_float), ("material", ctypes.c_int32),
                ("_pad", ctypes.c_int32 * 3)]


RT_MAX_PLANES = RT_MAX_SPHERES = 16          # SBX_RT_MAX_PLANES, SBX_RT_MAX_SPHERES
LIGHT_POINT, LIGHT_DIR = 1, 2                # light.h:5-6
LIGHTING_COOK_TORRANCE, LIGHTING_PHONG = 0, 1


class RaytracerScene(ctypes.Structure):     # sbx_aux_raytracer_scene (the aux block of APP_RAYTRACER_SCENE, 1376 bytes)
    _fields_ = [("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("bounces", ctypes.c_int32),
                ("light_L", ctypes.c_float * 3), ("light_type", ctypes.c_int32),
                ("light_color", ctypes.c_float * 3), ("lighting", ctypes.c_int32),
                ("ambient", ctypes.c_float * 3), ("shadow", ctypes.c_int32),
                ("n_planes", ctypes.c_int32), ("n_spheres", ctypes.c_int32), ("_pad", ctypes.c_int32 * 2),
                ("materials", RtMaterial * 8), ("planes", RtPlane * RT_MAX_PLANES), ("spheres", RtSphere * RT_MAX_SPHERES)]


class EggPose(ctypes.Structure):            # sbx_aux_egg_pose (the aux block of APP_EGG_POSE and the pose of egg_eval, 64 bytes)
    _fields_ = [("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("turn_deg", ctypes.c_float),
                ("left_foot", ctypes.c_float * 3), ("femur", ctypes.c_float),
                ("right_foot", ctypes.c_float * 3), ("tibia", ctypes.c_float)]


class AtmosphereAir(ctypes.Structure):      # sbx_aux_atmosphere_air (the aux block of APP_ATMOSPHERE_AIR and the air of atmosphere_air_eval, 128 bytes)
    _fields_ = [("view", ctypes.c_int), ("num_samples", ctypes.c_int), ("num_samples_light", ctypes.c_int), ("reserved0", ctypes.c_int),
                ("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("hg_g", ctypes.c_float),
                ("sun_dir", ctypes.c_float * 3), ("sun_power", ctypes.c_float),
                ("betaR", ctypes.c_float * 3), ("hR", ctypes.c_float),
                ("betaM", ctypes.c_float * 3), ("hM", ctypes.c_float),
                ("earth_radius", ctypes.c_float), ("atmosphere_radius", ctypes.c_float),
                ("reserved", ctypes.c_float * 6)]


class PlanetWorld(ctypes.Structure):        # sbx_aux_planet_world (the aux block of APP_PLANET_WORLD, 224 bytes)
    _fields_ = [("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("tilt_deg", ctypes.c_float),
                ("sun_dir", ctypes.c_float * 3), ("spin_deg", ctypes.c_float),
                ("key_color", ctypes.c_float * 3), ("cloud_spin_deg", ctypes.c_float),
                ("terrain_offset", ctypes.c_float * 3), ("max_height", ctypes.c_float),
                ("cloud_offset", ctypes.c_float * 3), ("cld_coverage", ctypes.c_float),
                ("band", ctypes.c_float * 3), ("cld_fuzzy", ctypes.c_float),
                ("c_water", ctypes.c_float * 3), ("l_water", ctypes.c_float),
                ("c_grass", ctypes.c_float * 3), ("l_shore", ctypes.c_float),
                ("c_beach", ctypes.c_float * 3), ("l_grass", ctypes.c_float),
                ("c_rock", ctypes.c_float * 3), ("l_rock", ctypes.c_float),
                ("c_snow", ctypes.c_float * 3), ("absorb", ctypes.c_float),
                ("cloud_light", ctypes.c_float),
                ("terr_steps", ctypes.c_int), ("cloud_steps", ctypes.c_int), ("shadow_steps", ctypes.c_int),
                ("reserved", ctypes.c_uint * 4)]


class VinylDeck(ctypes.Structure):          # sbx_aux_vinyl_deck (the aux block of APP_VINYL_DECK and the deck of vinyl_eval, 128 bytes)
    _fields_ = [("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("platter_deg", ctypes.c_float),
                ("sun_dir", ctypes.c_float * 3), ("platter_tilt_deg", ctypes.c_float),
                ("groove_color", ctypes.c_float * 3), ("arm_tilt_deg", ctypes.c_float),
                ("dead_wax_color", ctypes.c_float * 3), ("ro_spec", ctypes.c_float),
                ("label_color", ctypes.c_float * 3), ("a_x", ctypes.c_float),
                ("logo_color", ctypes.c_float * 3), ("a_y", ctypes.c_float),
                ("shiny_color", ctypes.c_float * 3), ("shininess", ctypes.c_float)]


SDF_MAX_INSTR, SDF_MAX_STACK = 32, 4         # SBX_SDF_MAX_INSTR, SBX_SDF_MAX_STACK
SDF_PLANE, SDF_SPHERE, SDF_BOX, SDF_TORUS, SDF_Y_CYLINDER, SDF_CYLINDER, SDF_CAPSULE, SDF_BEZIER = range(1, 9)
SDF_ADD, SDF_SUB, SDF_INTERSECT, SDF_BLEND = range(16, 20)
SDF_OBJECT = 32


class SdfInstr(ctypes.Structure):           # sbx_sdf_instr, 80 bytes
    _fields_ = [("op", ctypes.c_int32), ("rot_axis", ctypes.c_int32), ("rot_deg", ctypes.c_float), ("material", ctypes.c_int32),
                ("offset", ctypes.c_float * 3), ("_pad", ctypes.c_float),
                ("a", ctypes.c_float * 4), ("b", ctypes.c_float * 4), ("c", ctypes.c_float * 4)]


class SdfScene(ctypes.Structure):           # sbx_aux_sdf_scene (the aux block of APP_SDF_SCENE, 2784 bytes)
    _fields_ = [("eye", ctypes.c_float * 3), ("fov", ctypes.c_float),
                ("look_at", ctypes.c_float * 3), ("march_steps", ctypes.c_int32),
                ("sun_dir", ctypes.c_float * 3), ("march_end", ctypes.c_float),
                ("background", ctypes.c_float * 3), ("shadow", ctypes.c_int32),
                ("fog_density", ctypes.c_float), ("fog_falloff", ctypes.c_float), ("view", ctypes.c_int32), ("checker_material", ctypes.c_int32),
                ("n_instr", ctypes.c_int32), ("_pad", ctypes.c_int32 * 3),
                ("materials", (ctypes.c_float * 4) * 8),
                ("program", SdfInstr * SDF_MAX_INSTR)]


assert ctypes.sizeof(SdfInstr) == 80 and ctypes.sizeof(SdfScene) == 2784 and SdfScene.program.offset == 224 and SdfScene.materials.offset == 96


def sdf_scene_check(scene, program_only=False):
    """The refusals of include/sbx.h for an SdfScene, on the host and in the C side's order: None if the block would be accepted,
    else a sentence saying what is wrong.  program_only: what sbx_sdf_eval checks (n_instr and the program)."""
    if not 1 <= scene.n_instr <= SDF_MAX_INSTR:
        return "n_instr must lie in 1..32"
    if not program_only:
        if not -1 <= scene.checker_material <= 7:
            return "checker_material must lie in -1..7"
        if not 1 <= scene.march_steps <= 512:
            return "march_steps must lie in 1..512"
        if scene.shadow not in (0, 1):
            return "shadow must be 0 or 1"
        if scene.view not in (0, 1):
            return "view must be 0 or 1"
    depth = 0
    for i in range(scene.n_instr):
        I = scene.program[i]
        prim, oper = SDF_PLANE <= I.op <= SDF_BEZIER, SDF_ADD <= I.op <= SDF_BLEND
        if not (prim or oper or I.op == SDF_OBJECT):
            return "unknown op"
        if not 0 <= I.rot_axis <= 3:
            return "rot_axis must lie in 0..3"
        if prim:
            depth += 1
            if depth > SDF_MAX_STACK:
                return "the stack exceeds SDF_MAX_STACK"
        elif oper:
            if depth < 2:
                return "the stack underflows at an operator"
            depth -= 1
        else:
            if not 0 <= I.material <= 7:
                return "an OBJECT's material must lie in 0..7"
            if depth < 1:
                return "the stack underflows at an OBJECT"
            depth -= 1
            if depth:
                return "the stack is not empty at an OBJECT after its pop"
    if scene.program[scene.n_instr - 1].op != SDF_OBJECT:
        return "the last instruction must be an OBJECT"
    return None


class SdfSceneBuilder:
    """Appends instructions to an SdfScene (the aux block of APP_SDF_SCENE; include/sbx.h has the semantics) and checks the block on
    the host the way the C side does.  Starts from sdf_ramp_scene's renderer settings with an empty program:

        b = SdfSceneBuilder(eye=(0, 3, 5))
        b.box((0, 1, 0), (1, 1, 1)).sphere((0, 1.5, 0), .8).sub().object(2)        # postfix: box, sphere, box minus sphere
        b.plane((0, 1, 0), 0).object(1)
        frame = renderer.render("sdf_scene", w, h, 0, aux=b.scene())

    Every primitive takes offset=, rot_axis= (0 none, 1 x, 2 y, 3 z) and rot_deg=.  scene() raises ValueError where the block would be
    refused."""

    def __init__(self, **settings):
        s = self.s = SdfScene()
        s.eye[:], s.look_at[:], s.fov = (0.0, 3.0, 5.0), (0.0, 0.0, 0.0), 1.0
        s.march_steps, s.march_end = 70, 20.0
        s.sun_dir[:] = (0.40824828, 0.81649655, 0.40824828)
        s.background[:] = (0.1, 0.1, 0.7)
        s.fog_density, s.fog_falloff, s.checker_material = 0.1, 0.5, 1
        for i, m in enumerate(((1, 1, 1), (0, .2, 0), (.1, .1, .1), (.1, .1, .1), (.1, .1, .1), (.4, .4, .4))):
            s.materials[i][:3] = m
        self.set(**settings)

    def set(self, **settings):
        for k, v in settings.items():
            if k == "materials":
                for i, m in (v.items() if hasattr(v, "items") else enumerate(v)):
                    self.s.materials[int(i)][:3] = [float(x) for x in m]
            elif k in ("eye", "look_at", "sun_dir", "background"):
                getattr(self.s, k)[:] = [float(x) for x in v]
            elif k in ("fov", "march_end", "fog_density", "fog_falloff"):
                setattr(self.s, k, float(v))
            elif k in ("march_steps", "shadow", "view", "checker_material"):
                setattr(self.s, k, int(v))
            else:
                raise ValueError("unknown setting %r" % k)
        return self

    def _add(self, op, offset=(0, 0, 0), a=(), b=(), c=(), rot_axis=0, rot_deg=0.0, material=0):
        if self.s.n_instr >= SDF_MAX_INSTR:
            raise ValueError("a program holds at most %d instructions" % SDF_MAX_INSTR)
        I = self.s.program[self.s.n_instr]
        I.op, I.rot_axis, I.rot_deg, I.material = int(op), int(rot_axis), float(rot_deg), int(material)
        I.offset[:] = [float(x) for x in offset]
        for dst, src in ((I.a, a), (I.b, b), (I.c, c)):
            dst[:] = [float(x) for x in tuple(src) + (0.0,) * (4 - len(tuple(src)))]
        self.s.n_instr += 1
        return self

    def plane(self, normal, d, **kw):
        return self._add(SDF_PLANE, a=tuple(normal) + (d,), **kw)

    def sphere(self, offset, r, **kw):
        return self._add(SDF_SPHERE, offset, (r,), **kw)

    def box(self, offset, half, **kw):
        return self._add(SDF_BOX, offset, tuple(half), **kw)

    def torus(self, offset, R, r, **kw):
        return self._add(SDF_TORUS, offset, (R, r), **kw)

    def y_cylinder(self, offset, r, h, **kw):
        return self._add(SDF_Y_CYLINDER, offset, (r, h), **kw)

    def cylinder(self, offset, p0, p1, r, **kw):
        return self._add(SDF_CYLINDER, offset, tuple(p0) + (r,), tuple(p1), **kw)

    def capsule(self, offset, a, b, r, **kw):
        return self._add(SDF_CAPSULE, offset, tuple(a) + (r,), tuple(b), **kw)

    def bezier(self, offset, a, b, c, thickness, **kw):
        return self._add(SDF_BEZIER, offset, tuple(a) + (thickness,), tuple(b), tuple(c), **kw)

    def add(self):
        return self._add(SDF_ADD)

    def sub(self):
        return self._add(SDF_SUB)

    def intersect(self):
        return self._add(SDF_INTERSECT)

    def blend(self, k):
        return self._add(SDF_BLEND, a=(k,))

    def object(self, material):
        return self._add(SDF_OBJECT, material=material)

    def check(self, program_only=False):
        return sdf_scene_check(self.s, program_only)

    def scene(self):
        why = self.check()
        if why:
            raise ValueError("sdf scene: " + why)
        return SdfScene.from_buffer_copy(self.s)


class Stats(ctypes.Structure):              # sbx_stats
    _fields_ = [("render_launches", ctypes.c_uint64), ("main_image_hits", ctypes.c_uint64),
                ("main_image_frames", ctypes.c_uint64), ("main_image_points", ctypes.c_uint64),
                ("_reserved", ctypes.c_uint64 * 4)]


class SharedHandle(ctypes.Structure):       # sbx_shared_handle
    _fields_ = [("opaque", ctypes.c_ubyte * 192)]


def app_id(app):
    """Accepts an int, 'APP_CLOUDS', 'clouds', ..."""
    if isinstance(app, int):
        return app
    key = str(app).upper()
    if not key.startswith("APP_"):
        key = "APP_" + key
    if key not in ALL_APPS:
        raise ValueError("unknown app %r" % (app,))
    return ALL_APPS[key]


def load_library(path=None):
    """dlopen libsbx.so and declare the prototypes of include/sbx.h.  Raises if it is not built."""
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError("libsbx.so is not built (%s). Run `python -m shaderbox_amd.build`; "
                          "there is no fallback path." % path)
    # Load order matters: PyTorch brings its own copy of the HIP runtime.  If libsbx.so (linked against the system
    # libamdhip64) is loaded first and torch afterwards, the process ends up with two runtimes and device enumeration
    # fails (observed: sbx_create -> SBX_ERR_NO_DEVICE on a GPU box).  torch is this package's device-memory/stream
    # provider anyway, so import it before the dlopen whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    vp, ci, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    try:
        lib.sbx_abi_version.argtypes = []
        got = int(lib.sbx_abi_version())
    except AttributeError:
        got = 1                              # (libraries before ABI 2 do not export the function)
    if got != SBX_ABI_VERSION:
        raise ImportError("%s has ABI %d, this package binds ABI %d (include/sbx.h): rebuild with `python -m shaderbox_amd.build`"
                          % (path, got, SBX_ABI_VERSION))
    lib.sbx_aux_clouds_defaults.argtypes = [ctypes.POINTER(AuxClouds)]
    lib.sbx_aux_clouds_defaults.restype = None
    lib.sbx_aux_sdf_ao_defaults.argtypes = [ctypes.POINTER(AuxSdfAo)]
    lib.sbx_aux_sdf_ao_defaults.restype = None
    lib.sbx_aux_clouds_ue4_defaults.argtypes = [ctypes.POINTER(AuxCloudsUe4)]
    lib.sbx_aux_clouds_ue4_defaults.restype = None
    lib.sbx_raytracer_scene_cornell.argtypes = [ctypes.POINTER(Uniforms), ci, ctypes.POINTER(RaytracerScene)]
    lib.sbx_raytracer_scene_cornell.restype = None
    lib.sbx_sdf_scene_ramp.argtypes = [ctypes.POINTER(Uniforms), ctypes.POINTER(SdfScene)]
    lib.sbx_sdf_scene_ramp.restype = None
    lib.sbx_sdf_eval.argtypes = [vp, ctypes.POINTER(SdfScene), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_sdf_scene_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(SdfScene), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_sdf_scene_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(SdfScene), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_egg_pose_default.argtypes = [ctypes.POINTER(Uniforms), ctypes.POINTER(EggPose)]
    lib.sbx_egg_pose_default.restype = None
    lib.sbx_egg_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(EggPose), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_egg_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(EggPose), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_atmosphere_air_default.argtypes = [ctypes.POINTER(Uniforms), ci, ctypes.POINTER(AtmosphereAir)]
    lib.sbx_atmosphere_air_default.restype = None
    lib.sbx_atmosphere_air_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(AtmosphereAir), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_atmosphere_air_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(AtmosphereAir), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_debug_atmosphere_air_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbx_planet_world_default.argtypes = [ctypes.POINTER(Uniforms), ctypes.POINTER(PlanetWorld)]
    lib.sbx_planet_world_default.restype = None
    lib.sbx_debug_planet_world_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbx_planet_world_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(PlanetWorld), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_planet_world_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(PlanetWorld), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_vinyl_deck_default.argtypes = [ctypes.POINTER(Uniforms), ctypes.POINTER(VinylDeck)]
    lib.sbx_vinyl_deck_default.restype = None
    lib.sbx_vinyl_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(VinylDeck), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_vinyl_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(VinylDeck), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_debug_vinyl_deck_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbx_raytracer_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(RaytracerScene), fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_raytracer_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(RaytracerScene), fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_debug_egg_pose_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbx_debug_raytracer_scene_launches.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.sbx_create.argtypes = [ci, ctypes.POINTER(vp)]
    lib.sbx_destroy.argtypes = [vp]
    lib.sbx_destroy.restype = None
    lib.sbx_render_rows.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, fp, vp]
    lib.sbx_render_rows_host.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, vp, vp]
    lib.sbx_render_rank.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, fp, vp]
    lib.sbx_pack_unorm8.argtypes = [vp, ci, ci, fp, vp, ci, vp]
    lib.sbx_set_output_format.argtypes = [vp, ci]
    lib.sbx_main_image.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ctypes.POINTER(ctypes.c_float * 2),
                                   ctypes.POINTER(ctypes.c_float * 4)]
    lib.sbx_main_image_batch.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ctypes.c_size_t, fp, fp]
    lib.sbx_render_points.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ctypes.c_size_t, fp, fp, vp]
    lib.sbx_render_rank_rows.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_rank_rows.argtypes = [ci, ci, ci, ci]
    lib.sbx_rank_rows_max.argtypes = [ci, ci, ci]
    lib.sbx_assemble.argtypes = [vp, ci, ci, ci, ci, fp, fp, vp]
    lib.sbx_split_rank_rows.argtypes = [ci, ci, ci, ci, ci, ci]
    lib.sbx_split_rows_max.argtypes = [ci, ci, ci, ci, ci]
    lib.sbx_render_split.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_assemble_split.argtypes = [vp, ci, ci, ci, ci, ci, ci, fp, fp, vp]
    lib.sbx_render_split_rgb.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_assemble_peers.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, fp, fp, vp]
    lib.sbx_span_table.argtypes = [ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, vp, vp, vp]
    lib.sbx_render_span_peer.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_render_span_root.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, fp, vp]
    lib.sbx_assemble_spans.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, fp, ctypes.c_int64, fp, vp]
    lib.sbx_fault_status.argtypes = [vp]
    lib.sbx_clear_fault.argtypes = [vp]
    lib.sbx_debug_raise_fault.argtypes = [vp, vp]
    lib.sbx_set_timing.argtypes = [vp, ci]
    lib.sbx_set_variant.argtypes = [vp, ci]
    lib.sbx_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.sbx_math_eval.argtypes = [vp, ctypes.c_char_p, fp, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_noise_eval.argtypes = [vp, ctypes.c_char_p, fp, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_atmosphere_eval.argtypes = [vp, ctypes.c_char_p, fp, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_atmosphere_eval.argtypes = [vp, ctypes.c_char_p, fp, fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_clouds_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(AuxClouds), ctypes.c_float, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_clouds_eval.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(AuxClouds), ctypes.c_float, fp, fp, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_uint64), vp]
    lib.sbx_planet_eval.argtypes = [vp, ctypes.c_char_p, ctypes.c_float, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_debug_planet_eval.argtypes = [vp, ctypes.c_char_p, ctypes.c_float, fp, fp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), vp]
    lib.sbx_worley_volume.argtypes = [vp, ci, fp, vp]
    lib.sbx_render_split_in_place.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_multi_create.argtypes = [ci, ctypes.POINTER(ci), ctypes.POINTER(vp)]
    lib.sbx_multi_destroy.argtypes = [vp]
    lib.sbx_multi_destroy.restype = None
    lib.sbx_multi_ranks.argtypes = [vp]
    lib.sbx_multi_uses_rccl.argtypes = [vp]
    lib.sbx_multi_set_split.argtypes = [vp, ci, ci, ci]
    lib.sbx_multi_set_variant.argtypes = [vp, ci]
    lib.sbx_multi_set_output_format.argtypes = [vp, ci]
    lib.sbx_multi_set_exchange.argtypes = [vp, ci]
    lib.sbx_multi_create_error.argtypes = []
    lib.sbx_multi_create_error.restype = ctypes.c_char_p
    lib.sbx_multi_set_noise_volumes.argtypes = [vp, ci, fp, ci, fp]
    lib.sbx_multi_render.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, fp, vp]
    lib.sbx_multi_rccl_selftest.argtypes = [ci, ctypes.POINTER(ci)]
    lib.sbx_multi_last_error.argtypes = [vp]
    lib.sbx_multi_last_error.restype = ctypes.c_char_p
    lib.sbx_set_noise_volumes.argtypes = [vp, ci, fp, ci, fp, vp]
    lib.sbx_set_texture2d.argtypes = [vp, ci, ci, ci, vp, vp]
    lib.sbx_checkerboard_texture.argtypes = [ci, ci, vp]
    lib.sbx_checkerboard_texture.restype = None
    lib.sbx_tex3d_eval.argtypes = [vp, ci, fp, fp, fp, ctypes.c_size_t, vp]
    lib.sbx_last_error.argtypes = [vp]
    lib.sbx_last_error.restype = ctypes.c_char_p
    lib.sbx_version.restype = ctypes.c_char_p
    lib.sbx_set_precision.argtypes = [vp, ci]
    lib.sbx_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.sbx_reset_stats.argtypes = [vp]
    # the store exchange (include/sbx.h sbx_shared_*)
    lib.sbx_shared_create.argtypes = [vp, ctypes.c_size_t, ci, ctypes.POINTER(vp)]
    lib.sbx_shared_export.argtypes = [vp, ctypes.POINTER(SharedHandle)]
    lib.sbx_shared_open.argtypes = [vp, ctypes.POINTER(SharedHandle), ctypes.POINTER(vp)]
    lib.sbx_shared_close.argtypes = [vp]
    lib.sbx_shared_close.restype = None
    lib.sbx_shared_frame.argtypes = [vp]
    lib.sbx_shared_frame.restype = vp
    lib.sbx_debug_tile_order.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint),
                                         ctypes.c_size_t]
    lib.sbx_debug_order_build.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.sbx_debug_clouds_hashtab.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int)] * 4
    lib.sbx_debug_clouds_hashtab_read.argtypes = [vp, ctypes.c_size_t, ctypes.c_size_t, vp]
    lib.sbx_debug_clouds_last_selection.argtypes = [vp, ctypes.POINTER(CloudsSelection)]
    lib.sbx_debug_clouds_select.argtypes = [ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ctypes.POINTER(CloudsSelection)]
    lib.sbx_debug_clouds_select_vt.argtypes = [ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, ctypes.POINTER(CloudsSelection)]
    lib.sbx_debug_clouds_viewtab.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)] + [ctypes.POINTER(ctypes.c_int)] * 3
    lib.sbx_debug_set_clouds_viewtab_cap.argtypes = [vp, ctypes.c_size_t]
    lib.sbx_debug_clouds_viewtab_key.argtypes = [ci, ctypes.POINTER(Uniforms), vp, vp, ci]
    lib.sbx_shared_bytes.argtypes = [vp]
    lib.sbx_shared_bytes.restype = ctypes.c_size_t
    lib.sbx_shared_frame_begin.argtypes = [vp, ci, vp]
    lib.sbx_shared_frame_end.argtypes = [vp, ci, vp]
    lib.sbx_render_split_in_place_rgb.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, fp, vp]
    lib.sbx_render_span_peer_in_place.argtypes = [vp, ci, ctypes.POINTER(Uniforms), vp, ci, ci, ci, ci, ci, ci, fp, vp]
    # include/sbx_test.h (test hooks and the landing model of the scaling tools)
    lib.sbx_shared_set_timeout_ms.argtypes = [vp, ci]
    lib.sbx_model_landing.argtypes = [vp, vp, vp, ctypes.c_size_t, ci, ctypes.c_float, vp]
    return lib


def clouds_defaults(lib=None):
    lib = lib or load_library()
    a = AuxClouds()
    lib.sbx_aux_clouds_defaults(ctypes.byref(a))
    return a


def sdf_ao_defaults(lib=None):
    lib = lib or load_library()
    a = AuxSdfAo()
    lib.sbx_aux_sdf_ao_defaults(ctypes.byref(a))
    return a


def cornell_scene(width, height, time, mouse=(0.0, 0.0), at_rest=False, lib=None):
    """sbx_raytracer_scene_cornell (host only, no GPU needed): the RaytracerScene that src/app_raytracer.h's setup_scene, setup_camera
    and FOV make of these uniforms — what APP_RAYTRACER_SCENE renders when aux is None.  at_rest: the `#if 1` of :29 off, `time`
    is not read."""
    lib = lib or load_library()
    u = uniforms(width, height, time, mouse)
    a = RaytracerScene()
    lib.sbx_raytracer_scene_cornell(ctypes.byref(u), 1 if at_rest else 0, ctypes.byref(a))
    return a


def raytracer_scene(planes=(), spheres=(), materials=(), light=(0.0, 3.8, 1.5), eye=(0.0, 2.0, 4.666), look_at=(0.0, 2.0, 0.0),
                    fov=0.57735026, bounces=2, light_type=LIGHT_POINT, lighting=LIGHTING_COOK_TORRANCE, shadow=True,
                    ambient=(0.01, 0.01, 0.01), light_color=(1.0, 1.0, 1.0)):
    """A RaytracerScene (the aux block of APP_RAYTRACER_SCENE) from plain Python values; the counts are filled from the lists.
        planes     [(direction xyz, distance, material id)]            at most 16; used as given, never normalised
        spheres    [(origin xyz, radius, material id)]                 at most 16; material 0 = the light bulb (flat, casts no shadow)
        materials  {id: dict(base_color=.., roughness=.., ior=.., reflectivity=.., metallic=.., translucency=..)} or a list of
                   such dicts for the ids 0, 1, ...; missing fields default to base_color (0, 0, 0), roughness .5, ior 1, the others 0;
                   slots not given stay zero
        light      lights[0].L: the position (LIGHT_POINT) or the direction to the light (LIGHT_DIR), used as given
        fov        the FOV factor of main.h:45 (tan of half the vertical angle); the default is tan(30 degrees)
    Values outside the ranges of include/sbx.h are refused by the render call (SBX_ERR_ARG), not here."""
    if len(planes) > RT_MAX_PLANES or len(spheres) > RT_MAX_SPHERES:
        raise ValueError("a scene holds at most %d planes and %d spheres" % (RT_MAX_PLANES, RT_MAX_SPHERES))
    a = RaytracerScene()
    a.eye[:], a.look_at[:], a.light_L[:] = [float(v) for v in eye], [float(v) for v in look_at], [float(v) for v in light]
    a.light_color[:], a.ambient[:] = [float(v) for v in light_color], [float(v) for v in ambient]
    a.fov, a.bounces, a.light_type, a.lighting, a.shadow = float(fov), int(bounces), int(light_type), int(lighting), int(bool(shadow))
    a.n_planes, a.n_spheres = len(planes), len(spheres)
    items = materials.items() if hasattr(materials, "items") else enumerate(materials)
    for i, m in items:
        if not 0 <= int(i) < 8:
            raise ValueError("material ids are 0..7")
        s = a.materials[int(i)]
        s.base_color[:] = [float(v) for v in m.get("base_color", (0.0, 0.0, 0.0))]
        s.roughness, s.ior = float(m.get("roughness", 0.5)), float(m.get("ior", 1.0))
        s.reflectivity, s.metallic, s.translucency = float(m.get("reflectivity", 0.0)), float(m.get("metallic", 0.0)), float(m.get("translucency", 0.0))
    for i, (n, d, mat) in enumerate(planes):
        a.planes[i].direction[:], a.planes[i].distance, a.planes[i].material = [float(v) for v in n], float(d), int(mat)
    for i, (o, r, mat) in enumerate(spheres):
        a.spheres[i].origin[:], a.spheres[i].radius, a.spheres[i].material = [float(v) for v in o], float(r), int(mat)
    return a


def sdf_ramp_scene(width, height, time, lib=None):
    """sbx_sdf_scene_ramp (host only, no GPU needed): the SdfScene that APP_SDF_SCENE renders when aux is None — app_sdf_ao.h's camera
    for `time`, its lights, materials and fog, and one ramp of its sdf_pipe plus the ground as a 20-instruction program."""
    lib = lib or load_library()
    u = uniforms(width, height, time)
    a = SdfScene()
    lib.sbx_sdf_scene_ramp(ctypes.byref(u), ctypes.byref(a))
    return a


def egg_pose_default(time, lib=None):
    """sbx_egg_pose_default (host only, no GPU needed): the EggPose that src/app_egg.h's setup_camera and sdf() make of `time` — what
    APP_EGG_POSE renders when aux is None, the frame of APP_EGG."""
    lib = lib or load_library()
    u = uniforms(1, 1, time)
    a = EggPose()
    lib.sbx_egg_pose_default(ctypes.byref(u), ctypes.byref(a))
    return a


def egg_pose(left_foot=(0.0, 1.5, 0.2), right_foot=(0.0, 0.9, -0.2), turn_deg=0.0, femur=0.8, tibia=0.75, eye=(0.0, 0.25, 5.25),
             look_at=(0.0, 0.25, 0.0), fov=1.0):
    """An EggPose (the aux block of APP_EGG_POSE, the pose of Renderer.egg_eval) from plain Python values, each rounded to binary32.
    The feet are left_foot_pos / right_foot_pos of src/app_egg.h:74, :77 (the pedals at u_time 0 are the defaults), turn_deg the angle
    of the turntable (:40), femur and tibia the bone lengths of the IK solver (:80-81), fov the FOV factor of main.h."""
    a = EggPose()
    a.eye[:], a.look_at[:] = [float(v) for v in eye], [float(v) for v in look_at]
    a.left_foot[:], a.right_foot[:] = [float(v) for v in left_foot], [float(v) for v in right_foot]
    a.fov, a.turn_deg, a.femur, a.tibia = float(fov), float(turn_deg), float(femur), float(tibia)
    return a


def atmosphere_air_default(time, view=0, lib=None):
    """sbx_atmosphere_air_default (host only, no GPU needed): the AtmosphereAir with the numbers of src/app_atmosphere.h and the sun its
    setup_scene makes of `time` — what APP_ATMOSPHERE_AIR renders when aux is None (view 0: APP_ATMOSPHERE's frame; view 1:
    APP_ATMOSPHERE_GROUND's)."""
    lib = lib or load_library()
    u = uniforms(1, 1, time)
    a = AtmosphereAir()
    lib.sbx_atmosphere_air_default(ctypes.byref(u), int(view), ctypes.byref(a))
    return a


def atmosphere_air(time=0.0, view=0, lib=None, **fields):
    """An AtmosphereAir: atmosphere_air_default(time, view) with the named fields of sbx_aux_atmosphere_air replaced, each float
    rounded to binary32."""
    a = atmosphere_air_default(time, view, lib)
    for name, value in fields.items():
        if name not in dict(AtmosphereAir._fields_):
            raise SbxError(SBX_ERR_ARG, "sbx_aux_atmosphere_air has no field %r" % (name,))
        if isinstance(getattr(a, name), int):
            setattr(a, name, int(value))
        elif isinstance(getattr(a, name), float):
            setattr(a, name, float(value))
        else:
            getattr(a, name)[:] = [float(v) for v in value]
    return a


def planet_world_default(time, lib=None):
    """sbx_planet_world_default (host only, no GPU needed): the PlanetWorld with the numbers of src/app_planet.h and the two spins it
    makes of `time` — what APP_PLANET_WORLD renders when aux is None, the frame of APP_PLANET."""
    lib = lib or load_library()
    u = uniforms(1, 1, time)
    a = PlanetWorld()
    lib.sbx_planet_world_default(ctypes.byref(u), ctypes.byref(a))
    return a


def planet_world(time=0.0, lib=None, **fields):
    """A PlanetWorld: planet_world_default(time) with the named fields of sbx_aux_planet_world replaced, each float rounded to
    binary32."""
    a = planet_world_default(time, lib)
    for name, value in fields.items():
        if name not in dict(PlanetWorld._fields_):
            raise SbxError(SBX_ERR_ARG, "sbx_aux_planet_world has no field %r" % (name,))
        if isinstance(getattr(a, name), int):
            setattr(a, name, int(value))
        elif isinstance(getattr(a, name), float):
            setattr(a, name, float(value))
        elif name == "reserved":
            getattr(a, name)[:] = [int(v) for v in value]
        else:
            getattr(a, name)[:] = [float(v) for v in value]
    return a


def vinyl_deck_default(time, lib=None):
    """sbx_vinyl_deck_default (host only, no GPU needed): the VinylDeck that src/app_vinyl.h makes of `time` — what APP_VINYL_DECK
    renders when aux is None, the frame of APP_VINYL."""
    lib = lib or load_library()
    u = uniforms(1, 1, time)
    a = VinylDeck()
    lib.sbx_vinyl_deck_default(ctypes.byref(u), ctypes.byref(a))
    return a


def vinyl_deck(time=0.0, lib=None, **fields):
    """A VinylDeck (the aux block of APP_VINYL_DECK, the deck of Renderer.vinyl_eval): vinyl_deck_default(time) with the named fields of
    sbx_aux_vinyl_deck replaced, each value rounded to binary32 — platter_deg=... over a frame sequence is the scratch."""
    a = vinyl_deck_default(time, lib)
    for name, value in fields.items():
        if name not in dict(VinylDeck._fields_):
            raise SbxError(SBX_ERR_ARG, "sbx_aux_vinyl_deck has no field %r" % (name,))
        if isinstance(getattr(a, name), float):
            setattr(a, name, float(value))
        else:
            getattr(a, name)[:] = [float(v) for v in value]
    return a


def checkerboard_texture(size=128, freq=16):
    """hlsltoy's t0 (CreateTextureCheckboard, util/hlsltoy/src/hlsltoy.cpp:66-87): a numpy uint32 array [size, size] of
    R8G8B8A8_UNORM words, ((x & freq) == (y & freq)) ? 0xff000000 : 0xffffffff.  The default texture of APP_2D_TEX is (128, 16).
    Pure Python; include/sbx.h's sbx_checkerboard_texture is the same rule in C."""
    import numpy as np
    i = np.arange(int(size), dtype=np.uint32)
    same = (i[None, :] & np.uint32(freq)) == (i[:, None] & np.uint32(freq))
    return np.where(same, np.uint32(0xff000000), np.uint32(0xffffffff)).astype(np.uint32)


def uniforms(width, height, time, mouse=(0.0, 0.0)):
    u = Uniforms()
    u.u_res[0], u.u_res[1] = float(width), float(height)
    u.u_mouse[0], u.u_mouse[1] = float(mouse[0]), float(mouse[1])
    u.u_time = float(time)
    return u


def clouds_select(app, width, height, time, mouse=(0.0, 0.0), aux=None, variant=0, ytab_rows=4096, table_range=0, point_list=False,
                  lib=None):
    """include/sbx_test.h sbx_debug_clouds_select (host only, no GPU needed): the kernel a launch of APP_CLOUDS, of its HEIGHT /
    LUMINANCE builds or of CLOUDS_SKY would take with a y table of `ytab_rows` rows and a ready hash table of range `table_range` at
    hand (0: none), as a dict of sbx_clouds_selection's fields"""
    lib = lib or load_library()
    u = uniforms(width, height, time, mouse)
    auxp = ctypes.cast(ctypes.byref(aux), ctypes.c_void_p) if aux is not None else None
    out = CloudsSelection()
    rc = lib.sbx_debug_clouds_select(app_id(app), ctypes.byref(u), auxp, int(variant), int(ytab_rows), int(table_range),
                                     1 if point_list else 0, ctypes.byref(out))
    if rc < 0:
        raise SbxError(rc, "sbx_debug_clouds_select: bad arguments")
    return out.as_dict()


def clouds_select_vt(app, width, height, time, mouse=(0.0, 0.0), aux=None, variant=0, ytab_rows=4096, table_range=0, point_list=False,
                     view_table=True, lib=None):
    """include/sbx_test.h sbx_debug_clouds_select_vt: clouds_select for a full-frame launch with "a ready view table of the frame's
    camera is at hand" as a further input; the dict has the record's `vt` as well"""
    lib = lib or load_library()
    u = uniforms(width, height, time, mouse)
    auxp = ctypes.cast(ctypes.byref(aux), ctypes.c_void_p) if aux is not None else None
    out = CloudsSelection()
    rc = lib.sbx_debug_clouds_select_vt(app_id(app), ctypes.byref(u), auxp, int(variant), int(ytab_rows), int(table_range),
                                        1 if point_list else 0, 1 if view_table else 0, ctypes.byref(out))
    if rc < 0:
        raise SbxError(rc, "sbx_debug_clouds_select_vt: bad arguments")
    return dict(out.as_dict(), vt=int(out.vt))


VIEWTAB_KEY_WORDS = 28


def clouds_viewtab_key(app, u, aux=None, lib=None):
    """include/sbx_test.h sbx_debug_clouds_viewtab_key (host only): the view-table key of a launch under the Uniforms `u` and the
    AuxClouds block `aux`, a numpy array of 28 uint32 words"""
    import numpy as np
    lib = lib or load_library()
    auxp = ctypes.cast(ctypes.byref(aux), ctypes.c_void_p) if aux is not None else None
    key = np.zeros(VIEWTAB_KEY_WORDS, dtype=np.uint32)
    rc = lib.sbx_debug_clouds_viewtab_key(app_id(app), ctypes.byref(u), auxp, ctypes.c_void_p(key.ctypes.data), VIEWTAB_KEY_WORDS)
    if rc < 0:
        raise SbxError(rc, "sbx_debug_clouds_viewtab_key: bad arguments")
    return key


def span_table(app, width, height, time, block_rows, nranks, root_rounds=1, rounds=1, mouse=(0.0, 0.0), aux=None, lib=None):
    """sbx_span_table (host only, no GPU needed): (table, rank_pixels, max_width) of the span exchange — table int32
    [nblocks, 4] = {x0, x1, offset in the owner's packed slab (pixels), owner} per global row-block; rank_pixels[r] = pixels of
    rank r's packed slab; max_width = the widest span among the peers' blocks."""
    import numpy as np
    lib = lib or load_library()
    u = uniforms(width, height, time, mouse)
    nb = shard.num_blocks(int(height), int(block_rows))
    table = np.zeros((nb, 4), dtype=np.int32)
    pix = np.zeros(int(nranks), dtype=np.int64)
    mw = ctypes.c_int32(0)
    auxp = ctypes.cast(ctypes.byref(aux), ctypes.c_void_p) if aux is not None else None
    rc = lib.sbx_span_table(app_id(app), ctypes.byref(u), auxp, int(block_rows), int(nranks), int(root_rounds), int(rounds),
                            table.ctypes.data_as(ctypes.c_void_p), pix.ctypes.data_as(ctypes.c_void_p),
                            ctypes.cast(ctypes.byref(mw), ctypes.c_void_p))
    if rc < 0:
        raise SbxError(rc, "sbx_span_table: bad arguments")
    return table, pix, int(mw.value)


class _RawDeviceArray:
    """A device pointer as an object torch.as_tensor understands (__cuda_array_interface__, no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class SharedFrame:
    """One sbx_shared (include/sbx.h, the store exchange): a frame in the OWNER's device memory that the other ranks of a split
    map and render into in place.  The owner gets it from Renderer.shared_create and may view it as a tensor; a peer gets it from
    Renderer.shared_open(handle bytes) and only ever passes its address to the render calls (the memory is another device's, or
    another process's)."""

    def __init__(self, renderer, handle, owner, nbytes):
        self.r, self.h, self.owner, self.nbytes = renderer, handle, bool(owner), int(nbytes)

    @property
    def ptr(self):
        return int(self.r.lib.sbx_shared_frame(self.h) or 0)

    def export(self):
        """the opaque handle as bytes, to be sent to the other ranks by any means (only the owner exports)"""
        hd = SharedHandle()
        self.r._check(self.r.lib.sbx_shared_export(self.h, ctypes.byref(hd)))
        return bytes(hd.opaque)

    def tensor(self, shape, dtype=None):
        """the owner's view of the frame as a device tensor (no copy)"""
        torch = self.r.torch
        dtype = dtype or self.r.pixel_dtype
        assert self.owner, "only the owner views the frame as a tensor; peers hold an address in another device / process"
        n = 1
        for v in shape:
            n *= int(v)
        assert n * (1 if dtype == torch.uint8 else 4) <= self.nbytes
        t = torch.as_tensor(_RawDeviceArray(self.ptr, shape, "|u1" if dtype == torch.uint8 else "<f4"), device=self.r.tdev)
        assert t.data_ptr() == self.ptr, "torch copied the shared frame instead of viewing it"
        t._sbx_keepalive = self
        return t

    def begin(self, rank):
        """owner (rank 0): the frame may be overwritten from here on in stream order; peer: wait for that"""
        self.r._check(self.r.lib.sbx_shared_frame_begin(self.h, int(rank), self.r._stream()))

    def end(self, rank):
        """peer: my rows of this frame are in place; owner: the stream continues when every peer's are"""
        self.r._check(self.r.lib.sbx_shared_frame_end(self.h, int(rank), self.r._stream()))

    def set_timeout_ms(self, ms):
        self.r._check(self.r.lib.sbx_shared_set_timeout_ms(self.h, int(ms)))

    def close(self):
        if self.h:
            self.r.lib.sbx_shared_close(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.r.ctx:
                self.close()
        except Exception:
            pass


class Renderer:
    """One sbx_ctx on one GPU.  Framebuffers are float32 torch tensors [rows, W, 4] on that GPU,
    row 0 = bottom row of the strip (reference convention, src/main.h:40-43) — or, after set_output_format("rgba8"), uint8
    tensors [rows, W, 4] (one R8G8B8A8_UNORM word per pixel, include/sbx.h), slabs included."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise SbxError(SBX_ERR_NO_DEVICE, "no GPU visible; shaderbox_amd has no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.device = int(device)
        h = ctypes.c_void_p()
        rc = self.lib.sbx_create(self.device, ctypes.byref(h))
        if rc != SBX_OK:
            raise SbxError(rc, "sbx_create failed (need a gfx950 device; there is no fallback)")
        self.ctx = h
        self.tdev = torch.device("cuda", self.device)
        self.pixel_dtype = torch.float32

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.sbx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != SBX_OK:
            raise SbxError(rc, (self.lib.sbx_last_error(self.ctx) or b"").decode())

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.tdev).cuda_stream)

    @staticmethod
    def uniforms(width, height, time, mouse=(0.0, 0.0)):
        u = Uniforms()
        u.u_res[0], u.u_res[1] = float(width), float(height)
        u.u_mouse[0], u.u_mouse[1] = float(mouse[0]), float(mouse[1])
        u.u_time = float(time)
        return u

    @staticmethod
    def _auxp(aux):
        return ctypes.cast(ctypes.byref(aux), ctypes.c_void_p) if aux is not None else None

    def set_output_format(self, fmt):
        """'rgba32f' (default) or 'rgba8': what the frame-granular calls write per pixel (sbx_set_output_format).  With 'rgba8'
        every frame / strip / slab buffer is a uint8 tensor with 4 bytes per pixel; points and main_image stay float."""
        code = {"rgba32f": SBX_FORMAT_RGBA32F, "rgba8": SBX_FORMAT_RGBA8}[fmt]
        self._check(self.lib.sbx_set_output_format(self.ctx, code))
        self.pixel_dtype = self.torch.uint8 if code == SBX_FORMAT_RGBA8 else self.torch.float32

    def set_precision(self, tier):
        """'exact' (default: bit-identical to the oracle) or '1e-4' (include/sbx.h SBX_PRECISION_1E4: APP_ATMOSPHERE and
        APP_ATMOSPHERE_GROUND with the hardware's binary32 exp2, within 1e-4 per channel of the exact frame; every other app ignores it)"""
        self._check(self.lib.sbx_set_precision(self.ctx, {"exact": 0, "1e-4": 1}[tier]))

    @property
    def rgba8(self):
        return self.pixel_dtype == self.torch.uint8

    def empty(self, shape, zero=False):
        """device buffer of the current pixel type (used by distributed.FramePlan)"""
        f = self.torch.zeros if zero else self.torch.empty
        return f(tuple(shape), dtype=self.pixel_dtype, device=self.tdev)

    def _is_pixels(self, t):
        return t.is_cuda and t.dtype == self.pixel_dtype and t.is_contiguous()

    def _buffer(self, rows, width, out):
        if out is None:
            return self.torch.empty((rows, width, 4), dtype=self.pixel_dtype, device=self.tdev)
        assert self._is_pixels(out)
        assert out.numel() >= rows * width * 4
        return out

    # -- the hot path ---------------------------------------------------------------------------
    def render(self, app, width, height, time, mouse=(0.0, 0.0), aux=None, rows=None, out=None):
        """Render rows [y0, y1) (default: the whole frame) of `app`; asynchronous on the current stream."""
        y0, y1 = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
        u = self.uniforms(width, height, time, mouse)
        buf = self._buffer(max(y1 - y0, 0), int(width), out)
        self._check(self.lib.sbx_render_rows(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), y0, y1,
                                             ctypes.c_void_p(buf.data_ptr()), self._stream()))
        return buf

    def render_to_host(self, app, width, height, time, out, mouse=(0.0, 0.0), aux=None, rows=None):
        """sbx_render_rows_host: rows [y0, y1) (default: the whole frame) into HOST memory `out` — a C-contiguous numpy array or CPU
        torch tensor (pinned or not) of rows x width x 4 float32 (uint8 with the RGBA8 format); returns `out` when the pixels are
        there (strips are copied out while the next ones render)."""
        y0, y1 = (0, int(height)) if rows is None else (int(rows[0]), int(rows[1]))
        u = self.uniforms(width, height, time, mouse)
        n = max(y1 - y0, 0) * int(width) * 4
        if hasattr(out, "data_ptr"):
            assert not out.is_cuda and out.is_contiguous() and out.numel() >= n and out.dtype == (self.torch.uint8 if self.rgba8 else self.torch.float32)
            ptr = out.data_ptr()
        else:
            import numpy as np
            assert out.flags["C_CONTIGUOUS"] and out.size >= n and out.dtype == (np.uint8 if self.rgba8 else np.float32)
            ptr = out.ctypes.data
        self._check(self.lib.sbx_render_rows_host(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), y0, y1,
                                                  ctypes.c_void_p(ptr), self._stream()))
        return out

    def render_rank(self, app, width, height, time, block_rows, rank, nranks, mouse=(0.0, 0.0), aux=None, out=None,
                    root_rounds=1, rounds=1):
        """Render the cyclic row-blocks of `rank` (optionally with root relief, shard.py); `out` has
        shard.rank_rows_max() rows (tail rows unused)."""
        u = self.uniforms(width, height, time, mouse)
        buf = self._buffer(shard.rank_rows_max(int(height), block_rows, nranks, root_rounds, rounds), int(width), out)
        self._check(self.lib.sbx_render_split(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows,
                                              rank, nranks, root_rounds, rounds, 0, 0x7fffffff,
                                              ctypes.c_void_p(buf.data_ptr()), self._stream()))
        return buf

    def pack_unorm8(self, frame, flip_y=True):
        """float RGBA rows [rows, W, 4] (device) -> uint8 [rows, W, 4], the R8G8B8A8_UNORM back-buffer write of hlsltoy
        (Direct3D float -> UNORM rule); flip_y puts the top row first."""
        assert frame.is_cuda and frame.dtype == self.torch.float32 and frame.is_contiguous() and frame.shape[-1] == 4
        rows, width = int(frame.shape[0]), int(frame.shape[1])
        out = self.torch.empty((rows, width, 4), dtype=self.torch.uint8, device=self.tdev)
        self._check(self.lib.sbx_pack_unorm8(self.ctx, width, rows, ctypes.c_void_p(frame.data_ptr()),
                                             ctypes.c_void_p(out.data_ptr()), 1 if flip_y else 0, self._stream()))
        return out

    def render_points(self, app, width, height, time, frag, mouse=(0.0, 0.0), aux=None, out=None):
        """mainImage at arbitrary fragCoords: `frag` is a float32 device tensor [n, 2]; returns [n, 4] (device).  u_res =
        (width, height) need not be whole numbers here.  Asynchronous on the current stream."""
        u = self.uniforms(width, height, time, mouse)
        frag = frag.to(self.tdev, self.torch.float32).contiguous().view(-1, 2)
        n = int(frag.shape[0])
        if out is None:
            out = self.torch.empty((n, 4), dtype=self.torch.float32, device=self.tdev)
        assert out.is_cuda and out.dtype == self.torch.float32 and out.is_contiguous() and out.numel() >= 4 * n
        self._check(self.lib.sbx_render_points(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), n,
                                               ctypes.c_void_p(frag.data_ptr()), ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def main_image_batch(self, app, width, height, time, frag_coords, mouse=(0.0, 0.0), aux=None):
        """sbx_main_image_batch: host arrays in, host arrays out — numpy float32 [n, 2] -> [n, 4]; synchronous."""
        import numpy as np
        u = self.uniforms(width, height, time, mouse)
        fc = np.ascontiguousarray(frag_coords, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((fc.shape[0], 4), dtype=np.float32)
        self._check(self.lib.sbx_main_image_batch(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), fc.shape[0],
                                                  fc.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def main_image(self, app, width, height, time, frag_coord, mouse=(0.0, 0.0), aux=None):
        """void mainImage(out vec4 fragColor, in vec2 fragCoord) (src/main.h:6-9) for hosts that loop over the
        pixels themselves: returns the RGBA tuple of mainImage at frag_coord.  For the centre of a pixel of the frame the
        first call renders the whole frame on the GPU and later calls read from the host copy; any other coordinate
        (off-centre, outside the frame) is evaluated exactly, by a one-point launch."""
        u = self.uniforms(width, height, time, mouse)
        fc = (ctypes.c_float * 2)(float(frag_coord[0]), float(frag_coord[1]))
        out = (ctypes.c_float * 4)()
        self._check(self.lib.sbx_main_image(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), ctypes.byref(fc),
                                            ctypes.byref(out)))
        return tuple(out)

    def render_rank_rows(self, app, width, height, time, block_rows, rank, nranks, r0, r1, slab, mouse=(0.0, 0.0),
                         aux=None, root_rounds=1, rounds=1):
        """Render slab rows [r0, r1) of `rank` into slab[r0:r1] (pipelined multi-GPU frames).  A slab whose last dimension
        is 3 is written without alpha (sbx_render_split_rgb: what crosses xGMI in the direct exchange)."""
        u = self.uniforms(width, height, time, mouse)
        if r1 <= r0:
            return slab
        assert self._is_pixels(slab) and slab.shape[-1] in ((4,) if self.rgba8 else (3, 4))
        assert slab.shape[1] == int(width) and slab.shape[0] >= r1
        view = slab[r0:r1]
        fn = self.lib.sbx_render_split_rgb if slab.shape[-1] == 3 else self.lib.sbx_render_split
        self._check(fn(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, rank, nranks, root_rounds, rounds,
                       int(r0), int(r1), ctypes.c_void_p(view.data_ptr()), self._stream()))
        return slab

    def render_rank_in_place(self, app, width, height, time, block_rows, rank, nranks, frame, mouse=(0.0, 0.0), aux=None,
                             root_rounds=1, rounds=1, channels=4):
        """The rows of `rank` at their global positions of the full-size `frame` [H, W, 4]; other rows are not touched.
        `frame` is a tensor of this device or a SharedFrame (the store exchange: the owner's frame mapped by a peer).
        channels = 3: only R, G, B of every float4 pixel are written (sbx_render_split_in_place_rgb; the alpha is in the frame)."""
        u = self.uniforms(width, height, time, mouse)
        if isinstance(frame, SharedFrame):
            assert frame.nbytes >= int(height) * int(width) * (4 if self.rgba8 else 16)
            ptr = frame.ptr
        else:
            assert self._is_pixels(frame)
            assert tuple(frame.shape) == (int(height), int(width), 4)
            ptr = frame.data_ptr()
        fn = self.lib.sbx_render_split_in_place_rgb if int(channels) == 3 else self.lib.sbx_render_split_in_place
        self._check(fn(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, rank, nranks, root_rounds, rounds,
                       ctypes.c_void_p(ptr), self._stream()))
        return frame

    def render_span_peer_in_place(self, app, width, height, time, block_rows, rank, nranks, frame, mouse=(0.0, 0.0), aux=None,
                                  root_rounds=1, rounds=1, channels=4):
        """The spans of peer `rank`'s row-blocks at their place in the owner's full-size frame (a SharedFrame, or a tensor of this
        device): sbx_render_span_peer_in_place, the store exchange with spans."""
        u = self.uniforms(width, height, time, mouse)
        ptr = frame.ptr if isinstance(frame, SharedFrame) else frame.data_ptr()
        self._check(self.lib.sbx_render_span_peer_in_place(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, rank, nranks,
                                                           root_rounds, rounds, 4 if self.rgba8 else int(channels), ctypes.c_void_p(ptr),
                                                           self._stream()))
        return frame

    # -- the store exchange (include/sbx.h sbx_shared_*) --------------------------------------------------------
    def shared_create(self, nbytes, nranks):
        """a frame of `nbytes` bytes on this device that `nranks` ranks render into (this renderer is its owner, rank 0)"""
        h = ctypes.c_void_p()
        self._check(self.lib.sbx_shared_create(self.ctx, int(nbytes), int(nranks), ctypes.byref(h)))
        return SharedFrame(self, h, True, nbytes)

    def shared_open(self, handle_bytes):
        """map the frame another rank exported (SharedFrame.export()) for rendering from this device"""
        hd = SharedHandle()
        assert len(handle_bytes) == ctypes.sizeof(hd)
        ctypes.memmove(ctypes.byref(hd), bytes(handle_bytes), ctypes.sizeof(hd))
        h = ctypes.c_void_p()
        self._check(self.lib.sbx_shared_open(self.ctx, ctypes.byref(hd), ctypes.byref(h)))
        return SharedFrame(self, h, False, int(self.lib.sbx_shared_bytes(h)))

    def model_landing(self, src, dst, nbytes, workgroups, duration_us):
        """include/sbx_test.h sbx_model_landing: the scaling tools' stand-in for RCCL's receive kernels on the frame's owner"""
        self._check(self.lib.sbx_model_landing(self.ctx, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), int(nbytes),
                                               int(workgroups), float(duration_us), self._stream()))

    def stats(self):
        st = Stats()
        self._check(self.lib.sbx_get_stats(self.ctx, ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k in ("render_launches", "main_image_hits", "main_image_frames", "main_image_points")}

    def raytracer_scene_launches(self):
        """include/sbx_test.h sbx_debug_raytracer_scene_launches: launches of APP_RAYTRACER_SCENE's own kernel by this context"""
        n = ctypes.c_uint64(0)
        self._check(self.lib.sbx_debug_raytracer_scene_launches(self.ctx, ctypes.byref(n)))
        return int(n.value)

    def reset_stats(self):
        self._check(self.lib.sbx_reset_stats(self.ctx))

    # -- the span exchange: only the expensive part of each row-block is sharded (include/sbx.h) ------------------
    def span_table(self, app, width, height, time, block_rows, nranks, root_rounds=1, rounds=1, mouse=(0.0, 0.0), aux=None):
        return span_table(app, width, height, time, block_rows, nranks, root_rounds, rounds, mouse, aux, lib=self.lib)

    def render_span_peer(self, app, width, height, time, block_rows, rank, nranks, r0, r1, slab, mouse=(0.0, 0.0), aux=None,
                         root_rounds=1, rounds=1):
        """Slab rows [r0, r1) (whole blocks) of peer `rank`, spans only, packed 3 floats per pixel into `slab` (a flat float32
        device buffer of >= 3 * rank_pixels[rank] floats: the table's offsets are absolute within it; 'rgba8': 4 bytes per
        pixel of a flat uint8 buffer)."""
        u = self.uniforms(width, height, time, mouse)
        if isinstance(slab, tuple):                       # (SharedFrame, byte offset): the rank's slab inside the owner's mapped landing area
            ptr = slab[0].ptr + int(slab[1])
        else:
            assert self._is_pixels(slab)
            ptr = slab.data_ptr()
        self._check(self.lib.sbx_render_span_peer(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, rank, nranks,
                                                  root_rounds, rounds, int(r0), int(r1), ctypes.c_void_p(ptr), self._stream()))
        return slab

    def render_span_root(self, app, width, height, time, block_rows, nranks, frame, mouse=(0.0, 0.0), aux=None, root_rounds=1,
                         rounds=1):
        """The owner's launch of the span exchange, in place over the whole `frame` [H, W, 4]: rank 0's row-blocks in full and
        every other block outside its span."""
        u = self.uniforms(width, height, time, mouse)
        assert self._is_pixels(frame)
        assert tuple(frame.shape) == (int(height), int(width), 4)
        self._check(self.lib.sbx_render_span_root(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, nranks,
                                                  root_rounds, rounds, ctypes.c_void_p(frame.data_ptr()), self._stream()))
        return frame

    def assemble_spans(self, app, width, height, time, block_rows, nranks, peers, stride_pixels, frame, mouse=(0.0, 0.0), aux=None,
                       root_rounds=1, rounds=1):
        """Scatter the peers' packed span slabs (`peers`: flat float32, slab of rank r at (r - 1) * stride_pixels * 3) into
        `frame`, alpha = 1; everything else in the frame is left as sbx_render_span_root wrote it."""
        u = self.uniforms(width, height, time, mouse)
        assert self._is_pixels(peers) and self._is_pixels(frame)
        assert peers.numel() >= (int(nranks) - 1) * int(stride_pixels) * (4 if self.rgba8 else 3)
        self._check(self.lib.sbx_assemble_spans(self.ctx, app_id(app), ctypes.byref(u), self._auxp(aux), block_rows, nranks,
                                                root_rounds, rounds, ctypes.c_void_p(peers.data_ptr()), int(stride_pixels),
                                                ctypes.c_void_p(frame.data_ptr()), self._stream()))
        return frame

    def assemble_peers(self, peers, width, height, block_rows, nranks, frame, root_rounds=1, rounds=1):
        """Root side of the direct exchange: scatter the slabs of ranks 1 .. nranks-1 (`peers` [nranks-1, rows_max, W, 3|4])
        to their rows of `frame` [H, W, 4] (alpha = 1 for 3-channel slabs); rank 0's rows are left as rendered in place."""
        if int(nranks) == 1:
            return frame
        ch = int(peers.shape[-1])
        need = (int(nranks) - 1) * shard.rank_rows_max(int(height), int(block_rows), int(nranks), root_rounds, rounds) * int(width) * ch
        if not (self._is_pixels(peers) and ch in ((4,) if self.rgba8 else (3, 4)) and peers.numel() >= need):
            raise ValueError("peers must be a contiguous device tensor of >= (nranks-1) * rows_max * W * C = %d elements of the "
                             "renderer's pixel type" % need)
        assert self._is_pixels(frame)
        assert tuple(frame.shape) == (int(height), int(width), 4)
        self._check(self.lib.sbx_assemble_peers(self.ctx, int(width), int(height), block_rows, nranks, root_rounds, rounds, ch,
                                                ctypes.c_void_p(peers.data_ptr()), ctypes.c_void_p(frame.data_ptr()),
                                                self._stream()))
        return frame

    def assemble(self, gathered, width, height, block_rows, nranks, out=None, root_rounds=1, rounds=1):
        """Root side: scatter the rank-major gathered slabs to their global rows -> [H, W, 4]."""
        frame = self._buffer(int(height), int(width), out)
        need = int(nranks) * shard.rank_rows_max(int(height), int(block_rows), int(nranks), root_rounds, rounds) * int(width) * 4
        if not (self._is_pixels(gathered) and gathered.numel() >= need):
            raise ValueError("gathered must be a contiguous device tensor of >= nranks * rows_max * W * 4 = %d elements of the "
                             "renderer's pixel type" % need)
        self._check(self.lib.sbx_assemble_split(self.ctx, int(width), int(height), block_rows, nranks, root_rounds, rounds,
                                                ctypes.c_void_p(gathered.data_ptr()), ctypes.c_void_p(frame.data_ptr()),
                                                self._stream()))
        return frame

    def fault_status(self):
        """0, or SBX_ERR_FAULT once a kernel on this device has reported an invariant violation (sticky until clear_fault)"""
        return int(self.lib.sbx_fault_status(self.ctx))

    def clear_fault(self):
        self._check(self.lib.sbx_clear_fault(self.ctx))

    def set_variant(self, variant):
        """0 = default kernels, 1 = per-lane cross-check kernels (bit-identical by specification)."""
        self._check(self.lib.sbx_set_variant(self.ctx, int(variant)))

    def tile_order(self, app, capacity=1 << 20):
        """include/sbx_test.h sbx_debug_tile_order: (tables built for the app's current launch shape, launches since the last one,
        the current table as a numpy array of bx | by << 16 words or None)"""
        import numpy as np
        built, since = ctypes.c_int(), ctypes.c_int()
        buf = (ctypes.c_uint * int(capacity))()
        n = self.lib.sbx_debug_tile_order(self.ctx, app_id(app), ctypes.byref(built), ctypes.byref(since), buf, int(capacity))
        self._check(min(n, 0))
        return built.value, since.value, (np.frombuffer(buf, dtype=np.uint32, count=n).copy() if n > 0 else None)

    def clouds_hashtab(self):
        """include/sbx_test.h sbx_debug_clouds_hashtab: (entries, bias) of the newest lattice-hash table, tables built so far, and
        whether the last APP_CLOUDS launch took a hash-table kernel"""
        v = [ctypes.c_int() for _ in range(4)]
        self._check(self.lib.sbx_debug_clouds_hashtab(self.ctx, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def clouds_viewtab(self):
        """include/sbx_test.h sbx_debug_clouds_viewtab: entries of the view table built or used last, tables built so far, whether
        the last APP_CLOUDS launch took a view-table kernel, and the reason where it did not (SBX_VIEWTAB_*)"""
        n = ctypes.c_size_t()
        v = [ctypes.c_int() for _ in range(3)]
        self._check(self.lib.sbx_debug_clouds_viewtab(self.ctx, ctypes.byref(n), *[ctypes.byref(x) for x in v]))
        return (int(n.value),) + tuple(x.value for x in v)

    def set_clouds_viewtab_cap(self, nbytes):
        """include/sbx_test.h sbx_debug_set_clouds_viewtab_cap: the byte cap of one view table"""
        self._check(self.lib.sbx_debug_set_clouds_viewtab_cap(self.ctx, int(nbytes)))

    def clouds_last_selection(self):
        """include/sbx_test.h sbx_debug_clouds_last_selection: the kernel the context's last launch of APP_CLOUDS, of its HEIGHT /
        LUMINANCE builds or of CLOUDS_SKY took, as a dict of sbx_clouds_selection's fields"""
        out = CloudsSelection()
        self._check(self.lib.sbx_debug_clouds_last_selection(self.ctx, ctypes.byref(out)))
        return out.as_dict()

    def clouds_hashtab_read(self, first, count):
        """include/sbx_test.h sbx_debug_clouds_hashtab_read: entries [first, first + count) of the newest table, a numpy float32 array"""
        import numpy as np
        out = np.empty(max(int(count), 1), dtype=np.float32)
        self._check(self.lib.sbx_debug_clouds_hashtab_read(self.ctx, int(first), int(count), ctypes.c_void_p(out.ctypes.data)))
        return out[:int(count)]

    def order_build(self, cost, gx, gy):
        """include/sbx_test.h sbx_debug_order_build: the dispatch order's sort (csrc/kern_util.hip launch_order_build) run on the
        `gx * gy` cost words `cost` -> the table, a numpy array of gx * gy words x | y << 16"""
        import numpy as np
        cost = np.ascontiguousarray(cost, dtype=np.uint32)
        n = int(gx) * int(gy)
        assert cost.size == n, (cost.size, gx, gy)
        table = np.empty(max(n, 1), dtype=np.uint32)
        self._check(self.lib.sbx_debug_order_build(self.ctx, ctypes.c_void_p(cost.ctypes.data), int(gx), int(gy),
                                                   ctypes.c_void_p(table.ctypes.data), self._stream()))
        return table[:n]

    def set_timing(self, enabled=True):
        self._check(self.lib.sbx_set_timing(self.ctx, 1 if enabled else 0))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self._check(self.lib.sbx_last_kernel_ms(self.ctx, ctypes.byref(ms)))
        return ms.value

    def noise(self, fn, xyz, params=(0.0, 0.0, 0.0)):
        """Library noise functions (noise_iq / hash_w / noise_w / fbm_worley_tile / worley_fbm) over points xyz[n,3] -> [n,3]."""
        xyz = xyz.to(self.tdev, self.torch.float32).contiguous().view(-1, 3)
        par = (ctypes.c_float * 3)(*[float(v) for v in params])
        out = self.torch.empty_like(xyz)
        self._check(self.lib.sbx_noise_eval(self.ctx, fn.encode(), ctypes.c_void_p(xyz.data_ptr()),
                                            ctypes.cast(par, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()),
                                            xyz.shape[0], self._stream()))
        return out

    # The eval entries (include/sbx.h sbx_<family>_eval): per family, function name -> floats per element (in, out).  A new entry adds
    # its row here and a public method that calls _eval.
    EVAL_WIDTHS = {
        "atmosphere": {"get_incident_light": (6, 3), "get_sun_light": (6, 3)},
        "atmosphere_air": {"get_incident_light": (6, 3), "get_sun_light": (6, 3)},
        "clouds": {"render": (6, 4), "render_clouds": (6, 4), "render_sky_color": (3, 3), "density_func": (3, 1), "illuminate_volume": (6, 1)},
        "planet": {"render": (6, 4), "terrain_march": (6, 4), "sdf_terrain_map": (3, 2), "sdf_terrain_map_detail": (3, 2),
                   "sdf_terrain_normal": (3, 3), "clouds_density": (4, 1), "illuminate": (4, 3), "background": (3, 3)},
        "planet_world": {"render": (6, 4), "terrain_march": (6, 4), "sdf_terrain_map": (3, 2), "sdf_terrain_map_detail": (3, 2),
                         "sdf_terrain_normal": (3, 3), "clouds_density": (4, 1), "illuminate": (4, 3), "background": (3, 3)},
        "egg": {"ik_solver": (8, 3), "sdf": (3, 2), "sdf_normal": (3, 3), "shadowmarch": (6, 1), "render_scene": (6, 4)},
        "vinyl": {"sdf": (3, 2), "sdf_normal": (3, 3), "sdf_shadow": (6, 1), "illuminate": (7, 3), "render": (6, 5)},
        "sdf": {"sdf": (3, 2)},
        "raytracer": {"raytrace_iteration": (7, 8), "illuminate": (10, 3), "shadow": (3, 2), "render": (6, 4)},
        "sdf_scene": {"sdf": (3, 2), "sdf_normal": (3, 3), "sdf_ao": (6, 1), "sdf_shadow": (6, 1), "illuminate": (9, 3), "render_impl": (6, 5),
                      "render": (6, 4)},
    }
    CLOUDS_EVAL_WIDTHS, PLANET_EVAL_WIDTHS = EVAL_WIDTHS["clouds"], EVAL_WIDTHS["planet"]
    EGG_EVAL_WIDTHS, VINYL_EVAL_WIDTHS = EVAL_WIDTHS["egg"], EVAL_WIDTHS["vinyl"]

    def _eval(self, family, fn, x, lead, counts=None, mid=(), named=True):
        """sbx_<family>_eval or, with `counts` (what the twin writes its counters to), sbx_debug_<family>_eval of include/sbx_test.h
        over x -> [n, floats out].  The call is (ctx, fn, *lead, in, *mid, out, n[, counts], stream): `lead` the family's own arguments
        (its block by reference or None, u_time), `mid` what its prototype puts between in and out; named=False: the entry takes no fn."""
        widths = self.EVAL_WIDTHS[family]
        if fn not in widths:
            raise SbxError(SBX_ERR_ARG, "unknown %s function %r" % (family.replace("_", " "), fn))
        win, wout = widths[fn]
        x = x.to(self.tdev, self.torch.float32).contiguous().view(x.numel() // win, win)
        out = self.torch.empty((x.shape[0], wout), dtype=self.torch.float32, device=self.tdev)
        args = (self.ctx,) + ((fn.encode(),) if named else ()) + tuple(lead) + (ctypes.c_void_p(x.data_ptr()),) + tuple(mid) + \
               (ctypes.c_void_p(out.data_ptr()), x.shape[0])
        if counts is None:
            self._check(getattr(self.lib, "sbx_%s_eval" % family)(*args, self._stream()))
        else:
            self._check(getattr(self.lib, "sbx_debug_%s_eval" % family)(*args, counts, self._stream()))
        return out

    @staticmethod
    def _by_ref(block):
        return None if block is None else ctypes.byref(block)

    @staticmethod
    def _sun_mid(sun_dir):
        """sbx_atmosphere_eval's sun_dir, which sits between in and out"""
        return (None if sun_dir is None else ctypes.cast((ctypes.c_float * 3)(*[float(v) for v in sun_dir]), ctypes.c_void_p),)

    def atmosphere_eval(self, fn, rays, sun_dir=(0.0, 1.0, 0.0)):
        """The Rayleigh/Mie solver over rays[n, 6] (origin xyz, direction xyz; include/sbx.h sbx_atmosphere_eval) -> [n, 3]:
        fn 'get_incident_light' = linear RGB for the sun direction `sun_dir` (used as given), 'get_sun_light' = (overground,
        optical_depthR, optical_depthM) along the ray (sun_dir may be None)."""
        return self._eval("atmosphere", fn, rays, (), mid=self._sun_mid(sun_dir))

    def atmosphere_eval_counted(self, fn, rays, sun_dir=(0.0, 1.0, 0.0)):
        """include/sbx_test.h sbx_debug_atmosphere_eval: atmosphere_eval that waits -> (out, waves that ran the fast forms)"""
        waves = ctypes.c_uint(0)
        return self._eval("atmosphere", fn, rays, (), ctypes.byref(waves), mid=self._sun_mid(sun_dir)), waves.value

    def atmosphere_air_eval(self, fn, rays, air):
        """The Rayleigh/Mie solver over rays[n, 6] under an AtmosphereAir (include/sbx.h sbx_atmosphere_air_eval) -> [n, 3]: fn
        'get_incident_light' or 'get_sun_light', as atmosphere_eval, with every number of the solver and the sun read from `air`
        (its view, eye, look_at and fov are not)."""
        return self._eval("atmosphere_air", fn, rays, (self._by_ref(air),))

    def atmosphere_air_eval_counted(self, fn, rays, air):
        """include/sbx_test.h sbx_debug_atmosphere_air_eval: atmosphere_air_eval that waits -> (out, waves that ran the fast body)"""
        waves = ctypes.c_uint(0)
        return self._eval("atmosphere_air", fn, rays, (self._by_ref(air),), ctypes.byref(waves)), waves.value

    def clouds_eval(self, fn, x, u_time=0.0, aux=None):
        """APP_CLOUDS' volume and sky over the caller's elements (include/sbx.h sbx_clouds_eval): fn 'render' / 'render_clouds' over rays
        x[n, 6] (origin xyz, direction xyz) -> [n, 4]; 'render_sky_color' over directions x[n, 3] -> [n, 3]; 'density_func' over points
        x[n, 3] -> [n, 1]; 'illuminate_volume' over x[n, 6] (origin xyz, V xyz) -> [n, 1].  aux: an AuxClouds, a dict of the fields
        that differ from the defaults, or None = the defaults.  u_time enters through the wind offset alone."""
        return self._eval("clouds", fn, x, (self._by_ref(self._clouds_aux(aux)), float(u_time)))

    def clouds_eval_counted(self, fn, x, u_time=0.0, aux=None):
        """include/sbx_test.h sbx_debug_clouds_eval: clouds_eval that waits -> (out, (noise cells whose hashes came from the context's
        table, cells hashed in place))"""
        counts = (ctypes.c_uint64 * 2)(0, 0)
        return self._eval("clouds", fn, x, (self._by_ref(self._clouds_aux(aux)), float(u_time)), counts), (int(counts[0]), int(counts[1]))

    def planet_eval(self, fn, x, u_time=0.0):
        """APP_PLANET's terrain, cloud shell and shading over the caller's elements (include/sbx.h sbx_planet_eval): fn 'render' /
        'terrain_march' over rays x[n, 6] (origin xyz, direction xyz; planet at 0, radius 1) -> [n, 4]; 'sdf_terrain_map' /
        'sdf_terrain_map_detail' over points x[n, 3] -> [n, 2]; 'sdf_terrain_normal' x[n, 3] -> [n, 3]; 'clouds_density' over x[n, 4]
        (cloud.pos xyz, cloud.height) -> [n, 1]; 'illuminate' over x[n, 4] (pos xyz, df.y) -> [n, 3]; 'background' over directions
        x[n, 3] -> [n, 3].  u_time enters through rot / rot_cloud alone."""
        return self._eval("planet", fn, x, (float(u_time),))

    def planet_eval_counted(self, fn, x, u_time=0.0):
        """include/sbx_test.h sbx_debug_planet_eval: planet_eval that waits -> (out, (waves with every guarded short form on, waves
        that took the plain form for at least one part))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("planet", fn, x, (float(u_time),), counts), (int(counts[0]), int(counts[1]))

    def egg_eval(self, fn, x, pose=None):
        """src/IK.h's solver and APP_EGG's field, normal, shadow march and trace over the caller's elements under an EggPose
        (include/sbx.h sbx_egg_eval): fn 'ik_solver' over x[n, 8] (start xyz, goal xyz, L1, L2) -> [n, 3], pose not read; 'sdf' over
        points x[n, 3] -> [n, 2] (distance, material id); 'sdf_normal' x[n, 3] -> [n, 3]; 'shadowmarch' over rays x[n, 6] (origin
        xyz, direction xyz) -> [n, 1]; 'render_scene' over rays x[n, 6] -> [n, 4] (rgb, depth).  Only the pose's turn_deg, feet and
        bones are read."""
        return self._eval("egg", fn, x, (self._by_ref(pose),))

    def egg_eval_counted(self, fn, x, pose=None):
        """include/sbx_test.h sbx_debug_egg_eval: egg_eval that waits -> (out, (waves that took the witnessed roots only, waves that
        re-ran with the IEEE roots))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("egg", fn, x, (self._by_ref(pose),), counts), (int(counts[0]), int(counts[1]))

    def vinyl_eval(self, fn, x, deck):
        """APP_VINYL's field, normal, soft shadow, shading and trace over the caller's elements under a VinylDeck (include/sbx.h
        sbx_vinyl_eval): fn 'sdf' over points x[n, 3] -> [n, 2] (distance, material id); 'sdf_normal' x[n, 3] -> [n, 3]; 'sdf_shadow'
        over rays x[n, 6] (origin xyz, direction xyz) -> [n, 1]; 'illuminate' over x[n, 7] (eye xyz, hit xyz, material id) -> [n, 3];
        'render' over rays x[n, 6] -> [n, 5] (linear rgb, t, material id or 0).  The deck's camera fields are not read."""
        return self._eval("vinyl", fn, x, (self._by_ref(deck),))

    def vinyl_eval_counted(self, fn, x, deck):
        """include/sbx_test.h sbx_debug_vinyl_eval: vinyl_eval that waits -> (out, (waves that took the witnessed roots only, waves
        that re-ran with the IEEE roots))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("vinyl", fn, x, (self._by_ref(deck),), counts), (int(counts[0]), int(counts[1]))

    def raytracer_eval(self, fn, x, scene):
        """src/app_raytracer.h's trace, shading, shadow test and render over the caller's elements under a RaytracerScene (include/sbx.h
        sbx_raytracer_eval): fn 'raytrace_iteration' over x[n, 7] (origin xyz, direction xyz, mat_to_ignore) -> [n, 8] (hit.t, material
        id, hit.origin xyz, hit.normal xyz); 'illuminate' over x[n, 10] (eye xyz, hit.origin xyz, hit.normal xyz, material id) ->
        [n, 3]; 'shadow' over hit origins x[n, 3] -> [n, 2] (shadow_hit.t, length(shadow_line)); 'render' over rays x[n, 6] -> [n, 4]
        (linear rgb, depth).  The scene's eye, look_at and fov are not read."""
        return self._eval("raytracer", fn, x, (self._by_ref(scene),))

    def raytracer_eval_counted(self, fn, x, scene):
        """include/sbx_test.h sbx_debug_raytracer_eval: raytracer_eval that waits -> (out, (waves that took the witnessed roots only,
        waves that re-ran with the IEEE roots))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("raytracer", fn, x, (self._by_ref(scene),), counts), (int(counts[0]), int(counts[1]))

    def sdf_scene_eval(self, fn, x, scene):
        """APP_SDF_SCENE's field, normal, ambient occlusion, soft shadow, shading, trace and fogged render over the caller's elements under
        an SdfScene (include/sbx.h sbx_sdf_scene_eval): fn 'sdf' over points x[n, 3] -> [n, 2] (distance, material id); 'sdf_normal'
        x[n, 3] -> [n, 3]; 'sdf_ao' over x[n, 6] (hit.origin xyz, hit.normal xyz) -> [n, 1]; 'sdf_shadow' over rays x[n, 6] (origin
        xyz, direction xyz) -> [n, 1]; 'illuminate' over x[n, 9] (hit.origin xyz, hit.normal xyz, material id, ao, sh) -> [n, 3];
        'render_impl' over rays x[n, 6] -> [n, 5] (rgb, t, material id or -1); 'render' over rays x[n, 6] -> [n, 4] (linear rgb after
        the fog, t).  The scene's eye, look_at and fov are not read."""
        return self._eval("sdf_scene", fn, x, (self._by_ref(scene),))

    def sdf_scene_eval_counted(self, fn, x, scene):
        """include/sbx_test.h sbx_debug_sdf_scene_eval: sdf_scene_eval that waits -> (out, (waves that took the witnessed roots only,
        waves that re-ran with the IEEE roots))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("sdf_scene", fn, x, (self._by_ref(scene),), counts), (int(counts[0]), int(counts[1]))

    def sdf_eval(self, scene, xyz):
        """sdf(pos) of an SdfScene's program over points xyz[n, 3] (include/sbx.h sbx_sdf_eval) -> [n, 2]: the distance and the
        nearest object's material id as a float.  Only the program of `scene` is read."""
        return self._eval("sdf", "sdf", xyz, (ctypes.byref(scene),), named=False)

    def atmosphere_air_launches(self):
        """include/sbx_test.h sbx_debug_atmosphere_air_launches: (APP_ATMOSPHERE_AIR launches of this context, those that took the
        literal tier, those that took the plain kernel)"""
        c = (ctypes.c_uint64 * 3)(0, 0, 0)
        self._check(self.lib.sbx_debug_atmosphere_air_launches(self.ctx, c))
        return int(c[0]), int(c[1]), int(c[2])

    def planet_world_eval(self, fn, x, world):
        """planet_eval under a PlanetWorld (include/sbx.h sbx_planet_world_eval): the same eight names and element layouts, with the
        numbers and the three angles read from `world` (its eye, look_at and fov are not)."""
        return self._eval("planet_world", fn, x, (self._by_ref(world),))

    def planet_world_eval_counted(self, fn, x, world):
        """include/sbx_test.h sbx_debug_planet_world_eval: planet_world_eval that waits -> (out, (waves with every guarded short form
        on, waves that took the plain form for at least one part))"""
        counts = (ctypes.c_uint * 2)(0, 0)
        return self._eval("planet_world", fn, x, (self._by_ref(world),), counts), (int(counts[0]), int(counts[1]))

    def planet_world_launches(self):
        """include/sbx_test.h sbx_debug_planet_world_launches: APP_PLANET_WORLD launches of this context by what ran -> (the literal
        tier's short-form kernels, the run-time kernel, a plain kernel)"""
        c = (ctypes.c_uint64 * 3)(0, 0, 0)
        self._check(self.lib.sbx_debug_planet_world_launches(self.ctx, c))
        return int(c[0]), int(c[1]), int(c[2])

    def _clouds_aux(self, aux):
        if aux is None or isinstance(aux, AuxClouds):
            return aux
        a = clouds_defaults(self.lib)
        for name, v in dict(aux).items():
            if isinstance(getattr(a, name), ctypes.Array):
                setattr(a, name, (ctypes.c_float * 3)(*[float(c) for c in v]))
            else:
                setattr(a, name, v)
        return a

    def vinyl_deck_launches(self):
        """include/sbx_test.h sbx_debug_vinyl_deck_launches: (APP_VINYL_DECK launches of this context, those of them an untame deck sent
        to the reference form)"""
        c = (ctypes.c_uint64 * 2)(0, 0)
        self._check(self.lib.sbx_debug_vinyl_deck_launches(self.ctx, c))
        return int(c[0]), int(c[1])

    def egg_pose_launches(self):
        """include/sbx_test.h sbx_debug_egg_pose_launches: (APP_EGG_POSE launches of this context, those of them an untame pose sent
        to the reference form)"""
        c = (ctypes.c_uint64 * 2)(0, 0)
        self._check(self.lib.sbx_debug_egg_pose_launches(self.ctx, c))
        return int(c[0]), int(c[1])

    def worley_volume(self, size=128):
        """The ddsvolgen noise volume: float32 [size, size, size, 4] (z, y, x, rgba)."""
        out = self.torch.empty((size, size, size, 4), dtype=self.torch.float32, device=self.tdev)
        self._check(self.lib.sbx_worley_volume(self.ctx, int(size), ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_noise_volumes(self, shape_rgba, detail_rgba):
        """Bind the two 3-D noise textures of APP_CLOUDS' USE_NOISE_TEX build (t1 = shape, t2 = Worley detail): float32
        device tensors [size, size, size, 4] as worley_volume() / ddsvolgen produce them.  The library keeps its own copy
        of the .r channel; render with app 'clouds_tex' afterwards (same stream)."""
        for v in (shape_rgba, detail_rgba):
            assert v.is_cuda and v.dtype == self.torch.float32 and v.is_contiguous() and v.dim() == 4 and v.shape[3] == 4
            assert v.shape[0] == v.shape[1] == v.shape[2]
        self._check(self.lib.sbx_set_noise_volumes(self.ctx, int(shape_rgba.shape[0]), ctypes.c_void_p(shape_rgba.data_ptr()),
                                                   int(detail_rgba.shape[0]), ctypes.c_void_p(detail_rgba.data_ptr()),
                                                   self._stream()))

    def set_texture2d(self, texels):
        """Bind the t0 texture of APP_2D_TEX (sbx_set_texture2d): a CUDA tensor [height, width, 4] float32 (RGBA32F) or uint8
        (R8G8B8A8_UNORM), or [height, width] int32 words; row 0 at v = 0.  None restores hlsltoy's 128x128 checkerboard.
        The library copies the texels on the current stream and returns when the copy is done."""
        if texels is None:
            self._check(self.lib.sbx_set_texture2d(self.ctx, 0, 0, 0, None, self._stream()))
            return
        t = self.torch
        assert texels.is_cuda and texels.is_contiguous()
        if texels.dtype in (t.float32, t.uint8):
            assert texels.dim() == 3 and texels.shape[2] == 4
            fmt = SBX_FORMAT_RGBA32F if texels.dtype == t.float32 else SBX_FORMAT_RGBA8
        else:
            assert texels.dim() == 2 and texels.element_size() == 4 and not texels.is_floating_point()
            fmt = SBX_FORMAT_RGBA8
        self._check(self.lib.sbx_set_texture2d(self.ctx, int(texels.shape[1]), int(texels.shape[0]), fmt,
                                               ctypes.c_void_p(texels.data_ptr()), self._stream()))

    def tex3d(self, rgba, xyz):
        """SampleLevel(linear, wrap, 0).r of an RGBA32F device volume at points xyz[n, 3] (the texture-filter spec)."""
        assert rgba.is_cuda and rgba.dtype == self.torch.float32 and rgba.is_contiguous() and rgba.shape[3] == 4
        xyz = xyz.to(self.tdev, self.torch.float32).contiguous().view(-1, 3)
        out = self.torch.empty((xyz.shape[0],), dtype=self.torch.float32, device=self.tdev)
        self._check(self.lib.sbx_tex3d_eval(self.ctx, int(rgba.shape[0]), ctypes.c_void_p(rgba.data_ptr()),
                                            ctypes.c_void_p(xyz.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                            xyz.shape[0], self._stream()))
        return out

    def math(self, fn, a, b=None):
        """Evaluate the device math spec elementwise (parity tests)."""
        a = a.to(self.tdev, self.torch.float32).contiguous()
        bp = None
        if b is not None:
            b = b.to(self.tdev, self.torch.float32).contiguous()
            bp = ctypes.c_void_p(b.data_ptr())
        out = self.torch.empty_like(a)
        self._check(self.lib.sbx_math_eval(self.ctx, fn.encode(), ctypes.c_void_p(a.data_ptr()), bp,
                                           ctypes.c_void_p(out.data_ptr()), a.numel(), self._stream()))
        return out


class MultiRenderer:
    """One sbx_multi: a single process driving `devices` (rank i on devices[i]; rank 0 owns the frame).  With distinct
    devices the row-blocks travel over RCCL inside the library; repeated devices run the same schedule with device copies
    (N ranks on one GPU).  Frames are float32 torch tensors [H, W, 4] on devices[0]."""

    def __init__(self, devices):
        import torch
        if not torch.cuda.is_available():
            raise SbxError(SBX_ERR_NO_DEVICE, "no GPU visible; shaderbox_amd has no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        rc = self.lib.sbx_multi_create(len(self.devices), arr, ctypes.byref(h))
        if rc != SBX_OK:
            raise SbxError(rc, "sbx_multi_create failed: " + (self.lib.sbx_multi_create_error() or b"").decode())
        self.m = h
        self.tdev = torch.device("cuda", self.devices[0])

    def close(self):
        if getattr(self, "m", None):
            self.lib.sbx_multi_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SBX_OK:
            raise SbxError(rc, (self.lib.sbx_multi_last_error(self.m) or b"").decode())

    @property
    def uses_rccl(self):
        return self.lib.sbx_multi_uses_rccl(self.m) == 1

    def set_split(self, block_rows=8, root_rounds=1, rounds=1):
        self._check(self.lib.sbx_multi_set_split(self.m, int(block_rows), int(root_rounds), int(rounds)))

    def set_output_format(self, fmt):
        """'rgba32f' or 'rgba8' on every rank (sbx_multi_set_output_format): render() then returns / fills uint8 [H, W, 4]"""
        code = {"rgba32f": SBX_FORMAT_RGBA32F, "rgba8": SBX_FORMAT_RGBA8}[fmt]
        self._check(self.lib.sbx_multi_set_output_format(self.m, code))
        self.pixel_dtype = self.torch.uint8 if code == SBX_FORMAT_RGBA8 else self.torch.float32

    def set_variant(self, variant):
        self._check(self.lib.sbx_multi_set_variant(self.m, int(variant)))

    def set_exchange(self, mode):
        """'slabs' (default): one send / receive per peer of its whole 3-channel slab + one scatter kernel on rank 0;
        'blocks': one send / receive pair per row-block straight into the final rows (the round-2 form);
        'spans': the span exchange — only the expensive interval of every row-block is dealt to the peers and sent, rank 0
        renders the rest in place (include/sbx.h); 'peer_stores': every rank writes its pixels straight into rank 0's frame
        through peer access (no RCCL, no slabs, nothing for rank 0 to land or scatter; unmeasured on more than one device)."""
        self._check(self.lib.sbx_multi_set_exchange(self.m, {"slabs": 0, "blocks": 1, "spans": 2, "peer_stores": 3}[mode] if isinstance(mode, str) else int(mode)))

    def set_noise_volumes(self, shape_rgba, detail_rgba):
        self._check(self.lib.sbx_multi_set_noise_volumes(self.m, int(shape_rgba.shape[0]), ctypes.c_void_p(shape_rgba.data_ptr()),
                                                         int(detail_rgba.shape[0]), ctypes.c_void_p(detail_rgba.data_ptr())))

    def render(self, app, width, height, time, mouse=(0.0, 0.0), aux=None, out=None):
        """The whole frame over all ranks; asynchronous on the current stream of devices[0]."""
        u = Renderer.uniforms(width, height, time, mouse)
        dt = getattr(self, "pixel_dtype", self.torch.float32)
        if out is None:
            out = self.torch.empty((int(height), int(width), 4), dtype=dt, device=self.tdev)
        assert out.is_cuda and out.dtype == dt and out.is_contiguous() and out.numel() >= int(height) * int(width) * 4
        stream = ctypes.c_void_p(self.torch.cuda.current_stream(self.tdev).cuda_stream)
        self._check(self.lib.sbx_multi_render(self.m, app_id(app), ctypes.byref(u), Renderer._auxp(aux),
                                              ctypes.c_void_p(out.data_ptr()), stream))
        return out
