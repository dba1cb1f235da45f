"""The aux sets of the reference builds: tests/golden/reference_aux_sets.json read into aux blocks and into make rules.

TEST INFRASTRUCTURE ONLY (oracle/README.md).  In the reference's C++ form an aux uniform is a compile-time constant
(`_uniform(type, name, default)` is `const type name = default`, src/uniform_buffer.h:13), so a reference build has ONE aux block
compiled in.  The fixture names the blocks that get a build of their own: a set name mapped to the fields that differ from the
defaults.  `python aux_sets.py` prints the make rules of those builds (oracle/Makefile includes the output as _ref/aux_sets.mk):
per set, one -D'SBX_REF_AUX_<field>(d)=<literal>' for every field the set names (oracle/glsl_env.h has the pass-throughs).

One binary32 value per field goes both ways: `literal()` writes %.9g of it, which -fsingle-precision-constant reads back to the
same binary32, and `block()` stores it in the bytes the oracle and the kernels take, so no case depends on decimal rounding.
"""
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(os.path.dirname(_HERE), "tests", "golden", "reference_aux_sets.json")

# the aux blocks (cbuffer b1) as include/sbx.h lays them out, with the defaults of src/uniform_buffer.h:41-54,58-59
LAYOUT = {
    "clouds": np.dtype([("wind_dir", "<f4", 3), ("_pad0", "<f4"), ("sun_dir", "<f4", 3), ("_pad1", "<f4"),
                        ("sun_color", "<f4", 3), ("_pad2", "<f4"), ("sun_power", "<f4"), ("cld_march_steps", "<i4"),
                        ("illum_march_steps", "<i4"), ("sigma_scattering", "<f4"), ("cld_coverage", "<f4"), ("cld_thick", "<f4"),
                        ("atm_radius", "<f4"), ("atm_ground_y", "<f4")]),
    "sdf_ao": np.dtype([("fog_density", "<f4"), ("fog_falloff", "<f4"), ("_pad", "<f4", 2)]),
}
DEFAULTS = {
    "clouds": {"wind_dir": (0, 0, .2), "sun_dir": (0, 0, -1), "sun_color": (1., .7, .55), "sun_power": 8.,
               "cld_march_steps": 100, "illum_march_steps": 6, "sigma_scattering": .15, "cld_coverage": .535, "cld_thick": 125.,
               "atm_radius": 5000., "atm_ground_y": 4750.},
    "sdf_ao": {"fog_density": .1, "fog_falloff": .5},
}
# the reference builds that compile each block, with their header and defines (oracle/Makefile has the same two for the defaults)
BUILDS = {
    "clouds": (("clouds", "app_clouds.h", "-DAPP_CLOUDS"), ("clouds_sky", "app_clouds.h", "-DAPP_CLOUDS -DSKY_SPHERE")),
    "sdf_ao": (("sdf_ao", "app_sdf_ao.h", "-DAPP_SDF_AO"),),
}
KIND_OF = {build: kind for kind, builds in BUILDS.items() for build, _, _ in builds}


def fields(kind):
    return [n for n in LAYOUT[kind].names if not n.startswith("_pad")]


def load():
    """{kind: {set name: {field: value}}} of the fixture, checked: known kinds and fields, names fit for a file name"""
    with open(FIXTURE) as f:
        sets = json.load(f)
    for kind, by_name in sets.items():
        assert kind in LAYOUT, "aux sets: unknown block %r" % kind
        for name, over in by_name.items():
            assert name.isidentifier() and name != "defaults", "aux sets: bad set name %r" % name
            assert over and set(over) <= set(fields(kind)), "aux sets: %s names fields the %s block lacks" % (name, kind)
    return sets


def block(kind, over=None):
    """the aux block of `kind` with the fields of `over` in place of the defaults: a numpy record of LAYOUT[kind]"""
    b = np.zeros((), dtype=LAYOUT[kind])
    for name, v in dict(DEFAULTS[kind], **(over or {})).items():
        assert b.dtype[name].kind != "i" or v == int(v), "aux sets: %s is an integer field" % name
        b[name] = v
    return b


def same_block(kind, a, b):
    """field for field over the bits (padding aside): -0 is not 0, a NaN equals only the same NaN"""
    return all(np.array_equal(np.asarray(a[n]).view(np.uint32), np.asarray(b[n]).view(np.uint32)) for n in fields(kind))


def from_bytes(kind, aux):
    """the block a caller passes (a ctypes structure of shaderbox_amd, bytes, or a record of `block`) as a record"""
    raw = aux.tobytes() if isinstance(aux, np.ndarray) else bytes(aux)
    if len(raw) != LAYOUT[kind].itemsize:
        raise ValueError("aux block of %d bytes, the %s block has %d" % (len(raw), kind, LAYOUT[kind].itemsize))
    return np.frombuffer(raw, dtype=LAYOUT[kind])[0]


def literal(value):
    """the C++ text of one field of a block: integers as integers, floats as %.9g of the binary32 value with a decimal point or
    an exponent, vec3 as vec3(a,b,c); negative numbers in parentheses where they stand alone"""
    value = np.asarray(value)

    def num(v):
        if value.dtype.kind == "i":
            return "%d" % int(v)
        s = "%.9g" % float(np.float32(v))
        assert "n" not in s, "aux sets: inf and NaN have no literal"
        return s if ("." in s or "e" in s) else s + ".0"
    if np.ndim(value):
        return "vec3(%s)" % ",".join(num(v) for v in value)
    return "(%s)" % num(value)


def defines(kind, over):
    b = block(kind, over)
    return " ".join("-D'SBX_REF_AUX_%s(d)=%s'" % (n, literal(b[n])) for n in fields(kind) if n in over)


def build_names(sets=None):
    """every aux-set build: `<build>@<set>`, in the fixture's order"""
    sets = load() if sets is None else sets
    return [b + "@" + name for kind, by_name in sets.items() for name in by_name for b, _, _ in BUILDS[kind]]


def make_rules():
    sets = load()
    out = ["# generated by oracle/aux_sets.py from tests/golden/reference_aux_sets.json: the aux-set builds of `make ref`",
           "REF_AUX_NAMES = " + " ".join(build_names(sets))]
    for kind, by_name in sets.items():
        for name, over in by_name.items():
            for b, hdr, defs in BUILDS[kind]:
                t = "_ref/libsbx_ref_%s@%s.so" % (b, name)
                out += ["%s: REF_HDR = %s" % (t, hdr), "%s: REF_DEFS = %s %s" % (t, defs, defines(kind, over))]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.stdout.write(make_rules())
