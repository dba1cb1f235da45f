"""numpy restatement of the three builds of src/app_sdf_ao.h: SBX_APP_SDF_AO ("default", both `#if 0` blocks off as shipped),
SBX_APP_SDF_AO_SHADOW ("shadow", the block at :269-274 on) and SBX_APP_SDF_AO_NORMALS ("normals", the block at :217-219 on);
include/sbx.h, DESIGN.md §5.11.

The CPU oracle renders the shipped build only and is not to grow, so the GPU tests of the two other builds compare against this
module.  It is pinned from two sides (tests/test_sdf_ao_builds_cpu.py): build "default" equals Oracle.render("sdf_ao") in every
bit — which covers everything the three builds share: camera, march, sdf, normal, AO, lights, materials, fog, epilogue — and
builds "shadow" / "normals" equal frames that the reference header itself rendered with the one `#if 0` turned to `#if 1`
(tests/golden/sdf_ao_builds/, tools/make_golden_builds.py).

mainImage -> render -> render_impl -> sdf_shadow / illuminate, vectorised over pixels, in binary32 step by step in the oracle's
operation order (oracle/ovec.h: dot = (x x + y y) + z z, normalize = three divisions by sqrtf; oracle/sbx_math_ref.h: min / max as
compare-and-select, mix = x (1 - a) + y a), every value an explicit np.float32 so that nothing widens to float64.  sin, cos, exp
and pow are the oracle's (Oracle.math).  sdf is restated here (a known-answer hook per point would take minutes per frame) and
pinned against the hook `sdf_ao.sdf`; the vector algebra and the camera are tests/model_common.py's.
"""
import concurrent.futures
import functools
import struct

import numpy as np

from tests.model_common import (F, ONE, TWO, ZERO, _const, _f, _sincos, builds_fixture, dot, fmax, fmin, get_primary_ray,
                                 normalize, op_add2, oracle, point_cam, same_bits)

BUILDS = ("default", "shadow", "normals")
FOG_DENSITY, FOG_FALLOFF = F(.1), F(.5)             # src/uniform_buffer.h:56-60 (oracle/ref_lib.h sdf_ao_aux_t)
SIZE = (F(1.3), F(1.), F(1.25))                     # :52
MATERIALS = np.array([[1, 1, 1], [0, .2, 0], [.1, .1, .1], [.1, .1, .1], [.1, .1, .1], [.4, .4, .4]], dtype=F)   # :35-43
FOV = F(1.)                                         # :313


def aux_bytes(aux):
    """the sbx_aux_sdf_ao block (16 bytes) for Oracle.render / the C ABI; aux = (fog_density, fog_falloff) or None"""
    return None if aux is None else struct.pack("4f", float(F(aux[0])), float(F(aux[1])), 0.0, 0.0)


# ---- the scene -----------------------------------------------------------------------------------------------------------

_ROT = {}


def _rot():
    """(s, c) of rotate_around_x(-90) and rotate_around_y(180) (:63, :134; util.h:53-69)"""
    if not _ROT:
        _ROT["x"] = _sincos(-90.0)
        _ROT["y"] = _sincos(180.0)
    return _ROT["x"], _ROT["y"]


def sd_box(p, b):                                   # sdf.h:67-73
    return fmax(np.abs(p[0]) - b[0], fmax(np.abs(p[1]) - b[1], np.abs(p[2]) - b[2]))


def sd_y_cylinder(p, r, h):                         # sdf.h:85-93
    return fmax(np.sqrt(p[0] * p[0] + p[2] * p[2]) - r, np.abs(p[1]) - h / TWO)


def _mul_rx(p, s, c):                               # mul(p, rotate_around_x): columns (1,0,0), (0,c,-s), (0,s,c)
    return ((p[0] * ONE + p[1] * ZERO) + p[2] * ZERO, (p[0] * ZERO + p[1] * c) + p[2] * (-s), (p[0] * ZERO + p[1] * s) + p[2] * c)


def _mul_ry(p, s, c):                               # mul(p, rotate_around_y): columns (c,0,s), (0,1,0), (-s,0,c)
    return ((p[0] * c + p[1] * ZERO) + p[2] * s, (p[0] * ZERO + p[1] * ONE) + p[2] * ZERO, (p[0] * (-s) + p[1] * ZERO) + p[2] * c)


def sdf_pipe(pos):                                  # :54-113
    (sx, cx), _ = _rot()
    size = SIZE
    p = (pos[0], pos[1] - size[1], pos[2])
    b = sd_box(p, size)
    p = (p[0] - F(.7), p[1] - F(.5), p[2])
    p = _mul_rx(p, sx, cx)
    c = sd_y_cylinder(p, size[1] + F(.55), TWO * size[2] + F(.1))
    pipe = (fmax(b, -c), _const(2, b))              # op_sub, mat_pipe

    p = (pos[0], pos[1] - size[1], pos[2])
    p = (p[0] - (-size[0] + F(.525)), p[1] - size[1], p[2])
    p = _mul_rx(p, sx, cx)
    coping = (sd_y_cylinder(p, F(.025), TWO * size[2]), _const(5, b))

    p = (pos[0], pos[1] - size[1] * TWO, pos[2])
    rail = sd_box((p[0] + size[0], p[1] + F(-.25), p[2] + ZERO), (F(.025), F(.05), size[2]))
    B = (F(.025), F(.125), F(.025))
    H = F(-.125)
    x, y = p[0] + size[0], p[1] + H
    bar_1 = sd_box((x, y, p[2] + ZERO), B)
    bar_2 = sd_box((x, y, p[2] + size[2] / TWO), B)
    bar_3 = sd_box((x, y, p[2] + size[2]), B)
    bar_4 = sd_box((x, y, p[2] + (-size[2] / TWO)), B)
    bar_5 = sd_box((x, y, p[2] + (-size[2])), B)
    b_a = fmin(bar_1, bar_2)
    b_b = fmin(b_a, bar_3)
    b_c = fmin(bar_4, bar_5)
    bars = fmin(b_b, b_c)
    railing = (fmin(rail, bars), _const(4, b))      # mat_deck
    deck = op_add2(railing, coping)
    return op_add2(pipe, deck)


def sdf(px, py, pz):
    """sdf(pos) (:115-150) -> (distance, material id as float), arrays like px"""
    _, (sy, cy) = _rot()
    size = SIZE
    with np.errstate(all="ignore"):
        pos = (_f(px), _f(py), _f(pz))
        B = F(.15)
        p = (pos[0], pos[1] - B, pos[2])
        bottom = (sd_box(p, (F(2.25) * size[0], B, size[2])), _const(3, pos[0]))
        pipe1 = sdf_pipe((p[0] + F(1.25) * size[0], p[1] + ZERO, p[2] + ZERO))
        p = (p[0] - F(1.25) * size[0], p[1], p[2])
        p = _mul_ry(p, sy, cy)
        pipe2 = sdf_pipe(p)
        pipe = op_add2(pipe1, pipe2)
        ref = (sd_box(pos, (F(.025), F(15), F(.025))), _const(0, pos[0]))
        ground = (((ZERO * pos[0] + ONE * pos[1]) + ZERO * pos[2]) + ZERO, _const(1, pos[0]))
        g = op_add2(ground, ref)
        b = op_add2(pipe, bottom)
        return op_add2(b, g)


def sdf_normal(p):                                  # :152-163
    dt = F(0.001)
    with np.errstate(all="ignore"):
        v = (sdf(p[0] + dt, p[1] + ZERO, p[2] + ZERO)[0] - sdf(p[0] - dt, p[1], p[2])[0],
             sdf(p[0] + ZERO, p[1] + dt, p[2] + ZERO)[0] - sdf(p[0], p[1] - dt, p[2])[0],
             sdf(p[0] + ZERO, p[1] + ZERO, p[2] + dt)[0] - sdf(p[0], p[1], p[2] - dt)[0])
        return normalize(v)


def sdf_ao(origin, normal):                         # :165-181 -> c
    dt = F(.5)
    occlusion = np.zeros(origin[0].shape, dtype=F)
    with np.errstate(all="ignore"):
        for k in range(1, 6):
            i = F(k)
            s = dt * i
            d = sdf(origin[0] + s * normal[0], origin[1] + s * normal[1], origin[2] + s * normal[2])[0]
            pw = oracle().math("pow", _f([2.0]), i)[0]
            occlusion = occlusion + ONE / pw * (dt * i - d)
        return ONE - fmin(fmax(occlusion, ZERO), ONE)


def sun_dir():                                      # :209
    return normalize((F(1), F(2), F(1)))


def sdf_shadow(ox, oy, oz, trace=None):
    """sdf_shadow({origin, sun_dir}) (:183-207), the statements of :192-204 in their order.  trace: a dict that receives "exit", per
    ray 0 = the loop ran out, 1 = `t > end`, 2 = `d.x < .005`."""
    steps, end, penumbra_factor, darkest = 20, F(20.), F(32.), F(.05)
    o = (_f(ox), _f(oy), _f(oz))
    n = o[0].size
    dr = sun_dir()
    t = np.zeros(n, dtype=F)
    umbra = np.ones(n, dtype=F)
    out = np.zeros(n, dtype=F)
    how = np.zeros(n, dtype=np.int8)
    done = np.zeros(n, dtype=bool)
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            if act.size == 0:
                break
            ta = t[act]
            d = sdf(o[0][act] + dr[0] * ta, o[1][act] + dr[1] * ta, o[2][act] + dr[2] * ta)[0]
            brk = ta > end
            dark = ~brk & (d < F(.005))
            go = ~brk & ~dark
            out[act[dark]] = darkest
            done[act[dark]] = True
            how[act[dark]] = 2
            how[act[brk]] = 1
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], penumbra_factor * d[go] / tn)
            act = act[go]
    out = np.where(done, out, umbra)
    if trace is not None:
        trace["exit"] = how
    return out


# ---- the pixel -----------------------------------------------------------------------------------------------------------

def camera(u_time):
    """(eye, look_at) of setup_camera (:45-50): eye = mul(rotate_around_y(u_time * 50), (0, 3, 5))"""
    with np.errstate(all="ignore"):
        s, c = _sincos(F(u_time) * F(50.))
        col0, col1, col2 = (c, ZERO, s), (ZERO, ONE, ZERO), (-s, ZERO, c)
        v = (F(0), F(3), F(5))
        eye = tuple((col0[k] * v[0] + col1[k] * v[1]) + col2[k] * v[2] for k in range(3))
    return eye, (ZERO, ZERO, ZERO)


def render_impl(build, ro, rd, parts=None):
    """render_impl (:245-285) for rays (ro, rd[3][n]) -> (rgb[n, 3], t[n]).  parts: a dict that receives hit, p, normal, ao, sh, mat."""
    n = rd[0].size
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(70):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k] + rd[k][act] * ta for k in range(3))
            d, m = sdf(*pi)
            brk = ta > F(20.)
            h = ~brk & (d < F(.005))
            go = ~brk & ~h
            ih = act[h]
            hit[ih] = True
            mat[ih] = m[h].astype(np.int32)
            for k in range(3):
                p[k][ih] = pi[k][h]
            t[act[go]] = ta[go] + d[go]
            act = act[go]
        rgb = np.empty((n, 3), dtype=F)
        rgb[:] = (F(.1), F(.1), F(.7))              # background :9-12
        ih = np.flatnonzero(hit)
        if parts is not None:
            parts.update(hit=hit, p=np.stack(p, axis=1), mat=mat)
        if ih.size:
            ph = tuple(c[ih] for c in p)
            nrm = sdf_normal(ph)
            if parts is not None:
                parts["normal"] = np.stack(nrm, axis=1)
            if build == "normals":                  # illuminate :217-219 compiled in
                rgb[ih] = np.stack(nrm, axis=1)
                return rgb, t
            ao = sdf_ao(ph, nrm)
            sd = sun_dir()
            sh = np.ones(ih.size, dtype=F)
            if build == "shadow":                   # :269-274 compiled in
                sh = sdf_shadow(ph[0] + sd[0] * F(0.05), ph[1] + sd[1] * F(0.05), ph[2] + sd[2] * F(0.05))
            if parts is not None:
                parts.update(ao=ao, sh=sh)
            # illuminate :220-242
            sun_ray = fmax(ZERO, dot(sd, nrm))
            key = sh * sun_ray
            accum = [ZERO + key * c for c in (F(1.2), F(1.3), F(1.))]
            hem = ao * nrm[1]
            accum = [a + hem * c for a, c in zip(accum, (F(.15), F(.15), F(.4)))]
            ind = fmax(ZERO, dot((sd[0] * F(-1), sd[1] * F(0), sd[2] * F(-1)), nrm))
            fill = ao * ind
            accum = [a + fill * c for a, c in zip(accum, (F(.4), F(.28), F(.2)))]
            mh = mat[ih]
            ok = (mh >= 0) & (mh < len(MATERIALS))
            mat_c = np.where(ok[:, None], MATERIALS[np.clip(mh, 0, len(MATERIALS) - 1)], ZERO).astype(F)
            ground = mh == 1
            pat = np.floor(ph[0] * F(.5)) + np.floor(ph[2] * F(.5))   # checkboard_pattern util.h:95-101
            cb = pat - TWO * np.floor(pat / TWO)
            lo, hi = mat_c - F(.15) * mat_c, mat_c + F(.15) * mat_c
            mixed = lo * (ONE - cb)[:, None] + hi * cb[:, None]
            mat_c = np.where(ground[:, None], mixed, mat_c)
            rgb[ih] = np.stack(accum, axis=1) * mat_c
    return rgb, t


def main_image(build, width, height, u_time, fx, fy, aux=None, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]; aux = (fog_density, fog_falloff) or None for the defaults"""
    assert build in BUILDS, build
    density, falloff = (FOG_DENSITY, FOG_FALLOFF) if aux is None else (F(aux[0]), F(aux[1]))
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), FOV)
    eye, look_at = camera(u_time)
    rd = get_primary_ray(pcx, pcy, eye, look_at)
    rgb, t = render_impl(build, eye, rd, parts)
    o = oracle()
    with np.errstate(all="ignore"):                 # render :287-311
        e0 = o.math("exp", _f(-eye[1] * falloff).reshape(1))[0]
        e1 = o.math("exp", (-t) * rd[1] * falloff)
        fog = density * e0 * (ONE - e1) / (rd[1] * falloff)
        col = np.abs(rgb * (ONE - fog)[:, None] + ONE * fog[:, None])
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = o.math("pow", np.ascontiguousarray(col).ravel(), F(1) / F(2.2)).reshape(col.shape)
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, aux=None, rows=None, threads=8):
    """float32 [rows, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre); large frames go by row bands on `threads`
    threads (numpy and the oracle's math release the interpreter lock)"""
    ys = np.arange(height) if rows is None else np.asarray(list(rows))
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    band = max(1, 16384 // max(int(width), 1))
    bands = [ys[i:i + band] for i in range(0, len(ys), band)]
    _rot()

    def one(b):
        return main_image(build, width, height, u_time, fx, (b.astype(F) + F(.5))[:, None], aux)

    if len(bands) <= 1 or threads <= 1:
        return np.concatenate([one(b) for b in bands], axis=0)
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as ex:
        return np.concatenate(list(ex.map(one, bands)), axis=0)


fixture = functools.partial(builds_fixture, "sdf_ao")     # tests/golden/sdf_ao_builds/ decoded: tests/model_common.py
