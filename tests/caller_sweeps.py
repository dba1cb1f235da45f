"""Seeded random TAME blocks for the three apps whose shortcuts are derived from the caller's data: poses of SBX_APP_EGG_POSE, decks of
SBX_APP_VINYL_DECK and airs of SBX_APP_ATMOSPHERE_AIR's run-time tier.  `egg_pose(cls, seed)`,
`vinyl_deck(cls, seed)` and `atmosphere_air(cls, seed)` return what the models' pose(...), deck(...) and air(...) return, every value
rounded to binary32 once, the same block for the same (cls, seed) on every run.  CASES names the classes and their seeds;
`egg_pose_tame`, `vinyl_deck_tame` and `atmosphere_air_tame` state in Python the rule by which the library's predicates of those names
admit a block to the culled, witnessed kernels and to the fast body.  tests/test_caller_sweeps_cpu.py asserts of the models alone that
every block is tame and that the frames show what the sweep is about; tests/test_gpu_caller_sweeps.py (poses, decks) and
tests/test_gpu_caller_sweeps_air.py (airs) hold the kernels to the models over them.

A plain module (pytest does not collect it).  It reads the three model modules and nothing else of the project; the generators compute
in binary64 except where they place a camera relative to the figure, which takes the model's own binary32 rotation (at a turn of
1e9 degrees a binary64 cosine of the same angle is another rotation altogether)."""
import numpy as np

from tests import atmosphere_air_model as M
from tests import egg_pose_model as E
from tests import vinyl_deck_model as D

F = np.float32
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
CASES = {
    "egg_pose": {
        "studio": SEEDS,          # the whole figure from outside, any side
        "close": SEEDS,           # .4 - 2.0 from a joint, cameras inside the bounding sphere among them
        "giant": SEEDS,           # bones of 5 ... 3000: the bounds' absolute margins are the size of an ulp
        "spun": SEEDS,            # studio under a turn of 1e3 ... 1e9 degrees
    },
    "vinyl_deck": {
        "tilted": SEEDS,          # the shipped camera; tilts up to 90 degrees, any sun above
        "orbit": SEEDS,           # the camera moves: any side, .5 - 1.5 of the shipped distance
        "wild": SEEDS,            # orbit's camera; angles up to 1e9, an un-normalised sun, colours and constants of either sign
    },
    "atmosphere_air": {
        "ground": SEEDS,          # the dome from 1 m - 3 km up, the eye off the y axis, any sun above -5 degrees
        "aloft": SEEDS,           # 3 - 59 km up; the dome or the camera, which then looks down into the planet
        "thick": SEEDS,           # ground under betas of 3 - 100 times more: tau crosses the ballot's 80 inside the lit sky
        "lopsided": SEEDS,        # ground with one beta 0., -0. or negative: the dead-ray exit is off
        "dusk": SEEDS,            # the sun 12 degrees under to 3 over the local horizon, either view
    },
}
_STREAM = {"studio": 11, "close": 12, "giant": 13, "spun": 14, "tilted": 21, "orbit": 22, "wild": 23,
           "ground": 41, "aloft": 42, "thick": 43, "lopsided": 44, "dusk": 45}


def _rng(cls, seed):
    return np.random.default_rng([_STREAM[cls], int(seed)])


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _log_uniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


# ---- SBX_APP_EGG_POSE -----------------------------------------------------------------------------------------------------------------

OFFSET = np.array([0., .5, 3.5])                     # app_egg.h:40-41: p = rot_y(turn_deg) P - (0, .5, 3.5)
GROUND_Y = -1.7                                      # :136-138: the ground is the plane P.y = -(1.2 + .5)


def rot_y(turn_deg):
    """the model's rot_y of a turn (binary32 sine and cosine of the binary32 angle) as a binary64 matrix: p = R P - OFFSET"""
    c0, c1, c2 = E.rotate_around_y(F(turn_deg))
    return np.array([c0, c1, c2], dtype=np.float64).T


def world(R, m):
    """where a point at m of the figure's space is in the world: rot_y^T (m + (0, .5, 3.5))"""
    return R.T @ (np.asarray(m, dtype=np.float64) + OFFSET)


def _foot(rng, pelvis, femur, tibia):
    """a foot at a distance from its pelvis inside the open reach interval (|f - t|, f + t), 5 % in from both ends, any direction"""
    lo, hi = abs(femur - tibia), femur + tibia
    return pelvis + _unit(rng) * rng.uniform(lo + .05 * (hi - lo), hi - .05 * (hi - lo))


def egg_pose(cls, seed):
    """A tame pose of class cls.  Every class: a turn in +-360 degrees, femur and tibia in [.3, 1.5], each foot within its reach in any
    direction, fov in [.6, 1.2].
      studio  the eye 1.5 - 2.5 from the figure's centre at an elevation of 5 - 60 degrees on any side, look_at jittered by .3
      close   the eye .4 - 2.0 (log-uniform) from a pelvis point, a knee or a foot, looking at it; one eye in five inside the egg
      giant   femur and tibia log-uniform in [5, 3000]; the eye .3 - 1.2 from a point of a leg, looking at it or along the leg
      spun    studio with a turn of either sign and a log-uniform magnitude in [1e3, 1e9]"""
    rng = _rng(cls, seed)
    if cls == "spun":
        turn = float(rng.choice([-1., 1.]) * _log_uniform(rng, 1e3, 1e9))
    else:
        turn = rng.uniform(-360., 360.)
    femur, tibia = _log_uniform(rng, 5., 3000., 2) if cls == "giant" else rng.uniform(.3, 1.5, 2)
    lf = _foot(rng, np.array([0., 0., .2]), femur, tibia)
    rf = _foot(rng, np.array([0., 0., -.2]), femur, tibia)
    rider = dict(turn_deg=turn, femur=femur, tibia=tibia)
    S = E.scene_of(E.pose(lf, rf, **rider))           # the knees as the model's ik_solver places them
    R = rot_y(turn)
    knee_l, knee_r = np.array(S["knee_l"], dtype=np.float64), np.array(S["knee_r"], dtype=np.float64)
    fov = rng.uniform(.6, 1.2)
    if cls in ("studio", "spun"):
        centre = world(R, (0., -.1, 0.))             # between the egg (p.y = .65) and the wheel's hub (p.y = -1.2)
        az, el = rng.uniform(0., 2. * np.pi), np.radians(rng.uniform(5., 60.))     # above the figure's centre, so above the ground
        eye = centre + np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)]) * rng.uniform(1.5, 2.5)
        look_at = centre + rng.uniform(-.3, .3, 3)
    elif cls == "close":
        # members sit at -pelvis, -knee, -foot of the figure's space (:111-116)
        joints = [np.array([0., 0., .2]), knee_l, lf, np.array([0., 0., -.2]), knee_r, rf]
        target = world(R, -joints[rng.integers(len(joints))])
        eye = target + _unit(rng) * _log_uniform(rng, .4, 2.0)
        look_at = target
        if rng.uniform() < .2:                      # from within the egg's middle sphere (:47): every march ends at its first step
            eye = world(R, np.array([0., .65, 0.]) + _unit(rng) * rng.uniform(0., .4))
        if eye[1] < GROUND_Y + .1:                   # not from under the ground: mirrored about the joint, or lifted above the plane
            eye[1] = max(2. * target[1] - eye[1], GROUND_Y + .1 + abs(eye[1] - GROUND_Y))
    else:
        # A leg is the quadratic Bezier curve from -pelvis to -foot whose CONTROL point is -knee (:111-116): at this scale it passes
        # hundreds of units from its knee, so "near a knee" is near the curve at a parameter s, and s = 1 is the foot.  Half of the
        # points of a leg are under the ground plane, where every march ends at its first step: the point is drawn again until it is
        # 1.5 above it, and where both legs dive at once, s is halved until it is (the pelvis end always is).
        point = lambda s: world(R, -((1. - s) ** 2 * a + 2. * s * (1. - s) * k + s * s * c))  # noqa: E731
        for _ in range(64):
            left = rng.uniform() < .5
            a, k, c = (np.array([0., 0., .2 if left else -.2]), knee_l if left else knee_r, lf if left else rf)
            s = 1. if rng.uniform() < .25 else rng.uniform(.02, 1.)
            if point(s)[1] > GROUND_Y + 1.5:
                break
        while point(s)[1] <= GROUND_Y + 1.5:
            s *= .5
        target = point(s)
        eye = target + _unit(rng) * rng.uniform(.3, 1.2)
        look_at = target
        if rng.uniform() < .5:                       # along the leg instead of at it
            along = R.T @ -(2. * (1. - s) * (k - a) + 2. * s * (c - k))
            look_at = eye + along / np.linalg.norm(along) * rng.choice([-1., 1.])
    return E.pose(lf, rf, eye=eye, look_at=look_at, fov=fov, **rider)


def _finite(*values):
    return bool(np.isfinite(np.array(values, dtype=np.float64)).all())


def egg_pose_tame(P):
    """The rule of egg_pose_tame (shaderbox_amd/csrc/sbx_frames.hip:177-191) as far as the model states a pose's frame: every value
    of the block finite and within 1e4 in magnitude, the angle within 1e10 (:183); every derived frame constant finite (:184-190), which
    for the model's scene means the rotation, the knees and the toes (the Bezier frames, the foot cylinders and the bounding sphere of
    :186-190 are functions of those) and a camera whose eye differs from look_at (fwd = normalize(0) is 0 / 0, :188) with a view that
    is not parallel to the up vector (util.h:12: right = cross(up, fwd) is zero there and every ray is the view's own)."""
    a = E.block(P)
    bound = np.full(16, F(1e4))
    bound[7] = F(1e10)
    if not (np.isfinite(a).all() and (np.abs(a) <= bound).all()):
        return False
    S = E.scene_of(P)
    if not _finite(*S["rot_y"][0], *S["rot_y"][2], *S["knee_l"], *S["knee_r"], *S["left_toe"], *S["right_toe"]):
        return False
    return _camera_stands(P["eye"], P["look_at"])


def _camera_stands(eye, look_at):
    view = np.array(look_at, dtype=F) - np.array(eye, dtype=F)       # util.h:10, in binary32 as the frame forms it
    return bool(view.any() and (view[0] != 0 or view[2] != 0) and np.isfinite(view).all())


# ---- SBX_APP_VINYL_DECK ---------------------------------------------------------------------------------------------------------------

SHIPPED_EYE = np.array(D.SHIPPED_EYE, dtype=np.float64)
SHIPPED_LOOK_AT = np.array(D.SHIPPED_LOOK_AT, dtype=np.float64)
PIVOT = np.array([-7., 0., -5.])                     # the tonearm's base (app_vinyl.h:131), for the tests' points near it


def _sun_above(rng, fields):
    """A random direction in the upper half space with a length in [.5, 2], drawn again until it stands at least 37 degrees off the
    disc's own plane on the side the eye is on.  illuminate's ro_spec / sqrt(dot(L, N) * dot(V, N)) (:331) is a NaN wherever the sun and the
    eye are on different sides of a groove's normal — a frame of a low sun over a steep disc is mostly NaN and shows the culls
    nothing (`wild` draws any sun and keeps those frames).  The disc's plane is the model's: the y row of platter_rot."""
    side = np.sign(_off_the_disc(fields, fields.get("eye", SHIPPED_EYE)))
    for _ in range(256):
        d = _unit(rng)
        d[1] = abs(d[1])
        if side * _off_the_disc(fields, d) >= .6:
            break
    return d * rng.uniform(.5, 2.)


def _off_the_disc(fields, v):
    """the sine of the angle between v and the disc's own plane under the deck's angles, signed: the y of v in the platter's space"""
    S = D.scene_of(D.deck(**fields))
    v = np.asarray(v, dtype=np.float64)
    return float(D.V.vec_mat(tuple(F(c) for c in v / np.linalg.norm(v)), S["platter_rot"])[1])


def _orbit_camera(rng):
    """the eye above the disc on a hemisphere around the shipped look_at at .5 - 1.5 of the shipped distance, look_at jittered by up
    to 2, fov in [.6, 1.4] — but no wider than 1.15 / that factor, so that the deck is not a speck in a wide view from afar"""
    d = _unit(rng)
    d[1] = abs(d[1]) * .5 + .7                       # an elevation that keeps the eye above the disc's plane from look_at's 2.5 below it
    factor = rng.uniform(.5, 1.5)
    dist = np.linalg.norm(SHIPPED_EYE - SHIPPED_LOOK_AT) * factor
    return dict(eye=SHIPPED_LOOK_AT + d / np.linalg.norm(d) * dist, look_at=SHIPPED_LOOK_AT + _unit(rng) * rng.uniform(0., 2.),
                fov=rng.uniform(.6, min(1.4, 1.15 / factor)))


def vinyl_deck(cls, seed):
    """A tame deck of class cls.
      tilted  the shipped camera; platter_tilt_deg and arm_tilt_deg in +-90, platter_deg in +-720, _sun_above; the shipped colours
      orbit   _orbit_camera; both tilts in +-10, platter_deg in +-720, _sun_above; the shipped colours
      wild    _orbit_camera; the three angles of either sign and a log-uniform magnitude in [1, 1e9]; a sun in any direction with a
              log-uniform length in [1e-2, 1e4]; colours in [-.5, 1], ro_spec in [-.1, .3], a_x in [-.05, .1], a_y in [-.5, 1] and
              shininess in [-10, 80]"""
    rng = _rng(cls, seed)
    if cls == "tilted":
        fields = dict(arm_tilt_deg=rng.uniform(-90., 90.), platter_deg=rng.uniform(-720., 720.))
        for _ in range(256):                         # no disc that the shipped eye sees edge-on, within 30 degrees of its plane: a sliver, and
            fields["platter_tilt_deg"] = rng.uniform(-90., 90.)          # dot(V, N) changes sign from groove to groove
            if abs(_off_the_disc(fields, SHIPPED_EYE)) >= .5:
                break
        return D.deck(sun_dir=_sun_above(rng, fields), **fields)
    fields = _orbit_camera(rng)
    if cls == "orbit":
        fields.update(platter_tilt_deg=rng.uniform(-10., 10.), arm_tilt_deg=rng.uniform(-10., 10.), platter_deg=rng.uniform(-720., 720.))
        return D.deck(sun_dir=_sun_above(rng, fields), **fields)
    angle = lambda: float(rng.choice([-1., 1.]) * _log_uniform(rng, 1., 1e9))  # noqa: E731
    fields.update(platter_deg=angle(), platter_tilt_deg=angle(), arm_tilt_deg=angle(), sun_dir=_unit(rng) * _log_uniform(rng, 1e-2, 1e4))
    for name in ("groove_color", "dead_wax_color", "label_color", "logo_color", "shiny_color"):
        fields[name] = rng.uniform(-.5, 1., 3)
    fields.update(ro_spec=rng.uniform(-.1, .3), a_x=rng.uniform(-.05, .1), a_y=rng.uniform(-.5, 1.), shininess=rng.uniform(-10., 80.))
    return D.deck(**fields)


def vinyl_deck_tame(deck):
    """The rule of vinyl_deck_tame (shaderbox_amd/csrc/sbx_frames.hip:602-613): every value of the block finite; the first sixteen
    (camera, angles, sun; the groove colour's three floats are skipped) within 1e4 in magnitude, the three angles within 1e10
    (:606-607); every derived frame constant finite (:608-612): the two matrices and a camera as for a pose."""
    a = D.block(deck)
    if not np.isfinite(a).all():
        return False
    for i in range(12):
        if not abs(a[i]) <= (F(1e10) if i in (7, 11) else F(1e4)):
            return False
    if not abs(a[15]) <= F(1e10):
        return False
    S = D.scene_of(deck)
    if not _finite(*[c for col in S["platter_rot"] for c in col], *[c for col in S["wobble"] for c in col]):
        return False
    return _camera_stands(deck["eye"], deck["look_at"])


# ---- SBX_APP_ATMOSPHERE_AIR -----------------------------------------------------------------------------------------------------------

EARTH_RADIUS = 6360e3                                # app_atmosphere.h:37; every block keeps it, which is what tame means
AIR_SIZE = (64, 36)                                  # the frame on which the lit condition is stated
LIT_SHARE = .10
SUN_DRAWS = 16
TILT_LO = 12.                                        # degrees: how far the eye's zenith is off +y at the least
LOOK_AHEAD = 4096.                                   # metres from the eye to look_at: a coordinate of 6.4e6 m moves in steps of .5 m


def air_lit_share(A, width=AIR_SIZE[0], height=AIR_SIZE[1]):
    """the share of a frame's pixels that are sky with a colour above 0 (a NaN pixel is not lit)"""
    fx, fy = M.frame_coords(width, height)
    rgb, ground = M.parts(A, width, height, fx, fy)
    with np.errstate(all="ignore"):
        return float(((rgb > 0).any(axis=-1) & ~ground).mean())


def _local_frame(up):
    """two unit vectors that span the eye's horizon plane, from the world's x axis (up is never within 50 degrees of it)"""
    east = np.cross(up, [1., 0., 0.])
    east /= np.linalg.norm(east)
    return east, np.cross(up, east)


def _local_sun(rng, up, lo_deg, hi_deg):
    """a sun at an elevation in [lo, hi] degrees over the horizon of an eye whose zenith is `up`, at any azimuth, with a length of
    sqrt(1 + u), u uniform in +-9e-5: inside the tame domain's |dot(sun, sun) - 1| <= 1e-4 and never a unit vector"""
    e, a = np.radians(rng.uniform(lo_deg, hi_deg)), rng.uniform(0., 2. * np.pi)
    east, north = _local_frame(up)
    return (np.sin(e) * up + np.cos(e) * (np.cos(a) * east + np.sin(a) * north)) * np.sqrt(1. + rng.uniform(-9e-5, 9e-5))


def atmosphere_air(cls, seed):
    """A tame block of class cls that is not the literal tier's: the reference's radii, scale heights and counts bit for bit, and
    every other number another.  Every class: hg_g uniform in +-.95, sun_power log-uniform in [1, 100], each beta its reference value
    times a log-uniform factor in [.3, 3], a sun of _local_sun, and an eye at up (earth_radius + h), `up` TILT_LO ... 35 degrees off +y.
    The dome's zenith is +y wherever the eye is, so the eye's own nadir — the rays within 9 degrees of it pass within 1000 km of the
    centre and leave the class — is a spot inside the dome's circle, not the circle's edge; a dome block (view 0) has fov in
    [.8, 1.4] and an `up` that leans along the frame's long axis (within 40 degrees of +-x), which brings both into the frame.  A
    camera block (view 1) has fov in [.6, 1.4], an `up` that leans any way and look_at = eye + LOOK_AHEAD unit(d) with d.y in
    [-.3, .5]: an eye off the axis is below the plane y = earth_radius, whose test then admits the rays that dive into the planet.
      ground    view 0; h log-uniform in [1, 3e3] m; the sun -5 ... 90 degrees over the eye's horizon
      aloft     h uniform in [3e3, 59e3]; view 0 or 1, half each
      thick     ground, with betaR and betaM each times one more log-uniform factor in [3, 100]
      lopsided  ground, with one of the six betas 0., -0. or -(1e-9 ... 1e-6): AtmAir.dead_ok is off
      dusk      ground's h; view 0 or 1; the sun -12 ... 3 degrees over the horizon, drawn again (SUN_DRAWS times at most, and in view 1
                look_at with it: a camera that looks into the planet shows no sky under any sun) until LIT_SHARE of the 64x36 frame is lit"""
    rng = _rng(cls, seed)
    view = 0 if cls in ("ground", "thick", "lopsided") else int(rng.integers(2))
    fields = dict(view=view, hg_g=rng.uniform(-.95, .95), sun_power=_log_uniform(rng, 1., 100.), fov=rng.uniform(.6 if view else .8, 1.4))
    betaR = np.array(M.E.BETA_R, dtype=np.float64) * _log_uniform(rng, .3, 3., 3)
    betaM = np.array(M.E.BETA_M, dtype=np.float64) * _log_uniform(rng, .3, 3., 3)
    if cls == "thick":
        betaR, betaM = betaR * _log_uniform(rng, 3., 100.), betaM * _log_uniform(rng, 3., 100.)
    if cls == "lopsided":
        odd = (0., -0., -_log_uniform(rng, 1e-9, 1e-6))[rng.integers(3)]
        (betaR, betaM)[rng.integers(2)][rng.integers(3)] = odd
    tilt = np.radians(rng.uniform(TILT_LO, 35.))
    lean = np.radians(rng.uniform(0., 360.) if view else rng.uniform(-40., 40.) + rng.choice([0., 180.]))
    up = np.array([np.sin(tilt) * np.cos(lean), np.cos(tilt), np.sin(tilt) * np.sin(lean)])
    eye = up * (EARTH_RADIUS + (rng.uniform(3e3, 59e3) if cls == "aloft" else _log_uniform(rng, 1., 3e3)))
    fields.update(betaR=betaR, betaM=betaM, eye=eye)
    lo, hi = (-12., 3.) if cls == "dusk" else (-5., 90.)
    for _ in range(SUN_DRAWS if cls == "dusk" else 1):
        if view:
            a = rng.uniform(0., 2. * np.pi)
            d = np.array([np.cos(a), rng.uniform(-.3, .5), np.sin(a)])
            fields["look_at"] = eye + d / np.linalg.norm(d) * LOOK_AHEAD
        A = M.air(sun_dir=_local_sun(rng, up, lo, hi), **fields)
        if cls != "dusk" or air_lit_share(A) >= LIT_SHARE:
            break
    return A


def atmosphere_air_tame(A):
    """The rule of atmosphere_air_tame (shaderbox_amd/csrc/sbx_frames.hip:361-369): earth_radius, atmosphere_radius, hR and hM the
    reference's bit for bit and the counts 16 and 8 (air_default_geometry), and a sun whose three values are finite with
    |dot(sun, sun) - 1| <= 1e-4 in binary32, the dot summed as (x x + y y) + z z (air_sun_ok).  Nothing else of the block is asked:
    the betas, the eye and the rest are judged ray by ray on the device (csrc/sbx_atmosphere.h "CALLER'S AIR")."""
    return M.tame(A)
