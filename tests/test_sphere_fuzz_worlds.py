"""Random sphere worlds and cameras for the 1024-lane ring kernel (spheres_ldsn1024x144, K.ldsn_ring(); DESIGN.md §2,
"Camera rays against per-tile lists"), and what can be checked of them without a device.

make_case(rtw, seed) draws, from np.random.default_rng(3000 + seed) alone, a world inside F_SPHERES (spheres and moving
spheres; solid and checker textures; Lambertian, Metal, Dielectric, DiffuseLight; no wrappers: a world is moved by
adding an offset to its centres) and two or three cameras with their frames.  The world class is seed % 5:

  cluster  the r = 1000 ground (always-list) and 16-40 BVH spheres of radius 0.1-0.6, among them a glass ball with a
           negative-radius shell inside it, a coincident pair of different materials (the tie rule), an overlapping
           pair, and moving spheres displaced by up to 3 radii over [0, 1]
  field    jumpy-balls in miniature: the ground and a jittered grid of 150 .. as many r = 0.2 balls as still select
           the ring kernel (found from rtw_scene_info 3 and 11 by committing: <= 144 node4s, a stack bound <= 16), half moving
  bare     no giant (rtw_scene_info 5 == 0): 17-40 spheres with radii spread over 0.02-3
  dome     a cluster (of 20-40) inside an emissive sphere of radius -500: no path ever misses
  offset   a cluster with every centre, the ground's too, shifted by (+-2^k, +-2^k / 4, +-2^k), k in {8, 11, 14}
           (k = 14: lengths x8, so that radii stay >> one ulp of the coordinates): the large-M case of the margins

The camera classes (D(o): the distance from o to the farthest corner of the BVH members' box, D0: rtw_scene_info 15,
that box's diagonal; the host uses the tile lists when the four corners of the lens' bounding square have D <= D0):

  near    all four lens corners within 0.95 D0.  Lens radius from {0, 0.05, 0.5, 2}, focused at 0.3-4 times the distance
          to the point looked at, vfov from {1, 20, 90, 150}, a rolled vup that is not orthogonal to the view, a shutter of
          [0, 1], [0.3, 0.35] or the one-ulp instant; the eye outside the balls, inside the glass ball, between ball
          and shell, or within one lens radius of a ball's surface ("touching": part of the lens is inside the ball)
  sky     near, above everything and looking up: every camera ray misses (checked here in double at the corners of the
          lens square and the image: a ray's direction is affine in both).  Not drawn for dome worlds
  border  the eye's D within 0.2 % of D0 and a lens radius of 0.5 or 2: some lens corners near and some far, so the
          lists stay off, except where the camera looks at the box's farthest corner from just inside D0 in a world
          large enough (half of them are so aimed): the host decides either way
  far     D = 1.5-5 D0: the lists stay off and every start takes the far-origin walk

"lens wider than its focus cone": lens radius > focus distance x tan(vfov / 2).  (For a camera made by Camera::new the
lens plane is orthogonal to the beam frame's z axis, so the beam test's "focus interval in front of the lens interval"
still holds there up to rounding; what the case exercises is a beam that narrows towards the focus plane and widens
again beyond it, the t < 1 and t > 1 slopes of rtw_tile_beam.h, with a lens larger than the image rectangle.)

A world is committed here with RTW_LIST_MAX=0 (the caller's `knobs` fixture sets it before make_case) and needs no
device: rtw_scene_info 3-23 are valid when the upload failed.  tests/test_gpu_sphere_fuzz.py renders the cases."""
import os

import numpy as np
import pytest

from test_gpu_far import F_SPHERES, selected_kernel

RING_KERNEL = (16, 0, 8, F_SPHERES, 1024, 144, 0, 0)
CLASSES = ("cluster", "field", "bare", "dome", "offset")
CAMERA_CLASSES = ("near", "sky", "border", "far")
GIANTS = {"cluster": 1, "field": 1, "bare": 0, "dome": 2, "offset": 1}
FRAMES = [(40, 24), (37, 21), (13, 9), (2, 2), (64, 5), (5, 64)]
SPPS = [1, 2, 3, 5]
DEPTHS = [50, 50, 50, 3, 1]
LENSES = [0.0, 0.05, 0.5, 2.0]
VFOVS = [1.0, 20.0, 90.0, 150.0]
OFFSET_K = [8, 11, 14]
INSTANT_T1 = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
SHUTTERS = [(0.0, 1.0), (0.3, 0.35), (0.25, INSTANT_T1)]
BG = (0.7, 0.8, 1.0)
N_DEFAULT = 35  # the default seed range of tests/test_gpu_sphere_fuzz.py
FIELD_MIN, FIELD_GRID = 150, 32

_CASES = {}    # seed -> (build, cameras, meta): drawn once, only read
_ORACLE = {}   # (seed, camera index) -> (frame, rays, rays at max_depth + 1): rendered once, never written


# ---------------------------------------------------------------------------------------------------- worlds
class _World:
    """A world as data: materials and primitives in order, replayed onto a Scene by build()."""

    def __init__(self):
        self.mats, self.prims = [], []  # ("kind", args...), (c0, c1 or None, radius, material index, in the BVH)
        self.tags = set()

    def mat(self, *m):
        self.mats.append(m)
        return len(self.mats) - 1

    def sphere(self, c, r, m, bvh=True):
        self.prims.append((np.asarray(c, np.float64), None, float(r), m, bvh))

    def moving(self, c0, c1, r, m):
        self.prims.append((np.asarray(c0, np.float64), np.asarray(c1, np.float64), float(r), m, True))

    def shifted(self, off, scale=1.0):
        """every length times scale, then every centre plus off"""
        w = _World()
        w.mats, w.tags = list(self.mats), set(self.tags)
        for c0, c1, r, m, bvh in self.prims:
            if bvh:
                w.prims.append((c0 * scale + off, None if c1 is None else c1 * scale + off, r * scale, m, bvh))
            else:  # the ground keeps its radius and its top at the cluster's floor
                w.prims.append((c0 + off, None, r, m, bvh))
        return w

    def boxes(self):
        """the BVH members' boxes as the flattener forms them: centres +- |r| over the motion, padded by
        1e-4 + 4e-5 x the box's largest |coordinate| (rtw_flatten.cpp pad_box)"""
        out = []
        for c0, c1, r, _m, bvh in self.prims:
            if bvh:
                a = c0.astype(np.float32).astype(np.float64)
                b = a if c1 is None else c1.astype(np.float32).astype(np.float64)
                lo, hi = np.minimum(a, b) - abs(r), np.maximum(a, b) + abs(r)
                e = 1e-4 + 4e-5 * max(np.abs(lo).max(), np.abs(hi).max())
                out.append((lo - e, hi + e))
        return out

    def bounds(self):
        """the box of the BVH members' boxes (rtw_flatten.cpp far_bound's B; D0 is its diagonal)"""
        bx = self.boxes()
        return np.min([b[0] for b in bx], axis=0), np.max([b[1] for b in bx], axis=0)

    def build(self, s):
        ids = []
        for m in self.mats:
            if m[0] == "lambert":
                ids.append(s.lambertian_solid(m[1]))
            elif m[0] == "checker":
                ids.append(s.lambertian(s.checker(s.solid_rgb(*m[1]), s.solid_rgb(*m[2]), m[3])))
            elif m[0] == "metal":
                ids.append(s.metal(m[1], m[2]))
            elif m[0] == "glass":
                ids.append(s.dielectric(m[1]))
            else:
                ids.append(s.diffuse_light(s.solid_rgb(*m[1])))
        for c0, c1, r, m, _bvh in self.prims:
            if c1 is None:
                s.sphere(tuple(c0), r, ids[m])
            else:
                s.moving_sphere(tuple(c0), 0.0, tuple(c1), 1.0, r, ids[m])


def _materials(w, rng):
    rgb = lambda lo, hi: tuple(float(x) for x in rng.uniform(lo, hi, 3))
    pool = [w.mat("lambert", rgb(0.1, 0.9)) for _ in range(3)]
    pool.append(w.mat("checker", rgb(0.1, 0.5), rgb(0.5, 0.95), float(rng.uniform(2, 12))))
    pool.append(w.mat("metal", rgb(0.5, 1.0), 0.0))
    pool.append(w.mat("metal", rgb(0.5, 1.0), float(rng.uniform(0.1, 0.8))))
    pool.append(w.mat("glass", float(rng.uniform(1.3, 1.9))))
    pool.append(w.mat("light", rgb(1.0, 6.0)))
    return pool


def _ground(w):
    g = w.mat("checker", (0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 10.0)
    w.sphere((0.0, -1000.0, 0.0), 1000.0, g, bvh=False)


def _cluster(rng, n_min=16):
    """n_min: the flattener takes a leaf out of the BVH when its box's diagonal is over 20 times the 95th
    percentile's, so with two giants (the dome) that percentile must fall on a member: 22 leaves or more"""
    w = _World()
    _ground(w)
    pool = _materials(w, rng)
    pick = lambda: int(rng.choice(pool))
    n = int(rng.integers(n_min, 41))
    xz = lambda: rng.uniform(-3.0, 3.0, 2)
    glass = w.mat("glass", 1.5)
    gx, gz = xz()
    w.glass = np.array([gx, 0.5, gz])
    w.sphere(w.glass, 0.5, glass)
    w.sphere(w.glass, -0.45, glass)  # the hollow shell
    w.tags.add("shell")
    cx, cz = xz()
    a, b = pool[int(rng.integers(0, 3))], pool[int(rng.integers(4, 8))]
    r = float(rng.uniform(0.2, 0.4))
    for m in (a, b):  # coincident: the later one wins the tie
        w.sphere((cx, r, cz), r, m)
    w.tags.add("coincident")
    ox, oz = xz()
    r1, r2 = rng.uniform(0.25, 0.6, 2)
    w.sphere((ox, r1, oz), r1, pick())
    w.sphere((ox + 0.6 * (r1 + r2), r2, oz + 0.3 * r2), r2, pick())  # centres closer than r1 + r2
    w.tags.add("overlap")
    n_mov = int(rng.integers(3, 7))
    for _ in range(n_mov):
        x, z = xz()
        r = float(rng.uniform(0.1, 0.4))
        c0 = np.array([x, r + float(rng.uniform(0, 0.5)), z])
        d = rng.normal(0, 1, 3)
        d = d / np.linalg.norm(d) * float(rng.uniform(0.5, 3.0)) * r  # up to 3 radii over the shutter
        d[1] = abs(d[1])
        w.moving(c0, c0 + d, r, pick())
    w.tags.add("moving")
    while sum(p[4] for p in w.prims) < n:
        x, z = xz()
        r = float(rng.uniform(0.1, 0.6))
        w.sphere((x, r + float(rng.choice([0.0, 0.0, rng.uniform(0, 1.0)])), z), r, pick())
    return w


def _field_world(rng_seed, n):
    """ground + the first n cells of a jittered grid in rings around its middle (so that a world of n + 1 balls is
    the world of n and one more), r = 0.2, half of them moving"""
    rng = np.random.default_rng(rng_seed)
    w = _World()
    _ground(w)
    pool = _materials(w, rng)
    g = FIELD_GRID
    jit = rng.uniform(0.0, 0.9, (g * g, 2))
    up = rng.uniform(0.0, 0.6, g * g)  # 3 radii
    mats = rng.choice(pool, g * g)
    order = sorted(range(g * g), key=lambda k: (max(abs(k // g - g // 2), abs(k % g - g // 2)), k))
    for q, k in enumerate(order[:n]):
        c = np.array([k // g - g // 2 + jit[k, 0], 0.2, k % g - g // 2 + jit[k, 1]])
        if q % 2:
            w.moving(c, c + np.array([0.0, up[k], 0.0]), 0.2, int(mats[k]))
        else:
            w.sphere(c, 0.2, int(mats[k]))
    return w


def _bare(rng):
    w = _World()
    pool = _materials(w, rng)
    n = int(rng.integers(17, 41))
    radii = list(np.exp(rng.uniform(np.log(0.02), np.log(3.0), n - 5)))
    radii += [0.02, 3.0, float(rng.uniform(1.0, 3.0)), float(rng.uniform(1.0, 3.0)), float(rng.uniform(1.0, 3.0))]
    for q, r in enumerate(radii):
        c = rng.uniform(-1, 1, 3) * np.array([5.0, 2.5, 5.0])
        if r < 0.3 and q % 3 == 0:
            d = rng.normal(0, 1, 3)
            w.moving(c, c + d / np.linalg.norm(d) * float(rng.uniform(0.5, 3.0)) * r, r, int(rng.choice(pool)))
        else:
            w.sphere(c, r, int(rng.choice(pool)))
    return w


def _commit(rtw, w):
    """-> the committed scene (flattened; uploaded where there is a device)"""
    assert os.environ.get("RTW_TUNING") == "1" and os.environ.get("RTW_LIST_MAX") == "0", \
        "make_case commits with RTW_LIST_MAX=0: set it through the knobs fixture first"
    s = rtw.Scene()
    w.build(s)
    try:
        s.commit()
    except rtw.RtwError:
        assert rtw.device_count() == 0
    return s


def _selects_ring(s):
    return selected_kernel(s) == RING_KERNEL and s.info(3) <= 144 and s.info(11) <= 16


def _field(rtw, rng, seed):
    """-> (world, the largest count that selects the ring kernel).  The count is drawn between FIELD_MIN and that
    bound, every third field world takes the bound itself."""
    ws = int(rng.integers(1 << 30))
    n_max = FIELD_MIN
    assert _selects_ring(_commit(rtw, _field_world(ws, n_max)))
    for n in range(FIELD_MIN + 10, FIELD_GRID * FIELD_GRID, 10):
        if not _selects_ring(_commit(rtw, _field_world(ws, n))):
            break
        n_max = n
    n = n_max if (seed // 5) % 3 == 1 else int(rng.integers(FIELD_MIN, n_max + 1))
    while not _selects_ring(_commit(rtw, _field_world(ws, n))):  # (node counts are not quite monotonic in n)
        n -= 1
    w = _field_world(ws, n)
    w.n_max = n_max
    return w


# ---------------------------------------------------------------------------------------------------- cameras
def _far_dist(o, lo, hi):
    """D(o): the distance to the box's farthest corner"""
    return float(np.sqrt((np.maximum(np.abs(o - lo), np.abs(o - hi)) ** 2).sum()))


def _lens_corners(cam):
    c = cam.c
    o, u, v = (np.array(list(getattr(c, k)), np.float64) for k in ("origin", "u", "v"))
    R = abs(float(c.lens_radius))
    return [o + a * R * u + b * R * v for a in (-1, 1) for b in (-1, 1)]


def _all_rays_rise(cam, floor_y):
    """every camera ray starts above floor_y and points upwards by a margin: checked at the corners of the lens
    square and of the image (0 <= s, t <= 1 + a pixel; origin and direction are affine in all four)"""
    c = cam.c
    llc, hor, ver = (np.array(list(getattr(c, k)), np.float64) for k in ("lower_left_corner", "horizontal", "vertical"))
    for A in _lens_corners(cam):
        if A[1] < floor_y:
            return False
        for su in (0.0, 2.0):  # s, t < (w - 1 + 1) / (w - 1) <= 2, reached on a 2-pixel frame
            for sv in (0.0, 2.0):
                d = llc + su * hor + sv * ver - A
                if d[1] < 0.05 * np.linalg.norm(d):
                    return False
    return True


def _unit(v):
    return v / np.linalg.norm(v)


def _vup(rng, view):
    """rolled, neither parallel nor orthogonal to the view"""
    while True:
        v = _unit(rng.normal(0, 1, 3))
        c = abs(float(v @ _unit(view)))
        if 0.05 < c < 0.9:
            return v


def _solve_dist(mid, d, lo, hi, target):
    """t >= 0 with D(mid + t d) = target (D grows with t along a ray from the box's middle)"""
    a, b = 0.0, 1.0
    while _far_dist(mid + b * d, lo, hi) < target:
        b *= 2.0
    for _ in range(80):
        m = 0.5 * (a + b)
        a, b = (m, b) if _far_dist(mid + m * d, lo, hi) < target else (a, m)
    return 0.5 * (a + b)


def _new_camera(rtw, eye, at, vup, vfov, aspect, lens, focus, shutter, tags):
    cam = rtw.Camera.new(tuple(float(x) for x in eye), tuple(float(x) for x in at), tuple(float(x) for x in vup),
                         float(vfov), float(aspect), 2.0 * lens, float(focus), shutter[0], shutter[1])
    cam.tags = dict(tags, lens=lens, vfov=vfov, focus=float(focus), shutter=SHUTTERS.index(shutter),
                    wide=bool(lens > focus * np.tan(np.radians(vfov) / 2)))
    return cam


def _camera(rtw, rng, cls, w, wcls, lo, hi, d0, aspect, scale):
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    grounded = wcls != "bare"
    floor = lo[1] if grounded else -np.inf  # the ground's top is the members' floor (they rest on it)
    shutter = SHUTTERS[int(rng.integers(3))]
    point = lambda f: mid + half * rng.uniform(-f, f, 3)
    for attempt in range(400):
        lens = float(rng.choice(LENSES))
        vfov = float(rng.choice(VFOVS))
        ratio = float(rng.choice([0.3, 0.6, 1.5, 4.0]))
        if cls == "near":
            kinds = ["outside", "outside", "touching"] + (["inside_glass", "between"] if hasattr(w, "glass") else [])
            kind = str(rng.choice(kinds))
            at = point(0.6)
            if kind == "outside":
                eye = point(1.5)
                if grounded:
                    eye[1] = max(eye[1], floor + 0.05 * scale)
            elif kind == "touching":
                if lens == 0.0:
                    lens = float(rng.choice(LENSES[1:]))
                bvh = [p for p in w.prims if p[4] and p[1] is None and p[2] > 0]
                c, _c1, r, _m, _b = bvh[int(rng.integers(len(bvh)))]
                eye = c + _unit(rng.normal(0, 1, 3)) * (r + float(rng.uniform(0.05, 0.95)) * lens)
            else:
                g = w.glass
                eye = g + _unit(rng.normal(0, 1, 3)) * scale * (0.475 if kind == "between" else float(rng.uniform(0, 0.4)))
            tags = {"eye": kind}
        elif cls == "sky":
            lens = float(rng.choice(LENSES))
            eye = point(0.5)
            eye[1] = hi[1] + lens + float(rng.uniform(0.1, 0.6)) * scale
            tilt = float(rng.uniform(0, 0.45)) if attempt < 300 else 0.0
            h = _unit(np.array([rng.normal(), 0.0, rng.normal()]))
            at = eye + np.cos(tilt) * np.array([0.0, 1.0, 0.0]) + np.sin(tilt) * h
            tags = {"eye": "above"}
        else:
            d = _unit(rng.normal(0, 1, 3))
            if grounded:
                d[1] = abs(d[1]) + 0.1
                d = _unit(d)
            aimed = False
            if cls == "border":
                # half of them look at the box's farthest corner from just inside D0: D's gradient is then along the
                # view, the lens plane across it, and D rises over the lens only by ~R²/D, which in the larger worlds
                # is less than the 0.2 %: the host turns the lists on.  Any other view has a lens corner beyond D0
                lens = float(rng.choice([0.5, 2.0]))
                aimed = bool(rng.uniform() < 0.5)
                target = d0 * (1.0 + float(rng.uniform(-0.002, 0.0 if aimed else 0.002)))
            else:
                target = max(float(rng.uniform(1.5, 5.0)) * d0, 1.2 * d0 + 3.0 * lens)
            eye = mid + _solve_dist(mid, d, lo, hi, target) * d
            at = np.where(np.abs(eye - lo) > np.abs(eye - hi), lo, hi) if aimed else point(0.3)
            tags = {"eye": "outside", "aimed": aimed}
        view = at - eye
        dist = float(np.linalg.norm(view))
        if dist < 1e-3 * scale:
            continue
        focus = ratio * dist
        cam = _new_camera(rtw, eye, at, _vup(rng, view), vfov, aspect, lens, focus, shutter, tags)
        Ds = [_far_dist(A, lo, hi) for A in _lens_corners(cam)]
        if cls in ("near", "sky") and max(Ds) > 0.95 * d0:
            continue
        if cls == "sky" and not _all_rays_rise(cam, hi[1] + 0.05 * scale):
            continue
        if cls == "far" and min(Ds) < 1.1 * d0:
            continue
        cam.tags["D"] = (min(Ds) / d0, max(Ds) / d0)
        return cam
    raise AssertionError(f"no {cls} camera found for a {wcls} world")


# ---------------------------------------------------------------------------------------------------- cases
def make_case(rtw, seed, cache=True):
    """-> (build(scene): adds the world, [(camera, class, w, h, spp, max_depth), ...]).  Everything is drawn from
    np.random.default_rng(3000 + seed); needs RTW_TUNING=1 and RTW_LIST_MAX=0 in the environment, and no device."""
    if cache and seed in _CASES:
        return _CASES[seed][:2]
    rng = np.random.default_rng(3000 + seed)
    wcls = CLASSES[seed % 5]
    scale, k = 1.0, None
    if wcls == "cluster":
        w = _cluster(rng)
    elif wcls == "field":
        w = _field(rtw, rng, seed)
    elif wcls == "bare":
        w = _bare(rng)
    elif wcls == "dome":
        w = _cluster(rng, n_min=20)
        light = w.mat("light", tuple(float(x) for x in rng.uniform(0.5, 3.0, 3)))
        w.sphere(rng.uniform(-2, 2, 3), -float(rng.uniform(480, 520)), light, bvh=False)
    else:
        base = _cluster(rng)
        k = OFFSET_K[(seed // 5) % 3]
        scale = 8.0 if k == 14 else 1.0
        sign = rng.choice([-1.0, 1.0], 3)
        off = sign * np.array([2.0 ** k, 2.0 ** k / 4, 2.0 ** k])
        w = base.shifted(off, scale)
        w.glass = base.glass * scale + off
    s = _commit(rtw, w)
    lo, hi = w.bounds()
    d0 = s.info(15) / 1000.0
    assert d0 >= 6.5 * scale, d0  # at the box's middle a lens of radius 2 then has all four corners within 0.95 D0
    # (info 15 is in thousandths, and the flattener's boxes are f32: a few ulps of the largest coordinate)
    ulp = float(np.spacing(np.float32(max(np.abs(lo).max(), np.abs(hi).max()))))
    assert abs(d0 - np.linalg.norm(hi - lo)) <= 1e-3 + 1e-5 * d0 + 8 * ulp, (d0, np.linalg.norm(hi - lo))
    second = ("sky", "border", "far")[(seed // 5) % 3]
    classes = ["near", "near" if (second == "sky" and wcls == "dome") else second]
    if rng.uniform() < 0.6:
        classes.append(str(rng.choice([c for c in CAMERA_CLASSES if not (c == "sky" and wcls == "dome")])))
    cams = []
    for cls in classes:
        fw, fh = FRAMES[int(rng.integers(len(FRAMES)))]
        spp, depth = int(rng.choice(SPPS)), int(rng.choice(DEPTHS))
        cams.append((_camera(rtw, rng, cls, w, wcls, lo, hi, d0, fw / fh, scale), cls, fw, fh, spp, depth))
    meta = {"class": wcls, "k": k, "tags": set(w.tags), "n_bvh": sum(p[4] for p in w.prims), "d0": d0, "lo": lo, "hi": hi,
            "n_max": getattr(w, "n_max", None), "boxes": w.boxes()}
    if cache:
        _CASES[seed] = (w.build, cams, meta)
    return w.build, cams


def case_meta(rtw, seed):
    make_case(rtw, seed)
    return _CASES[seed][2]


def committed(rtw, seed, device=None):
    """-> (a freshly built and committed scene of the seed's world, its text, its images)"""
    build, _cams = make_case(rtw, seed)
    s = rtw.Scene()
    build(s)
    text, imgs = s.dump(), s.images()
    if device is None:
        try:
            s.commit()
        except rtw.RtwError:
            assert rtw.device_count() == 0
    else:
        s.commit(device=device)
    return s, text, imgs


def oracle_frame(rtw, orc, seed, ci, frame=None):
    """-> (the ITERATIVE oracle's frame, its rays, its rays with one more segment allowed); a shared, read-only
    result.  frame = (w, h, spp) overrides the case's own."""
    key = (seed, ci, frame)
    if key not in _ORACLE:
        build, cams = make_case(rtw, seed)
        cam, _cls, w, h, spp, depth = cams[ci]
        if frame:
            w, h, spp = frame
        s = rtw.Scene()
        build(s)
        o = orc.OracleScene(s.dump(), s.images())
        oc = orc.camera_from_fields(cam.as_dict())
        r, rays = o.render(oc, BG, w, h, spp, seed=seed, max_depth=depth, integrator=orc.ITERATIVE)
        _r1, rays1 = o.render(oc, BG, w, h, spp, seed=seed, max_depth=depth + 1, integrator=orc.ITERATIVE)
        r.setflags(write=False)
        _ORACLE[key] = (r, rays, rays1)
    return _ORACLE[key]


def sky_mask(frame, spp):
    """pixels that are spp backgrounds summed in order in f32: every path of the pixel missed everything"""
    t = np.zeros(3, np.float32)
    for _ in range(spp):
        t = t + np.array(BG, np.float32)
    return (frame.view(np.uint32) == t.view(np.uint32)).all(axis=2)


# ---------------------------------------------------------------------------------------------------- CPU tests
SEEDS = range(N_DEFAULT)


def test_generator_is_deterministic(rtw, knobs):
    knobs.setenv("RTW_LIST_MAX", "0")
    for seed in (0, 1, 2, 3, 4, 9, 16):
        a, b = make_case(rtw, seed, cache=False), make_case(rtw, seed, cache=False)
        texts = []
        for build, _ in (a, b):
            s = rtw.Scene()
            build(s)
            texts.append(s.dump())
        assert texts[0] == texts[1]
        assert len(a[1]) == len(b[1]) and 2 <= len(a[1]) <= 3
        for (ca, *ra), (cb, *rb) in zip(a[1], b[1]):
            assert ra == rb and bytes(ca.c) == bytes(cb.c) and ca.tags == cb.tags


@pytest.mark.parametrize("seed", SEEDS)
def test_world_selects_the_ring_kernel(rtw, knobs, seed):
    knobs.setenv("RTW_LIST_MAX", "0")
    s, _text, _imgs = committed(rtw, seed)
    meta = case_meta(rtw, seed)
    assert selected_kernel(s) == RING_KERNEL
    assert s.info(14) == 1, "no sphere tests in the BVH"
    assert s.info(9) & ~F_SPHERES == 0, hex(s.info(9))
    assert s.info(5) == GIANTS[meta["class"]], (meta["class"], s.info(5))
    assert s.info(0) - s.info(5) == meta["n_bvh"] >= 16
    assert s.info(3) <= 144 and s.info(11) <= 16
    if meta["class"] == "field":
        assert FIELD_MIN <= meta["n_bvh"] <= meta["n_max"] and meta["n_max"] >= 300, meta["n_max"]


def test_camera_classes_are_what_they_claim(rtw, knobs):
    """near / sky: every lens corner within 0.95 D0; border: the eye within 0.2 % of D0 (and a lens that straddles);
    far: every corner beyond 1.1 D0, the eye 1.5-5 D0 away (a little more under a wide lens)."""
    knobs.setenv("RTW_LIST_MAX", "0")
    for seed in SEEDS:
        _build, cams = make_case(rtw, seed)
        meta = case_meta(rtw, seed)
        for cam, cls, w, h, spp, depth in cams:
            eye = np.array(list(cam.c.origin), np.float64)
            D = _far_dist(eye, meta["lo"], meta["hi"]) / meta["d0"]
            dmin, dmax = cam.tags["D"]
            if cls in ("near", "sky"):
                assert dmax <= 0.95
            elif cls == "border":
                assert abs(D - 1.0) <= 0.002 + 1e-4 and cam.tags["lens"] >= 0.5
            else:
                assert dmin >= 1.1 and 1.5 - 1e-3 <= D <= 5.0 + 1e-3 + 3.0 * cam.tags["lens"] / meta["d0"]
            assert (w, h) in FRAMES and spp in SPPS and depth in DEPTHS


def test_coverage(rtw, knobs):
    """Every world and camera class and every named ingredient occurs in the default range."""
    knobs.setenv("RTW_LIST_MAX", "0")
    n = {}

    def count(key):
        n[key] = n.get(key, 0) + 1
    for seed in SEEDS:
        _build, cams = make_case(rtw, seed)
        meta = case_meta(rtw, seed)
        count(("world", meta["class"]))
        for t in meta["tags"]:
            count(("has", t))
        if meta["k"] is not None:
            count(("k", meta["k"]))
        if meta["class"] == "field" and meta["n_bvh"] == meta["n_max"]:
            count(("field", "full"))
        for cam, cls, w, h, spp, depth in cams:
            count(("camera", cls))
            count(("frame", (w, h)))
            t = cam.tags
            if cls == "near":
                count(("lens", t["lens"]))
                count(("vfov", t["vfov"]))
                count(("eye", t["eye"]))
                count(("shutter", t["shutter"]))
                count(("focus", "short" if t["focus"] < np.linalg.norm(
                    np.array(list(cam.c.origin)) - 0.5 * (meta["lo"] + meta["hi"])) else "long"))
                if t["wide"]:
                    count(("near", "wide lens"))
            if cls == "border":
                count(("border lens", t["lens"]))
                count(("border", "every lens corner within D0" if t["D"][1] < 1.0 else "a lens corner beyond D0"))
    print(sorted(n.items(), key=str))
    want = [("world", c) for c in CLASSES] + [("camera", c) for c in CAMERA_CLASSES] + \
           [("has", t) for t in ("shell", "coincident", "overlap", "moving")] + [("k", k) for k in OFFSET_K] + \
           [("lens", x) for x in LENSES] + [("vfov", x) for x in VFOVS] + [("shutter", x) for x in range(3)] + \
           [("eye", e) for e in ("outside", "inside_glass", "between", "touching")] + \
           [("focus", "short"), ("focus", "long"), ("near", "wide lens"), ("field", "full")] + \
           [("frame", f) for f in FRAMES]
    missing = [k for k in want if n.get(k, 0) < 1]
    assert not missing, missing
    assert all(n[("world", c)] == N_DEFAULT // 5 for c in CLASSES)
    assert n[("has", "shell")] == n[("has", "coincident")] == n[("has", "overlap")] == 3 * (N_DEFAULT // 5)
    assert n[("camera", "near")] >= N_DEFAULT and n[("near", "wide lens")] >= 2
    assert min(n[("camera", c)] for c in ("sky", "border", "far")) >= 5


def test_oracle_premises(rtw, orc, knobs):
    """What the GPU comparison is meant to exercise, asserted on the oracle's frames alone."""
    knobs.setenv("RTW_LIST_MAX", "0")
    near = mixed = cases = limited = 0
    for seed in SEEDS:
        _build, cams = make_case(rtw, seed)
        meta = case_meta(rtw, seed)
        for ci, (cam, cls, w, h, spp, depth) in enumerate(cams):
            r, rays, rays1 = oracle_frame(rtw, orc, seed, ci)
            sky = sky_mask(r, spp)
            cases += 1
            assert not np.isnan(r).all(), f"seed {seed} camera {ci}: an all-NaN frame"
            assert rays1 >= rays
            limited += rays1 > rays  # a path that took max_depth segments goes on when allowed one more
            if cls == "near":
                near += 1
                mixed += 0 < sky.sum() < sky.size
            if cls == "sky":
                assert sky.all() and rays == w * h * spp, f"seed {seed} camera {ci}: {sky.sum()} of {sky.size} sky"
            if meta["class"] == "dome":
                assert not sky.any(), f"seed {seed} camera {ci}: {sky.sum()} sky pixels under the dome"
    print(f"{cases} cases, {near} near of which {mixed} mixed, {limited} reach the depth limit")
    assert 4 * mixed >= near, (mixed, near)
    assert 10 * limited >= cases, (limited, cases)


def test_list_premises_estimated(rtw, knobs):
    """The host's beam test over the members' boxes before far_bound's sphere pads: some near case has a tile with more than 15
    candidates (overflow at the default cap) and some near case has none above 12 (no overflow, with room for the
    pads): what tests/test_gpu_sphere_fuzz.py then asserts of rtw_scene_info 25."""
    knobs.setenv("RTW_LIST_MAX", "0")
    over = fits = 0
    for seed in SEEDS:
        _build, cams = make_case(rtw, seed)
        boxes = case_meta(rtw, seed)["boxes"]
        for cam, cls, w, h, _spp, _depth in cams:
            if cls != "near":
                continue
            worst = 0
            for tile in range(rtw.n_tiles(w, h)):
                n = 0
                for lo, hi in boxes:
                    n += rtw.diag_tile_beam(cam, w, h, tile, lo, hi)
                    if n > 15:
                        break
                worst = max(worst, n)
                if worst > 15:
                    break
            over += worst > 15
            fits += worst <= 12
    assert over >= 1 and fits >= 1, (over, fits)
