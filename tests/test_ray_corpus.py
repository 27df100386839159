"""The oracle's entries for rays the caller chooses (oracle_hit_rays, oracle_scatter_rays, oracle_sample_rays), and a
corpus of such rays for random worlds: what tests/test_gpu_ray_corpus.py holds the ray-query kernels to.  Nothing here
needs a device.

1. The entries are tied to the established reference before anything trusts them: oracle_sample_rays over a frame's
   camera rays, summed per pixel in sample order in float32, is oracle_render's frame bit for bit with its ray count
   (three presets and a mixed, a mesh and a sphere fuzz world; both integrators); the loop oracle_hit_rays ->
   oracle_scatter_rays written here in Python gives oracle_sample_rays' records; oracle_scatter_rays on a one-material
   scene is oracle_scatter on explicit draws.

2. corpus(rtw, orc, case, env) makes, from np.random.default_rng(corpus_seed(case)) and the world's own primitive
   list (parsed from its dump), N_RAYS rays shuffled so that one wave mixes every class of CLASSES:

     inside_medium   origins inside a ConstantMedium's boundary (sphere, cuboid, under Translation / YRotation)
     inside_glass    inside a Dielectric sphere         inside_hollow  inside a negative-radius sphere
     between_shells  between a sphere and the negative-radius shell inside it
     surface         a previous hit point (the oracle's) fed back as the origin, with a new direction: into the
                     normal's hemisphere, grazing, or anywhere (the t = 0.001 self-intersection edge)
     rect_plane      a point exactly in a rect's (or a cuboid side's) plane, aimed off the plane
     tri_edge        a point on a triangle's edge
     silhouette      aimed as tests/test_gpu_hit_rays.py::_silhouette aims, the targets preferably under wrappers, moving
                     spheres taken at the ray's own time
     axis            directions with two components exactly +0 or -0
     unnormalised    directions of length 1e-3 .. 1e3 (a medium's free path scales with |d|)
     far             origins 1e3 .. 2^14 units out, aimed at the world (the far-origin walk)
     times           time exactly 0, exactly 1, and the float32 next to each inside, aimed at moving spheres
     streams         stream words whose high or whose low 32 bits are zero (xoroshiro64*'s two state words)
     plain           origins uniform in the bounds, random directions: the control

   A class the world has no ingredient for gives its share to `plain`.  Every ray is legal for the host calls: a
   time within [0, 1], a non-zero stream word.  No class was found not comparable, so none is left out.
   The first DEPTH_SUBSET rays are sampled at max_depth 1, 2 and 3 as well as 50.

   The worlds come from the existing builders by import: tests/test_gpu_fuzz.py's mixed worlds (seeds 0 .. and 329,
   the world of test_nan_throughput_world_bit_exact, which supplies the NaN throughputs) and its mesh worlds capped at
   MESH_TRIANGLES triangles, and tests/test_sphere_fuzz_worlds.py's cluster, bare, dome and offset worlds.
   RTW_RAY_SEEDS (default 12) scales the number of worlds for long offline runs.

3. Coverage is a condition, asserted here from the oracle's answers alone (test_coverage), and so is the count of
   exact-t ties between distinct objects (test_ties_stay_under_the_cap): TIE_CAP per world."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_sphere_fuzz_worlds as sphere_worlds
from test_gpu_fuzz import mesh_world, mixed_world
from test_gpu_scatter_rays import _oracle_camera_rays

f32 = np.float32
N_RAYS = 2048
DEPTH_SUBSET = 256
MESH_TRIANGLES = 2000
# Ties: a ray meets two objects at one t exactly where objects coincide -- the sphere worlds' coincident pair, two of
# at least 16 members -- or where it runs through an edge two sides share.  About 400 of a world's rays are aimed at a
# member drawn uniformly (silhouette, three quarters of times) or start on a member's surface or end there by chance
# (surface, plain, streams, unnormalised, inside the bounds), so a world of 16 members expects about 2/16 of them, 50,
# with a deviation of about 7: the cap is 128, the rays compared in full stay above 93 %.  (The 13 default worlds: 21 at
# the most; 121 worlds of one long run: 85.)
TIE_CAP = 128
CLASSES = ("inside_medium", "inside_glass", "inside_hollow", "between_shells", "surface", "rect_plane", "tri_edge",
           "silhouette", "axis", "unnormalised", "far", "times", "streams", "plain")
NAN_WORLD = 329  # tests/test_gpu_fuzz.py::test_nan_throughput_world_bit_exact


def cases(n=None):
    """The worlds of a run of size n (RTW_RAY_SEEDS, default 12): n/2 mixed worlds and the NaN world, n/6 mesh worlds,
    n/3 sphere worlds (the field class left out: its builder commits dozens of trial worlds)."""
    n = int(os.environ.get("RTW_RAY_SEEDS", "12")) if n is None else n
    spheres = [k for k in range(5 * n) if k % 5 != 1][:max(4, n // 3)]
    return [("mixed", k) for k in range(max(1, n // 2))] + [("mixed", NAN_WORLD)] + \
        [("mesh", k) for k in range(max(2, n // 6))] + [("spheres", k) for k in spheres]


CASES = cases()
DEFAULT_CASES = cases(12)
case_id = lambda c: f"{c[0]}-{c[1]}"


# ---------------------------------------------------------------------------------------------------- worlds
def build_world(rtw, case, env):
    """-> (the uncommitted scene, background, a camera with its frame (cam, w, h, spp, max_depth)).  env: the knobs
    fixture (the sphere worlds are drawn under RTW_LIST_MAX=0, and the GPU test commits them so)."""
    kind, seed = case
    if kind == "mixed":
        s, cam, bg = mixed_world(rtw, seed, 12, 8)
        return s, bg, (cam, 12, 8, 2, 50)
    if kind == "mesh":
        s, cam, bg = mesh_world(rtw, seed, MESH_TRIANGLES)
        return s, bg, (cam, 12, 8, 2, 50)
    env.setenv("RTW_LIST_MAX", "0")
    build, cams = sphere_worlds.make_case(rtw, seed)
    s = rtw.Scene()
    build(s)
    cam, _cls, w, h, spp, depth = cams[0]
    return s, sphere_worlds.BG, (cam, w, h, spp, depth)


_WORLDS = {}


def world_text(rtw, case, env):
    """-> (dump text, images, background): made once"""
    if case not in _WORLDS:
        s, bg, _frame = build_world(rtw, case, env)
        _WORLDS[case] = (s.dump(), s.images(), bg)
    return _WORLDS[case]


def parse_dump(text):
    """The world's own primitive list -> (materials [(kind, texture or None)], texture kinds, primitives).  A primitive:
    kind, P (its floats as dumped), mat, chain (the wrappers around it, outermost first: ("t", offset) / ("r", degrees)),
    medium (None, or the index of the ConstantMedium it bounds)."""
    fl = float.fromhex
    mats, texs, prims, chain, stack, medium, n_media = [], [], [], [], [], None, 0
    for line in text.split("\n"):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "tex":
            texs.append(tok[2])
        elif tok[0] == "mat":
            mats.append((tok[2], int(tok[3]) if tok[2] in ("lambertian", "light", "isotropic") else None))
        elif tok[0] == "begin":
            stack.append(tok[1])
            if tok[1] == "translate":
                chain.append(("t", np.array([fl(x) for x in tok[2:5]])))
            elif tok[1] == "rotate_y":
                chain.append(("r", fl(tok[2])))
            elif tok[1] == "medium":
                medium, n_media = n_media, n_media + 1
        elif tok[0] == "end":
            k = stack.pop()
            if k in ("translate", "rotate_y"):
                chain.pop()
            elif k == "medium":
                medium = None
        elif tok[0] in ("sphere", "msphere", "cuboid"):
            prims.append(dict(kind=tok[0], P=np.array([fl(x) for x in tok[1:-1]]), mat=int(tok[-1]),
                              chain=tuple(chain), medium=medium))
        elif tok[0] == "rect":
            prims.append(dict(kind="rect", axis=("xy", "xz", "yz").index(tok[1]), P=np.array([fl(x) for x in tok[2:-1]]),
                              mat=int(tok[-1]), chain=tuple(chain), medium=medium))
        elif tok[0] == "tri":
            prims.append(dict(kind="tri", P=np.array([fl(x) for x in tok[1:10]]), mat=int(tok[-1]), chain=tuple(chain),
                              medium=medium))
    return mats, texs, prims


def _rot(p, deg, inverse=False):
    """transformations.rs:115-148: the point of the rotated object in the world (or back)"""
    s, c = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    if inverse:
        s = -s
    p = np.asarray(p, np.float64)
    return np.stack([c * p[..., 0] + s * p[..., 2], p[..., 1], -s * p[..., 0] + c * p[..., 2]], axis=-1)


def to_world(p, chain):
    for op, a in reversed(chain):
        p = p + a if op == "t" else _rot(p, a)
    return p


def to_local(p, chain):
    for op, a in chain:
        p = p - a if op == "t" else _rot(p, a, inverse=True)
    return p


def inside_medium(prims, o):
    """per origin: inside the boundary of some ConstantMedium (a strict interior test in double)"""
    out = np.zeros(len(o), bool)
    for p in prims:
        if p["medium"] is None:
            continue
        q = to_local(np.asarray(o, np.float64), p["chain"])
        if p["kind"] == "sphere":
            out |= np.linalg.norm(q - p["P"][:3], axis=1) < abs(p["P"][3]) * (1 - 1e-6)
        else:
            out |= ((q > p["P"][:3] + 1e-6) & (q < p["P"][3:6] - 1e-6)).all(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------- the classes
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _ball(rng, m, r_lo=0.0, r_hi=1.0):
    """uniform in the shell r_lo <= |x| <= r_hi"""
    r = (rng.uniform(r_lo ** 3, r_hi ** 3, (m, 1))) ** (1.0 / 3.0)
    return _unit(rng.normal(size=(m, 3))) * r


def _centre(p, t=0.0):
    P = p["P"]
    return P[:3] if p["kind"] == "sphere" else P[:3] + (P[4:7] - P[:3]) * ((t - P[3]) / (P[7] - P[3]))


def _radius(p):
    return abs(p["P"][3] if p["kind"] == "sphere" else p["P"][8])


def _rect_point(rng, axis, a0, a1, b0, b1, k, edge=False):
    a, b = rng.uniform(a0, a1), (rng.choice([b0, b1]) if edge else rng.uniform(b0, b1))
    return np.array({0: (a, b, k), 1: (a, k, b), 2: (k, a, b)}[axis])


def _cuboid_side(rng, P):
    p0, p1 = P[:3], P[3:6]
    axis = int(rng.integers(3))  # rectangular.rs:177-234: xy sides at z, xz at y, yz at x
    ia, ib, ik = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}[axis]
    return axis, p0[ia], p1[ia], p0[ib], p1[ib], rng.choice([p0[ik], p1[ik]])


class _Gen:
    def __init__(self, orc, text, imgs, seed):
        self.rng = np.random.default_rng(seed)
        self.mats, self.texs, self.prims = parse_dump(text)
        self.scene = orc.OracleScene(text, imgs)
        world = [p for p in self.prims if p["medium"] is None]
        self.small = [p for p in world if not (p["kind"] == "sphere" and abs(p["P"][3]) > 100)]
        pts = []
        for p in self.small + [p for p in self.prims if p["medium"] is not None]:
            if p["kind"] in ("sphere", "msphere"):
                r = _radius(p)
                for t in (0.0, 1.0):
                    pts += [to_world(_centre(p, t) + r * np.array(c), p["chain"]) for c in
                            ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
            elif p["kind"] == "rect":
                a0, a1, b0, b1, k = p["P"]
                pts += [to_world(np.array({0: (a, b, k), 1: (a, k, b), 2: (k, a, b)}[p["axis"]]), p["chain"])
                        for a in (a0, a1) for b in (b0, b1)]
            elif p["kind"] == "cuboid":
                pts += [to_world(np.array([p["P"][3 * i], p["P"][1 + 3 * j], p["P"][2 + 3 * k]]), p["chain"])
                        for i in (0, 1) for j in (0, 1) for k in (0, 1)]
            else:
                pts += [to_world(v, p["chain"]) for v in p["P"].reshape(3, 3)]
        pts = np.array(pts)
        self.lo, self.hi = pts.min(axis=0), pts.max(axis=0)
        self.mid, self.half = 0.5 * (self.lo + self.hi), 0.5 * (self.hi - self.lo)
        self.moving = [p for p in self.small if p["kind"] == "msphere"]

    # every class: m -> (origins [k, 3], directions [k, 3][, times [k]][, streams [k]]) as a dict, k <= m
    def box(self, m):
        return self.rng.uniform(self.lo, self.hi, (m, 3))

    def _pick(self, pool):
        return pool[int(self.rng.integers(len(pool)))]

    def _from(self, pool, m, point):
        if not pool:
            return None
        o = np.array([point(self._pick(pool)) for _ in range(m)])
        return dict(o=o, d=self.rng.normal(size=(m, 3)) * self.rng.uniform(0.3, 3.0, (m, 1)))

    def inside_medium(self, m):
        def point(p):
            if p["kind"] == "sphere":
                return to_world(p["P"][:3] + _ball(self.rng, 1, 0, 0.98)[0] * abs(p["P"][3]), p["chain"])
            return to_world(self.rng.uniform(p["P"][:3], p["P"][3:6]), p["chain"])
        return self._from([p for p in self.prims if p["medium"] is not None], m, point)

    def _spheres(self, test):
        return [p for p in self.small if p["kind"] == "sphere" and p["medium"] is None and test(p)]

    def inside_glass(self, m):
        pool = self._spheres(lambda p: p["P"][3] > 0 and self.mats[p["mat"]][0] == "dielectric")
        return self._from(pool, m, lambda p: to_world(p["P"][:3] + _ball(self.rng, 1, 0, 0.95)[0] * p["P"][3], p["chain"]))

    def inside_hollow(self, m):
        pool = self._spheres(lambda p: p["P"][3] < 0)
        return self._from(pool, m, lambda p: to_world(p["P"][:3] + _ball(self.rng, 1, 0, 0.95)[0] * -p["P"][3], p["chain"]))

    def between_shells(self, m):
        out = self._spheres(lambda p: p["P"][3] > 0)
        pairs = [(a, b) for a in out for b in self._spheres(lambda p: p["P"][3] < 0)
                 if (a["P"][:3] == b["P"][:3]).all() and a["chain"] == b["chain"] and -b["P"][3] < a["P"][3]]

        def point(ab):
            a, b = ab
            lo, hi = -b["P"][3], a["P"][3]
            w = 0.05 * (hi - lo)
            return to_world(a["P"][:3] + _ball(self.rng, 1, lo + w, hi - w)[0], a["chain"])
        return self._from(pairs, m, point)

    def surface(self, m):
        """the oracle's hit points of rays aimed into the bounds, fed back as origins"""
        rng, got_o, got_n = self.rng, [], []
        for _ in range(8):
            o = self.box(2 * m)
            probe = np.zeros(2 * m, _RAY)
            probe["origin"], probe["direction"] = o, self.box(2 * m) - o
            probe["time"], probe["stream"] = rng.random(2 * m), rng.integers(1, 1 << 63, 2 * m, dtype=np.uint64)
            h = self.scene.hit_rays(probe)
            ok = (h["flags"] & 1) != 0
            got_o += list(h["p"][ok])
            got_n += list(h["normal"][ok])
            if len(got_o) >= m:
                break
        if not got_o:
            return None
        o, n = np.array(got_o[:m], np.float64), np.array(got_n[:m], np.float64)
        k = len(o)
        d = rng.normal(size=(k, 3))
        how = rng.integers(0, 3, k)
        up = (d * n).sum(axis=1) < 0
        d[(how == 0) & up] *= -1  # into the normal's hemisphere
        tang = _unit(d - n * (d * n).sum(axis=1, keepdims=True) / np.maximum((n * n).sum(axis=1, keepdims=True), 1e-30))
        graze = tang + n * rng.uniform(-0.02, 0.02, (k, 1))
        d[how == 1] = graze[how == 1]
        return dict(o=o, d=d)

    def rect_plane(self, m):
        pool = [p for p in self.small if p["kind"] in ("rect", "cuboid")]

        def point(p):
            side = (p["axis"], *p["P"]) if p["kind"] == "rect" else _cuboid_side(self.rng, p["P"])
            return to_world(_rect_point(self.rng, *side), p["chain"])
        return self._from(pool, m, point)

    def tri_edge(self, m):
        def point(p):
            v = p["P"].reshape(3, 3)
            e = int(self.rng.integers(3))
            return to_world(v[e] + self.rng.uniform() * (v[(e + 1) % 3] - v[e]), p["chain"])
        return self._from([p for p in self.small if p["kind"] == "tri"], m, point)

    def _outline(self, p, o, t):
        """tests/test_gpu_hit_rays.py::_silhouette's point for primitive p, in the world"""
        rng = self.rng
        if p["kind"] in ("sphere", "msphere"):
            c = to_world(_centre(p, t), p["chain"])
            perp = _unit(np.cross(c - o, rng.normal(size=3)))
            return c + perp * _radius(p) * (1.0 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-6, -3))
        if p["kind"] == "tri":
            v = p["P"].reshape(3, 3)
            return to_world(v[0] + rng.uniform() * (v[1] - v[0]), p["chain"])
        side = (p["axis"], *p["P"]) if p["kind"] == "rect" else _cuboid_side(rng, p["P"])
        return to_world(_rect_point(rng, *side, edge=True), p["chain"])

    def silhouette(self, m):
        rng = self.rng
        wrapped = [p for p in self.small if p["chain"]]
        o = self.mid + _unit(rng.normal(size=(m, 3))) * np.linalg.norm(self.half) * rng.uniform(1.5, 3.0, (m, 1))
        t = rng.random(m).astype(f32)
        d = np.zeros((m, 3))
        for q in range(m):
            pool = wrapped if wrapped and q % 2 else (self.moving if self.moving and q % 4 == 0 else self.small)
            d[q] = self._outline(self._pick(pool), o[q], float(t[q])) - o[q]
        return dict(o=o, d=d, t=t)

    def axis(self, m):
        rng = self.rng
        o, d = self.box(m), np.zeros((m, 3))
        d[:, 1] = -0.0
        ax = rng.integers(0, 3, m)
        k = np.arange(m)
        d[k, ax] = rng.choice([-1.0, 1.0, 2.5], m)
        d[k, (ax + 1 + rng.integers(0, 2, m)) % 3] = -0.0
        far = rng.random(m) < 0.5  # half start outside the bounds, on the side the direction comes from
        o[k[far], ax[far]] = (self.mid - 3 * self.half * np.sign(d[k, ax])[:, None])[k[far], ax[far]]
        return dict(o=o, d=d)

    def unnormalised(self, m):
        o = self.box(m)
        return dict(o=o, d=_unit(self.box(m) - o) * 10.0 ** self.rng.uniform(-3, 3, (m, 1)))

    def far(self, m):
        rng = self.rng
        o = self.mid + _unit(rng.normal(size=(m, 3))) * 2.0 ** rng.uniform(np.log2(1e3), 14, (m, 1))
        d = self.box(m) - o
        d[::2] = _unit(d[::2])
        return dict(o=o, d=d)

    def times(self, m):
        rng = self.rng
        one = f32(1.0)
        t = rng.choice(np.array([0.0, 1.0, np.nextafter(f32(0), one), np.nextafter(one, f32(0))], f32), m)
        o = self.box(m)
        d = self.box(m) - o
        for q in range(m):
            if self.moving and q % 4:
                p = self._pick(self.moving)
                d[q] = to_world(_centre(p, float(t[q])) + _ball(rng, 1, 0, 1.1)[0] * _radius(p), p["chain"]) - o[q]
        return dict(o=o, d=d, t=t)

    def streams(self, m):
        rng = self.rng
        x = rng.integers(1, 1 << 32, m, dtype=np.uint64)
        o = self.box(m)
        return dict(o=o, d=self.box(m) - o, s=np.where(np.arange(m) % 2 == 0, x << np.uint64(32), x))

    def plain(self, m):
        return dict(o=self.box(m), d=self.rng.normal(size=(m, 3)))


def corpus_seed(case):
    """The default worlds keep the numbers they were first drawn with (the regression tests of
    tests/test_gpu_ray_corpus.py name rays of theirs); every other world's follows from its kind and seed alone, so a
    long run's ray can be drawn again whatever RTW_RAY_SEEDS was."""
    if case in DEFAULT_CASES:
        return 7000 + DEFAULT_CASES.index(case)
    return 10000 + 1000 * ("mixed", "mesh", "spheres").index(case[0]) + case[1]


_RAY = np.dtype([("origin", f32, 3), ("direction", f32, 3), ("time", f32), ("reserved", np.uint32), ("stream", np.uint64)])
_CORPUS = {}


def corpus(rtw, orc, case, env, cache=True):
    """-> (rays as rtw.RAY_DTYPE, class index per ray): read-only, made once per case"""
    if cache and case in _CORPUS:
        return _CORPUS[case]
    assert rtw.RAY_DTYPE == _RAY
    text, imgs, _bg = world_text(rtw, case, env)
    g = _Gen(orc, text, imgs, corpus_seed(case))
    share = N_RAYS // len(CLASSES)
    parts, label = [], []
    for ci, name in enumerate(CLASSES[:-1]):
        part = getattr(g, name)(share)
        if part is not None:
            parts.append(part)
            label += [ci] * len(part["o"])
    rest = N_RAYS - len(label)
    parts.append(g.plain(rest))
    label += [len(CLASSES) - 1] * rest
    rays = np.zeros(N_RAYS, _RAY)
    at = 0
    for part in parts:
        k = len(part["o"])
        rays["origin"][at:at + k], rays["direction"][at:at + k] = part["o"], part["d"]
        rays["time"][at:at + k] = part["t"] if "t" in part else g.rng.random(k).astype(f32)
        rays["stream"][at:at + k] = part["s"] if "s" in part else g.rng.integers(1, 1 << 63, k, dtype=np.uint64)
        at += k
    perm = g.rng.permutation(N_RAYS)
    rays, label = rays[perm], np.array(label)[perm]
    assert np.isfinite(rays["origin"]).all() and np.isfinite(rays["direction"]).all()
    assert ((rays["time"] >= 0) & (rays["time"] <= 1)).all() and (rays["stream"] != 0).all()
    rays.setflags(write=False)
    label.setflags(write=False)
    if cache:
        _CORPUS[case] = (rays, label)
    return rays, label


_ANSWERS = {}


def answers(rtw, orc, case, env):
    """The oracle on the case's corpus -> dict(scene, hits, tie, scatter (on the oracle's own hits), samples {max_depth:
    records}): read-only, computed once and shared by the CPU conditions here and the GPU comparisons."""
    if case not in _ANSWERS:
        text, imgs, bg = world_text(rtw, case, env)
        rays, _label = corpus(rtw, orc, case, env)
        o = orc.OracleScene(text, imgs)
        hits, tie = o.hit_rays(rays, ties=True)
        a = dict(scene=o, bg=bg, hits=hits, tie=tie, scatter=o.scatter_rays(rays, hits, bg),
                 samples={50: o.sample_rays(rays, bg, 50)})
        for depth in (1, 2, 3):
            a["samples"][depth] = o.sample_rays(rays[:DEPTH_SUBSET], bg, depth)
        for v in (a["hits"], a["tie"], a["scatter"], *a["samples"].values()):
            v.setflags(write=False)
        _ANSWERS[case] = a
    return _ANSWERS[case]


def words(rec):
    rec = np.ascontiguousarray(rec)
    return np.frombuffer(rec.tobytes(), np.uint32).reshape(len(rec), rec[:1].nbytes // 4)


def same(got, want, fields, what):
    """bit for bit, field by field on uint32 views (NaN patterns and the sign of zero included)"""
    for name in fields:
        a, b = words(got[name]), words(want[name])
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of the {len(a)} records compared, first {bad[0]}: " \
                              f"{got[name][bad[0]]} vs {want[name][bad[0]]}"


# ---------------------------------------------------------------------------------------------------- 1. the entries
PRESETS = [("jumpy-balls", 16 / 9, 16, 9, 2, 50), ("smokey-cornell-box", 1.0, 10, 10, 2, 50), ("earth", 16 / 9, 16, 9, 2, 4)]
FUZZ = [("mixed", 0), ("mesh", 0), ("spheres", 0)]  # a medium (asserted below), a mesh and a sphere world


@functools.lru_cache(maxsize=None)
def _preset(rtw, name, aspect):
    s = rtw.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    return s.dump(), s.images(), cam, tuple(bg)


def _frame(rtw, orc, which, env):
    """-> (oracle scene, camera, background, w, h, spp, max_depth)"""
    if which[0] in ("mixed", "mesh", "spheres"):
        s, bg, (cam, w, h, spp, depth) = build_world(rtw, which, env)
        return orc.OracleScene(s.dump(), s.images()), cam, bg, w, h, spp, depth
    name, aspect, w, h, spp, depth = which
    text, imgs, cam, bg = _preset(rtw, name, aspect)
    return orc.OracleScene(text, imgs), cam, bg, w, h, spp, depth


@pytest.mark.parametrize("which", PRESETS + FUZZ, ids=lambda w: f"{w[0]}-{w[1] if isinstance(w[1], int) else w[5]}")
def test_camera_ray_samples_sum_to_the_render(rtw, orc, knobs, which):
    o, cam, bg, w, h, spp, depth = _frame(rtw, orc, which, knobs)
    ocam = orc.camera_from_fields(cam.as_dict())
    rays = _oracle_camera_rays(orc, ocam, w, h, spp, 11)
    for integrator in (orc.ITERATIVE, orc.RECURSIVE):
        ref, ref_rays = o.render(ocam, bg, w, h, spp, seed=11, max_depth=depth, integrator=integrator)
        got = o.sample_rays(rays, bg, depth, integrator=integrator)
        with np.errstate(all="ignore"):
            pixel = np.zeros((h * w, 3), f32)
            for k in range(spp):  # float32, in sample order (lib.rs:78-95)
                pixel = pixel + got["color"].reshape(h * w, spp, 3)[:, k]
        assert pixel.dtype == f32
        assert (words(pixel) == words(ref.reshape(h * w, 3))).all(), (which, integrator)
        assert int(got["segments"].sum()) == ref_rays
        assert (got["segments"] <= depth).all() and (got["reserved"] == 0).all()
        assert np.isin(got["flags"], (orc.END_MISS, orc.END_NO_SCATTER, orc.END_DEPTH)).all()
    none = o.sample_rays(rays, bg, 0)  # lib.rs:98-100
    assert (words(none["color"]) == 0).all() and (none["segments"] == 0).all() and (none["flags"] == 0).all()
    assert (none["stream"] == rays["stream"]).all()
    if which == FUZZ[0]:
        assert any(m[0] == "isotropic" for m in parse_dump(build_world(rtw, which, knobs)[0].dump())[0]), "a medium"


def compose(orc, o, rays, bg, max_depth):
    """sample_ray (lib.rs:97-117) as the loop oracle_hit_rays -> oracle_scatter_rays, the colour as T * terminal in numpy
    float32 -> oracle_sample_rays' records.  What rtw.h says of rtw_sample.stream is what falls out of it: the out
    ray's word at the path's last step."""
    n = len(rays)
    rec = np.zeros(n, orc.SAMPLE_RECORD)
    rec["stream"] = rays["stream"]
    T, path, cur = np.ones((n, 3), f32), np.arange(n), np.array(rays)
    with np.errstate(all="ignore"):
        for depth in range(max_depth, 0, -1):
            if len(cur) == 0:
                break
            sc = o.scatter_rays(cur, o.hit_rays(cur), bg)
            rec["segments"][path] += 1
            alive = (sc["flags"] & orc.SCATTER_SCATTERED) != 0
            miss = (sc["flags"] & orc.SCATTER_MISS) != 0
            end = path[~alive]
            rec["color"][end] = T[end] * sc["emitted"][~alive]
            rec["stream"][end] = sc["stream"][~alive]
            rec["flags"][end] = np.where(miss[~alive], orc.END_MISS, orc.END_NO_SCATTER)
            T[path[alive]] = T[path[alive]] * sc["attenuation"][alive]
            path, nxt = path[alive], np.zeros(int(alive.sum()), _RAY)
            for name in ("origin", "direction", "time", "stream"):
                nxt[name] = sc[name][alive]
            cur = nxt
            if depth == 1:
                rec["color"][path] = T[path] * f32(0.0)
                rec["stream"][path] = cur["stream"]
                rec["flags"][path] = orc.END_DEPTH
    return rec


@pytest.mark.parametrize("case", FUZZ, ids=case_id)
def test_the_python_loop_gives_the_sample_records(rtw, orc, knobs, case):
    a = answers(rtw, orc, case, knobs)
    rays, _label = corpus(rtw, orc, case, knobs)
    fields = ("color", "segments", "stream", "flags", "reserved")
    same(compose(orc, a["scene"], rays, a["bg"], 50), a["samples"][50], fields, f"{case} at depth 50")
    for depth in (1, 2, 3):
        same(compose(orc, a["scene"], rays[:DEPTH_SUBSET], a["bg"], depth), a["samples"][depth], fields,
             f"{case} at depth {depth}")
    rec = a["samples"][50]
    same(a["scene"].sample_rays(rays, a["bg"], 50, orc.RECURSIVE), rec, ("segments", "stream", "flags"),
         "the recursion walks the same paths")
    # rtw.h on rtw_sample.stream, end case by end case, from oracle_scatter_rays on the oracle's own first segment:
    # a miss and a light draw nothing, an absorbed Metal ray has drawn
    one = a["samples"][1]
    sc = a["scatter"][:DEPTH_SUBSET]
    ended = one["flags"] != orc.END_DEPTH
    assert (one["stream"] == sc["stream"]).all()
    miss = (sc["flags"] & orc.SCATTER_MISS) != 0
    assert (one["stream"][miss] == rays["stream"][:DEPTH_SUBSET][miss]).all() and miss.any()
    assert (ended == (miss | ((sc["flags"] & orc.SCATTER_SCATTERED) == 0))).all()


def _one_material(orc, kind_line, rgb):
    return orc.OracleScene(f"rtwscene 1\ntex 0 solid {rgb[0]} {rgb[1]} {rgb[2]}\nmat 0 {kind_line}\nsphere 0 0 0 1 0\n")


def _records(rng, n):
    """random (ray, hit record) pairs, a quarter grazing, the normal against the ray (tests/test_gpu_scatter_rays.py)"""
    normal = _unit(rng.normal(size=(n, 3)))
    d = rng.normal(size=(n, 3))
    tang = rng.normal(size=(n, 3))
    tang = _unit(tang - normal * (tang * normal).sum(axis=1, keepdims=True))
    graze = rng.random(n) < 0.25
    d[graze] = (tang + normal * rng.uniform(-0.05, 0.05, (n, 1)))[graze]
    d = (d * rng.uniform(0.1, 5.0, (n, 1))).astype(f32)
    normal = normal.astype(f32)
    normal[(d.astype(np.float64) * normal.astype(np.float64)).sum(axis=1) > 0] *= f32(-1)
    rays = np.zeros(n, _RAY)
    rays["origin"], rays["direction"] = rng.uniform(-5, 5, (n, 3)), d
    rays["time"], rays["stream"] = rng.random(n), rng.integers(1, 1 << 63, n, dtype=np.uint64)
    hits = np.zeros(n, np.dtype([("p", f32, 3), ("normal", f32, 3), ("t", f32), ("u", f32), ("v", f32),
                                 ("material", np.uint32), ("flags", np.uint32)]))
    hits["p"], hits["normal"], hits["t"] = rng.uniform(-5, 5, (n, 3)), normal, rng.uniform(0.01, 9, n)
    hits["u"], hits["v"] = rng.random(n), rng.random(n)
    hits["flags"] = 1 | np.where(np.arange(n) % 2 == 0, 2, 0)
    return rays, hits


MATERIALS = [(0, "lambertian 0", (0.8, 0.3, 0.1), 0.0), (1, "metal 0.9 0.8 0.7 1.0", (0.9, 0.8, 0.7), 1.0),
             (1, "metal 0.6 0.7 0.8 0.3", (0.6, 0.7, 0.8), 0.3), (2, "dielectric 1.5", (1.0, 1.0, 1.0), 1.5)]


@pytest.mark.parametrize("kind,line,rgb,param", MATERIALS, ids=[m[1].split()[0] + str(m[3]) for m in MATERIALS])
def test_scatter_rays_equal_oracle_scatter_on_explicit_draws(orc, kind, line, rgb, param):
    n, n_draws = 1500, 96
    rays, hits = _records(np.random.default_rng(31 + kind), n)
    got = _one_material(orc, line, rgb).scatter_rays(rays, hits, (0.1, 0.2, 0.3))
    L = orc.lib()
    draws, out, used, after = np.zeros(n_draws, np.uint32), np.zeros(6, f32), C.c_uint32(), C.c_uint64()
    dp = draws.ctypes.data_as(C.POINTER(C.c_uint32))
    want = np.zeros(n, orc.SCATTER_RECORD)
    n_used = np.zeros(n, int)
    for k in range(n):
        state = int(rays["stream"][k])
        L.oracle_rng_stream(state, n_draws, dp, C.byref(after))
        ray7 = np.array([*rays["origin"][k], *rays["direction"][k], rays["time"][k]], f32)
        rec7 = np.array([*hits["p"][k], *hits["normal"][k], float(hits["flags"][k] >> 1 & 1)], f32)
        ok = L.oracle_scatter(kind, orc.fp(orc.f32([*rgb, param])), orc.fp(ray7), orc.fp(rec7), dp, n_draws,
                              out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(used))
        assert used.value < n_draws
        L.oracle_rng_stream(state, used.value, dp, C.byref(after))
        n_used[k] = used.value
        want[k] = (out[3:6] if ok else (0, 0, 0), (0, 0, 0), hits["p"][k], out[0:3], rays["time"][k], 1 if ok else 0,
                   after.value if used.value else state)
    same(got, want, orc.SCATTER_RECORD.names, line)
    scattered = (got["flags"] & 1) != 0
    if param == 1.0:
        assert (~scattered).sum() >= 50 and scattered.sum() >= 500, "the fuzz-1 Metal absorbs some"
        assert (got["stream"][~scattered] != rays["stream"][~scattered]).all(), "an absorbed Metal ray has drawn"
    if kind == 2:
        assert set(np.unique(n_used)) == {0, 1} and scattered.all()


def test_scatter_rays_light_isotropic_and_miss(orc):
    """The kinds oracle_scatter has no number for, against what the reference's lines say."""
    n = 600
    rays, hits = _records(np.random.default_rng(41), n)
    bg = (0.1, 0.2, 0.3)
    light = _one_material(orc, "light 0", (4.0, 3.0, 2.0)).scatter_rays(rays, hits, bg)
    assert (light["flags"] == 0).all() and (light["stream"] == rays["stream"]).all()  # light_source.rs:18-24
    assert (words(light["emitted"]) == words(np.tile(np.array([4, 3, 2], f32), (n, 1)))).all()
    assert (words(light["attenuation"]) == 0).all() and (words(light["origin"]) == words(hits["p"])).all()
    iso = _one_material(orc, "isotropic 0", (0.5, 0.25, 0.75)).scatter_rays(rays, hits, bg)
    assert (iso["flags"] == 1).all() and (words(iso["emitted"]) == 0).all()  # material.rs:155-165
    assert (words(iso["attenuation"]) == words(np.tile(np.array([0.5, 0.25, 0.75], f32), (n, 1)))).all()
    L = orc.lib()
    draws, after = np.zeros(96, np.uint32), C.c_uint64()
    for k in range(n):  # vec3.rs:97-108: x, y, z in [-1, 1) until inside the unit sphere
        L.oracle_rng_stream(int(rays["stream"][k]), 96, draws.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(after))
        for trip in range(32):
            v = np.array([L.oracle_u32_to_range(int(draws[3 * trip + c]), -1.0, 1.0) for c in range(3)], f32)
            if f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) < 1:
                break
        L.oracle_rng_stream(int(rays["stream"][k]), 3 * (trip + 1), draws.ctypes.data_as(C.POINTER(C.c_uint32)),
                            C.byref(after))
        assert (words(iso["direction"][k:k + 1]) == words(v[None])).all() and iso["stream"][k] == after.value, k
    hits["flags"] = 0
    miss = _one_material(orc, "light 0", (4.0, 3.0, 2.0)).scatter_rays(rays, hits, bg)
    assert (miss["flags"] == orc.SCATTER_MISS).all() and (words(miss["emitted"]) == words(np.tile(np.array(bg, f32), (n, 1)))).all()
    same(miss, rays, ("origin", "direction", "time", "stream"), "a miss copies the ray through")


# ---------------------------------------------------------------------------------------------------- 2. the corpus
def test_corpus_is_deterministic(rtw, orc, knobs):
    for case in FUZZ:
        a, b = corpus(rtw, orc, case, knobs, cache=False), corpus(rtw, orc, case, knobs, cache=False)
        assert (words(a[0]) == words(b[0])).all() and (a[1] == b[1]).all() and len(a[0]) == N_RAYS


def test_classes_are_what_they_claim(rtw, orc, knobs):
    n = dict.fromkeys(CLASSES, 0)
    for case in DEFAULT_CASES:
        rays, label = corpus(rtw, orc, case, knobs)
        _mats, _texs, prims = parse_dump(world_text(rtw, case, knobs)[0])
        of = lambda name: rays[label == CLASSES.index(name)]
        for name in CLASSES:
            n[name] += len(of(name))
        r = of("inside_medium")
        assert inside_medium(prims, r["origin"]).mean() >= 0.95 if len(r) else True  # (float32 origins near a face)
        r = of("axis")
        assert ((r["direction"] == 0).sum(axis=1) == 2).all() and np.signbit(r["direction"]).any()
        r = of("unnormalised")
        ln = np.linalg.norm(r["direction"].astype(np.float64), axis=1)
        assert ln.min() < 1e-2 and ln.max() > 1e2 and ln.min() >= 0.9e-3 and ln.max() <= 1.1e3
        r = of("far")  # 1e3 .. 2^14 from the middle of the bounds, which the plain origins fill
        dist = np.linalg.norm(r["origin"].astype(np.float64) - np.median(of("plain")["origin"], axis=0), axis=1)
        assert dist.min() >= 900 and dist.max() <= 2.0 ** 14 + 100 and dist.max() >= 4000
        r = of("times")
        one = f32(1.0)
        assert set(np.unique(r["time"])) <= {f32(0), one, np.nextafter(f32(0), one), np.nextafter(one, f32(0))}
        assert len(np.unique(r["time"])) == 4
        r = of("streams")
        hi, lo = r["stream"] >> np.uint64(32), r["stream"] & np.uint64(0xFFFFFFFF)
        assert ((hi == 0) != (lo == 0)).all() and (hi == 0).any() and (lo == 0).any()
        # one wave mixes the classes: every 64 consecutive rays hold at least half of the classes present
        present = len(np.unique(label))
        assert min(len(np.unique(label[k:k + 64])) for k in range(0, N_RAYS, 64)) >= present // 2
    print(n)
    assert all(v >= 100 for v in n.values()), n


def _strip(text, what):
    """the dump without its `begin <what>` groups (for test_coverage: which winners lie under a YRotation)"""
    out, skip = [], 0
    for line in text.split("\n"):
        tok = line.split()
        if skip:
            skip += (tok[:1] == ["begin"]) - (tok[:1] == ["end"])
            continue
        if tok[:2] == ["begin", what]:
            skip = 1
            continue
        out.append(line)
    return "\n".join(out)


def test_coverage(rtw, orc, knobs):
    """Over the default worlds, from the oracle's answers alone: every end kind; every material kind and branch and every
    texture kind reached by oracle_scatter_rays; a medium the winner for rays that start inside and outside it; a winner
    under a YRotation; a path that exhausts max_depth 50 and a NaN throughput (world 329 supplies it)."""
    n = {}

    def count(key, k):
        n[key] = n.get(key, 0) + int(k)
    for case in DEFAULT_CASES:
        a = answers(rtw, orc, case, knobs)
        rays, label = corpus(rtw, orc, case, knobs)
        text, imgs, _bg = world_text(rtw, case, knobs)
        mats, texs, prims = parse_dump(text)
        hits, sc = a["hits"], a["scatter"]
        hit = (hits["flags"] & orc.HIT_HIT) != 0
        kind = np.array([mats[m][0] for m in hits["material"]])
        tex = np.array([texs[mats[m][1]] if mats[m][1] is not None else "-" for m in hits["material"]])
        scattered = (sc["flags"] & orc.SCATTER_SCATTERED) != 0
        through = (sc["direction"].astype(np.float64) * hits["normal"].astype(np.float64)).sum(axis=1) < 0
        count("lambertian", (hit & (kind == "lambertian")).sum())
        count("metal scattered", (hit & (kind == "metal") & scattered).sum())
        count("metal absorbed", (hit & (kind == "metal") & ~scattered).sum())
        count("dielectric reflected", (hit & (kind == "dielectric") & ~through).sum())
        count("dielectric refracted", (hit & (kind == "dielectric") & through).sum())
        count("light", (hit & (kind == "light")).sum())
        count("isotropic", (hit & (kind == "isotropic")).sum())
        for t in ("solid", "checker", "noise", "image", "uvdebug"):
            count(t, (hit & (tex == t)).sum())
        inside = inside_medium(prims, rays["origin"])
        count("medium from inside", (hit & (kind == "isotropic") & inside).sum())
        count("medium from outside", (hit & (kind == "isotropic") & ~inside).sum())
        for depth, rec in a["samples"].items():
            for name, flag in (("miss", orc.END_MISS), ("no scatter", orc.END_NO_SCATTER), ("depth", orc.END_DEPTH)):
                count(f"end {name}", (rec["flags"] == flag).sum())
        count("depth 50 exhausted", (a["samples"][50]["flags"] == orc.END_DEPTH).sum())
        count("nan", np.isnan(a["samples"][50]["color"]).any(axis=1).sum())
        if "rotate_y" in text:
            # The winner lies under a YRotation when the world without its media (their leaf keys, which key the free
            # paths, shift when leaves go) has the same winner, and loses it when the rotated groups go too
            bare = _strip(text, "medium")
            h1 = orc.OracleScene(bare, imgs).hit_rays(rays)
            h2 = orc.OracleScene(_strip(bare, "rotate_y"), imgs).hit_rays(rays)
            count("under a rotation", (hit & (words(h1) == words(hits)).all(axis=1) & (h1["t"] != h2["t"])).sum())
    print(sorted(n.items()))
    want = ["lambertian", "metal scattered", "metal absorbed", "dielectric reflected", "dielectric refracted", "light",
            "isotropic", "solid", "checker", "noise", "image", "uvdebug", "medium from inside", "medium from outside",
            "end miss", "end no scatter", "end depth", "depth 50 exhausted", "nan", "under a rotation"]
    few = {k: n.get(k, 0) for k in want if n.get(k, 0) < 10}
    assert not few, few


def test_ties_stay_under_the_cap(rtw, orc, knobs):
    """tests/test_gpu_ray_corpus.py compares a tied ray by t and material only: the oracle's count of them per world."""
    worst = {case_id(c): int(answers(rtw, orc, c, knobs)["tie"].sum()) for c in CASES}
    print(worst)
    assert max(worst.values()) <= TIE_CAP, worst
