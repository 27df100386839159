"""Closest-hit ray queries on the GPU (rtw_hit_rays, rtw_hit_rays_device; Hittable::hit, hittable/mod.rs:22-69).

A query runs the scene's own walk -- the kernel variant its renders select -- on rays the test chooses and returns the
hit records themselves, so the tie rule, the far-origin walk, the 16-bit, half-node and LDS-node walks and the hit
record are compared ray by ray: against the oracle's primitive tests folded as the reference's list loop folds them
(oracle_hit_primitive over the primitives in builder order with t_max = the closest so far, hittable/mod.rs:57-69), and
against the oracle's render for wrappers, groups, media and uv.  Every comparison is bit for bit.

Ray sets hold 4,099 rays (no multiple of 64: the last wave is partial).  The oracle's records are computed once per
world and shared by the tests."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4099
_F = C.POINTER(C.c_float)
f32 = np.float32


# ---------------------------------------------------------------- worlds of unwrapped primitives, in builder order
# A primitive is (kind, params, material slot[, vertex normals [3, 3], vertex uvs [3, 2]]): kind and params as
# oracle_hit_primitive takes them (0 sphere cx cy cz r; 1 moving sphere c0 t0 c1 t1 r; 2 rect axis a0 a1 b0 b1 k;
# 3 triangle 9 floats).
def _sphere_prims(rng, n_static=60, n_dup=12, n_moving=36, box=4.0):
    c = rng.uniform(-box, box, (n_static - n_dup, 3)).astype(f32)
    r = rng.uniform(0.3, 0.8, n_static - n_dup).astype(f32)
    prims = [(0, np.array([*c[k], r[k]], f32), k % 7) for k in range(len(c))]
    # coincident copies (exact-t ties: the later one must win), with another material
    prims += [(0, prims[k][1].copy(), 7) for k in range(n_dup)]
    for k in range(n_moving):
        c0 = rng.uniform(-box, box, 3).astype(f32)
        c1 = c0 + rng.uniform(-0.5, 0.5, 3).astype(f32)
        prims.append((1, np.array([*c0, 0.0, *c1, 1.0, rng.uniform(0.2, 0.6)], f32), k % 7))
    return prims


def _rect_prims(rng, n, box=4.0):
    prims = []
    for k in range(n):
        a0, b0 = rng.uniform(-box, box - 1, 2)
        prims.append((2, np.array([k % 3, a0, a0 + rng.uniform(0.5, 3), b0, b0 + rng.uniform(0.5, 3),
                                   rng.uniform(-box, box)], f32), k % 6))
    return prims


def _tri_prims(rng, n=100, box=4.0):
    prims = []
    for k in range(n):
        v = (rng.uniform(-box, box, (1, 3)) + rng.uniform(-1, 1, (3, 3))).astype(f32)
        if k % 2:  # with vertex normals and uvs
            prims.append((3, v.reshape(-1), 0, rng.uniform(-1, 1, (3, 3)).astype(f32),
                          rng.uniform(0, 1, (3, 2)).astype(f32)))
        else:
            prims.append((3, v.reshape(-1), 0))
    return prims


def _build(rtw, prims, mats_of):
    """The world of `prims` through the builder API, in their order (consecutive primitives of one kind in one
    call) -> (committed scene, material id per primitive)."""
    s = rtw.Scene()
    mats = mats_of(s)
    mat_ids = [mats[p[2]] for p in prims]
    k = 0
    while k < len(prims):
        kind = prims[k][0]
        e = k
        while e < len(prims) and prims[e][0] == kind and (kind != 3 or (len(prims[e]) > 3) == (len(prims[k]) > 3)):
            e += 1
        P = np.array([p[1] for p in prims[k:e]], f32)
        m = mat_ids[k:e]
        if kind == 0:
            s.spheres(P[:, :3], P[:, 3], m)
        elif kind == 1:
            s.moving_spheres(P[:, 0:3], P[:, 3], P[:, 4:7], P[:, 7], P[:, 8], m)
        elif kind == 2:
            s.rects(P[:, 0].astype(np.uint32), P[:, 1], P[:, 2], P[:, 3], P[:, 4], P[:, 5], m)
        else:  # one material per triangles call
            assert len(set(m)) == 1
            if len(prims[k]) > 3:
                s.triangles(P.reshape(-1), m[0], normals=np.array([p[3] for p in prims[k:e]], f32).reshape(-1),
                            uvs=np.array([p[4] for p in prims[k:e]], f32).reshape(-1))
            else:
                s.triangles(P.reshape(-1), m[0])
        k = e
    return s, np.array(mat_ids, np.uint32)


def _sphere_mats(s):
    return [s.lambertian_solid((0.1 * k, 0.5, 0.5)) for k in range(1, 5)] + \
        [s.metal((0.8, 0.7, 0.6), 0.1), s.dielectric(1.5), s.diffuse_light(s.solid_rgb(3, 3, 3)),
         s.lambertian(s.checker(s.solid_rgb(0.2, 0.3, 0.1), s.solid_rgb(0.9, 0.9, 0.9), 10.0))]


def _box_mats(s):
    return [s.lambertian_solid((0.1 * k, 0.5, 0.5)) for k in range(1, 4)] + \
        [s.metal((0.8, 0.7, 0.6), 0.1), s.dielectric(1.5), s.diffuse_light(s.solid_rgb(3, 3, 3))]


def _mesh_mats(s):
    return [s.lambertian_solid((0.73, 0.73, 0.73))]


# ---------------------------------------------------------------- rays
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _silhouette(rng, prims, o):
    """A point just off (or on) the outline of a random primitive, per origin: a sphere's tangent point as seen
    from the origin moved in or out by up to 1e-3 of the radius; a point on a rect's or a triangle's edge."""
    out = np.zeros_like(o)
    for q in range(len(o)):
        p = prims[rng.integers(len(prims))]
        kind, P = p[0], p[1].astype(np.float64)
        if kind in (0, 1):
            c, r = (P[:3], P[3]) if kind == 0 else (P[:3], P[8])
            perp = _unit(np.cross(c - o[q], rng.normal(size=3)))
            out[q] = c + perp * r * (1.0 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-6, -3))
        elif kind == 2:
            a = rng.uniform(P[1], P[2]), rng.choice([P[3], P[4]])
            out[q] = {0: (a[0], a[1], P[5]), 1: (a[0], P[5], a[1]), 2: (P[5], a[0], a[1])}[int(P[0])]
        else:
            v = P.reshape(3, 3)
            out[q] = v[0] + rng.uniform() * (v[1] - v[0])
    return out


def _ray_mix(rng, prims, n=N, box=4.0):
    """From inside the bounds, grazing, axis-parallel (components exactly 0 and -0) and missing rays, shuffled."""
    n_in, n_graze, n_axis = n * 3 // 8, n // 4, n // 5
    n_miss = n - n_in - n_graze - n_axis
    o = [rng.uniform(-box, box, (n_in, 3))]
    d = [rng.normal(size=(n_in, 3))]
    og = _unit(rng.normal(size=(n_graze, 3))) * rng.uniform(8, 12, (n_graze, 1))
    o.append(og)
    d.append(_silhouette(rng, prims, og) - og)
    oa = rng.uniform(-box, box, (n_axis, 3))
    da = np.zeros((n_axis, 3))
    da[:, 1] = -0.0
    ax = rng.integers(0, 3, n_axis)
    da[np.arange(n_axis), ax] = rng.choice([-1.0, 1.0, 2.5], n_axis)
    z = (ax + 1 + rng.integers(0, 2, n_axis)) % 3
    da[np.arange(n_axis), z] = -0.0
    oa[np.arange(n_axis), ax] = -3 * box * np.sign(da[np.arange(n_axis), ax])
    o.append(oa)
    d.append(da)
    om = _unit(rng.normal(size=(n_miss, 3))) * rng.uniform(9, 12, (n_miss, 1))
    o.append(om)
    d.append(om + rng.normal(size=(n_miss, 3)))  # pointing away
    o, d = np.concatenate(o).astype(f32), np.concatenate(d).astype(f32)
    perm = rng.permutation(n)
    return o[perm], d[perm], rng.uniform(0, 1, n).astype(f32)


# ---------------------------------------------------------------- the oracle's flat list (hittable/mod.rs:57-69)
def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _flat_oracle(orc, rtw, prims, mat_ids, o, d, t):
    """-> (records as the GPU must return them, rays whose winner tied an earlier primitive's t exactly)."""
    fn = orc.lib().oracle_hit_primitive
    rr = np.ascontiguousarray(np.concatenate([o, d, t[:, None]], axis=1), f32)
    pp = [(int(p[0]), np.ascontiguousarray(p[1], f32)) for p in prims]
    ptr = [(k, a.ctypes.data_as(_F)) for k, a in pp]
    out = (C.c_float * 10)()
    rec = np.zeros(len(rr), rtw.HIT_DTYPE)
    rec["t"] = np.inf
    ties = 0
    tmin = f32(0.001)
    for q in range(len(rr)):
        rp = C.cast(rr.ctypes.data + 28 * q, _F)
        closest, win, tie = f32(np.inf), -1, False
        for k, (kind, p) in enumerate(ptr):
            if fn(kind, p, rp, tmin, closest, out):
                tie = win >= 0 and out[0] == closest
                closest, win = f32(out[0]), k
                h = np.array(out[:10], f32)
        if win < 0:
            continue
        ties += tie
        r = rec[q]
        r["t"], r["p"], r["normal"], r["u"], r["v"] = h[0], h[1:4], h[4:7], h[7], h[8]
        front = h[9] != 0
        if len(prims[win]) > 3:  # vertex normals and uvs: triangular.rs:315-323 from the test's barycentrics (the
            # default uvs (0,0), (1,0), (0,1) make the oracle's (u, v) the barycentrics themselves), in f32
            tn, tuv = prims[win][3], prims[win][4]
            bu, bv = h[7], h[8]
            w = f32(f32(f32(1.0) - bu) - bv)
            hn = (tn[0] * w + tn[1] * bu) + tn[2] * bv
            r["u"] = f32(f32(w * tuv[0][0]) + f32(bu * tuv[1][0])) + f32(bv * tuv[2][0])
            r["v"] = f32(f32(w * tuv[0][1]) + f32(bu * tuv[1][1])) + f32(bv * tuv[2][1])
            front = _dot(d[q], hn) < 0
            r["normal"] = hn if front else -hn
        r["material"], r["key"] = mat_ids[win], win
        r["flags"] = rtw.HIT_HIT | (rtw.HIT_FRONT_FACE if front else 0)
    return rec, ties


WORLDS = {"spheres": (lambda rng: _sphere_prims(rng), _sphere_mats),
          "rects": (lambda rng: _rect_prims(rng, 90), _box_mats),
          "triangles": (lambda rng: _tri_prims(rng), _mesh_mats),
          "rect-list": (lambda rng: _rect_prims(rng, 30), _box_mats)}


@functools.lru_cache(maxsize=None)
def _case(rtw, orc, name):
    """(primitives, rays, the oracle's records, ties) of a world: computed once, never changed."""
    rng = np.random.default_rng(sorted(WORLDS).index(name) + 77)
    prims = WORLDS[name][0](rng)
    o, d, t = _ray_mix(rng, prims)
    s = rtw.Scene()  # (uncommitted: only the material ids, which the builder hands out in order)
    mats = WORLDS[name][1](s)
    mat_ids = np.array([mats[p[2]] for p in prims], np.uint32)
    rec, ties = _flat_oracle(orc, rtw, prims, mat_ids, o, d, t)
    rec.setflags(write=False)
    return prims, (o, d, t), rec, ties


def _same(got, want, what=""):
    a = np.frombuffer(got.tobytes(), np.uint32).reshape(len(got), 12)
    b = np.frombuffer(want.tobytes(), np.uint32).reshape(len(want), 12)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} records differ, first ray {bad[0]}: gpu {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


def _query(rtw, orc, name):
    prims, (o, d, t), rec, _ = _case(rtw, orc, name)
    s, _ids = _build(rtw, prims, WORLDS[name][1])
    s.commit(device=0)
    return s, s.hit_rays(o, d, t, device=0), rec


def _cfg(s):
    """rtw_scene_info 16-23: stack, spill, occ, feat, blk, ncap, half, s16 of the selected kernel"""
    return dict(zip(("stack", "spill", "occ", "feat", "blk", "ncap", "half", "s16"), (s.info(k) for k in range(16, 24))))


F_LIST, F_TRI = 1 << 16, 1 << 3
F_ALL = ((1 << 16) - 1) | (1 << 17)


# ---------------------------------------------------------------- 1. records against the oracle's primitive tests
@pytest.mark.parametrize("name", ["spheres", "rects", "triangles"])
def test_records_match_the_flat_oracle(gpu, orc, name):
    prims, _rays, rec, ties = _case(gpu, orc, name)
    assert 60 <= len(prims) <= 120
    hits = (rec["flags"] & gpu.HIT_HIT) != 0
    assert hits.mean() >= 0.25 and (~hits).mean() >= 0.10, (hits.mean(), "the oracle's own mix")
    if name == "spheres":
        assert ties >= 20, ties
    s, got, _ = _query(gpu, orc, name)
    assert s.info(3) > 0, "the world must have a BVH"
    _same(got, rec, name)


# ---------------------------------------------------------------- 2. the same world in every walk
SPHERE_WALKS = {
    None: dict(blk=1024, ncap=144, half=0),
    "RTW_LDS_NODES=0": dict(ncap=0, blk=256, occ=6),
    "RTW_LDSN_WAVES=6": dict(blk=512, ncap=224),
    "RTW_LDSN_WAVES=7": dict(blk=448, ncap=160),
    "RTW_HALF_NODES=1": dict(ncap=144, blk=512, half=1),
    # (alone the knob changes nothing here: pick_kernel reads it where it selects a 5-wave kernel, and a sphere world
    # that fits stays on its LDS-node kernel; with RTW_OCC=5 it is the all-features kernel)
    "RTW_GENERIC=1": dict(blk=1024, ncap=144, half=0),
    "RTW_GENERIC=1,RTW_OCC=5": dict(feat=F_ALL, ncap=0, occ=5, blk=256),
    "RTW_STACK_LDS=4": dict(stack=4, spill=1, feat=F_ALL),
}
TRI_WALKS = {
    None: dict(s16=1, half=1, occ=7),
    "RTW_MESH_S16=0": dict(s16=0, half=1, occ=5),
    "RTW_MESH_S16=6": dict(s16=1, half=1, occ=6),
    "RTW_HALF_NODES=0": dict(s16=0, half=0, occ=5),
}
LIST_WALKS = {
    None: dict(feat=lambda f: f & F_LIST and f != (F_ALL | F_LIST), occ=8),
    "RTW_LIST_ALL=1": dict(feat=F_ALL | F_LIST),
}


def _set(knobs, knob):
    for kv in (knob or "").split(","):
        if kv:
            knobs.setenv(*kv.split("="))


def _walk(rtw, orc, knobs, name, knob, want):
    _set(knobs, knob)
    s, got, rec = _query(rtw, orc, name)
    cfg = _cfg(s)
    for k, v in want.items():
        assert v(cfg[k]) if callable(v) else cfg[k] == v, (knob, k, cfg)
    _same(got, rec, f"{name} under {knob}")
    return cfg


@pytest.mark.parametrize("knob", list(SPHERE_WALKS)[1:])
def test_sphere_world_in_every_walk(gpu, orc, knobs, knob):
    _walk(gpu, orc, knobs, "spheres", knob, SPHERE_WALKS[knob])


def test_sphere_world_default_is_the_lds_node_1024_kernel(gpu, orc, knobs):
    _walk(gpu, orc, knobs, "spheres", None, SPHERE_WALKS[None])


@pytest.mark.parametrize("knob", list(TRI_WALKS))
def test_triangle_world_in_every_walk(gpu, orc, knobs, knob):
    cfg = _walk(gpu, orc, knobs, "triangles", knob, TRI_WALKS[knob])
    assert cfg["feat"] & F_TRI and cfg["ncap"] == 0


@pytest.mark.parametrize("knob", list(LIST_WALKS))
def test_rect_world_in_list_mode(gpu, orc, knobs, knob):
    prims, _rays, rec, _ = _case(gpu, orc, "rect-list")
    assert len(prims) <= 32 and ((rec["flags"] & 1) != 0).mean() >= 0.25
    _set(knobs, knob)
    s, got, _ = _query(gpu, orc, "rect-list")
    assert s.info(3) == 0, "list mode has no BVH"
    cfg = _cfg(s)
    for k, v in LIST_WALKS[knob].items():
        assert v(cfg[k]) if callable(v) else cfg[k] == v, (knob, k, cfg)
    _same(got, rec, f"rect-list under {knob}")


def _in_plane_world(rtw, n_far):
    """One xy rect in the plane z = 0 (leaf 0) and n_far rects far behind the ray below."""
    s = rtw.Scene()
    m = s.lambertian_solid((0.5, 0.5, 0.5))
    s.xy_rect(0.0, 1.0, 0.0, 1.0, 0.0, m)
    k = np.arange(n_far, dtype=f32)
    s.rects(np.full(n_far, 2), k, k + 1, k, k + 1, -20.0 - k, [m] * n_far)
    return s.commit(device=0), m


@pytest.mark.parametrize("knob", [None, "RTW_LIST_ALL=1", "RTW_LIST_MAX=0"])
def test_in_plane_ray_follows_the_kernels_nan_rule(gpu, knobs, knob):
    """A ray lying in a rect's plane has t = 0 / 0 there, which the reference's comparisons all pass
    (rectangular.rs:33-41): both list-mode loops report that hit with t = NaN, the BVH kernels a miss (DESIGN.md §2,
    "In-plane bounces").  Its neighbours, ordinary rays through the same rect, are unaffected."""
    _set(knobs, knob)
    s, m = _in_plane_world(gpu, 12)
    assert (s.info(3) > 0) == (knob == "RTW_LIST_MAX=0")
    o = np.array([[0.25, 0.5, 3.0], [0.25, 0.5, 0.0], [0.75, 0.5, 3.0]], f32)
    d = np.array([[0, 0, -1], [1, 0, 0], [0, 0, -1]], f32)
    got = s.hit_rays(o, d, device=0)
    both = gpu.HIT_HIT | gpu.HIT_FRONT_FACE
    assert (got["flags"][[0, 2]] == both).all() and (got["t"][[0, 2]] == 3.0).all() and (got["key"] == 0).all()
    if s.info(3) > 0:
        assert got["flags"][1] == 0 and np.isinf(got["t"][1])
    else:
        assert got["flags"][1] & gpu.HIT_HIT and np.isnan(got["t"][1]) and got["material"][1] == m


# ---------------------------------------------------------------- 3. wrappers, groups, media, uv: the oracle's render
W3, H3, SEED3 = 48, 27, 5
BG3 = (0.125, 0.375, 0.875)


def _wrapped_world(rtw, uv):
    """Built as tests/test_gpu_fuzz.py builds its worlds: Translation / YRotation chains, BvhNode groups inside
    rotations, cuboids, a sphere-bounded and a cuboid-bounded medium.  Every surface material is a DiffuseLight of its
    own solid colour (or, with `uv`, of UVDebug) -> (scene, {colour: material id}, wrapped material ids, medium ids)."""
    rng = np.random.default_rng(4242)
    s = rtw.Scene()
    f = lambda *shape: rng.uniform(-1, 1, shape).astype(f32)
    colour_of, wrapped = {}, set()

    def light(is_wrapped):
        c = (float(f32(1 + len(colour_of))), float(f32(0.5 + 0.25 * len(colour_of))), 2.0)
        m = s.diffuse_light(s.uv_debug() if uv else s.solid_rgb(*c))
        colour_of[c] = m
        if is_wrapped:
            wrapped.add(m)
        return m

    def tris(n, w):
        for _ in range(n // 2):
            p = f(2, 1, 3) * 3 + f(2, 3, 3)
            s.triangles(p.reshape(-1), light(w), normals=f(2, 3, 3).reshape(-1),
                        uvs=rng.uniform(0, 1, (2, 3, 2)).astype(f32).reshape(-1))

    def moving(n, w):
        c0 = f(n, 3) * 3
        s.moving_spheres(c0, np.zeros(n), c0 + f(n, 3) * 0.5, np.ones(n), rng.uniform(0.3, 0.7, n),
                         [light(w) for _ in range(n)])

    n = 6
    s.spheres(f(n, 3) * 4, rng.uniform(0.3, 0.9, n), [light(False) for _ in range(n)])
    a0, b0 = f(4) * 4, f(4) * 4
    s.rects(rng.integers(0, 3, 4), a0, a0 + rng.uniform(0.5, 3, 4), b0, b0 + rng.uniform(0.5, 3, 4), f(4) * 4,
            [light(False) for _ in range(4)])
    for _ in range(3):
        with s.translate(tuple(f(3) * 3)), s.rotate_y(float(rng.uniform(-180, 180))):
            s.cuboid(tuple(f(3) - 1.5), tuple(f(3) + 1.5), light(True))
    with s.rotate_y(float(rng.uniform(-90, 90))):
        with s.bvh():
            tris(12, True)
            moving(4, True)
    with s.translate(tuple(f(3))), s.rotate_y(33.0), s.translate(tuple(f(3))):
        s.spheres(f(5, 3) * 3, rng.uniform(0.3, 0.8, 5), [light(True) for _ in range(5)])
    with s.bvh():
        s.spheres(f(8, 3) * 4, rng.uniform(0.2, 0.6, 8), [light(False) for _ in range(8)])
        tris(6, False)
    media = []
    L = rtw.lib()
    for boundary in ("sphere", "cuboid"):
        iso = C.c_uint32()
        # (both between the camera and the world's middle, so that camera rays cross them)
        assert L.rtw_begin_constant_medium(s._p, float(rng.uniform(1.0, 2.0)), s.solid_rgb(0.8, 0.8, 0.8),
                                           C.byref(iso)) == 0
        if boundary == "sphere":
            s.sphere((3.2, 1.0, 3.6), 1.2, 0)
        else:
            with s.translate((-2.5, 0.5, 3.0)):
                s.cuboid(tuple(f(3) * 0.2 - 1), tuple(f(3) * 0.2 + 1), 0)
        assert L.rtw_end(s._p) == 0
        media.append(int(iso.value))
    return s, colour_of, wrapped, media


def _camera_rays(orc, cam, w, h, seed):
    """The primary rays of a w x h, 1-spp frame as the render makes them (lib.rs:84-86, camera.rs:66-74), in the
    image's order (row r = h - 1 - j), each with the path's stream state after its camera draws."""
    L = orc.lib()
    o, d, t, st = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w), f32), np.zeros((h, w), np.uint64)
    draws, out, used, after = np.zeros(64, np.uint32), np.zeros(7, f32), C.c_uint32(), C.c_uint64()
    dp = draws.ctypes.data_as(C.POINTER(C.c_uint32))
    for j in range(h):
        for i in range(w):
            state = L.oracle_path_state(seed, j, i, 0)
            L.oracle_rng_stream(state, 64, dp, C.byref(after))
            u = f32(f32(i) + f32(L.oracle_u32_to_f32(int(draws[0])))) / f32(w - 1)
            v = f32(f32(j) + f32(L.oracle_u32_to_f32(int(draws[1])))) / f32(h - 1)
            L.oracle_get_ray(C.byref(cam), u, v, C.cast(draws.ctypes.data + 8, C.POINTER(C.c_uint32)), 62,
                             out.ctypes.data_as(_F), C.byref(used))
            assert used.value <= 60
            L.oracle_rng_stream(state, 2 + used.value, dp, C.byref(after))
            r = h - 1 - j
            o[r, i], d[r, i], t[r, i], st[r, i] = out[0:3], out[3:6], out[6], after.value
    return o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1), st.reshape(-1)


@functools.lru_cache(maxsize=None)
def _wrapped_case(rtw, orc, uv):
    s, colour_of, wrapped, media = _wrapped_world(rtw, uv)
    cam = rtw.Camera.new((9.0, 3.0, 10.0), (0, 0, 0), (0, 1, 0), 40.0, W3 / H3, 0.1, 13.0)
    ocam = orc.camera_from_fields(cam.as_dict())
    img, _rays = orc.OracleScene(s.dump(), s.images()).render(ocam, BG3, W3, H3, 1, seed=SEED3, max_depth=1)
    img.setflags(write=False)
    return _camera_rays(orc, ocam, W3, H3, SEED3), img.reshape(-1, 3), colour_of, wrapped, media


def test_wrapped_world_winners_match_the_oracle_render(gpu, orc):
    (o, d, t, st), img, colour_of, wrapped, media = _wrapped_case(gpu, orc, False)
    # what the oracle's pixel says of each ray: background = miss, black = a medium's Isotropic, else the light
    want = np.full(len(img), -2, np.int64)
    want[(img == f32(BG3)).all(axis=1)] = -1
    want[(img == 0).all(axis=1)] = -3
    for c, m in colour_of.items():
        want[(img == f32(c)).all(axis=1)] = m
    assert (want != -2).all(), "every pixel is the background, black or one light's colour"
    assert np.isin(want, list(wrapped)).mean() >= 0.15 and (want == -3).sum() >= 20, \
        (np.isin(want, list(wrapped)).mean(), (want == -3).sum())
    s, *_ = _wrapped_world(gpu, False)
    s.commit(device=0)
    assert s.info(3) > 0
    got = s.hit_rays(o, d, t, st, device=0)
    hit = (got["flags"] & gpu.HIT_HIT) != 0
    mat = np.where(hit, got["material"].astype(np.int64), -1)
    mat[hit & np.isin(got["material"], media)] = -3
    bad = np.flatnonzero(mat != want)
    assert bad.size == 0, f"{bad.size} rays: first {bad[0]}: gpu {got[bad[0]]}, oracle material {want[bad[0]]}"


def test_wrapped_world_uv_matches_the_oracle_render(gpu, orc):
    (o, d, t, st), img, _colours, _wrapped, media = _wrapped_case(gpu, orc, True)
    s, *_ = _wrapped_world(gpu, True)
    s.commit(device=0)
    got = s.hit_rays(o, d, t, st, device=0)
    surf = ((got["flags"] & gpu.HIT_HIT) != 0) & ~np.isin(got["material"], media)
    assert surf.mean() >= 0.2
    # a UVDebug light's pixel is (u, v, 0)
    uv = np.stack([got["u"], got["v"], np.zeros(len(got), f32)], axis=1)[surf]
    ref = img[surf]
    same = (uv.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(uv) & np.isnan(ref))
    assert same.all(), f"{(~same.all(axis=1)).sum()} rays' (u, v) differ from the oracle's pixels"
    miss = (got["flags"] & gpu.HIT_HIT) == 0
    assert (img[miss] == f32(BG3)).all() and (img[~miss & ~surf] == 0).all()


# ---------------------------------------------------------------- 4. far origins
def _far_prims(rng):
    prims = [(0, np.array([0, -1000, 0, 1000], f32), 7)]
    for k in range(100):
        r = f32(rng.uniform(0.05, 0.6))
        prims.append((0, np.array([rng.uniform(-6, 6), r, rng.uniform(-6, 6), r], f32), k % 7))
    return prims


def _far_rays(rng, prims, n=N):
    """From 1,000-5,000 units away (above the ground), aimed just outside balls, as tests/test_far_bound.py aims:
    past the centre at a miss distance rho in [r, r + 1.5 reach(D, r)]."""
    U = 2.0 ** -24
    k = rng.integers(1, len(prims), n)
    c = np.array([prims[q][1][:3] for q in k], np.float64)
    r = np.array([prims[q][1][3] for q in k], np.float64)
    D = rng.uniform(1000.0, 5000.0, n)
    u1 = _unit(rng.normal(size=(n, 3)))
    u1[:, 1] = np.abs(u1[:, 1]) + 0.2
    u1 = _unit(u1)
    o = c + u1 * D[:, None]
    x = 40.0 * U * (D * D + r * r)
    reach = np.minimum(x / (2.0 * r), np.sqrt(x)) + U * D
    rho = r + rng.uniform(0.0, 1.0, n) * 1.5 * reach
    w = rng.normal(size=(n, 3))
    w -= u1 * (w * u1).sum(axis=1, keepdims=True)
    d = (c + _unit(w) * rho[:, None] - o) * rng.uniform(0.3, 3.0, (n, 1))
    return o.astype(f32), d.astype(f32), np.zeros(n, f32)


@functools.lru_cache(maxsize=None)
def _far_case(rtw, orc):
    rng = np.random.default_rng(31)  # (a seed whose rays give the spurious hits asserted below)
    prims = _far_prims(rng)
    o, d, t = _far_rays(rng, prims)
    mats = _sphere_mats(rtw.Scene())
    rec, _ = _flat_oracle(orc, rtw, prims, np.array([mats[p[2]] for p in prims], np.uint32), o, d, t)
    rec.setflags(write=False)
    # spurious: the oracle reports a ball although the ray's line passes outside it (exact distance, float64)
    P = np.array([p[1] for p in prims], np.float64)
    ball = ((rec["flags"] & 1) != 0) & (rec["key"] > 0)
    oc = o.astype(np.float64) - P[rec["key"], :3]
    dd = d.astype(np.float64)
    dist = np.linalg.norm(np.cross(oc, dd), axis=1) / np.linalg.norm(dd, axis=1)
    return prims, (o, d, t), rec, int((ball & (dist > P[rec["key"], 3])).sum())


@pytest.mark.parametrize("knob", [None, "RTW_STACK_LDS=4"])
def test_far_origin_rays(gpu, orc, knobs, knob):
    prims, (o, d, t), rec, spurious = _far_case(gpu, orc)
    assert spurious >= 50, spurious
    _set(knobs, knob)
    s, _ = _build(gpu, prims, _sphere_mats)
    s.commit(device=0)
    assert s.info(14) == 1 and s.info(5) == 1, "the far-origin path is on, the ground always-tested"
    cfg = _cfg(s)
    assert (cfg["stack"], cfg["spill"]) == ((4, 1) if knob else (16, 0)) and (cfg["ncap"] > 0) == (knob is None), cfg
    _same(s.hit_rays(o, d, t, device=0), rec, f"far rays under {knob}")


# ---------------------------------------------------------------- 5. launch shapes
@pytest.fixture(scope="module")
def sphere_scene(gpu, orc):
    prims, _, _, _ = _case(gpu, orc, "spheres")
    s, _ = _build(gpu, prims, _sphere_mats)
    return s.commit(device=0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_small_launches(gpu, orc, sphere_scene, n):
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    _same(sphere_scene.hit_rays(o[:n], d[:n], t[:n], device=0), rec[:n], f"n = {n}")


def test_more_than_one_grid_pass_and_staging_chunk(gpu, orc, sphere_scene):
    """The ray set repeated past 1.2 M rays: more than the resident lanes of every variant (at most 256 CUs x 2,048)
    and more than one 2^20-ray staging chunk."""
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    reps = 1_200_000 // N + 1
    got, st = sphere_scene.hit_rays(np.tile(o, (reps, 1)), np.tile(d, (reps, 1)), np.tile(t, reps), device=0,
                                    want_stats=True)
    assert len(got) == reps * N > 1_200_000 and st["rays"] == len(got) and st["paths"] == 0 and st["kernel_ms"] > 0
    a = np.frombuffer(got.tobytes(), np.uint32).reshape(reps, N * 12)
    bad = np.flatnonzero((a != a[0]).any(axis=1))
    assert bad.size == 0, f"repetitions {bad[:8].tolist()} differ from the first"
    _same(got[:N], rec, "first repetition")


def test_device_entry_point_on_a_torch_stream(gpu, orc, sphere_scene):
    import torch
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    rays = gpu.make_rays(o, d, t)
    dev = torch.device("cuda:0")
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to(dev)
    d_hits = torch.zeros(N * 48, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        assert sphere_scene.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), N, 0, stream.cuda_stream) is None
    stream.synchronize()
    got = np.frombuffer(d_hits.cpu().numpy().tobytes(), gpu.HIT_DTYPE)
    _same(got, sphere_scene.hit_rays(o, d, t, device=0), "device vs host entry point")
    _same(got, rec, "device entry point")
    st = sphere_scene.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), N, 0, stream.cuda_stream, want_stats=True)
    assert st["rays"] == N and st["paths"] == 0 and st["kernel_ms"] > 0 and st["node_visits"] == 0


def test_degenerate_rays_leave_their_neighbours_alone(gpu, orc, sphere_scene):
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    o, d = o.copy(), d.copy()
    where = np.array([0, 63, 64, 700, 1999, 2048, 4000, N - 1])
    d[where[0:3]] = 0.0
    o[where[3:6]] = np.nan
    d[where[6:8]] = np.inf
    got = sphere_scene.hit_rays(o, d, t, device=0)  # RTW_OK (hit_rays raises otherwise)
    keep = np.ones(N, bool)
    keep[where] = False
    _same(got[keep], rec[keep], "rays beside the degenerate ones")
    sphere_scene.render_status(0)


# ---------------------------------------------------------------- 6. errors
def test_guard_trip_is_einval_and_reported(gpu, orc):
    prims, (o, d, t), _, _ = _case(gpu, orc, "spheres")
    s, _ = _build(gpu, prims, _sphere_mats)
    s.commit(device=0)
    s.diag_corrupt_bvh(0)
    rays = gpu.make_rays(o[:64], d[:64], t[:64])
    hits = np.zeros(64, gpu.HIT_DTYPE)
    L = gpu.lib()
    rp, hp = rays.ctypes.data_as(C.POINTER(gpu.rtw_ray)), hits.ctypes.data_as(C.POINTER(gpu.rtw_hit))
    assert L.rtw_hit_rays(s._p, 0, 64, rp, hp, None) == gpu.RTW_EINVAL
    assert "guard" in L.rtw_last_error().decode()
    # through the device entry point (no wait), rtw_render_status reports it
    import torch
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    d_hits = torch.zeros(64 * 48, dtype=torch.uint8, device="cuda:0")
    assert L.rtw_hit_rays_device(s._p, 0, 64, d_rays.data_ptr(), d_hits.data_ptr(), None, None) == 0
    assert L.rtw_render_status(s._p, 0) == gpu.RTW_EINVAL
    assert L.rtw_render_status(s._p, 0) == 0  # reported once, then cleared


def test_bad_time_through_the_device_entry_point(gpu, orc, sphere_scene):
    import torch
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    n = 200
    t = t[:n].copy()
    bad = np.array([5, 64, 130])
    t[bad] = [np.nan, 1.5, -0.01]
    rays = gpu.make_rays(o[:n], d[:n], t)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    sphere_scene.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, 0, 0, want_stats=True)
    got = np.frombuffer(d_hits.cpu().numpy().tobytes(), gpu.HIT_DTYPE)
    assert (got["flags"][bad] == gpu.HIT_BAD_RAY).all() and np.isinf(got["t"][bad]).all()
    keep = np.ones(n, bool)
    keep[bad] = False
    _same(got[keep], rec[:n][keep], "rays beside the bad ones")
    with pytest.raises(gpu.RtwError) as e:  # the host call scans the times first
        sphere_scene.hit_rays(o[:n], d[:n], t, device=0)
    assert e.value.code == gpu.RTW_EINVAL
