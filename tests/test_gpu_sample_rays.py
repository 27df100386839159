"""Radiance queries on the GPU (rtw_sample_rays*: Raytracer::sample_ray, lib.rs:97-117, for rays the caller chooses,
every path traced to its end in one persistent launch of the scene's own path-kernel variant).

Every comparison is bit for bit, on uint32 views.  Three references, each computed once per world and shared:
  * the oracle's render of a frame: the records of the frame's camera rays, summed per pixel in sample order in
    float32, are its image, and the sum of their `segments` its ray count;
  * the composed loop written here, camera_rays -> (hit_rays -> scatter_rays)* per path over the host queries, which
    gives every path's colour, segment count, final stream word and end kind: for camera rays and for rays no camera
    made (origins inside the worlds, random directions, times and stream words).
  * for the rays no camera made, the oracle's own sample_ray on them as well (oracle_sample_rays, which
    tests/test_ray_corpus.py ties to the oracle's render): the composed loop runs the kernels' shared bodies, so it moves
    with them; tests/test_gpu_ray_corpus.py holds all three queries to the oracle on a corpus of such rays.
The composed loop's records do not depend on the walk (tests/test_gpu_hit_rays.py pins hit_rays in every walk), so the
knob cases compare the fused kernel of each variant against the records made once under the default knobs."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS, LIGHT, ABSORBED, DEPTH = 0, 1, 2, 3  # how the composed loop saw a path end
# the frames of tests/test_gpu_scatter_rays.py::test_own_integrator_equals_the_oracle_render, and the cow
FRAMES = [
    ("jumpy-balls", 16 / 9, 48, 27, 2, 50),
    ("cornell-box", 1.0, 24, 24, 4, 50),
    ("cornell-box", 1.0, 24, 24, 4, 3),  # depth exhaustion
    ("smokey-cornell-box", 1.0, 24, 24, 3, 50),  # media: the stream word keys the free path; Isotropic
    ("earth", 16 / 9, 32, 18, 2, 50),  # sphere uv into an image
    ("two-perlin-spheres", 16 / 9, 32, 18, 2, 50),
    ("textured-monument", 16 / 9, 32, 18, 2, 50),  # triangle uv
    ("book2-final-scene", 1.0, 24, 24, 2, 50),
    ("wavefront-cow-obj", 16 / 9, 32, 18, 2, 50),  # the S16 mesh walk; the solid-light shortcut
]
SEED = 11


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _words(rec):
    return np.frombuffer(np.ascontiguousarray(rec).tobytes(), np.uint32).reshape(len(rec), -1)


def _same_records(got, want, what):
    a, b = _words(got), _words(want)
    assert a.shape == b.shape, what
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} records differ, first {bad[0]}: {got[bad[0]]} vs " \
                          f"{want[bad[0]]}"


def _compose(rtw, s, rays, bg, max_depth):
    """sample_ray (lib.rs:97-117) per path as the loop hit_rays -> scatter_rays over the host queries, without the fused
    kernel -> (records as rtw_sample_rays must return them, end kind per path)."""
    n = len(rays)
    rec = np.zeros(n, rtw.SAMPLE_DTYPE)
    rec["stream"] = rays["stream"]  # max_depth = 0: copied through (lib.rs:98-100)
    kind = np.full(n, -1)
    T, path, cur = np.ones((n, 3), f32), np.arange(n), rays.copy()
    with np.errstate(all="ignore"):
        for depth in range(max_depth, 0, -1):
            if len(cur) == 0:
                break
            hits = s.hit_rays(cur["origin"], cur["direction"], cur["time"], cur["stream"], device=0)
            rec["segments"][path] += 1
            out, sc = s.scatter_rays(cur, hits, bg, device=0)
            assert not (sc["flags"] & rtw.SCATTER_BAD).any()
            alive = (sc["flags"] & rtw.SCATTER_SCATTERED) != 0
            miss = (sc["flags"] & rtw.SCATTER_MISS) != 0
            end = path[~alive]
            rec["color"][end] = T[end] * sc["emitted"][~alive]  # an absorbed ray: T * 0
            rec["stream"][end] = out["stream"][~alive]
            rec["flags"][end] = np.where(miss[~alive], rtw.SAMPLE_END_MISS, rtw.SAMPLE_END_NO_SCATTER)
            # a light draws nothing: the segment's own word; an absorbed Metal ray carries the advanced word
            kind[end] = np.where(miss[~alive], MISS,
                                 np.where(out["stream"][~alive] == cur["stream"][~alive], LIGHT, ABSORBED))
            T[path[alive]] = T[path[alive]] * sc["attenuation"][alive]
            path, cur = path[alive], out[alive]
            if depth == 1:  # lib.rs:98-100: black, times the attenuations above it
                rec["color"][path] = T[path] * f32(0.0)
                rec["stream"][path] = cur["stream"]
                rec["flags"][path] = rtw.SAMPLE_END_DEPTH
                kind[path] = DEPTH
    assert rec["color"].dtype == f32
    rec.setflags(write=False)
    return rec, kind


@functools.lru_cache(maxsize=None)
def _world(rtw, name, aspect):
    s = rtw.Scene()
    cam, bg = s.preset(name, aspect, seed=3)
    text, imgs = s.dump(), s.images()
    s.commit(device=0)
    return s, cam, bg, text, imgs


@functools.lru_cache(maxsize=None)
def _frame(rtw, orc, frame):
    """A frame's camera rays, its fused records and stats (default knobs), the composed loop's records and end kinds,
    and the oracle's image and ray count: made once, never changed."""
    name, aspect, w, h, spp, max_depth = frame
    s, cam, bg, text, imgs = _world(rtw, name, aspect)
    rays = s.camera_rays(cam, w, h, spp, SEED, device=0)
    rays.setflags(write=False)
    got, st = s.sample_rays(rays, bg, max_depth, device=0, want_stats=True)
    want, kind = _compose(rtw, s, rays, bg, max_depth)
    ref, ref_rays = orc.OracleScene(text, imgs).render(orc.camera_from_fields(cam.as_dict()), bg, w, h, spp, seed=SEED,
                                                       max_depth=max_depth)
    return rays, got, st, want, kind, ref, ref_rays


def _stray_rays(rtw, name, n, seed):
    """n rays no camera made: origins inside the world, random directions, times within the camera's shutter."""
    rng = np.random.default_rng(seed)
    _s, cam, _bg, _t, _i = _world(rtw, name, 16 / 9 if name == "jumpy-balls" else 1.0)
    if name == "jumpy-balls":  # above the ground sphere, among the balls
        o = rng.uniform((-10, 0.05, -10), (10, 3, 10), (n, 3))
    else:  # inside the 555-unit box
        o = rng.uniform(10, 545, (n, 3))
    d = rng.normal(size=(n, 3)) * rng.uniform(0.1, 5.0, (n, 1))
    t = rng.uniform(cam.c.time0, cam.c.time1, n).astype(f32)
    t = np.clip(t, f32(cam.c.time0), f32(cam.c.time1))
    rays = rtw.make_rays(o, d, t, rng.integers(1, 1 << 63, n, dtype=np.uint64))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def _stray(rtw, name, max_depth):
    aspect = 16 / 9 if name == "jumpy-balls" else 1.0
    s, _cam, bg, _t, _i = _world(rtw, name, aspect)
    rays = _stray_rays(rtw, name, 2000, 5 + max_depth)
    got, st = s.sample_rays(rays, bg, max_depth, device=0, want_stats=True)
    want, kind = _compose(rtw, s, rays, bg, max_depth)
    return rays, got, st, want, kind


@functools.lru_cache(maxsize=None)
def _stray_oracle(rtw, orc, name, max_depth):
    """oracle_sample_rays (sample_ray_iter on the flat list, tests/test_ray_corpus.py) on the stray rays: the reference
    that shares no code with the kernels"""
    _s, _cam, bg, text, imgs = _world(rtw, name, 16 / 9 if name == "jumpy-balls" else 1.0)
    rec = orc.OracleScene(text, imgs).sample_rays(_stray(rtw, name, max_depth)[0], bg, max_depth)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def _material_world(rtw):
    """Five spheres, one per material, one Metal with fuzz 1 (it absorbs grazing rays): 120 rays aimed at each from
    all around, a list-mode world of every material kind -> (scene, background, rays, fused, composed, kinds, dump)."""
    s = rtw.Scene()
    ids = [s.lambertian_solid((0.8, 0.3, 0.1)), s.metal((0.9, 0.8, 0.7), 1.0), s.metal((0.6, 0.7, 0.8), 0.3),
           s.dielectric(1.5), s.diffuse_light(s.solid_rgb(4.0, 3.0, 2.0))]
    for k, m in enumerate(ids):
        s.sphere((3.0 * k, 0.0, 0.0), 1.0, m)
    text = s.dump()
    s.commit(device=0)
    rng = np.random.default_rng(21)
    n = 600
    which = np.repeat(np.arange(5), n // 5)
    centre = (which * 3.0)[:, None] * np.array([1.0, 0.0, 0.0])
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.where(which == 1, rng.uniform(3.0, 4.0, n), rng.uniform(1.5, 4.0, n))
    o = centre + u * dist[:, None]
    # aimed at a point of the disk through the centre that faces the origin, uniform over the disk; the fuzz-1 Metal's
    # rays from 3 to 4 radii away at 0.93 to 0.97 of the radius: impact parameters 0.89 to 0.94, so the reflected unit
    # direction stands 0.46 to 0.34 above the surface and the unit-ball offset takes it below for 0.18 to 0.24 of the
    # ball (the cap of height h = 1 - that, h^2 (3 - h) / 4): about 25 of its 120 rays are expected to be absorbed, and
    # the test below asks for 10
    p = np.cross(u, rng.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    r = np.where(which == 1, rng.uniform(0.93, 0.97, n), np.sqrt(rng.random(n)) * 0.97)
    d = (centre + p * r[:, None]) - o
    rays = rtw.make_rays(o, d, rng.random(n).astype(f32), rng.integers(1, 1 << 63, n, dtype=np.uint64))
    rays.setflags(write=False)
    bg = (0.25, 0.5, 0.75)
    got = s.sample_rays(rays, bg, 50, device=0)
    want, kind = _compose(rtw, s, rays, bg, 50)
    return s, bg, rays, got, want, kind, text


# ---------------------------------------------------------------- 1. against the oracle's render
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}-{f[2]}x{f[3]}x{f[4]}-d{f[5]}")
def test_camera_ray_samples_sum_to_the_oracle_render(gpu, orc, frame):
    name, aspect, w, h, spp, max_depth = frame
    rays, got, st, _want, _kind, ref, ref_rays = _frame(gpu, orc, frame)
    assert got.dtype == gpu.SAMPLE_DTYPE and len(got) == w * h * spp
    assert not (got["flags"] & gpu.SAMPLE_BAD_RAY).any() and (got["reserved"] == 0).all()
    with np.errstate(all="ignore"):
        pixel = np.zeros((h * w, 3), f32)
        Ls = got["color"].reshape(h * w, spp, 3)
        for k in range(spp):  # float32 throughout, in sample order, as reduce_kernel
            pixel = pixel + Ls[:, k]
    img = pixel.reshape(h, w, 3)
    assert img.dtype == f32
    bad = np.argwhere(_bits(img) != _bits(ref))
    assert bad.size == 0, f"{len(bad)} mismatching components, first {bad[:4].tolist()}: " \
                          f"samples {img[tuple(bad[0][:2])]} oracle {ref[tuple(bad[0][:2])]}"
    segments = int(got["segments"].astype(np.uint64).sum())
    assert segments == ref_rays == st["rays"], (segments, ref_rays, st["rays"])
    assert st["paths"] == len(rays) and st["kernel_ms"] > 0 and st["total_ms"] > 0
    # the same frame through the render
    s, cam, bg, _t, _i = _world(gpu, name, aspect)
    rimg, rst = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED, max_depth=max_depth).render()
    assert (_bits(rimg) == _bits(img)).all() and rst["rays"] == segments


# ---------------------------------------------------------------- 2. against the composed loop, per path
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}-{f[2]}x{f[3]}x{f[4]}-d{f[5]}")
def test_camera_ray_samples_equal_the_composed_loop(gpu, orc, frame):
    _rays, got, _st, want, kind, _ref, _n = _frame(gpu, orc, frame)
    assert (kind >= 0).all()
    _same_records(got, want, frame[0])


@pytest.mark.parametrize("name,max_depth", [("jumpy-balls", 50), ("cornell-box", 3), ("cornell-box", 50)])
def test_stray_ray_samples_equal_the_composed_loop(gpu, orc, name, max_depth):
    rays, got, st, want, kind = _stray(gpu, name, max_depth)
    assert len(rays) == 2000 and (kind >= 0).all()
    _same_records(got, want, f"{name} at depth {max_depth}")
    _same_records(got, _stray_oracle(gpu, orc, name, max_depth), f"{name} at depth {max_depth}, against the oracle")
    assert st["rays"] == int(want["segments"].sum()) and st["paths"] == 2000
    assert (want["segments"] <= max_depth).all() and (want["segments"] >= 1).all()


def test_material_world_samples_equal_the_composed_loop(gpu, orc):
    s, bg, rays, got, want, kind, text = _material_world(gpu)
    assert s.info(3) == 0 and s.info(19) == (((1 << 16) - 1) | (1 << 17)) | (1 << 16), "the all-features list kernel"
    _same_records(got, want, "one sphere per material")
    _same_records(got, orc.OracleScene(text).sample_rays(rays, bg, 50), "one sphere per material, against the oracle")
    assert (kind == ABSORBED).sum() >= 10, "the fuzz-1 Metal absorbs"


def test_every_end_kind_occurs(gpu, orc):
    """In the composed loop's own account of the paths compared above."""
    kinds = [_frame(gpu, orc, f)[4] for f in FRAMES]
    kinds += [_stray(gpu, "jumpy-balls", 50)[4], _stray(gpu, "cornell-box", 3)[4], _stray(gpu, "cornell-box", 50)[4],
              _material_world(gpu)[5]]
    count = np.bincount(np.concatenate(kinds), minlength=4)
    assert (count >= 10).all(), dict(zip(("miss", "light", "absorbed", "depth"), count.tolist()))
    assert np.bincount(_stray(gpu, "cornell-box", 3)[4], minlength=4)[DEPTH] >= 100
    # the stray paths' ends in the oracle's account: a miss, no scatter (a light, an absorbed ray), depth
    ends = np.array([gpu.SAMPLE_END_MISS, gpu.SAMPLE_END_NO_SCATTER, gpu.SAMPLE_END_NO_SCATTER, gpu.SAMPLE_END_DEPTH])
    for name, max_depth in (("jumpy-balls", 50), ("cornell-box", 3), ("cornell-box", 50)):
        assert (_stray_oracle(gpu, orc, name, max_depth)["flags"] == ends[_stray(gpu, name, max_depth)[4]]).all()


# ---------------------------------------------------------------- 3. regeneration and every walk
def _cfg(s):
    """rtw_scene_info 16-23: stack, spill, occ, feat, blk, ncap, half, s16 of the selected kernel"""
    return dict(zip(("stack", "spill", "occ", "feat", "blk", "ncap", "half", "s16"), (s.info(k) for k in range(16, 24))))


def _set(knobs, knob):
    for kv in (knob or "").split(","):
        if kv:
            knobs.setenv(*kv.split("="))


def test_small_batches_regenerate_to_the_same_records(gpu, knobs):
    """20,000 camera rays: by default the small-launch rule hands out 128 at a time, so few waves run full pools; with
    RTW_BATCH=64 every refill is one wave-load and 313 waves regenerate from the dispenser throughout."""
    s, cam, bg, _t, _i = _world(gpu, "jumpy-balls", 16 / 9)
    rays = s.camera_rays(cam, 100, 100, 2, SEED, device=0)
    assert len(rays) == 20000
    base, st0 = s.sample_rays(rays, bg, 50, device=0, want_stats=True)
    knobs.setenv("RTW_BATCH", "64")
    got, st1 = s.sample_rays(rays, bg, 50, device=0, want_stats=True)
    _same_records(got, base, "RTW_BATCH=64")
    assert st0["rays"] == st1["rays"] == int(base["segments"].sum())
    knobs.setenv("RTW_REGEN_MIN", "1")
    _same_records(s.sample_rays(rays, bg, 50, device=0), base, "RTW_BATCH=64, RTW_REGEN_MIN=1")


F_LIST, F_TRI = 1 << 16, 1 << 3
F_ALL = ((1 << 16) - 1) | (1 << 17)
SPHERES, TRIANGLES, RECTS = FRAMES[0], FRAMES[8], FRAMES[1]
WALKS = [
    (SPHERES, None, dict(blk=1024, ncap=144, half=0, occ=8)),
    (SPHERES, "RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
    (SPHERES, "RTW_LDS_NODES=0", dict(ncap=0, blk=256, occ=6)),
    (SPHERES, "RTW_HALF_NODES=1", dict(ncap=144, blk=512, half=1)),
    (SPHERES, "RTW_LDSN_BLK=512", dict(ncap=144, blk=512, half=0)),
    (SPHERES, "RTW_GENERIC=1,RTW_OCC=5", dict(feat=F_ALL, ncap=0, occ=5, blk=256)),
    (TRIANGLES, None, dict(s16=1, half=1, occ=7)),
    (TRIANGLES, "RTW_STACK_LDS=4", dict(stack=4, spill=1, feat=F_ALL)),
    (TRIANGLES, "RTW_MESH_S16=0", dict(s16=0, half=1, occ=5)),
    (TRIANGLES, "RTW_MESH_S16=6", dict(s16=1, half=1, occ=6)),
    (TRIANGLES, "RTW_GENERIC=1", dict(feat=F_ALL, s16=0, occ=5)),
    (RECTS, None, dict(feat=lambda f: f & F_LIST and f != (F_ALL | F_LIST), occ=8)),
    (RECTS, "RTW_LIST_ALL=1", dict(feat=F_ALL | F_LIST)),
    (RECTS, "RTW_GENERIC=1", dict(feat=F_ALL | F_LIST)),
]


@pytest.mark.parametrize("frame,knob,cfg", WALKS, ids=[f"{f[0]}-{k}" for f, k, _c in WALKS])
def test_every_walk_equals_the_composed_loop(gpu, orc, knobs, frame, knob, cfg):
    rays, _got, st0, want, _kind, _ref, _n = _frame(gpu, orc, frame)  # (made under the default knobs)
    s, _cam, bg, _t, _i = _world(gpu, frame[0], frame[1])
    _set(knobs, knob)
    have = _cfg(s)
    for k, v in cfg.items():
        assert v(have[k]) if callable(v) else have[k] == v, (knob, k, have)
    got, st = s.sample_rays(rays, bg, frame[5], device=0, want_stats=True)
    _same_records(got, want, f"{frame[0]} under {knob}")
    assert st["rays"] == st0["rays"]


# ---------------------------------------------------------------- 4. shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_small_launches(gpu, orc, n):
    rays, _got, _st, want, _kind, _ref, _n = _frame(gpu, orc, SPHERES)
    s, _cam, bg, _t, _i = _world(gpu, "jumpy-balls", 16 / 9)
    got, st = s.sample_rays(rays[:n], bg, 50, device=0, want_stats=True)
    _same_records(got, want[:n], f"n = {n}")
    assert st["rays"] == int(want["segments"][:n].sum()) and st["paths"] == n


def test_second_staging_chunk_and_more_rays_than_resident_lanes(gpu):
    """2^20 + 65 rays through the host form: 20,000 camera rays tiled, every copy's records equal to the first's."""
    s, cam, bg, _t, _i = _world(gpu, "jumpy-balls", 16 / 9)
    rays = s.camera_rays(cam, 100, 100, 2, SEED, device=0)
    first = s.sample_rays(rays, bg, 50, device=0)
    total, nb = (1 << 20) + 65, len(rays)
    reps = total // nb + 1
    got, st = s.sample_rays(np.tile(rays, reps)[:total], bg, 50, device=0, want_stats=True)
    assert len(got) == total and st["paths"] == total and st["kernel_ms"] > 0
    a = _words(got)
    full = a[:(reps - 1) * nb].reshape(reps - 1, nb * 8)
    bad = np.flatnonzero((full != _words(first).reshape(-1)).any(axis=1))
    assert bad.size == 0, f"copies {bad[:8].tolist()} differ from a launch of the 20,000 alone"
    tail = a[(reps - 1) * nb:]
    assert len(tail) > 65 and (tail == a[:len(tail)]).all(), "the last, partial copy (across the chunk boundary)"
    assert st["rays"] == int(got["segments"].astype(np.uint64).sum()), "segments are summed over the staging chunks"


def test_max_depth_0_and_1(gpu, orc):
    rays, _got, _st, _want, _kind, _ref, _n = _frame(gpu, orc, SPHERES)
    s, _cam, bg, _t, _i = _world(gpu, "jumpy-balls", 16 / 9)
    got, st = s.sample_rays(rays, bg, 0, device=0, want_stats=True)  # lib.rs:98-100
    assert (_bits(got["color"]) == 0).all(), "+0"
    assert (got["segments"] == 0).all() and (got["flags"] == 0).all() and (got["stream"] == rays["stream"]).all()
    assert st["rays"] == 0 and st["paths"] == len(rays)
    want, kind = _compose(gpu, s, rays, bg, 1)
    got = s.sample_rays(rays, bg, 1, device=0)
    _same_records(got, want, "max_depth = 1")
    assert (got["segments"] == 1).all() and (kind == DEPTH).sum() > len(rays) // 4 and (kind == MISS).any()
    depth = kind == DEPTH
    assert (_bits(got["color"][depth]) & 0x7FFFFFFF == 0).all(), "T * 0"


# ---------------------------------------------------------------- 5. bad and degenerate rays, 6. the device form
def _device_samples(gpu, s, rays, bg, max_depth, stream=None, want_stats=False):
    import torch
    dev = torch.device("cuda:0")
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.full((n * 32,), 0xAB, dtype=torch.uint8, device=dev)
    st = s.sample_rays_device(d_rays.data_ptr(), bg, max_depth, d_out.data_ptr(), n, 0,
                              stream.cuda_stream if stream is not None else 0, want_stats=want_stats)
    torch.cuda.synchronize(dev)
    out = np.frombuffer(d_out.cpu().numpy().tobytes(), gpu.SAMPLE_DTYPE)
    return (out, st) if want_stats else out


def test_bad_and_degenerate_rays_leave_their_neighbours_alone(gpu, orc):
    """(sample_kernel mends the caller's generator state with xoro_seed before anything can draw from it, so the zero
    stream word below cannot reach a rejection loop.)"""
    rays, _got, _st, want, _kind, _ref, _n = _frame(gpu, orc, SPHERES)
    s, _cam, bg, _t, _i = _world(gpu, "jumpy-balls", 16 / 9)
    n = 200
    good = _device_samples(gpu, s, rays[:n], bg, 50)
    _same_records(good, want[:n], "device form")
    r = rays[:n].copy()
    bad = np.array([5, 63, 64, 129])
    r["time"][bad[0]], r["time"][bad[1]], r["time"][bad[2]] = 2.0, np.nan, -0.25
    r["stream"][bad[3]] = 0
    odd = np.array([7, 65, 100, 130, 131, 199])
    r["direction"][odd[0]] = 0.0
    r["direction"][odd[1]] = (np.nan, 1.0, 0.0)
    r["origin"][odd[2]] = (np.inf, 0.0, 0.0)
    r["origin"][odd[3]] = np.nan
    r["direction"][odd[4]] = (np.inf, -np.inf, 1.0)
    r["origin"][odd[5]], r["direction"][odd[5]] = 0.0, 0.0
    got = _device_samples(gpu, s, r, bg, 50)
    assert (got["flags"][bad] == gpu.SAMPLE_BAD_RAY).all()
    w = _words(got[bad])
    assert (np.delete(w, 6, axis=1) == 0).all(), "every other field of a bad record is 0"
    ends = (gpu.SAMPLE_END_MISS, gpu.SAMPLE_END_NO_SCATTER, gpu.SAMPLE_END_DEPTH)
    assert np.isin(got["flags"][odd], ends).all() and (got["segments"][odd] >= 1).all()
    assert (got["segments"][odd] <= 50).all() and (got["reserved"] == 0).all()
    keep = np.ones(n, bool)
    keep[bad] = keep[odd] = False
    _same_records(got[keep], good[keep], "records beside the bad and the degenerate ones")
    s.render_status(device=0)  # no guard trip
    # the host form scans: RTW_EINVAL naming the first bad record
    with pytest.raises(gpu.RtwError) as e:
        s.sample_rays(r, bg, 50, device=0)
    assert e.value.code == gpu.RTW_EINVAL and "ray 5" in str(e.value)
    r["time"][bad[:3]] = 0.5
    with pytest.raises(gpu.RtwError) as e:
        s.sample_rays(r, bg, 50, device=0)
    assert e.value.code == gpu.RTW_EINVAL and "ray 129" in str(e.value) and "stream" in str(e.value)


def test_device_form_between_two_renders_on_a_torch_stream(gpu, orc):
    import torch
    name, aspect, w, h, spp, max_depth = SPHERES
    rays, _got, st0, want, _kind, ref, ref_rays = _frame(gpu, orc, SPHERES)
    s, cam, bg, _t, _i = _world(gpu, name, aspect)
    dev = torch.device("cuda:0")
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    img = [torch.zeros((h, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    rt = gpu.Raytracer(s, cam, bg, w, h, spp, seed=SEED, max_depth=max_depth)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        rt.render_device(img[0].data_ptr(), 0, stream_ptr=stream.cuda_stream)
        assert s.sample_rays_device(d_rays.data_ptr(), bg, max_depth, d_out.data_ptr(), n, 0,
                                    stream.cuda_stream) is None
        rst = rt.render_device(img[1].data_ptr(), 0, stream_ptr=stream.cuda_stream, want_stats=True)
    stream.synchronize()
    for k in range(2):
        assert (_bits(img[k].cpu().numpy()) == _bits(ref)).all(), f"render {k + 1}"
    assert rst["rays"] == ref_rays
    _same_records(np.frombuffer(d_out.cpu().numpy().tobytes(), gpu.SAMPLE_DTYPE), want, "samples between two renders")
    got, st = _device_samples(gpu, s, rays, bg, max_depth, stream=stream, want_stats=True)
    _same_records(got, want, "with stats")
    assert st["rays"] == ref_rays == st0["rays"] and st["paths"] == n and st["kernel_ms"] > 0 and st["total_ms"] > 0
