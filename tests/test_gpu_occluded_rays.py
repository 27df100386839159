"""rtw_occluded_rays / rtw_occluded_rays_device (occluded_kernel) on the GPU against the definition
occluded = hit and not t > T on the ORACLE's closest-hit record, for every ray of tests/test_ray_corpus.py's worlds.

The bound of ray k follows from k % 10 and the oracle's record (bounds() below): +inf, t itself (the bound is inclusive),
its two float neighbours, t / 2, 2 t, 0.001, a bound below 0.001, FLT_MAX; a miss gets 10^u for a seeded u in [-3, 3]
in the t-derived classes, and so does a hit whose t is NaN (list mode's in-plane hit: a NaN bound would be a bad ray,
and the hit occludes under every bound).  k % 10 == 9 stands for t_max = NULL: every world is queried a second time
without bounds and compared with the hit flag.  No ray is excluded; tied rays need no care, since the hit flag and t are
exact for them too.

Then the walks of tests/test_gpu_ray_corpus.py's table, the key-0 trap (a seeded best would make the bound exclusive for
the leaf with key 0), the in-plane (NaN) hit, launch sizes around a wave, a call across a staging chunk, the device
form on a torch stream, far origins and the traversal guard."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_hit_rays import N, _build, _case, _far_case, _sphere_mats
from test_gpu_ray_corpus import F_LIST, LIST_WORLD, WALKS, WALK_CASES, _cfg, _scene
from test_ray_corpus import CASES, answers, case_id, corpus

pytestmark = pytest.mark.gpu

f32 = np.float32
FLT_MAX = np.finfo(f32).max
BELOW = np.array([0.0, 0.0005, -1.0, -np.inf], f32)  # class 7: bounds under t_min = 0.001


def bounds(rec, seed, first=0):
    """T per ray from its index (first + k) % 10 and its record, as the module docstring says -> float32 [n]"""
    n = len(rec)
    k = np.arange(first, first + n)
    t = rec["t"].astype(f32)
    hit = ((rec["flags"] & 1) != 0) & ~np.isnan(t)
    loose = (f32(10.0) ** np.random.default_rng(seed).uniform(-3, 3, n)).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        by_t = {1: t, 2: np.nextafter(t, f32(0)), 3: np.nextafter(t, f32(np.inf)), 4: t / f32(2), 5: t * f32(2)}
    T = np.full(n, np.inf, f32)  # classes 0 and 9
    for c, v in by_t.items():
        T = np.where(k % 10 == c, np.where(hit, v, loose), T)
    T = np.where(k % 10 == 6, f32(0.001), T)
    T = np.where(k % 10 == 7, BELOW[(k // 10) % 4], T)
    T = np.where(k % 10 == 8, FLT_MAX, T).astype(f32)
    assert not np.isnan(T).any()
    return T


def expected(rec, T):
    """the contract on a closest-hit record: (flags & RTW_HIT_HIT) && !(t > T); a NaN t passes the compare"""
    hit = (rec["flags"] & 1) != 0
    with np.errstate(invalid="ignore"):
        return (hit & ~(rec["t"].astype(f32) > T)).astype(np.uint8)


def _occluded(s, rays, T, **kw):
    return s.occluded_rays(rays["origin"], rays["direction"], rays["time"], rays["stream"], T, device=0, **kw)


def _check(s, rays, rec, seed, what):
    T = bounds(rec, seed)
    want = expected(rec, T)
    got, st = _occluded(s, rays, T, want_stats=True)
    assert got.dtype == np.uint8 and got.shape == (len(rays),)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {len(rays)} answers differ, first ray {bad[0]}: got {got[bad[0]]}, " \
                          f"t = {rec['t'][bad[0]]!r}, T = {T[bad[0]]!r}"
    assert st["rays"] == len(rays) and st["paths"] == 0 and st["kernel_ms"] > 0 and st["total_ms"] > 0
    nob = _occluded(s, rays, None)  # t_max = NULL: the hit flag
    bad = np.flatnonzero(nob != (rec["flags"] & 1))
    assert bad.size == 0, f"{what}, no bounds: {bad.size} answers differ from the hit flag, first ray {bad[0]}"
    s.render_status(device=0)
    return want, T


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_answers_equal_the_definition_on_the_oracles_records(gpu, orc, knobs, case):
    a = answers(gpu, orc, case, knobs)
    rays, _label = corpus(gpu, orc, case, knobs)
    s, _bg = _scene(gpu, case, knobs)
    want, T = _check(s, rays, a["hits"], 100 + CASES.index(case), case_id(case))
    # the bounds decide something: both answers occur among the hits
    hit = (a["hits"]["flags"] & 1) != 0
    assert want[hit].min() == 0 and want[hit].max() == 1 and not want[~hit].any()


def _walks():
    for case in WALK_CASES:
        for knob, cfg in WALKS["list" if case == LIST_WORLD else case[0]]:
            yield case, knob, cfg


@pytest.mark.parametrize("case,knob,cfg", list(_walks()), ids=[f"{case_id(c)}-{k}" for c, k, _ in _walks()])
def test_every_walk_equals_the_definition(gpu, orc, knobs, case, knob, cfg):
    a = answers(gpu, orc, case, knobs)
    rays, _label = corpus(gpu, orc, case, knobs)
    s, _bg = _scene(gpu, case, knobs)  # (committed under the default knobs)
    base = _cfg(s)
    if case == LIST_WORLD:
        assert s.info(3) == 0 and base["feat"] & F_LIST, "list mode"
    for kv in knob.split(","):
        knobs.setenv(*kv.split("="))
    have = _cfg(s)
    for k, v in cfg.items():
        assert have[k] == v, (knob, k, have)
    assert have != base or case == LIST_WORLD, "the knob selects another kernel"
    _check(s, rays, a["hits"], 200 + CASES.index(case), f"{case_id(case)} under {knob}")


# ---------------------------------------------------------------- the bound is inclusive for the leaf with key 0 too
@pytest.mark.parametrize("knob", [None, "RTW_LIST_MAX=0", "RTW_LIST_ALL=1"])
def test_the_bound_is_inclusive_for_key_0(gpu, orc, knobs, knob):
    """Two spheres; every ray hits the first one (key 0) and nothing else.  T == t exactly occludes, the float below t
    does not -- in the world's default variant, with a BVH (RTW_LIST_MAX=0) and in list mode."""
    if knob:
        knobs.setenv(*knob.split("="))
    s = gpu.Scene()
    m = s.lambertian_solid((0.5, 0.5, 0.5))
    s.sphere((0.0, 0.0, -3.0), 1.0, m)
    s.sphere((40.0, 0.0, -3.0), 1.0, m)
    text = s.dump()
    s.commit(device=0)
    assert (s.info(3) > 0) == (knob == "RTW_LIST_MAX=0")
    rng = np.random.default_rng(5)
    n = 130
    o = rng.uniform(-0.5, 0.5, (n, 3)).astype(f32)
    d = (np.array([0.0, 0.0, -3.0]) + rng.uniform(-0.5, 0.5, (n, 3)) - o).astype(f32)
    o[0], d[0] = (0, 0, 0), (0, 0, -1)  # t = 2 exactly
    rays = gpu.make_rays(o, d, np.zeros(n, f32), np.arange(1, n + 1, dtype=np.uint64))
    rec = orc.OracleScene(text).hit_rays(rays)
    assert ((rec["flags"] & 1) != 0).all() and rec["t"][0] == 2.0
    assert (s.hit_rays(o, d, device=0)["key"] == 0).all(), "the winner is the leaf with key 0"
    t = rec["t"].astype(f32)
    assert (_occluded(s, rays, t) == 1).all(), "T == t"
    assert (_occluded(s, rays, np.nextafter(t, f32(0))) == 0).all(), "T just below t"
    assert (_occluded(s, rays, np.nextafter(t, f32(np.inf))) == 1).all(), "T just above t"
    s.render_status(device=0)


# ---------------------------------------------------------------- the in-plane (NaN) hit
def _in_plane_world(rtw, n_far):
    """tests/test_gpu_hit_rays.py::_in_plane_world: one xy rect in the plane z = 0 (leaf 0), n_far rects far behind"""
    s = rtw.Scene()
    m = s.lambertian_solid((0.5, 0.5, 0.5))
    s.xy_rect(0.0, 1.0, 0.0, 1.0, 0.0, m)
    k = np.arange(n_far, dtype=f32)
    s.rects(np.full(n_far, 2), k, k + 1, k, k + 1, -20.0 - k, [m] * n_far)
    return s.commit(device=0)


@pytest.mark.parametrize("knob", [None, "RTW_LIST_ALL=1", "RTW_LIST_MAX=0"])
def test_in_plane_hit_occludes_under_every_bound(gpu, knobs, knob):
    """A ray in a rect's plane hits it with t = NaN in the list-mode loops, and a NaN passes `!(t > T)`: occluded for
    T = inf, 1 and 0.  A BVH variant reports no such hit, and the answer follows its own rtw_hit_rays record.  The
    neighbours (t = 3 through the same rect) are ordinary."""
    if knob:
        knobs.setenv(*knob.split("="))
    s = _in_plane_world(gpu, 12)
    listed = s.info(3) == 0
    assert listed == (knob != "RTW_LIST_MAX=0")
    o = np.array([[0.25, 0.5, 3.0], [0.25, 0.5, 0.0], [0.75, 0.5, 3.0]], f32)
    d = np.array([[0, 0, -1], [1, 0, 0], [0, 0, -1]], f32)
    rec = s.hit_rays(o, d, device=0)
    assert bool(rec["flags"][1] & 1) == listed and (not listed or np.isnan(rec["t"][1]))
    for T in (np.inf, 1.0, 0.0):
        got = s.occluded_rays(o, d, None, None, np.full(3, T, f32), device=0)
        assert list(got) == list(expected(rec, f32(T))), (knob, T, got)
        assert got[1] == (1 if listed else 0) and got[0] == got[2] == (1 if T >= 3.0 else 0)
    s.render_status(device=0)


# ---------------------------------------------------------------- launch shapes
@pytest.fixture(scope="module")
def sphere_scene(gpu, orc):
    prims, _, _, _ = _case(gpu, orc, "spheres")
    s, _ = _build(gpu, prims, _sphere_mats)
    return s.commit(device=0)


def _sphere_rays(gpu, orc):
    _, (o, d, t), rec, _ = _case(gpu, orc, "spheres")
    return gpu.make_rays(o, d, t), rec  # the oracle's flat-list records


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_small_launches(gpu, orc, sphere_scene, n):
    rays, rec = _sphere_rays(gpu, orc)
    T = bounds(rec, 300)[:n]
    got = _occluded(sphere_scene, rays[:n], T)
    assert got.shape == (n,) and (got == expected(rec[:n], T)).all(), f"n = {n}"
    sphere_scene.render_status(0)


def test_a_call_across_a_staging_chunk(gpu, orc, sphere_scene):
    """2^20 + 65 rays: two staging chunks, the second a wave and a lane, and more than one grid pass.  Expected from
    the same build's rtw_hit_rays records for the same array."""
    rays, _rec = _sphere_rays(gpu, orc)
    n = (1 << 20) + 65
    big = np.tile(rays, n // N + 1)[:n]
    rec = sphere_scene.hit_rays(big["origin"], big["direction"], big["time"], big["stream"], device=0)
    T = bounds(rec, 301)
    got, st = _occluded(sphere_scene, big, T, want_stats=True)
    want = expected(rec, T)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} answers differ, first ray {bad[0]}"
    assert st["rays"] == n and st["paths"] == 0 and st["kernel_ms"] > 0
    assert 0 < want.sum() < ((rec["flags"] & 1) != 0).sum()
    sphere_scene.render_status(0)


# ---------------------------------------------------------------- the device form
def _device_call(gpu, s, rays, T, tail=64):
    """on a torch stream, over an output prefilled with 0xAB and `tail` more bytes -> (answers, the tail)"""
    import torch
    dev = torch.device("cuda:0")
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).to(dev)
    d_T = torch.from_numpy(np.ascontiguousarray(T, f32)).to(dev) if T is not None else None
    d_out = torch.full((n + tail,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        assert s.occluded_rays_device(d_rays.data_ptr(), d_T.data_ptr() if d_T is not None else 0, d_out.data_ptr(), n,
                                      0, stream.cuda_stream) is None
    stream.synchronize()
    st = s.occluded_rays_device(d_rays.data_ptr(), d_T.data_ptr() if d_T is not None else 0, d_out.data_ptr(), n, 0,
                                stream.cuda_stream, want_stats=True)
    assert st["rays"] == n and st["paths"] == 0 and st["kernel_ms"] > 0
    out = d_out.cpu().numpy()
    return out[:n], out[n:]


def test_device_form_on_a_torch_stream(gpu, orc, sphere_scene):
    rays, rec = _sphere_rays(gpu, orc)
    T = bounds(rec, 302)
    for n in (N, 65):
        got, tail = _device_call(gpu, sphere_scene, rays[:n], T[:n])
        assert (got == expected(rec[:n], T[:n])).all(), n
        assert (tail == 0xAB).all(), "nothing is written beyond n bytes"
    got, tail = _device_call(gpu, sphere_scene, rays, None)
    assert (got == (rec["flags"] & 1)).all() and (tail == 0xAB).all()
    sphere_scene.render_status(0)


def test_bad_rays_through_the_device_form(gpu, orc, sphere_scene):
    """A bad time or a NaN t_max comes back RTW_OCCLUDED_BAD_RAY, untraced, its neighbours intact; the host form
    answers RTW_EINVAL for the same arrays."""
    rays, rec = _sphere_rays(gpu, orc)
    n = 200
    rays, T = rays[:n].copy(), bounds(rec, 303)[:n].copy()
    bad_time, bad_T = np.array([5, 64, 130]), np.array([63, 131])
    rays["time"][bad_time] = [np.nan, 1.5, -0.01]
    T[bad_T] = np.nan
    got, tail = _device_call(gpu, sphere_scene, rays, T)
    bad = np.concatenate([bad_time, bad_T])
    assert (got[bad] == gpu.OCCLUDED_BAD_RAY).all() and (tail == 0xAB).all()
    keep = np.ones(n, bool)
    keep[bad] = False
    assert (got[keep] == expected(rec[:n], T)[keep]).all(), "rays beside the bad ones"
    for arrays in ((rays, np.where(np.isnan(T), f32(1), T)), (np.delete(rays, bad_time), np.delete(T, bad_time))):
        with pytest.raises(gpu.RtwError) as e:  # the host call scans first
            _occluded(sphere_scene, *arrays)
        assert e.value.code == gpu.RTW_EINVAL
    sphere_scene.render_status(0)


def test_degenerate_rays_leave_their_neighbours_alone(gpu, orc, sphere_scene):
    rays, rec = _sphere_rays(gpu, orc)
    rays, T = rays.copy(), bounds(rec, 304)
    where = np.array([0, 63, 64, 700, 1999, 2048, 4000, N - 1])
    rays["direction"][where[0:3]] = 0.0
    rays["origin"][where[3:6]] = np.nan
    rays["direction"][where[6:8]] = np.inf
    keep = np.ones(N, bool)
    keep[where] = False
    for got in (_occluded(sphere_scene, rays, T), _device_call(gpu, sphere_scene, rays, T)[0]):
        assert (got[keep] == expected(rec, T)[keep]).all(), "rays beside the degenerate ones"
        assert (got[where] <= 1).all()
    sphere_scene.render_status(0)


# ---------------------------------------------------------------- far origins, the guard
@pytest.mark.parametrize("knob", [None, "RTW_STACK_LDS=4"])
def test_far_origin_rays(gpu, orc, knobs, knob):
    prims, (o, d, t), rec, spurious = _far_case(gpu, orc)
    assert spurious >= 50, spurious
    if knob:
        knobs.setenv(*knob.split("="))
    s, _ = _build(gpu, prims, _sphere_mats)
    s.commit(device=0)
    assert s.info(14) == 1 and s.info(5) == 1, "the far-origin path is on, the ground always-tested"
    cfg = _cfg(s)
    assert (cfg["stack"], cfg["spill"]) == ((4, 1) if knob else (16, 0)) and (cfg["ncap"] > 0) == (knob is None), cfg
    _check(s, gpu.make_rays(o, d, t), rec, 305, f"far rays under {knob}")


def test_guard_trip_is_einval_and_reported(gpu, orc):
    """A corrupt tree (the test hook's cycle): the bounded walk trips its guard, the wave leaves its loop as
    hit_kernel's does, and the call reports RTW_EINVAL -- or, unwaited, the next rtw_render_status does."""
    import torch
    prims, (o, d, t), _, _ = _case(gpu, orc, "spheres")
    s, _ = _build(gpu, prims, _sphere_mats)
    s.commit(device=0)
    s.diag_corrupt_bvh(0)
    rays = gpu.make_rays(o[:64], d[:64], t[:64])
    out = np.zeros(64, np.uint8)
    L = gpu.lib()
    rp, op = rays.ctypes.data_as(C.POINTER(gpu.rtw_ray)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.rtw_occluded_rays(s._p, 0, 64, rp, None, op, None) == gpu.RTW_EINVAL
    assert "guard" in L.rtw_last_error().decode()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
    d_out = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    assert L.rtw_occluded_rays_device(s._p, 0, 64, d_rays.data_ptr(), None, d_out.data_ptr(), None, None) == 0
    assert L.rtw_render_status(s._p, 0) == gpu.RTW_EINVAL
    assert L.rtw_render_status(s._p, 0) == 0  # reported once, then cleared
